"""The CPU-side screening that tests/test_token_local_widths_gpu.py relies on, kept as tests so that an edit of a seed, a width list
or a shape there is screened again before it reaches a GPU.

The e4m3 bar of assert_ln_fp8_close compares the kernel's fp32 LayerNorm with a float64 one after quantisation.  fp32 rounding may
move a value across an e4m3 rounding tie; the bar allows that on < 0.5 % of the elements and by a relative step <= 0.126, which is
one code step for a NORMAL e4m3 code.  In e4m3's subnormal range (|y| below 2^-6 / 448 of the row maximum, about one element in
10^4 of a LayerNorm'd row) one code step is a relative step between 1/7 and 1, so an input with a value there that sits on a tie
to within fp32 rounding cannot meet the bar whatever the kernel does.  The screening therefore keeps a seed only if
  (a) the code-flip share of an fp32 torch LayerNorm is under half of the 0.5 % cap (ln_flip_share), and
  (b) a restatement of ln_modulate_kernel in fp32 in the kernel's own summation order (lane partial sums, xor butterfly, the W wave
      sums in order; the row mean is bit-identical to the kernel's, and it is the mean's rounding that decides such ties) meets all
      three assertions of the bar, and the bf16 bar."""
import torch

import test_token_local_widths_gpu as T
from oracle import wan_ref as R
from test_kernels_gpu import assert_bf16_close, assert_ln_fp8_close

_XOR = {o: torch.arange(64) ^ o for o in (32, 16, 8, 4, 2, 1)}


def wave_sum(v):
    """[..., 64] -> [...]: v += shfl_xor(v, o) for o = 32 ... 1 (every lane ends with the same bits)."""
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., _XOR[o]]
    return v[..., 0]


def row_sum(part, W):
    """part [rows, W, 64] -> [rows]: wave sums, then the W of them added in order from 0 (row_sum<W> of csrc/elementwise.hip)."""
    ws = wave_sum(part)
    if W == 1:
        return ws[:, 0]
    t = torch.zeros(ws.shape[0])
    for i in range(W):
        t = t + ws[:, i]
    return t


def ln_kernel_f32(x, a, W):
    """ln_modulate_kernel<d / 256 / W, W> on x [rows, d] f32, before the output conversion."""
    rows, d = x.shape
    NV = d // 256 // W
    v = x.reshape(rows, NV, W, 64, 4)                      # float4 index within the row = (i * W + sub) * 64 + lane
    s = torch.zeros(rows, W, 64)
    for i in range(NV):
        s = s + ((v[:, i, :, :, 0] + v[:, i, :, :, 1]) + (v[:, i, :, :, 2] + v[:, i, :, :, 3]))
    v = v - (row_sum(s, W) / torch.tensor(float(d)))[:, None, None, None, None]
    q = torch.zeros(rows, W, 64)
    for i in range(NV):
        u = v[:, i]
        q = q + ((u[..., 0] * u[..., 0] + u[..., 1] * u[..., 1]) + (u[..., 2] * u[..., 2] + u[..., 3] * u[..., 3]))
    rstd = torch.rsqrt(row_sum(q, W) / torch.tensor(float(d)) + torch.tensor(T.EPS))
    y = (v * rstd[:, None, None, None, None]).reshape(rows, d)
    if a["weight"] is not None:
        y = y * a["weight"]
    if a["bias"] is not None:
        y = y + a["bias"]
    if a["scale"] is not None:
        y = y * (1.0 + a["scale"])
    if a["shift"] is not None:
        y = y + a["shift"]
    return y


def default_waves(nvec):
    return 4 if (nvec >= 16 and nvec % 4 == 0) else 2 if (nvec >= 8 and nvec % 2 == 0) else 1


def test_ln_seeds_meet_the_e4m3_bar_in_fp32_on_the_cpu():
    waves = {256 * n: {default_waves(n)} for n in T.LN_SUPPORTED_N}
    for d, W in T.LN_FORCED:
        waves[d].add(W)
    fails, worst = [], (-1.0, (0, 0, ""))
    for d in sorted(waves):
        x, p, ref = T.ln_case(d)
        for mode in T.LN_MODES:
            for rows in T.LN_ROWS:
                share = T.ln_flip_share(d, rows, mode)
                worst = max(worst, (share, (d, rows, mode)))
                if not share < 2.5e-3:
                    fails.append(f"d={d} rows={rows} {mode}: fp32 torch LayerNorm flips {share:.3%} of the e4m3 codes (half the cap: 0.25 %)")
            for W in sorted(waves[d]):
                y = ln_kernel_f32(x, T.ln_args(p, mode), W)
                for rows in T.LN_ROWS:
                    what = f"kernel-order fp32 d={d} W={W} rows={rows} {mode}"
                    T.collect(fails, assert_ln_fp8_close, *R.quantize_rows_fp8(y[:rows]), ref[mode][:rows], what)
                    T.collect(fails, assert_bf16_close, y[:rows].to(torch.bfloat16), ref[mode][:rows], what)
    print(f"largest e4m3 flip share of an fp32 torch LayerNorm: {worst[0]:.4%} at (d, rows, mode) = {worst[1]}")
    T.finish(fails)


def test_gemv_fp32_summation_order_error_is_far_under_the_bar():
    """The measurement behind test_gemv_every_row_count: fp32 in the kernel's order against float64, as a fraction of what
    assert_f32_close(rtol=2e-5) allows.  Under half at every K, so the bar is used unchanged."""
    for N, K in T.GEMV_NK:
        x8, w, _ = T.gemv_inputs(N, K)
        ref = T.gemv_ref(x8, w, None, 0, 0)
        err = float((T.gemv_f32_restatement(x8, w).double() - ref).abs().max())
        allowed = 2e-5 * 10 * float(ref.pow(2).mean().sqrt()) + 2e-5 * float(ref.abs().max())
        print(f"gemv N={N} K={K}: fp32 max err {err:.3g}, allowed {allowed:.3g} ({err / allowed:.2%})")
        assert err < 0.5 * allowed
