"""Every width instantiation of the DiT's token-local kernels (csrc/elementwise.hip, csrc/fp8.hip) against float64 restatements
on the CPU of the same operation, on the identical inputs: the 24 (vectors per lane x waves per row) LayerNorm + modulate kernels
in their bf16 and e4m3 forms, the 10 RMSNorm + RoPE kernels, the 8 GEMV kernels, and the row strides / channel counts of
quantize_rows and patchify that the other suites never pass.  test_kernels_gpu.py samples four widths; this file walks the tables.

Nothing is fitted here.  The bars are the project's existing ones: the per-op bf16 rule |d| <= 2^-7 |ref| + 2^-8 rms(ref)
(assert_bf16_close), the three e4m3 assertions of test_ln_modulate_fp8 (assert_ln_fp8_close), rtol 2e-5 for the GEMV
(assert_f32_close), bit-exactness for quantize_rows and patchify.  The inputs are benign (no outlier channels).

Every output buffer carries sentinel guard rows behind its last row and, where the row stride is wider than the row, sentinel
guard columns; all of them are checked after the launch.  Each test collects its failures and asserts once, so one run names every
broken width.  The supported-width lists below are literals on purpose: a change to an instantiation table in the library is then
a conscious edit here, not something a copy of the selection rule would follow silently."""
import math

import pytest
import torch
import torch.nn.functional as F

from infinicube_amd import native
from infinicube_amd.videogen.ops import RopeTable
from oracle import wan_ref as R
from test_kernels_gpu import assert_bf16_close, assert_f32_close, assert_ln_fp8_close, rnd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FP8 = torch.float8_e4m3fn
GUARD = 9.0          # bf16 / f32 sentinel
GUARD_BYTE = 0x5A    # e4m3 sentinel (as a byte)
GUARD_SCALE = 7.0    # row-scale sentinel
EPS = 1e-6

# ---- LayerNorm + modulate: d = 256 n -------------------------------------------------------------------------------------------
# default rule -> (vectors per lane, waves per row): n = 1..7 -> (n, 1); 8, 10, 12, 14 -> (n / 2, 2); 16, 20, 24, 28, 32 -> (n / 4, 4)
LN_SUPPORTED_N = (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28, 32)
LN_UNSUPPORTED_N = (9, 11, 13, 15, 17, 18, 19, 21, 22, 23, 25, 26, 27, 29, 30, 31)
# (d, ln_waves_per_row): the eight kernels only the option reaches: (8,1) (10,1) (12,1) (20,1) (10,2) (2,4) (3,4) (3,2)
LN_FORCED = ((2048, 1), (2560, 1), (3072, 1), (5120, 1), (5120, 2), (2048, 4), (3072, 4), (1536, 2))
LN_ROWS = (1, 7, 66)      # 7: three live waves in the last W = 1 block, one live + one dead row in the last W = 2 block; 66 = 2 mod 4
LN_MODES = ("plain", "affine", "modulate", "all")
LN_ZERO_ROW = 3           # an all-zero input row (inside the rows = 7 and rows = 66 cases)
LN_STDS, LN_OFFSETS = (0.5, 2.0, 8.0), (0.0, 0.5, -3.0)
# input seed per width, screened on the CPU before any GPU run (ln_case; tests/test_token_local_widths_cpu.py is the screening):
# 5000 + n unless that seed failed it (n = 7, 8, 32: a value in e4m3's subnormal range on a rounding tie), then the next of + 1000 k
LN_SEED = {n: 5000 + n for n in LN_SUPPORTED_N}
LN_SEED.update({7: 7007, 8: 6008, 32: 9032})

# ---- RMSNorm + RoPE: d = 128 n, NV = ceil(n / 4) in {1, 2, 3, 4, 5, 6, 8, 10, 12, 16} ----------------------------------------
RMS_SUPPORTED_N = tuple(range(1, 25)) + (29, 30, 31, 32, 37, 38, 39, 40, 45, 46, 47, 48, 61, 62, 63, 64)
RMS_UNSUPPORTED_N = (25, 26, 27, 28, 33, 34, 35, 36, 41, 42, 43, 44, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60)
RMS_ROWS = 9              # two full 4-row blocks plus one row
RMS_GRID, RMS_TOK0 = (3, 4, 5), 13   # tokens 13..21: starts mid-row (column 3 of row 2), crosses the frame 0 | 1 boundary at 20

# ---- GEMV ----------------------------------------------------------------------------------------------------------------------
GEMV_NK = ((1, 8), (5, 264), (1537, 520), (64, 5120))   # N % 4 != 0 (dead waves in the last block), K / 8 = 33, 65: partial lane strides


def finish(fails):
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:16])


def collect(fails, fn, *args, **kw):
    try:
        fn(*args, **kw)
    except AssertionError as e:
        fails.append(str(e))


def launched(fails, what, fn, *args, **kw):
    """A supported width that returns an error is a failure of that width, not the end of the sweep."""
    try:
        fn(*args, **kw)
        return True
    except native.NativeError as e:
        fails.append(f"{what}: {e}")
        return False


# =================================================================================================================================
# 1. LayerNorm + modulate
# =================================================================================================================================
_LN = {}


def ln_case(d):
    """Inputs [66, d] and the float64 reference per mode for width d, made once on the CPU and never modified; the smaller row counts
    are its leading rows (LayerNorm is row-local).  std / offset cycle through the nine combinations of
    test_randomised_token_local_kernels.  The seeds (LN_SEED) were screened on the CPU before the first GPU run: for each
    (d, rows, mode) used here, an fp32 torch LayerNorm of these inputs, quantised with R.quantize_rows_fp8, was compared with the
    quantised float64 reference (ln_flip_share), and a seed is kept only where the share of differing e4m3 codes is below half of
    the 0.5 % cap of assert_ln_fp8_close.  Measured: at most 0.024 % (d = 8192, rows = 1, modulate: two codes of 8192), i.e. a
    twentieth of the cap.  tests/test_token_local_widths_cpu.py repeats the screening, and says why three seeds were changed."""
    if d not in _LN:
        n = d // 256
        seed = LN_SEED[n]
        i = LN_SUPPORTED_N.index(n)
        x = rnd((66, d), seed, LN_STDS[i % 3]) + LN_OFFSETS[(i // 3) % 3]
        x[LN_ZERO_ROW] = 0.0
        p = dict(w=1 + rnd((d,), seed + 100, 0.1), b=rnd((d,), seed + 200, 0.1), sh=rnd((d,), seed + 300, 0.3), sc=rnd((d,), seed + 400, 0.3))
        ref = {}
        for mode in LN_MODES:
            aff, mod = mode in ("affine", "all"), mode in ("modulate", "all")
            y = R.layer_norm(x.double(), p["w"].double() if aff else None, p["b"].double() if aff else None, EPS)
            ref[mode] = R.modulate(y, p["sh"].double(), p["sc"].double()) if mod else y
        _LN[d] = (x, p, ref)
    return _LN[d]


def ln_args(p, mode):
    aff, mod = mode in ("affine", "all"), mode in ("modulate", "all")
    return dict(weight=p["w"] if aff else None, bias=p["b"] if aff else None, shift=p["sh"] if mod else None, scale=p["sc"] if mod else None)


def ln_flip_share(d, rows, mode):
    """CPU only: share of e4m3 codes on which an fp32 torch LayerNorm (+ fp32 modulate) differs from the float64 reference."""
    x, p, ref = ln_case(d)
    a = ln_args(p, mode)
    y = R.layer_norm(x[:rows], a["weight"], a["bias"], EPS)
    if a["scale"] is not None:
        y = R.modulate(y, a["shift"], a["scale"])
    (q32, s32), (q64, s64) = R.quantize_rows_fp8(y), R.quantize_rows_fp8(ref[mode][:rows])
    deq, want = q32 * s32[:, None], q64 * s64[:, None]
    return float((((deq - want).abs() / want.abs().clamp_min(1e-20)) > 1e-6).float().mean())   # the measure of assert_ln_fp8_close


def run_ln(hip_ops, d, rows, mode, fp8, strided, fails, tag=""):
    x, p, ref = ln_case(d)
    y = ref[mode][:rows]
    what = f"ln {'e4m3' if fp8 else 'bf16'}{tag} d={d} rows={rows} {mode}{' strided' if strided else ''}"
    ldx, ldo = (d + 4, d + 8) if strided else (d, d)
    xb = torch.full((rows, ldx), 1e30)            # anything read from the pad columns wrecks the row statistics
    xb[:, :d] = x[:rows]
    xg = xb.to(DEV)[:, :d]
    kw = {k: (None if v is None else v.to(DEV)) for k, v in ln_args(p, mode).items()}
    if fp8:
        buf = torch.full((rows + 2, ldo), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        scb = torch.full((rows + 2,), GUARD_SCALE, device=DEV)
        if not launched(fails, what, hip_ops.ln_modulate_fp8, xg, buf.view(FP8)[:rows, :d], scb[:rows], eps=EPS, **kw):
            return
        got, sc = buf.cpu(), scb.cpu()
        if not bool((got[rows:] == GUARD_BYTE).all()) or not bool((sc[rows:] == GUARD_SCALE).all()):
            fails.append(what + ": wrote past the last row")
        if not bool((got[:rows, d:] == GUARD_BYTE).all()):
            fails.append(what + ": wrote into the pad columns")
        codes = got[:rows, :d].contiguous().view(FP8).float()
        collect(fails, assert_ln_fp8_close, codes, sc[:rows], y, what)
        if rows > LN_ZERO_ROW and mode == "plain":   # a zero row stays zero only without bias / shift; the other modes check it against y
            if float(sc[LN_ZERO_ROW]) != 1.0 or bool((got[LN_ZERO_ROW, :d] != 0).any()):
                fails.append(what + f": all-zero row gave scale {float(sc[LN_ZERO_ROW])} / non-zero codes")
    else:
        buf = torch.full((rows + 2, ldo), GUARD, dtype=torch.bfloat16, device=DEV)
        if not launched(fails, what, hip_ops.ln_modulate, xg, buf[:rows, :d], eps=EPS, **kw):
            return
        got = buf.cpu()
        if not bool((got[rows:] == GUARD).all()):
            fails.append(what + ": wrote past the last row")
        if not bool((got[:rows, d:] == GUARD).all()):
            fails.append(what + ": wrote into the pad columns")
        collect(fails, assert_bf16_close, got[:rows, :d], y, what)


def run_ln_width(hip_ops, d, fp8, fails, tag=""):
    for mode in LN_MODES:
        for rows in LN_ROWS:
            run_ln(hip_ops, d, rows, mode, fp8, False, fails, tag)
        run_ln(hip_ops, d, 7, mode, fp8, True, fails, tag)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "e4m3"])
def test_ln_modulate_every_default_width(hip_ops, fp8):
    """The 16 kernels the default rule selects, each at rows 1 / 7 / 66, four modes, and once through column views of wider buffers."""
    fails = []
    for n in LN_SUPPORTED_N:
        run_ln_width(hip_ops, 256 * n, fp8, fails)
    finish(fails)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "e4m3"])
def test_ln_modulate_forced_waves_per_row(hip_ops, fp8):
    """The 8 kernels reachable only through the ln_waves_per_row option (tools/ew_bench.py's A/B switch)."""
    fails = []
    try:
        for d, W in LN_FORCED:
            assert hip_ops.lib.icv_set_option(b"ln_waves_per_row", W) == 0
            run_ln_width(hip_ops, d, fp8, fails, tag=f" W={W}")
    finally:
        hip_ops.lib.icv_set_option(b"ln_waves_per_row", 0)
    finish(fails)


def test_ln_modulate_unsupported_widths_launch_nothing(hip_ops):
    """Half of the multiples of 256 have no instantiation: both entry points return a status, name the width, and write nothing."""
    fails = []
    for n in LN_UNSUPPORTED_N:
        d = 256 * n
        x = rnd((2, d), 5100 + n).to(DEV)
        out = torch.full((3, d), GUARD, dtype=torch.bfloat16, device=DEV)
        q = torch.full((3, d), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        sc = torch.full((3,), GUARD_SCALE, device=DEV)
        for name, call in (("icv_ln_modulate", lambda: hip_ops.ln_modulate(x, out[:2], eps=EPS)),
                           ("icv_ln_modulate_fp8", lambda: hip_ops.ln_modulate_fp8(x, q.view(FP8)[:2], sc[:2], eps=EPS))):
            try:
                call()
                fails.append(f"{name} d={d}: returned 0")
            except native.NativeError as e:
                if f"unsupported d={d} " not in str(e):
                    fails.append(f"{name} d={d}: the error does not name the width: {e}")
        torch.cuda.synchronize()
        if not (bool((out == GUARD).all()) and bool((q == GUARD_BYTE).all()) and bool((sc == GUARD_SCALE).all())):
            fails.append(f"ln d={d}: an output buffer changed although the call failed")
    finish(fails)


# =================================================================================================================================
# 2. RMSNorm + RoPE
# =================================================================================================================================
def rms_ref(x, w, freqs=None):
    """float64 RMSNorm over the whole row, then the pair rotation; x is bf16 (exact in float64)."""
    y = R.rms_norm(x.double(), w.double(), EPS)
    return y if freqs is None else R.rope_apply(y, freqs, x.shape[1] // 128)


def guarded(x, extra=2):
    """x [..., rows, d] bf16 -> device copy with `extra` sentinel rows behind the last row."""
    buf = torch.full(x.shape[:-2] + (x.shape[-2] + extra, x.shape[-1]), GUARD, dtype=torch.bfloat16)
    buf[..., :x.shape[-2], :] = x
    return buf.to(DEV)


def test_rmsnorm_rope_every_width(hip_ops):
    """All 40 supported d = 128 n (10 kernels; every n % 4 != 0 leaves lanes past the row end in the last vector): q and k through
    the two-plane launch with RoPE on a shard that starts mid-row and crosses a frame boundary, and the single-tensor launch."""
    T, Hp, Wp = RMS_GRID
    rope = RopeTable.build(T, Hp, Wp, DEV)
    freqs = R.rope_freqs_3d(128, T, Hp, Wp)[RMS_TOK0: RMS_TOK0 + RMS_ROWS]
    fails = []
    for n in RMS_SUPPORTED_N:
        d = 128 * n
        planes = rnd((3, RMS_ROWS, d), 6000 + n).to(torch.bfloat16)
        w0, w1 = 1 + rnd((d,), 6100 + n, 0.1), 1 + rnd((d,), 6200 + n, 0.1)
        g = guarded(planes)
        if not (launched(fails, f"rms+rope d={d}", hip_ops.rmsnorm_rope, g[0, :RMS_ROWS], w0.to(DEV), g[1, :RMS_ROWS], w1.to(DEV), EPS, rope, RMS_TOK0)
                and launched(fails, f"rms only d={d}", hip_ops.rmsnorm_rope, g[2, :RMS_ROWS], w0.to(DEV), eps=EPS)):
            continue
        got = g.cpu()
        if not bool((got[:, RMS_ROWS:] == GUARD).all()):
            fails.append(f"rmsnorm d={d}: wrote past the last row")
        collect(fails, assert_bf16_close, got[0, :RMS_ROWS], rms_ref(planes[0], w0, freqs), f"rms+rope q d={d}")
        collect(fails, assert_bf16_close, got[1, :RMS_ROWS], rms_ref(planes[1], w1, freqs), f"rms+rope k d={d}")
        collect(fails, assert_bf16_close, got[2, :RMS_ROWS], rms_ref(planes[2], w0), f"rms only d={d}")
    finish(fails)


def test_rmsnorm_rope_unsupported_widths_launch_nothing(hip_ops):
    fails = []
    for n in RMS_UNSUPPORTED_N:
        d = 128 * n
        x = rnd((RMS_ROWS, d), 6300 + n).to(torch.bfloat16)
        g = x.to(DEV)
        try:
            hip_ops.rmsnorm_rope(g, torch.ones((d,), device=DEV), eps=EPS)
            fails.append(f"icv_rmsnorm_rope d={d}: returned 0")
        except native.NativeError as e:
            if not str(e).endswith(f"unsupported d={d}"):
                fails.append(f"icv_rmsnorm_rope d={d}: the error does not name the width: {e}")
        torch.cuda.synchronize()
        if not torch.equal(g.cpu(), x):
            fails.append(f"icv_rmsnorm_rope d={d}: the tensor changed although the call failed")
    finish(fails)


@pytest.mark.parametrize("d", [256, 1664, 5120])
def test_rmsnorm_rope_in_place_on_the_k_half_of_a_packed_kv_buffer(hip_ops, d):
    """The sequence-parallel call: K normalised and rotated in place inside a [n, 2 d] K|V buffer (ld = 2 d)."""
    T, Hp, Wp = RMS_GRID
    rope = RopeTable.build(T, Hp, Wp, DEV)
    freqs = R.rope_freqs_3d(128, T, Hp, Wp)[RMS_TOK0: RMS_TOK0 + RMS_ROWS]
    kv = rnd((RMS_ROWS, 2 * d), 6400 + d).to(torch.bfloat16)
    w = (1 + rnd((d,), 6500 + d, 0.1)).to(DEV)
    g = guarded(kv)
    hip_ops.rmsnorm_rope(g[:RMS_ROWS, :d], w, eps=EPS, rope=rope, tok0=RMS_TOK0)
    k_alone = kv[:, :d].contiguous().to(DEV)
    hip_ops.rmsnorm_rope(k_alone, w, eps=EPS, rope=rope, tok0=RMS_TOK0)
    got = g.cpu()
    fails = []
    if not bool((got[RMS_ROWS:] == GUARD).all()):
        fails.append("wrote past the last row")
    if not torch.equal(got[:RMS_ROWS, d:], kv[:, d:]):
        fails.append("the V half changed")
    if not torch.equal(got[:RMS_ROWS, :d], k_alone.cpu()):
        fails.append("the K half differs from the same launch on a contiguous copy")
    collect(fails, assert_bf16_close, got[:RMS_ROWS, :d], rms_ref(kv[:, :d], w.cpu(), freqs), f"packed K|V d={d}")
    finish(fails)


@pytest.mark.parametrize("T", [21, 32])
def test_rope_on_the_production_grids(hip_ops, T):
    """The 81-frame (21 x 30 x 52) and 125-frame (32 x 30 x 52) token grids at d = 1536: the first 66 tokens, 66 tokens across
    the frame 10 | 11 boundary, and the last 66 tokens, against R.rope_freqs_3d at those token indices."""
    Hp, Wp, d, rows = 30, 52, 1536, 66
    S = T * Hp * Wp
    rope = RopeTable.build(T, Hp, Wp, DEV)
    freqs_all = R.rope_freqs_3d(128, T, Hp, Wp)
    planes = rnd((2, rows, d), 6600 + T).to(torch.bfloat16)
    w0, w1 = 1 + rnd((d,), 6700, 0.1), 1 + rnd((d,), 6701, 0.1)
    fails = []
    for tok0 in (0, 11 * Hp * Wp - 33, S - rows):
        freqs = freqs_all[tok0: tok0 + rows]
        g = guarded(planes)
        hip_ops.rmsnorm_rope(g[0, :rows], w0.to(DEV), g[1, :rows], w1.to(DEV), EPS, rope, tok0)
        got = g.cpu()
        if not bool((got[:, rows:] == GUARD).all()):
            fails.append(f"T={T} tok0={tok0}: wrote past the last row")
        collect(fails, assert_bf16_close, got[0, :rows], rms_ref(planes[0], w0, freqs), f"rope grid T={T} tok0={tok0} q")
        collect(fails, assert_bf16_close, got[1, :rows], rms_ref(planes[1], w1, freqs), f"rope grid T={T} tok0={tok0} k")
    finish(fails)


# =================================================================================================================================
# 3. GEMV
# =================================================================================================================================
def gemv_inputs(N, K):
    return rnd((8, K), 7000 + K), rnd((N, K), 7100 + K, 1.0 / math.sqrt(K)).to(torch.bfloat16), rnd((N,), 7200 + K, 0.1)


def gemv_ref(x, w, b, in_act, out_act):
    """float64, the weights exactly as bf16."""
    h = x.double()
    h = F.silu(h) if in_act else h
    y = h @ w.double().t()
    if b is not None:
        y = y + b.double()
    return F.silu(y) if out_act else y


def gemv_f32_restatement(x, w):
    """CPU only: x [M, K] f32 @ w [N, K] bf16 in fp32 in the kernel's order: lane l adds the eight-element groups l, l + 64, ...
    (each group as four pair sums, one after the other), then the 64 lane sums meet in the xor butterfly 32, 16, ... 1."""
    M, K = x.shape
    N = w.shape[0]
    k8 = K // 8
    steps = (k8 + 63) // 64
    xp = torch.zeros((M, steps * 64, 8)); xp[:, :k8] = x.reshape(M, k8, 8)
    wp = torch.zeros((N, steps * 64, 8)); wp[:, :k8] = w.float().reshape(N, k8, 8)
    acc = torch.zeros((M, N, 64))
    for s in range(steps):
        xs, ws = xp[:, None, s * 64:(s + 1) * 64], wp[None, :, s * 64:(s + 1) * 64]
        for j in range(4):
            acc = acc + (xs[..., 2 * j] * ws[..., 2 * j] + xs[..., 2 * j + 1] * ws[..., 2 * j + 1])
    o = 32
    while o:
        acc = acc + acc[..., torch.arange(64) ^ o]
        o >>= 1
    return acc[..., 0]


@pytest.mark.parametrize("N,K", GEMV_NK)
def test_gemv_every_row_count(hip_ops, N, K):
    """M = 1..8 (one kernel each), the four activation combinations, with and without bias, against float64.
    Bar: assert_f32_close(rtol=2e-5), the existing GEMV bar, i.e. max err <= 2e-5 (10 rms + max |ref|).  It was known to hold at
    K = 256; for K = 5120 the fp32 restatement above (the kernel's summation order, M = 8, N = 64) was measured on the CPU against
    float64 before the first GPU run: max err 4.0e-7 against an allowed 2.5e-4, i.e. 0.16 % of the bar (0.20 % with SiLU'd inputs;
    0.03 %, 0.07 %, 0.16 % at K = 8, 264, 520), far below half of it, so the bar stands unchanged at every K.
    tests/test_token_local_widths_cpu.py repeats the measurement."""
    x8, w, b = gemv_inputs(N, K)
    xg, wg, bg = x8.to(DEV), w.to(DEV), b.to(DEV)
    fails = []
    for in_act in (0, 1):
        for out_act in (0, 1):
            for bias in (None, b):
                ref8 = gemv_ref(x8, w, bias, in_act, out_act)
                for M in range(1, 9):
                    what = f"gemv M={M} N={N} K={K} act=({in_act},{out_act}) bias={bias is not None}"
                    out = torch.full((M + 1, N), GUARD, device=DEV)
                    if not launched(fails, what, hip_ops.gemv, xg[:M], wg, None if bias is None else bg, out[:M], in_act, out_act):
                        continue
                    got = out.cpu()
                    if not bool((got[M] == GUARD).all()):
                        fails.append(what + ": wrote past the last row")
                    collect(fails, assert_f32_close, got[:M], ref8[:M], rtol=2e-5, what=what)
    finish(fails)


# =================================================================================================================================
# 4. Row strides of quantize_rows and patchify, the i2v channel count
# =================================================================================================================================
@pytest.mark.parametrize("src", ["bf16", "f32"])
def test_quantize_rows_fp8_strided_bit_exact(hip_ops, src):
    """src and out as column views of wider buffers (ld = ldo = K + 8): codes and scales bit-exact, pads and guard rows untouched."""
    fails = []
    for rows, K in ((5, 8), (7, 520), (9, 1536)):
        what = f"quantize_rows {src} rows={rows} K={K}"
        x = rnd((rows, K), 8000 + K, 3.0)
        x[:, ::7] *= 40.0
        x[rows // 2] = 0.0
        x[1] *= 1e-6
        xs = x.to(torch.bfloat16) if src == "bf16" else x
        xb = torch.full((rows, K + 8), 3e4, dtype=xs.dtype)      # a pad column read into the row maximum changes scale and codes
        xb[:, :K] = xs
        buf = torch.full((rows + 2, K + 8), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        scb = torch.full((rows + 2,), GUARD_SCALE, device=DEV)
        if not launched(fails, what, hip_ops.quantize_rows, xb.to(DEV)[:, :K], buf.view(FP8)[:rows, :K], scb[:rows]):
            continue
        got, sc = buf.cpu(), scb.cpu()
        qr, sr = R.quantize_rows_fp8(xs.float())
        if not torch.equal(sc[:rows], sr):
            fails.append(what + ": row scales differ")
        nbad = int((got[:rows, :K].contiguous().view(FP8).float() != qr).sum())
        if nbad:
            fails.append(what + f": {nbad} / {qr.numel()} e4m3 codes differ from the oracle")
        if not bool((got[rows:] == GUARD_BYTE).all()) or not bool((sc[rows:] == GUARD_SCALE).all()):
            fails.append(what + ": wrote past the last row")
        if not bool((got[:rows, K:] == GUARD_BYTE).all()):
            fails.append(what + ": wrote into the pad columns")
    finish(fails)


@pytest.mark.parametrize("C", [16, 36])
def test_patchify_channel_counts_and_strided_output(hip_ops, C):
    """C = 16 (t2v) and C = 36 (i2v: WAN_14B_I2V.in_dim), three grids, a shard that crosses a frame boundary where the grid has one,
    out as a column view with ldo = 4 C + 4; bit-exact against the reshape / permute restatement."""
    fails = []
    for (T, H8, W8), tok0, n in (((1, 2, 2), 0, 1), ((2, 4, 6), 4, 5), ((3, 8, 12), 17, 40)):
        what = f"patchify C={C} grid=({T},{H8},{W8}) tok0={tok0} n={n}"
        Hp, Wp = H8 // 2, W8 // 2
        lat = rnd((C, T, H8, W8), 8100 + C + T)
        buf = torch.full((n + 2, 4 * C + 4), GUARD, dtype=torch.bfloat16, device=DEV)
        if not launched(fails, what, hip_ops.patchify, lat.to(DEV), buf[:n, :4 * C], tok0, n):
            continue
        got = buf.cpu()
        ref = lat.reshape(C, T, Hp, 2, Wp, 2).permute(1, 2, 4, 0, 3, 5).reshape(T * Hp * Wp, C * 4)[tok0: tok0 + n]
        if not torch.equal(got[:n, :4 * C], ref.to(torch.bfloat16)):
            fails.append(what + ": tokens differ")
        if not bool((got[n:] == GUARD).all()):
            fails.append(what + ": wrote past the last row")
        if not bool((got[:n, 4 * C:] == GUARD).all()):
            fails.append(what + ": wrote into the pad columns")
    finish(fails)
