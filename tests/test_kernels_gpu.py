"""Per-kernel parity: libicvideo HIP kernels (through the C ABI) vs the CPU oracle.

Tolerance (SURVEY.md §8d, bf16 outputs vs fp32 oracle on identical bf16-rounded inputs):
    |delta| <= 2^-7 * |ref| + 2^-8 * rms(ref)      (attention: 2^-7 * |ref| + 2^-5 * rms(ref) and rms error <= 2^-7 * rms(ref))
fp32 outputs use rtol 1e-4 of rms unless noted.
"""
import math
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import wan_ref as R
from infinicube_amd.videogen.ops import RopeTable, EPI_BF16, EPI_GELU_BF16, EPI_RESID_F32, EPI_F32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def need_experiments(hip_ops):
    """The measured-slower A/B kernels (attention families 1, 3-6, the 4-wave GEMM) live under csrc/experiments/ and are
    compiled in only by `ICV_EXPERIMENTS=1 csrc/build.sh`; the shipped library does not carry them."""
    if hip_ops.lib.icv_set_option(b"require_experiments", 1) != 0:
        pytest.skip("libicvideo built without ICV_EXPERIMENTS=1")


EXPERIMENT_KERNELS = (1, 3, 4, 5, 6, 9)
ATTN_DEFAULT = 7   # icv_set_option("attn_kernel") value of the shipped default (tests restore it after an A/B switch)


def rnd(shape, seed, std=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * std).to(dtype)


def assert_bf16_close(got, ref, what="", abs_floor=2.0 ** -8, rms_bound=None):
    got, ref = got.float().cpu(), ref.float().cpu()
    rms = ref.pow(2).mean().sqrt()
    if rms_bound is not None:
        rms_err = (got - ref).pow(2).mean().sqrt()
        assert rms_err <= rms_bound * rms, f"{what}: rms err {rms_err:.4g} > {rms_bound:.3g} * rms {rms:.4g}"
    tol = (2.0 ** -7) * ref.abs() + abs_floor * rms
    bad = (got - ref).abs() > tol
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} outside tol; max err {(got - ref).abs().max():.4g}, rms {rms:.4g}"


def assert_f32_close(got, ref, rtol=1e-4, what=""):
    got, ref = got.float().cpu(), ref.float().cpu()
    rms = ref.pow(2).mean().sqrt()
    err = (got - ref).abs().max()
    assert err <= rtol * max(float(rms), 1e-12) * 10 + rtol * float(ref.abs().max()), f"{what}: max err {err:.4g} rms {rms:.4g}"


@pytest.mark.parametrize("d", [256, 1536, 5120])
@pytest.mark.parametrize("mode", ["plain", "modulate", "affine", "all"])
def test_ln_modulate(hip_ops, d, mode):
    rows = 37
    x = rnd((rows, d), 1, 2.0) + 0.5
    w = 1 + rnd((d,), 2, 0.1) if mode in ("affine", "all") else None
    b = rnd((d,), 3, 0.1) if mode in ("affine", "all") else None
    sh = rnd((d,), 4, 0.3) if mode in ("modulate", "all") else None
    sc = rnd((d,), 5, 0.3) if mode in ("modulate", "all") else None
    ref = R.layer_norm(x, w, b, 1e-6)
    if sc is not None:
        ref = R.modulate(ref, sh, sc)
    dv = lambda t: None if t is None else t.to(DEV)
    out = torch.empty((rows, d), dtype=torch.bfloat16, device=DEV)
    hip_ops.ln_modulate(x.to(DEV), out, dv(w), dv(b), dv(sh), dv(sc), 1e-6)
    assert_bf16_close(out, ref, f"ln d={d} {mode}")


@pytest.mark.parametrize("d", [256, 512, 1536, 5120])
def test_rmsnorm_rope(hip_ops, d):
    T, Hp, Wp = 3, 4, 5
    S = T * Hp * Wp
    tok0, n = 7, 41   # a shard in the middle of the grid
    heads = d // 128
    planes = rnd((3, n, d), 11).to(torch.bfloat16)
    w0, w1 = 1 + rnd((d,), 12, 0.1), 1 + rnd((d,), 13, 0.1)
    freqs = R.rope_freqs_3d(128, T, Hp, Wp)[tok0: tok0 + n]
    ref0 = R.rope_apply(R.rms_norm(planes[0].float(), w0, 1e-6), freqs, heads)
    ref1 = R.rope_apply(R.rms_norm(planes[1].float(), w1, 1e-6), freqs, heads)
    g = planes.to(DEV)
    rope = RopeTable.build(T, Hp, Wp, DEV)
    hip_ops.rmsnorm_rope(g[0], w0.to(DEV), g[1], w1.to(DEV), 1e-6, rope, tok0)
    assert_bf16_close(g[0], ref0, "rms+rope q")
    assert_bf16_close(g[1], ref1, "rms+rope k")
    assert torch.equal(g[2].cpu(), planes[2]), "v plane must be untouched"
    # no-rope, single tensor (cross-attention q / k)
    g2 = planes[2].clone().to(DEV)
    hip_ops.rmsnorm_rope(g2, w0.to(DEV), eps=1e-6)
    assert_bf16_close(g2, R.rms_norm(planes[2].float(), w0, 1e-6), "rms only")


GEMM_SHAPES = [(200, 256, 128), (1, 256, 64), (129, 64, 256), (1000, 1536, 1536), (777, 512, 8960), (300, 4608, 1536),
               (256, 256, 64), (2000, 768, 192), (513, 1280, 1024)]


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
@pytest.mark.parametrize("epi", [EPI_BF16, EPI_GELU_BF16, EPI_RESID_F32, EPI_F32])
def test_gemm(hip_ops, M, N, K, epi):
    a = rnd((M, K), 21).to(torch.bfloat16)
    w = rnd((N, K), 22, 1.0 / math.sqrt(K)).to(torch.bfloat16)
    bias = rnd((N,), 23, 0.1)
    acc = a.float() @ w.float().t() + bias
    if epi in (EPI_BF16, EPI_GELU_BF16):
        ref = F.gelu(acc, approximate="tanh") if epi == EPI_GELU_BF16 else acc
        out = torch.empty((M, N), dtype=torch.bfloat16, device=DEV)
        hip_ops.gemm(a.to(DEV), w.to(DEV), bias.to(DEV), out, epi)
        assert_bf16_close(out, ref, f"gemm {M}x{N}x{K} epi{epi}")
    elif epi == EPI_RESID_F32:
        resid, gate = rnd((M, N), 24), rnd((N,), 25)
        x = resid.clone().to(DEV)
        hip_ops.gemm(a.to(DEV), w.to(DEV), bias.to(DEV), x, epi, resid=x, gate=gate.to(DEV))
        assert_f32_close(x, resid + gate * acc, what="gemm resid gate (in place)")
        x2 = torch.empty((M, N), device=DEV)
        hip_ops.gemm(a.to(DEV), w.to(DEV), None, x2, epi, resid=resid.to(DEV))
        assert_f32_close(x2, resid + (acc - bias), what="gemm resid nogate nobias")
    else:
        out = torch.empty((M, N), device=DEV)
        hip_ops.gemm(a.to(DEV), w.to(DEV), bias.to(DEV), out, epi)
        assert_f32_close(out, acc, what="gemm f32")


@pytest.mark.parametrize("epi", [EPI_BF16, EPI_GELU_BF16, EPI_RESID_F32, EPI_F32])
def test_gemm256_mfma32_variant(hip_ops, epi):
    """gemm256 with v_mfma_f32_32x32x16_bf16 fragments (option gemm256_mfma = 32) against the oracle, incl.
    an M tail, a split-plane output and a transposition-detecting identity case."""
    hip_ops.lib.icv_set_option(b"gemm256", 1)
    hip_ops.lib.icv_set_option(b"gemm256_mfma", 32)
    try:
        for M, N, K in ((777, 512, 256), (1500, 1024, 2048), (256, 256, 64)):
            a = rnd((M, K), 221).to(torch.bfloat16)
            w = rnd((N, K), 222, 1.0 / math.sqrt(K)).to(torch.bfloat16)
            bias = rnd((N,), 223, 0.1)
            acc = a.float() @ w.float().t() + bias
            if epi in (EPI_BF16, EPI_GELU_BF16):
                out = torch.empty((M, N), dtype=torch.bfloat16, device=DEV)
                hip_ops.gemm(a.to(DEV), w.to(DEV), bias.to(DEV), out, epi)
                assert_bf16_close(out, F.gelu(acc, approximate="tanh") if epi == EPI_GELU_BF16 else acc, f"gemm256/32 {M}x{N}x{K}")
            elif epi == EPI_RESID_F32:
                resid, gate = rnd((M, N), 224), rnd((N,), 225)
                x = resid.clone().to(DEV)
                hip_ops.gemm(a.to(DEV), w.to(DEV), bias.to(DEV), x, epi, resid=x, gate=gate.to(DEV))
                assert_f32_close(x, resid + gate * acc, what="gemm256/32 resid")
            else:
                out = torch.empty((M, N), device=DEV)
                hip_ops.gemm(a.to(DEV), w.to(DEV), bias.to(DEV), out, epi)
                assert_f32_close(out, acc, what="gemm256/32 f32")
        if epi == EPI_F32:
            n = 256
            eye = torch.eye(n).to(torch.bfloat16)
            w = (torch.arange(n * n, dtype=torch.float32).reshape(n, n) % 251 - 125).to(torch.bfloat16)
            out = torch.empty((n, n), device=DEV)
            hip_ops.gemm(eye.to(DEV), w.to(DEV), None, out, EPI_F32)
            assert torch.equal(out.cpu(), w.float().t())
        if epi == EPI_BF16:
            M, d, K = 333, 256, 512
            a = rnd((M, K), 231).to(torch.bfloat16)
            w = rnd((3 * d, K), 232, 0.05).to(torch.bfloat16)
            bias = rnd((3 * d,), 233, 0.1)
            out = torch.full((3, M, d), 7.0, dtype=torch.bfloat16, device=DEV)
            hip_ops.gemm(a.to(DEV), w.to(DEV), bias.to(DEV), out, EPI_BF16, nsplit=d)
            assert_bf16_close(out, (a.float() @ w.float().t() + bias).reshape(M, 3, d).permute(1, 0, 2), "gemm256/32 split")
    finally:
        hip_ops.lib.icv_set_option(b"gemm256", 2)
        hip_ops.lib.icv_set_option(b"gemm256_mfma", 16)


@pytest.mark.parametrize("epi", [EPI_BF16, EPI_GELU_BF16, EPI_RESID_F32, EPI_F32])
def test_gemm256_ksplit_schedule_is_bit_identical(hip_ops, epi):
    """gemm256_sched 67 (round 4's A/B: the four LDS units of a stage cut by k-half, one k-step of all 32 accumulators per phase)
    adds the same products in the same k order per accumulator as the default schedule: bit-identical outputs - incl. an M
    tail, a strided A, a split-plane output, K of 1 / 2 / many tiles - and deterministic under repetition (race screen)."""
    lib = hip_ops.lib
    lib.icv_set_option(b"gemm256", 1)
    try:
        for M, N, K, pad in ((777, 512, 256, 0), (1500, 1024, 2048, 64), (256, 256, 64, 0), (300, 768, 128, 0), (2049, 256, 5120, 0)):
            a_full = rnd((M, K + pad), 321).to(torch.bfloat16).to(DEV)
            a = a_full[:, :K]
            w = rnd((N, K), 322, 1.0 / math.sqrt(K)).to(torch.bfloat16).to(DEV)
            bias = rnd((N,), 323, 0.1).to(DEV)
            resid, gate = rnd((M, N), 324).to(DEV), rnd((N,), 325).to(DEV)
            outs = {}
            for sched in (3, 67, 67):
                lib.icv_set_option(b"gemm256_sched", sched)
                if epi == EPI_RESID_F32:
                    out = resid.clone()
                    hip_ops.gemm(a, w, bias, out, epi, resid=out, gate=gate)
                elif epi == EPI_BF16 and N % 3 == 0:
                    out = torch.zeros((3, M, N // 3), dtype=torch.bfloat16, device=DEV)
                    hip_ops.gemm(a, w, bias, out, epi, nsplit=N // 3)
                else:
                    out = torch.zeros((M, N), dtype=torch.float32 if epi == EPI_F32 else torch.bfloat16, device=DEV)
                    hip_ops.gemm(a, w, bias, out, epi)
                torch.cuda.synchronize()
                outs.setdefault(sched, []).append(out)
            assert torch.equal(outs[67][0], outs[3][0]), f"k-split schedule differs from the default at M={M} N={N} K={K} epi={epi}"
            assert torch.equal(outs[67][0], outs[67][1]), "k-split schedule is not deterministic (race?)"
    finally:
        lib.icv_set_option(b"gemm256", 2)
        lib.icv_set_option(b"gemm256_sched", 3)


@pytest.mark.parametrize("variant", [0, 1])
def test_gemm_variants_agree_and_race_screen(hip_ops, variant):
    """128-tile kernel vs 256-tile 4-phase kernel on the same problem (compare both to the oracle),
    repeated to screen the counted-vmcnt schedule for races: every repeat must be bit-identical."""
    M, N, K = 1500, 1024, 2048
    a = rnd((M, K), 121).to(torch.bfloat16).to(DEV)
    w = rnd((N, K), 122, 1.0 / math.sqrt(K)).to(torch.bfloat16).to(DEV)
    bias = rnd((N,), 123, 0.1).to(DEV)
    ref = a.float().cpu() @ w.float().cpu().t() + bias.cpu()
    hip_ops.lib.icv_set_option(b"gemm256", variant)
    try:
        outs = []
        for _ in range(6):
            out = torch.empty((M, N), device=DEV)
            hip_ops.gemm(a, w, bias, out, EPI_F32)
            outs.append(out)
        torch.cuda.synchronize()
    finally:
        hip_ops.lib.icv_set_option(b"gemm256", 2)
    assert_f32_close(outs[0], ref, what=f"gemm variant {variant}")
    for o in outs[1:]:
        assert torch.equal(o, outs[0]), "non-deterministic GEMM result (race in the pipelined schedule?)"


def test_gemm_split_and_strided(hip_ops):
    M, d, K = 333, 256, 512
    a_full = rnd((M, K + 64), 31).to(torch.bfloat16)
    a = a_full[:, :K]            # strided A (lda = K + 64)
    w = rnd((3 * d, K), 32, 0.05).to(torch.bfloat16)
    bias = rnd((3 * d,), 33, 0.1)
    ref = (a.float() @ w.float().t() + bias).reshape(M, 3, d).permute(1, 0, 2)
    out = torch.full((3, M, d), 7.0, dtype=torch.bfloat16, device=DEV)
    hip_ops.gemm(a_full.to(DEV)[:, :K], w.to(DEV), bias.to(DEV), out, EPI_BF16, nsplit=d)
    assert_bf16_close(out, ref, "split qkv gemm")


def test_gemm_transposed_identity(hip_ops):
    """A = I with an ASYMMETRIC W catches any row/col swap of the MFMA C layout."""
    n = 128
    a = torch.eye(n).to(torch.bfloat16)
    w = (torch.arange(n * n, dtype=torch.float32).reshape(n, n) % 251 - 125).to(torch.bfloat16)
    out = torch.empty((n, n), device=DEV)
    hip_ops.gemm(a.to(DEV), w.to(DEV), None, out, EPI_F32)
    assert torch.equal(out.cpu(), w.float().t())


@pytest.mark.parametrize("M", [1, 3])
def test_gemv_and_time_path(hip_ops, M):
    K, N = 256, 1536
    x, w, b = rnd((M, K), 41), rnd((N, K), 42, 0.05).to(torch.bfloat16), rnd((N,), 43, 0.1)
    out = torch.empty((M, N), device=DEV)
    hip_ops.gemv(x.to(DEV), w.to(DEV), b.to(DEV), out, 1, 1)
    assert_f32_close(out, F.silu(F.silu(x) @ w.float().t() + b), rtol=2e-5, what="gemv silu/silu")
    hip_ops.gemv(x.to(DEV), w.to(DEV), None, out, 0, 0)
    assert_f32_close(out, x @ w.float().t(), rtol=2e-5, what="gemv plain")


def test_sinusoidal_bcast_cast(hip_ops):
    out = torch.empty((1, 256), device=DEV)
    hip_ops.sinusoidal(937.5, out)
    ref = R.sinusoidal_embedding_1d(256, torch.tensor([937.5], dtype=torch.float64)).float()
    assert (out.cpu() - ref).abs().max() < 2e-6
    a, b = rnd((5, 96), 51), rnd((96,), 52)
    o = torch.empty((5, 96), device=DEV)
    hip_ops.bcast_add(a.to(DEV), b.to(DEV), o)
    assert torch.equal(o.cpu(), a + b)
    src = rnd((1027,), 53)
    dst = torch.empty((1027,), dtype=torch.bfloat16, device=DEV)
    hip_ops.cast_bf16(src.to(DEV), dst)
    assert torch.equal(dst.cpu(), src.to(torch.bfloat16))


ATTN_CASES = [
    (256, 64, 1), (300, 300, 2), (256, 512, 2), (100, 32, 2), (33, 1, 1), (513, 1000, 3), (2240, 2240, 12),
]


@pytest.mark.parametrize("Sq,Skv,H", ATTN_CASES)
def test_attention(hip_ops, Sq, Skv, H):
    d = H * 128
    q, k, v = (rnd((Sq, d), 61).to(torch.bfloat16), rnd((Skv, d), 62).to(torch.bfloat16),
               rnd((Skv, d), 63).to(torch.bfloat16))
    ref = R.attention(q.float(), k.float(), v.float(), H)
    o = torch.zeros((Sq, d), dtype=torch.bfloat16, device=DEV)
    hip_ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), o, H, 1.0 / math.sqrt(128))
    # attention has TWO bf16 rounding points (P before the PV MFMA, then the output): per element
    # |delta| <= 2^-7 |ref| + 2^-5 rms (tails over millions of outputs), AND rms error <= 2^-7 rms
    # (measured: 0.23 % of rms, max 1.9 % of rms; identical for defer-max thresholds 0..8)
    assert_bf16_close(o, ref, f"attention Sq={Sq} Skv={Skv} H={H}", abs_floor=2.0 ** -5, rms_bound=2.0 ** -7)


@pytest.mark.experiments
@pytest.mark.parametrize("variant", [0, 1, 2, 3, 5, 7])
@pytest.mark.parametrize("thr", [0, 8])
def test_attention_variants(hip_ops, variant, thr):
    """Every kernel variant (stagger / QK interleave / setprio) and both defer-max settings must agree
    with the oracle; spiked keys force the rescale branch both early and in the last (masked) tile."""
    need_experiments(hip_ops)
    Sq, Skv, H = 520, 1100, 2
    d = H * 128
    q, k, v = (rnd((Sq, d), 161).to(torch.bfloat16), rnd((Skv, d), 162).to(torch.bfloat16), rnd((Skv, d), 163).to(torch.bfloat16))
    k[1090] = q[7] * 5.0
    k[70] = q[300] * 5.0
    ref = R.attention(q.float(), k.float(), v.float(), H)
    hip_ops.lib.icv_set_option(b"attn_kernel", 1)
    hip_ops.lib.icv_set_option(b"attn_variant", variant)
    hip_ops.lib.icv_set_option(b"attn_defer_max_log2", thr)
    try:
        o = torch.zeros((Sq, d), dtype=torch.bfloat16, device=DEV)
        hip_ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), o, H, 1.0 / math.sqrt(128))
        o2 = torch.zeros_like(o)
        hip_ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), o2, H, 1.0 / math.sqrt(128))
        torch.cuda.synchronize()
    finally:
        hip_ops.lib.icv_set_option(b"attn_kernel", ATTN_DEFAULT)
        hip_ops.lib.icv_set_option(b"attn_variant", 5)
        hip_ops.lib.icv_set_option(b"attn_defer_max_log2", 8)
    assert torch.equal(o, o2), "non-deterministic attention output (LDS staging race?)"
    assert_bf16_close(o, ref, f"attention variant {variant} thr {thr}", abs_floor=2.0 ** -5, rms_bound=2.0 ** -7)


@pytest.mark.parametrize("variant", [0, 1, 4, 5, 12, 13])
def test_attention2_variants(hip_ops, variant):
    """attn2.hip (128-key staged tile, two 64-key halves per barrier pair) in every variant, including
    Skv values that leave the second half of the last tile empty / partially masked."""
    H = 2
    d = H * 128
    hip_ops.lib.icv_set_option(b"attn_kernel", 2)
    hip_ops.lib.icv_set_option(b"attn2_variant", variant)
    try:
        for Sq, Skv in ((300, 1100), (64, 64), (257, 65), (100, 129), (513, 640)):
            q, k, v = (rnd((Sq, d), 171).to(torch.bfloat16), rnd((Skv, d), 172).to(torch.bfloat16), rnd((Skv, d), 173).to(torch.bfloat16))
            k[Skv - 1] = q[3] * 5.0
            ref = R.attention(q.float(), k.float(), v.float(), H)
            o = torch.zeros((Sq, d), dtype=torch.bfloat16, device=DEV)
            hip_ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), o, H, 1.0 / math.sqrt(128))
            o2 = torch.zeros_like(o)
            hip_ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), o2, H, 1.0 / math.sqrt(128))
            assert torch.equal(o, o2), "non-deterministic attention output (LDS staging race?)"
            assert_bf16_close(o, ref, f"attn2 variant {variant} Sq={Sq} Skv={Skv}", abs_floor=2.0 ** -5, rms_bound=2.0 ** -7)
        # scores that keep growing along the key axis (every tile outgrows the running reference: the rescale path,
        # lazy or not, fires again and again), and a row whose scores are hugely negative everywhere
        Sq, Skv = 130, 1500
        q = rnd((Sq, d), 174).to(torch.bfloat16)
        k = (rnd((Skv, d), 175) * torch.linspace(0.2, 6.0, Skv)[:, None]).to(torch.bfloat16)
        k[:, :128] += (q[5, :128].float() * torch.linspace(0.0, 3.0, Skv)[:, None]).to(torch.bfloat16)
        v = rnd((Skv, d), 176).to(torch.bfloat16)
        q[7] = -8.0 * k[:, :].float().mean(0).to(torch.bfloat16)
        ref = R.attention(q.float(), k.float(), v.float(), H)
        o = torch.zeros((Sq, d), dtype=torch.bfloat16, device=DEV)
        hip_ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), o, H, 1.0 / math.sqrt(128))
        assert torch.isfinite(o.float()).all()
        assert_bf16_close(o, ref, f"attn2 variant {variant} growing scores", abs_floor=2.0 ** -5, rms_bound=2.0 ** -7)
    finally:
        hip_ops.lib.icv_set_option(b"attn2_variant", 12); hip_ops.lib.icv_set_option(b"attn_kernel", ATTN_DEFAULT)


@pytest.mark.parametrize("variant", [0, 1, 4, 5, 6, 7, 8, 32, 128, 132])
def test_attention7_variants(hip_ops, variant):
    """attn7.hip (LDS-DMA ring + lazy max + persistent reference vector) at the generic scale; the unit-scale route is
    covered by test_attention_unit_scale[kernel 7]."""
    H = 2
    d = H * 128
    hip_ops.lib.icv_set_option(b"attn_kernel", ATTN_DEFAULT); hip_ops.lib.icv_set_option(b"attn7_variant", variant)
    try:
        for Sq, Skv in ((300, 1100), (64, 64), (257, 65), (33, 129), (513, 640), (1000, 3000), (1, 1)):
            q, k, v = (rnd((Sq, d), 191).to(torch.bfloat16), rnd((Skv, d), 192).to(torch.bfloat16), rnd((Skv, d), 193).to(torch.bfloat16))
            k[Skv - 1] = q[min(3, Sq - 1)] * 5.0
            k[Skv // 2] = q[min(40, Sq - 1)] * 5.0
            ref = R.attention(q.float(), k.float(), v.float(), H)
            o = torch.zeros((Sq, d), dtype=torch.bfloat16, device=DEV)
            hip_ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), o, H, 1.0 / math.sqrt(128))
            o2 = torch.zeros_like(o)
            hip_ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), o2, H, 1.0 / math.sqrt(128))
            assert torch.equal(o, o2), "non-deterministic attention output (LDS-DMA ring race?)"
            assert_bf16_close(o, ref, f"attn7 variant {variant} Sq={Sq} Skv={Skv}", abs_floor=2.0 ** -5, rms_bound=2.0 ** -7)
    finally:
        hip_ops.lib.icv_set_option(b"attn_kernel", ATTN_DEFAULT); hip_ops.lib.icv_set_option(b"attn7_variant", -1)


@pytest.mark.parametrize("unit", [0, 1])
def test_attention7_short_key_shape(hip_ops, unit):
    """The short-key launch shape of attn7 (4-wave blocks of 128 query rows on a two-stage ring, two blocks per CU; the
    cross-attention route): plain, summed-into-output (i2v image branch) and carried-state calls, generic and unit
    scale, ragged query / key counts incl. the 512-key and 257-key cross-attention sizes.  Forced for EVERY key count
    here with "attn7_short" so that multi-tile rings (9+ tiles) are exercised too."""
    H = 2
    d = H * 128
    fold = (1.0 / math.sqrt(128)) * math.log2(math.e)
    scale = math.log(2.0) if unit else 1.0 / math.sqrt(128)
    hip_ops.lib.icv_set_option(b"attn_kernel", ATTN_DEFAULT); hip_ops.lib.icv_set_option(b"attn7_short", 1 << 30)
    try:
        for Sq, Skv in ((300, 512), (129, 257), (128, 64), (1, 1), (513, 640), (1000, 1100), (257, 65)):
            q, kf, v = (rnd((Sq, d), 291).to(torch.bfloat16), rnd((Skv, d), 292), rnd((Skv, d), 293).to(torch.bfloat16))
            kf[Skv - 1] = q[min(3, Sq - 1)].float() * 5.0
            kf[Skv // 2] = q[min(40, Sq - 1)].float() * 5.0
            k = (kf * fold).to(torch.bfloat16) if unit else kf.to(torch.bfloat16)
            ref = R.attention(q.float(), k.float(), v.float(), H, scale=scale)
            qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
            o = torch.zeros((Sq, d), dtype=torch.bfloat16, device=DEV)
            hip_ops.attention(qd, kd, vd, o, H, scale)
            o2 = torch.zeros_like(o)
            hip_ops.attention(qd, kd, vd, o2, H, scale)
            assert torch.equal(o, o2), "non-deterministic attention output (LDS-DMA ring race?)"
            assert_bf16_close(o, ref, f"attn7 short shape unit={unit} Sq={Sq} Skv={Skv}", abs_floor=2.0 ** -5, rms_bound=2.0 ** -7)
            base = rnd((Sq, d), 294).to(torch.bfloat16)
            o3 = base.clone().to(DEV)
            hip_ops.attention_add(qd, kd, vd, o3, H, scale)
            assert_bf16_close(o3, base.float() + ref, f"attn7 short shape add Sq={Sq} Skv={Skv}", abs_floor=2.0 ** -5, rms_bound=2.0 ** -6)
            if Skv >= 2:
                acc = torch.empty((Sq, d), device=DEV); ml = torch.empty((Sq, H, 2), device=DEV)
                o4 = torch.zeros_like(o)
                cut = max(1, Skv // 3)
                hip_ops.attention_chunk(qd, kd[:cut], vd[:cut], o4, acc, ml, H, scale, first=True, last=False)
                hip_ops.attention_chunk(qd, kd[cut:], vd[cut:], o4, acc, ml, H, scale, first=False, last=True)
                assert_bf16_close(o4, ref, f"attn7 short shape chunked Sq={Sq} Skv={Skv}", abs_floor=2.0 ** -5, rms_bound=2.0 ** -7)
    finally:
        hip_ops.lib.icv_set_option(b"attn7_short", -1)


@pytest.mark.experiments
@pytest.mark.parametrize("variant", [0, 4])
def test_attention9_variants(hip_ops, variant):
    """attn9.hip (QK^T of the next 32-key block in the same basic block as the softmax of the current one) at the
    generic scale: ragged sizes, spikes late in the sequence, scores that keep outgrowing the lazy reference, a row with
    hugely negative scores; run-to-run determinism (LDS-DMA ring 3 tiles ahead).  Unit scale / carried state / minimum
    sizes: the parametrised tests below."""
    need_experiments(hip_ops)
    H = 2
    d = H * 128
    hip_ops.lib.icv_set_option(b"attn_kernel", 9); hip_ops.lib.icv_set_option(b"attn9_variant", variant)
    try:
        for Sq, Skv in ((300, 1100), (64, 64), (257, 65), (33, 129), (513, 640), (1000, 3000), (1, 1), (40, 31), (256, 192), (70, 97)):
            q, k, v = (rnd((Sq, d), 291).to(torch.bfloat16), rnd((Skv, d), 292).to(torch.bfloat16), rnd((Skv, d), 293).to(torch.bfloat16))
            k[Skv - 1] = q[min(3, Sq - 1)] * 5.0
            k[Skv // 2] = q[min(40, Sq - 1)] * 5.0
            ref = R.attention(q.float(), k.float(), v.float(), H)
            outs = []
            for _ in range(3):
                o = torch.zeros((Sq, d), dtype=torch.bfloat16, device=DEV)
                hip_ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), o, H, 1.0 / math.sqrt(128))
                outs.append(o)
            assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), "non-deterministic attention output (LDS-DMA ring race?)"
            assert_bf16_close(outs[0], ref, f"attn9 variant {variant} Sq={Sq} Skv={Skv}", abs_floor=2.0 ** -5, rms_bound=2.0 ** -7)
        Sq, Skv = 130, 1500
        q = rnd((Sq, d), 274).to(torch.bfloat16)
        k = (rnd((Skv, d), 275) * torch.linspace(0.2, 6.0, Skv)[:, None]).to(torch.bfloat16)
        k[:, :128] += (q[5, :128].float() * torch.linspace(0.0, 3.0, Skv)[:, None]).to(torch.bfloat16)
        v = rnd((Skv, d), 276).to(torch.bfloat16)
        q[7] = -8.0 * k[:, :].float().mean(0).to(torch.bfloat16)
        ref = R.attention(q.float(), k.float(), v.float(), H)
        o = torch.zeros((Sq, d), dtype=torch.bfloat16, device=DEV)
        hip_ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), o, H, 1.0 / math.sqrt(128))
        assert torch.isfinite(o.float()).all()
        assert_bf16_close(o, ref, f"attn9 variant {variant} growing scores", abs_floor=2.0 ** -5, rms_bound=2.0 ** -7)
    finally:
        hip_ops.lib.icv_set_option(b"attn_kernel", ATTN_DEFAULT); hip_ops.lib.icv_set_option(b"attn9_variant", 0)


@pytest.mark.experiment_kernels
@pytest.mark.parametrize("kernel,unit", [(2, 1), (2, 0), (7, 1), (7, 0), (9, 1), (9, 0)])
def test_attention_unit_scale(hip_ops, kernel, unit):
    """scale * log2(e) == 1 (the DiT folds the softmax scale into K and calls with scale = ln 2): the kernel then
    starts the S accumulator at -m_ref and takes exp2(S) directly.  Same answers as the generic path (unit=0)."""
    if kernel in EXPERIMENT_KERNELS:
        need_experiments(hip_ops)
    H = 2
    d = H * 128
    ln2, fold = math.log(2.0), (1.0 / math.sqrt(128)) * math.log2(math.e)
    hip_ops.lib.icv_set_option(b"attn_unit_scale", unit); hip_ops.lib.icv_set_option(b"attn_kernel", kernel)
    try:
        for Sq, Skv, grow in ((300, 1100, False), (64, 64, False), (257, 65, False), (130, 1500, True), (1, 1, False), (513, 640, False)):
            q = rnd((Sq, d), 181).to(torch.bfloat16)
            kf = rnd((Skv, d), 182)
            if grow:     # scores that keep outgrowing the running reference + one row with hugely negative scores
                kf = kf * torch.linspace(0.2, 6.0, Skv)[:, None]
                kf[:, :128] += q[5, :128].float() * torch.linspace(0.0, 3.0, Skv)[:, None]
                q[7] = (-8.0 * kf.mean(0)).to(torch.bfloat16)
            else:
                kf[Skv - 1] = q[min(3, Sq - 1)].float() * 5.0
            k = (kf * fold).to(torch.bfloat16)          # K carries the scale, rounded once
            v = rnd((Skv, d), 183).to(torch.bfloat16)
            ref = R.attention(q.float(), k.float(), v.float(), H, scale=ln2)
            o = torch.zeros((Sq, d), dtype=torch.bfloat16, device=DEV)
            hip_ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), o, H, ln2)
            assert torch.isfinite(o.float()).all()
            assert_bf16_close(o, ref, f"unit-scale={unit} Sq={Sq} Skv={Skv}", abs_floor=2.0 ** -5, rms_bound=2.0 ** -7)
            # key-axis chunks with carried state (sequence-parallel path) take the same route
            if Skv >= 640:
                acc = torch.empty((Sq, d), device=DEV); ml = torch.empty((Sq, H, 2), device=DEV)
                o2 = torch.zeros_like(o)
                cuts = [0, 100, 357, Skv]
                for c in range(3):
                    hip_ops.attention_chunk(q.to(DEV), k[cuts[c]:cuts[c + 1]].to(DEV), v[cuts[c]:cuts[c + 1]].to(DEV), o2, acc, ml, H, ln2,
                                            first=(c == 0), last=(c == 2))
                assert_bf16_close(o2, ref, f"unit-scale={unit} chunked Sq={Sq} Skv={Skv}", abs_floor=2.0 ** -5, rms_bound=2.0 ** -7)
    finally:
        hip_ops.lib.icv_set_option(b"attn_unit_scale", 1); hip_ops.lib.icv_set_option(b"attn_kernel", ATTN_DEFAULT)


@pytest.mark.experiments
@pytest.mark.parametrize("variant", [0, 4])
def test_attention3_variants(hip_ops, variant):
    """attn3.hip (one wave per SIMD, 64 query rows per wave, shared K/V fragments)."""
    need_experiments(hip_ops)
    H = 2
    d = H * 128
    hip_ops.lib.icv_set_option(b"attn_kernel", 3)
    hip_ops.lib.icv_set_option(b"attn3_variant", variant)
    try:
        for Sq, Skv in ((300, 1100), (64, 64), (257, 65), (33, 129), (513, 640), (1000, 3000)):
            q, k, v = (rnd((Sq, d), 191).to(torch.bfloat16), rnd((Skv, d), 192).to(torch.bfloat16), rnd((Skv, d), 193).to(torch.bfloat16))
            k[Skv - 1] = q[3] * 5.0
            k[Skv // 2] = q[min(40, Sq - 1)] * 5.0
            ref = R.attention(q.float(), k.float(), v.float(), H)
            o = torch.zeros((Sq, d), dtype=torch.bfloat16, device=DEV)
            hip_ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), o, H, 1.0 / math.sqrt(128))
            o2 = torch.zeros_like(o)
            hip_ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), o2, H, 1.0 / math.sqrt(128))
            assert torch.equal(o, o2), "non-deterministic attention output (LDS staging race?)"
            assert_bf16_close(o, ref, f"attn3 variant {variant} Sq={Sq} Skv={Skv}", abs_floor=2.0 ** -5, rms_bound=2.0 ** -7)
    finally:
        hip_ops.lib.icv_set_option(b"attn_kernel", ATTN_DEFAULT)
        hip_ops.lib.icv_set_option(b"attn3_variant", 0)


@pytest.mark.experiments
@pytest.mark.parametrize("variant", [0, 1, 4, 5, 6, 7])
def test_attention4_variants(hip_ops, variant):
    """attn4.hip (LDS-DMA staged 4-stage ring, counted vmcnt, optional stagger)."""
    need_experiments(hip_ops)
    H = 2
    d = H * 128
    hip_ops.lib.icv_set_option(b"attn_kernel", 4)
    hip_ops.lib.icv_set_option(b"attn4_variant", variant)
    try:
        for Sq, Skv in ((300, 1100), (64, 64), (257, 65), (33, 129), (513, 640), (1000, 3000), (40, 1), (256, 128), (256, 192)):
            q, k, v = (rnd((Sq, d), 201).to(torch.bfloat16), rnd((Skv, d), 202).to(torch.bfloat16), rnd((Skv, d), 203).to(torch.bfloat16))
            k[Skv - 1] = q[3] * 5.0
            k[Skv // 2] = q[min(40, Sq - 1)] * 5.0
            ref = R.attention(q.float(), k.float(), v.float(), H)
            outs = []
            for _ in range(3):
                o = torch.zeros((Sq, d), dtype=torch.bfloat16, device=DEV)
                hip_ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), o, H, 1.0 / math.sqrt(128))
                outs.append(o)
            assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), "non-deterministic output (DMA ring race?)"
            assert_bf16_close(outs[0], ref, f"attn4 variant {variant} Sq={Sq} Skv={Skv}", abs_floor=2.0 ** -5, rms_bound=2.0 ** -7)
    finally:
        hip_ops.lib.icv_set_option(b"attn_kernel", ATTN_DEFAULT)
        hip_ops.lib.icv_set_option(b"attn4_variant", 4)


@pytest.mark.experiments
def test_attention5(hip_ops):
    """attn5.hip: one wave per SIMD, asm PV MFMAs with AGPR accumulators, asm LDS-DMA ring."""
    need_experiments(hip_ops)
    H = 2
    d = H * 128
    hip_ops.lib.icv_set_option(b"attn_kernel", 5)
    try:
        for Sq, Skv in ((300, 1100), (64, 64), (257, 65), (33, 129), (513, 640), (1000, 3000), (40, 1), (256, 128), (256, 192)):
            q, k, v = (rnd((Sq, d), 401).to(torch.bfloat16), rnd((Skv, d), 402).to(torch.bfloat16), rnd((Skv, d), 403).to(torch.bfloat16))
            k[Skv - 1] = q[3] * 5.0
            k[Skv // 2] = q[min(40, Sq - 1)] * 5.0
            ref = R.attention(q.float(), k.float(), v.float(), H)
            outs = []
            for _ in range(3):
                o = torch.zeros((Sq, d), dtype=torch.bfloat16, device=DEV)
                hip_ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), o, H, 1.0 / math.sqrt(128))
                outs.append(o)
            assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), "non-deterministic output (hazard / DMA race?)"
            assert_bf16_close(outs[0], ref, f"attn5 Sq={Sq} Skv={Skv}", abs_floor=2.0 ** -5, rms_bound=2.0 ** -7)
    finally:
        hip_ops.lib.icv_set_option(b"attn_kernel", ATTN_DEFAULT)


@pytest.mark.experiment_kernels
@pytest.mark.parametrize("kernel", [2, 3, 4, 5, 6, 7, 9])
@pytest.mark.parametrize("chunks", [[700], [128, 572], [300, 100, 300], [64, 64, 64, 508]])
def test_attention_chunked_state(hip_ops, chunks, kernel):
    """Splitting the KEY axis over several launches with carried (O, m, l) state must reproduce the
    single-launch result: this is the kernel path the sequence-parallel K/V pipeline uses.  Chunks are
    also fed in a permuted order (key order is irrelevant to attention)."""
    if kernel in EXPERIMENT_KERNELS:
        need_experiments(hip_ops)
    Sq, H = 333, 3
    d = H * 128
    Skv = sum(chunks)
    q, k, v = (rnd((Sq, d), 181).to(torch.bfloat16).to(DEV), rnd((Skv, d), 182).to(torch.bfloat16).to(DEV),
               rnd((Skv, d), 183).to(torch.bfloat16).to(DEV))
    ref = R.attention(q.float().cpu(), k.float().cpu(), v.float().cpu(), H)
    acc = torch.empty((Sq, d), device=DEV)
    ml = torch.empty((Sq, H, 2), device=DEV)
    o = torch.zeros((Sq, d), dtype=torch.bfloat16, device=DEV)
    bounds = [0]
    for c in chunks:
        bounds.append(bounds[-1] + c)
    order = list(range(len(chunks)))[::-1]     # reversed chunk order
    hip_ops.lib.icv_set_option(b"attn_kernel", kernel)
    try:
        for j, ci in enumerate(order):
            lo, hi = bounds[ci], bounds[ci + 1]
            hip_ops.attention_chunk(q, k[lo:hi], v[lo:hi], o, acc, ml, H, 1.0 / math.sqrt(128),
                                    first=(j == 0), last=(j == len(order) - 1))
        torch.cuda.synchronize()
    finally:
        hip_ops.lib.icv_set_option(b"attn_kernel", ATTN_DEFAULT)
    assert_bf16_close(o, ref, f"chunked attention {chunks}", abs_floor=2.0 ** -5, rms_bound=2.0 ** -7)


def test_attention_strided_planes_and_spike(hip_ops):
    """q/k/v as planes of one [3, n, d] buffer (the fused-QKV layout) and a key that forces the
    online-softmax rescale late in the sequence (running max jumps at the last tile)."""
    n, H = 700, 2
    d = H * 128
    planes = rnd((3, n, d), 71).to(torch.bfloat16)
    planes[1, 650] = planes[0, 5] * 6.0   # key 650 ~ 6x query 5: a huge score in the last tile
    planes[1, 3] = planes[0, 400] * 4.0   # and an early spike for another query
    ref = R.attention(planes[0].float(), planes[1].float(), planes[2].float(), H)
    g = planes.to(DEV)
    o = torch.zeros((n, d), dtype=torch.bfloat16, device=DEV)
    hip_ops.attention(g[0], g[1], g[2], o, H, 1.0 / math.sqrt(128))
    assert_bf16_close(o, ref, "attention planes+spike", abs_floor=2.0 ** -5, rms_bound=2.0 ** -7)


def test_attention_permutation_invariance(hip_ops):
    """Size-independent property at a larger size: permuting the keys/values together must not
    change the output beyond rounding (checks tail masking + tile order independence)."""
    Sq, Skv, H = 1024, 4000, 4
    d = H * 128
    q, k, v = (rnd((Sq, d), 81).to(torch.bfloat16).to(DEV), rnd((Skv, d), 82).to(torch.bfloat16).to(DEV),
               rnd((Skv, d), 83).to(torch.bfloat16).to(DEV))
    perm = torch.randperm(Skv, generator=torch.Generator().manual_seed(5)).to(DEV)
    o1 = torch.empty((Sq, d), dtype=torch.bfloat16, device=DEV)
    o2 = torch.empty_like(o1)
    hip_ops.attention(q, k, v, o1, H, 1.0 / math.sqrt(128))
    hip_ops.attention(q, k[perm].contiguous(), v[perm].contiguous(), o2, H, 1.0 / math.sqrt(128))
    assert (o1.float() - o2.float()).abs().max() < 2e-2 * o1.float().abs().max()


def test_patchify_and_unpatchify_euler(hip_ops):
    C, T, H8, W8 = 16, 3, 8, 12
    Hp, Wp = H8 // 2, W8 // 2
    S = T * Hp * Wp
    lat = rnd((C, T, H8, W8), 91)
    tok0, n = 5, 40
    out = torch.zeros((n, 64), dtype=torch.bfloat16, device=DEV)
    hip_ops.patchify(lat.to(DEV), out, tok0, n)
    ref = lat.reshape(C, T, Hp, 2, Wp, 2).permute(1, 2, 4, 0, 3, 5).reshape(S, C * 4)[tok0: tok0 + n]
    assert torch.equal(out.cpu(), ref.to(torch.bfloat16))
    # conv-as-GEMM equivalence against F.conv3d
    w = rnd((32, C, 1, 2, 2), 92, 0.1)
    conv = R.patchify_tokens(lat.to(torch.bfloat16).float(), w.to(torch.bfloat16).float(), None)[tok0: tok0 + n]
    assert torch.allclose(out.cpu().float() @ w.to(torch.bfloat16).float().reshape(32, -1).t(), conv, atol=1e-4)
    # fused unpatchify + CFG + Euler on a shard
    hc, hu = rnd((n, 64), 93), rnd((n, 64), 94)
    full_c, full_u = torch.zeros((S, 64)), torch.zeros((S, 64))
    full_c[tok0: tok0 + n], full_u[tok0: tok0 + n] = hc, hu
    vel = R.unpatchify(full_u + 5.0 * (full_c - full_u), (T, Hp, Wp), C)
    lat_g = lat.clone().to(DEV)
    vel_g = torch.zeros_like(lat_g)
    hip_ops.unpatchify_cfg_euler(lat_g, hc.to(DEV), hu.to(DEV), 5.0, -0.125, tok0, n, vel_out=vel_g)
    assert torch.allclose(vel_g.cpu(), vel, atol=1e-5)
    assert torch.allclose(lat_g.cpu(), lat + vel * (-0.125), atol=1e-5)
    lat_g2 = lat.clone().to(DEV)
    hip_ops.unpatchify_cfg_euler(lat_g2, hc.to(DEV), None, 1.0, 0.5, tok0, n)
    assert torch.allclose(lat_g2.cpu(), lat + R.unpatchify(full_c, (T, Hp, Wp), C) * 0.5, atol=1e-5)


def test_unpatchify_cfg_euler_reference_rounding(hip_ops):
    """round_bf16 = 1: every intermediate of the CFG combine and the Euler update rounded through bf16, bit for bit
    equal to the host restatement (tests/oracle_ops.py), and different from the exact path."""
    from oracle_ops import OracleOps
    C, T, H8, W8 = 16, 3, 8, 12
    tok0, n = 5, 40
    lat = rnd((C, T, H8, W8), 95, 2.0)
    hc, hu = rnd((n, 64), 96), rnd((n, 64), 97)
    for with_u in (True, False):
        want = lat.clone()
        OracleOps().unpatchify_cfg_euler(want, hc, hu if with_u else None, 5.0, -0.0371, tok0, n, round_bf16=True)
        got = lat.clone().to(DEV)
        hip_ops.unpatchify_cfg_euler(got, hc.to(DEV), hu.to(DEV) if with_u else None, 5.0, -0.0371, tok0, n, round_bf16=True)
        assert torch.equal(got.cpu(), want), "reference-rounding Euler update differs from the host restatement"
        exact = lat.clone().to(DEV)
        hip_ops.unpatchify_cfg_euler(exact, hc.to(DEV), hu.to(DEV) if with_u else None, 5.0, -0.0371, tok0, n)
        assert not torch.equal(exact.cpu(), want)


def test_error_reporting(hip_ops):
    from infinicube_amd import native
    a = torch.zeros((8, 100), dtype=torch.bfloat16, device=DEV)   # K = 100 not a multiple of 64
    w = torch.zeros((8, 100), dtype=torch.bfloat16, device=DEV)
    with pytest.raises(native.NativeError, match="multiple of 64"):
        hip_ops.gemm(a, w, None, torch.empty((8, 8), dtype=torch.bfloat16, device=DEV), EPI_BF16)


# ---------------------------------------------------------------------------------------------------
# edge cases: minimum / ragged sizes through every kernel family (tails, clamps, masks)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.experiments
@pytest.mark.parametrize("variant", [0, 1, 4, 5])
def test_attention6_pingpong(hip_ops, variant):
    """attn6.hip (PV pipelined one tile behind QK^T, wave groups one phase apart): parity incl. ragged tails."""
    need_experiments(hip_ops)
    hip_ops.lib.icv_set_option(b"attn_kernel", 6); hip_ops.lib.icv_set_option(b"attn6_variant", variant)
    try:
        for Sq, Skv, H in ((300, 1000, 2), (257, 64, 1), (64, 65, 1), (512, 129, 3), (1, 1, 1), (2240, 2240, 2)):
            d = H * 128
            q, k, v = (rnd((Sq, d), 501).to(torch.bfloat16), rnd((Skv, d), 502).to(torch.bfloat16), rnd((Skv, d), 503).to(torch.bfloat16))
            ref = R.attention(q.float(), k.float(), v.float(), H)
            o = torch.empty((Sq, d), dtype=torch.bfloat16, device=DEV)
            o2 = torch.empty_like(o)
            hip_ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), o, H, 1.0 / math.sqrt(128))
            hip_ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), o2, H, 1.0 / math.sqrt(128))
            assert_bf16_close(o, ref, f"attn6 v{variant} Sq={Sq} Skv={Skv}", abs_floor=2.0 ** -5, rms_bound=2.0 ** -7)
            assert torch.equal(o, o2), "attn6 is not deterministic"
    finally:
        hip_ops.lib.icv_set_option(b"attn_kernel", ATTN_DEFAULT); hip_ops.lib.icv_set_option(b"attn6_variant", 5)


@pytest.mark.experiment_kernels
@pytest.mark.parametrize("kernel", [1, 2, 3, 4, 5, 6, 7, 9])
def test_attention_minimum_sizes(hip_ops, kernel):
    if kernel in EXPERIMENT_KERNELS:
        need_experiments(hip_ops)
    hip_ops.lib.icv_set_option(b"attn_kernel", kernel)
    try:
        for Sq, Skv, H in ((1, 1, 1), (1, 513, 2), (257, 1, 1), (31, 63, 3), (32, 64, 1), (255, 127, 2)):
            d = H * 128
            q, k, v = (rnd((Sq, d), 301).to(torch.bfloat16), rnd((Skv, d), 302).to(torch.bfloat16), rnd((Skv, d), 303).to(torch.bfloat16))
            ref = R.attention(q.float(), k.float(), v.float(), H)
            o = torch.full((Sq + 2, d), 9.0, dtype=torch.bfloat16, device=DEV)      # guard rows after the output
            hip_ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), o[:Sq], H, 1.0 / math.sqrt(128))
            assert_bf16_close(o[:Sq], ref, f"attention kernel {kernel} Sq={Sq} Skv={Skv}", abs_floor=2.0 ** -5, rms_bound=2.0 ** -7)
            assert bool((o[Sq:] == 9.0).all()), "wrote past the last query row"
    finally:
        hip_ops.lib.icv_set_option(b"attn_kernel", ATTN_DEFAULT)


# ---------------------------------------------------------------------------------------------------
# fp8 path (BASELINE.json config #5): row-scaled e4m3 quantisation and the K=128 fp8 MFMA GEMM
# ---------------------------------------------------------------------------------------------------
FP8 = torch.float8_e4m3fn


@pytest.mark.parametrize("rows,K,src", [(5, 128, "bf16"), (257, 1536, "bf16"), (64, 13824, "bf16"), (33, 5120, "f32"), (1, 8, "f32")])
def test_quantize_rows_fp8_bit_exact(hip_ops, rows, K, src):
    x = rnd((rows, K), 401, 3.0)
    x[:, ::7] *= 40.0                      # outlier channels
    x[rows // 2] = 0.0                     # an all-zero row -> scale 1, zeros
    if rows > 2:
        x[1] *= 1e-6                       # tiny row: the scale keeps it in range
    xs = x.to(torch.bfloat16) if src == "bf16" else x
    q = torch.zeros((rows + 1, K), dtype=torch.uint8, device=DEV).view(FP8)
    sc = torch.full((rows + 1,), 7.0, device=DEV)
    hip_ops.quantize_rows(xs.to(DEV), q[:rows], sc[:rows])
    qr, sr = R.quantize_rows_fp8(xs.float())
    assert torch.equal(sc[:rows].cpu(), sr), "row scales differ"
    got = q[:rows].cpu().float()
    nbad = int((got != qr).sum())
    assert nbad == 0, f"{nbad} / {got.numel()} e4m3 codes differ from the oracle (max |d| {float((got - qr).abs().max())})"
    assert float(sc[rows]) == 7.0 and bool((q[rows].view(torch.uint8) == 0).all()), "wrote past the last row"


@pytest.mark.parametrize("rows,d,mode", [(37, 1536, "mod"), (300, 5120, "mod"), (9, 256, "affine"), (130, 2048, "plain")])
def test_ln_modulate_fp8(hip_ops, rows, d, mode):
    x = rnd((rows, d), 411, 2.0) + 0.3
    x[:, 5] += 30.0
    kw = {}
    if mode == "mod":
        kw = dict(shift=rnd((d,), 412, 0.2), scale=rnd((d,), 413, 0.2))
    elif mode == "affine":
        kw = dict(weight=1.0 + rnd((d,), 414, 0.1), bias=rnd((d,), 415, 0.1))
    y = R.layer_norm(x, kw.get("weight"), kw.get("bias"), 1e-6)
    if "scale" in kw:
        y = y * (1.0 + kw["scale"]) + kw["shift"]
    q = torch.zeros((rows, d), dtype=torch.uint8, device=DEV).view(FP8)
    sc = torch.zeros((rows,), device=DEV)
    hip_ops.ln_modulate_fp8(x.to(DEV), q, sc, eps=1e-6, **{k: v.to(DEV) for k, v in kw.items()})
    assert_ln_fp8_close(q, sc, y, f"ln_modulate_fp8 {mode}")


def assert_ln_fp8_close(q, sc, y, what=""):
    """q: e4m3 rows (or their values as f32), sc: f32 row scales, y: the unquantised LayerNorm (+ modulate) rows they should encode."""
    q, sc, y = q.float().cpu(), sc.float().cpu(), y.cpu()
    qr, sr = R.quantize_rows_fp8(y)
    assert torch.allclose(sc, sr, rtol=1e-5, atol=0), f"{what}: row scales differ beyond f32 LN rounding"
    deq, ref = q * sc[:, None], qr * sr[:, None]
    # f32 LayerNorm rounding can flip an e4m3 rounding decision for values on a tie: allow one code step on <0.5 %
    step = (deq - ref).abs() / ref.abs().clamp_min(1e-20)
    share, worst = float((step > 1e-6).float().mean()), float(step.max())
    assert share < 5e-3 and worst <= 0.126, f"{what}: e4m3 codes differ on {share:.3%} of the elements, largest step {worst:.4g}"
    # and the quantisation itself: e4m3 keeps 2^-4 relative precision down to 2^-9 of the row maximum's scale
    tol = (2.0 ** -4) * y.abs() + (2.0 ** -10) * sr[:, None] * 448.0 / 256.0
    assert bool(((deq - y).abs() <= tol).all()), f"{what}: dequantised row off by more than e4m3 rounding"


@pytest.mark.parametrize("M,N,K,epi", [
    (256, 256, 128, "f32"), (300, 260, 256, "f32"), (1, 4, 128, "f32"), (513, 1536, 1536, "bf16"),
    (777, 1024, 512, "gelu"), (640, 512, 8960, "resid"), (515, 768, 384, "split")])
@pytest.mark.parametrize("sched", [3, 0])
def test_gemm_fp8(hip_ops, M, N, K, epi, sched):
    """sched 3 = two-phase main loop + batched residual epilogue (default), 0 = round 1's four-phase loop (A/B switch)."""
    hip_ops.lib.icv_set_option(b"gemm_fp8_sched", sched)
    try:
        _gemm_fp8_case(hip_ops, M, N, K, epi)
    finally:
        hip_ops.lib.icv_set_option(b"gemm_fp8_sched", 3)


def _gemm_fp8_case(hip_ops, M, N, K, epi):
    a = rnd((M, K), 421, 1.5)
    a[:, 3] *= 25.0
    w = rnd((N, K), 422, 1.0 / math.sqrt(K))
    bias = rnd((N,), 423, 0.1)
    aq, asc = R.quantize_rows_fp8(a)
    wq, wsc = R.quantize_rows_fp8(w)
    acc = (aq.double() @ wq.double().t()).float() * asc[:, None] * wsc[None, :] + bias
    A8, W8 = aq.to(FP8).to(DEV), wq.to(FP8).to(DEV)
    args = (A8, asc.to(DEV), W8, wsc.to(DEV), bias.to(DEV))
    if epi == "f32":
        out = torch.full((M + 1, N), 5.0, device=DEV)
        hip_ops.gemm_fp8(*args, out[:M], EPI_F32)
        assert_f32_close(out[:M], acc, rtol=1e-4, what=f"gemm_fp8 {M}x{N}x{K}")
        assert bool((out[M:] == 5.0).all()), "wrote past the last row"
    elif epi == "bf16":
        out = torch.empty((M, N), dtype=torch.bfloat16, device=DEV)
        hip_ops.gemm_fp8(*args, out, EPI_BF16)
        assert_bf16_close(out, acc, "gemm_fp8 bf16")
    elif epi == "gelu":
        out = torch.empty((M, N), dtype=torch.bfloat16, device=DEV)
        hip_ops.gemm_fp8(*args, out, EPI_GELU_BF16)
        assert_bf16_close(out, torch.nn.functional.gelu(acc, approximate="tanh"), "gemm_fp8 gelu", abs_floor=2.0 ** -8)
    elif epi == "resid":
        resid, gate = rnd((M, N), 424), rnd((N,), 425)
        out = resid.clone().to(DEV)
        hip_ops.gemm_fp8(*args, out, EPI_RESID_F32, resid=out, gate=gate.to(DEV))
        assert_f32_close(out, resid + gate * acc, rtol=1e-4, what="gemm_fp8 resid")
    else:
        ns = N // 3
        out = torch.empty((3, M, ns), dtype=torch.bfloat16, device=DEV)
        hip_ops.gemm_fp8(*args, out, EPI_BF16, nsplit=ns)
        assert_bf16_close(out, acc.reshape(M, 3, ns).permute(1, 0, 2), "gemm_fp8 split planes")


def test_gemm_fp8_rejects_bad_shapes(hip_ops):
    from infinicube_amd.native import NativeError
    a = torch.zeros((8, 192), dtype=torch.uint8, device=DEV).view(FP8)
    w = torch.zeros((8, 192), dtype=torch.uint8, device=DEV).view(FP8)
    s = torch.ones((8,), device=DEV)
    with pytest.raises(NativeError, match="multiple of 128"):
        hip_ops.gemm_fp8(a, s, w, s, None, torch.empty((8, 8), device=DEV), EPI_F32)


@pytest.mark.parametrize("Sq,Skv,H", [(300, 1100, 2), (64, 64, 1), (257, 65, 1), (130, 1500, 2), (1, 1, 1), (513, 640, 3)])
def test_attention_fp8(hip_ops, Sq, Skv, H):
    """fp8 attention (prepare: per-head power-of-two scales, transposed key-permuted V tiles; forward on the K=64 scaled
    MFMA).  Bar: against the oracle that applies the same e4m3 quantisation, rms error <= 3 % of the output rms (P is
    rounded against a lazy reference in the kernel and against the true max in the oracle); against the unquantised
    attention the fp8 noise itself stays below 8 % (short key sequences average it least)."""
    d = H * 128
    fold = (1.0 / math.sqrt(128)) * math.log2(math.e)
    q = rnd((Sq, d), 441).to(torch.bfloat16)
    kf = rnd((Skv, d), 442)
    kf[Skv - 1] = q[min(3, Sq - 1)].float() * 3.0                     # one strongly matching key late in the sequence
    k = (kf * fold).to(torch.bfloat16)
    v = (rnd((Skv, d), 443) * torch.linspace(0.5, 2.0, d)[None, :]).to(torch.bfloat16)
    ref8 = R.attention_fp8(q.float(), k.float(), v.float(), H)
    ref = R.attention(q.float(), k.float(), v.float(), H, scale=math.log(2.0))
    o = torch.full((Sq + 2, d), 9.0, dtype=torch.bfloat16, device=DEV)
    ws = hip_ops.attention_fp8_buffers(Sq, Skv, d, H)
    hip_ops.attention_fp8(q.to(DEV), k.to(DEV), v.to(DEV), o[:Sq], H, ws)
    o2 = torch.empty((Sq, d), dtype=torch.bfloat16, device=DEV)
    hip_ops.attention_fp8(q.to(DEV), k.to(DEV), v.to(DEV), o2, H, ws)
    got = o[:Sq].float().cpu()
    assert torch.isfinite(got).all() and torch.equal(o[:Sq], o2), "fp8 attention not finite / not deterministic"
    assert bool((o[Sq:] == 9.0).all()), "wrote past the last query row"
    # prepare: scales and e4m3 codes of K are exactly the oracle's
    amax = ws[3].cpu()
    assert torch.equal(amax[1], k.float().abs().reshape(Skv, H, 128).amax(dim=(0, 2)))
    e = torch.ceil(torch.log2(amax[1] / 448.0))
    kq_ref = (k.float().reshape(Skv, H, 128) * torch.exp2(-e)[None, :, None]).to(torch.float8_e4m3fn).reshape(Skv, d)
    assert torch.equal(ws[1].cpu().view(torch.uint8), kq_ref.view(torch.uint8)), "K e4m3 codes differ from the oracle"
    rms = float(ref.pow(2).mean().sqrt())
    e8 = float((got - ref8).pow(2).mean().sqrt()) / rms
    e0 = float((got - ref).pow(2).mean().sqrt()) / rms
    assert e8 <= 0.03 and e0 <= 0.08, f"fp8 attention Sq={Sq} Skv={Skv}: rms err vs fp8 oracle {e8:.4f}, vs unquantised {e0:.4f}"
    # key-axis chunks with carried state (sequence-parallel path): queries prepared once, every chunk prepared on its own
    if Skv >= 640:
        acc = torch.empty((Sq, d), device=DEV); ml = torch.empty((Sq, H, 2), device=DEV)
        o3 = torch.zeros((Sq, d), dtype=torch.bfloat16, device=DEV)
        cuts = [0, 100, 357, Skv]
        hip_ops.attention_fp8_prepare(ws, H, q=q.to(DEV))
        for c in range(3):
            kc, vc = k[cuts[c]:cuts[c + 1]].to(DEV), v[cuts[c]:cuts[c + 1]].to(DEV)
            hip_ops.attention_fp8_prepare(ws, H, k=kc, v=vc)
            hip_ops.attention_fp8_chunk(ws, Sq, kc.shape[0], o3, acc, ml, H, first=(c == 0), last=(c == 2))
        e3 = float((o3.float().cpu() - ref).pow(2).mean().sqrt()) / rms
        assert e3 <= 0.08, f"chunked fp8 attention vs unquantised: {e3:.4f}"


@pytest.mark.parametrize("Sq,m,W,H", [(300, 128, 3, 2), (130, 100, 4, 2), (257, 37, 2, 1), (64, 585, 8, 1)])
def test_attention_fp8_pieces_e4m3_on_the_wire(hip_ops, Sq, m, W, H):
    """The e4m3 wire format of the sequence-parallel fp8 mode (icv_attention_fp8_kv_amax / _quantize_kv / _fwd_pieces): W ranks'
    pieces of m keys each, every piece quantised on its own from its own rows with the GLOBAL per-head scales, consumed in place.
    (a) the e4m3 K codes inside every blob are exactly the oracle's; (b) with m a multiple of 64 the tiles of the piece-wise launch
    are the tiles of the unsharded launch in the same order, so the output is BIT-IDENTICAL to icv_attention_fp8_fwd on the
    concatenated rows; (c) ragged pieces (padding keys masked) meet the fp8 bars against the oracle; (d) two chunks of pieces
    with carried state agree with one."""
    d, Skv = H * 128, m * W
    fold = (1.0 / math.sqrt(128)) * math.log2(math.e)
    q = rnd((Sq, d), 541).to(torch.bfloat16)
    kf = rnd((Skv, d), 542)
    kf[Skv - 1] = q[min(3, Sq - 1)].float() * 3.0
    k = (kf * fold).to(torch.bfloat16)
    v = (rnd((Skv, d), 543) * torch.linspace(0.5, 2.0, d)[None, :]).to(torch.bfloat16)
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    ws = hip_ops.attention_fp8_buffers(Sq, Skv, d, H)
    o_ref = torch.empty((Sq, d), dtype=torch.bfloat16, device=DEV)
    hip_ops.attention_fp8(qd, kd, vd, o_ref, H, ws)                       # unsharded launch: also leaves the global abs-max in ws[3]
    amax = torch.zeros((3, H), device=DEV)
    hip_ops.attention_fp8_kv_amax(kd, vd, H, amax)
    assert torch.equal(amax[1:], ws[3][1:]), "per-head abs-max of K / V differs from the prepare pass"
    bb = hip_ops.attention_fp8_blob_bytes(m, H)
    mp = (m + 63) // 64 * 64
    assert bb == 2 * mp * d
    blobs = torch.full((W * bb + 64,), 0xAB, dtype=torch.uint8, device=DEV)
    for i in range(W):                                                     # "rank i" quantises its own rows
        hip_ops.attention_fp8_quantize_kv(kd[i * m:(i + 1) * m], vd[i * m:(i + 1) * m], H, amax, blobs[i * bb:(i + 1) * bb])
    assert bool((blobs[W * bb:] == 0xAB).all()), "wrote past the last blob"
    e = torch.ceil(torch.log2(amax[1].cpu() / 448.0))
    kq_ref = (k.float().reshape(Skv, H, 128) * torch.exp2(-e)[None, :, None]).to(torch.float8_e4m3fn).reshape(Skv, d).view(torch.uint8)
    for i in range(W):
        got_codes = blobs[i * bb: i * bb + m * d].cpu().reshape(m, d)
        assert torch.equal(got_codes, kq_ref[i * m:(i + 1) * m]), f"piece {i}: K e4m3 codes differ from the oracle"
    ws2 = hip_ops.attention_fp8_with_amax(ws, amax)
    hip_ops.attention_fp8_prepare(ws2, H, q=qd)
    o = torch.full((Sq + 2, d), 9.0, dtype=torch.bfloat16, device=DEV)
    hip_ops.attention_fp8_pieces(ws2, amax, blobs[: W * bb], m, W, Sq, o[:Sq], None, None, H, first=True, last=True)
    assert bool((o[Sq:] == 9.0).all()), "wrote past the last query row"
    got = o[:Sq].float().cpu()
    assert torch.isfinite(got).all()
    if m % 64 == 0:
        assert torch.equal(o[:Sq], o_ref), "tile-aligned pieces must reproduce the unsharded launch bit for bit"
    ref8 = R.attention_fp8(q.float(), k.float(), v.float(), H)
    ref = R.attention(q.float(), k.float(), v.float(), H, scale=math.log(2.0))
    rms = float(ref.pow(2).mean().sqrt())
    e8 = float((got - ref8).pow(2).mean().sqrt()) / rms
    e0 = float((got - ref).pow(2).mean().sqrt()) / rms
    assert e8 <= 0.03 and e0 <= 0.08, f"fp8 pieces Sq={Sq} m={m} W={W}: rms err vs fp8 oracle {e8:.4f}, vs unquantised {e0:.4f}"
    if W >= 2:      # two chunks of pieces (the first W-1 pieces, then the last one) with carried state
        acc = torch.empty((Sq, d), device=DEV); ml = torch.empty((Sq, H, 2), device=DEV)
        o3 = torch.zeros((Sq, d), dtype=torch.bfloat16, device=DEV)
        hip_ops.attention_fp8_pieces(ws2, amax, blobs[: (W - 1) * bb], m, W - 1, Sq, None, acc, ml, H, first=True, last=False)
        hip_ops.attention_fp8_pieces(ws2, amax, blobs[(W - 1) * bb: W * bb], m, 1, Sq, o3, acc, ml, H, first=False, last=True)
        e3 = float((o3.float().cpu() - got).pow(2).mean().sqrt()) / rms
        assert e3 <= 0.02, f"two chunks of pieces vs one: {e3:.4f}"


@pytest.mark.parametrize("Sq,m,W,H,own", [(300, 128, 4, 2, 1), (130, 100, 3, 2, 0), (520, 585, 8, 1, 5)])
def test_attention_fp8_pieces_gated_by_arrival_flags(hip_ops, Sq, m, W, H, own):
    """icv_attention_fp8_fwd_pieces_gated (round 6: the arrival-driven schedule for the e4m3 wire format).  (a) identity order, no flag,
    no separate own blob = the ungated launch bit for bit; (b) this rank's blob read from its own tensor (its slot in the gathered chunk
    holds NaN bytes) and the peers walked in pull order: the fp8 bars against the oracle; (c) two peers' blobs are NaN bytes when the
    launch starts and a side stream delivers them - copy, then flag - one at once, one 2 ms later: bit-identical to (b), nobody timed
    out; (d) a flag that never comes: the launch returns after the time-out with the position in the error word."""
    d, Skv = H * 128, m * W
    fold = (1.0 / math.sqrt(128)) * math.log2(math.e)
    q = rnd((Sq, d), 641).to(torch.bfloat16)
    kf = rnd((Skv, d), 642)
    kf[Skv - 1] = q[min(3, Sq - 1)].float() * 3.0
    k = (kf * fold).to(torch.bfloat16)
    v = (rnd((Skv, d), 643) * torch.linspace(0.5, 2.0, d)[None, :]).to(torch.bfloat16)
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    ws = hip_ops.attention_fp8_buffers(Sq, Skv, d, H)
    amax = torch.zeros((3, H), device=DEV)
    hip_ops.attention_fp8_kv_amax(kd, vd, H, amax)
    bb = hip_ops.attention_fp8_blob_bytes(m, H)
    blobs = torch.empty((W * bb,), dtype=torch.uint8, device=DEV)
    for i in range(W):
        hip_ops.attention_fp8_quantize_kv(kd[i * m:(i + 1) * m], vd[i * m:(i + 1) * m], H, amax, blobs[i * bb:(i + 1) * bb])
    ws2 = hip_ops.attention_fp8_with_amax(ws, amax)
    hip_ops.attention_fp8_prepare(ws2, H, q=qd)

    def launch(bl, gate):
        o = torch.zeros((Sq, d), dtype=torch.bfloat16, device=DEV)
        hip_ops.attention_fp8_pieces(ws2, amax, bl, m, W, Sq, o, None, None, H, first=True, last=True, gate=gate)
        return o

    o_plain = launch(blobs, None)
    o_a = launch(blobs, dict(seq=[(i, -1, 0) for i in range(W)]))
    assert torch.equal(o_a, o_plain), "(a) identity order without flags differs from the ungated launch"
    # (b) own blob elsewhere, pull order
    own_blob = blobs[own * bb:(own + 1) * bb].clone()
    staged = blobs.clone()
    poisoned = blobs.clone()
    poisoned[own * bb:(own + 1) * bb] = 0x7F                      # e4m3 NaN: reading the slot would show
    order = [own] + [(own + j) % W for j in range(1, W)]
    o_b = launch(poisoned, dict(seq=[(i, -1, 0) for i in order], own=(own_blob, own)))
    got = o_b.float().cpu()
    assert torch.isfinite(got).all(), "(b) the own piece was read from its slot in the gathered chunk"
    ref8 = R.attention_fp8(q.float(), k.float(), v.float(), H)
    ref = R.attention(q.float(), k.float(), v.float(), H, scale=math.log(2.0))
    rms = float(ref.pow(2).mean().sqrt())
    e8 = float((got - ref8).pow(2).mean().sqrt()) / rms
    e0 = float((got - ref).pow(2).mean().sqrt()) / rms
    assert e8 <= 0.03 and e0 <= 0.08, f"(b) gated fp8 pieces Sq={Sq} m={m} W={W}: rms err vs fp8 oracle {e8:.4f}, vs unquantised {e0:.4f}"
    if W >= 3:
        # (c) late peers
        early, late = order[1], order[2]
        flags = torch.zeros((8,), dtype=torch.int32, device=DEV)
        err = torch.zeros((1,), dtype=torch.int32, device=DEV)
        mark = torch.zeros((2,), dtype=torch.int32, device=DEV)
        side = torch.cuda.Stream(device=DEV, priority=-1)       # its own hardware-queue class: a default-class stream can share the launch's queue and never run (profiles/r06/stream_queue_share_probe.txt)
        for value in (3, 4):                                     # twice: the first pass pays the side stream's first-use costs
            for i in (early, late):
                poisoned[i * bb:(i + 1) * bb] = 0x7F
            torch.cuda.synchronize()
            seq = [(i, {early: 1, late: 2}.get(i, -1), value if i in (early, late) else 0) for i in order]
            o_c = torch.zeros((Sq, d), dtype=torch.bfloat16, device=DEV)
            hip_ops.attention_fp8_pieces(ws2, amax, poisoned, m, W, Sq, o_c, None, None, H, first=True, last=True,
                                         gate=dict(seq=seq, flags=flags, own=(own_blob, own), err=err, timeout_us=5_000_000))
            with torch.cuda.stream(side):
                poisoned[early * bb:(early + 1) * bb].copy_(staged[early * bb:(early + 1) * bb])
                hip_ops.flag_write(flags, 1, value)
                hip_ops.flag_write(mark, 0, 1, delay_us=2000)      # hold the stream: the late peer
                poisoned[late * bb:(late + 1) * bb].copy_(staged[late * bb:(late + 1) * bb])
                hip_ops.flag_write(flags, 2, value)
            torch.cuda.synchronize()
        assert int(err.item()) == 0, f"(c) a wave gave up waiting: err word {int(err.item()) & 0xffffffff:#x}"
        assert torch.isfinite(o_c.float()).all(), "(c) a blob was read before it landed"
        assert torch.equal(o_c, o_b), "(c) late blobs: result differs from the all-present launch in the same order"
        # (d) a flag that never comes
        import time
        err.zero_()
        seq = [(i, 5 if i == late else -1, 9 if i == late else 0) for i in order]
        torch.cuda.synchronize()
        t0 = time.time()
        hip_ops.attention_fp8_pieces(ws2, amax, poisoned, m, W, Sq, o_c, None, None, H, first=True, last=True,
                                     gate=dict(seq=seq, flags=flags, own=(own_blob, own), err=err, timeout_us=50_000))
        torch.cuda.synchronize()
        dt = time.time() - t0
        assert (int(err.item()) & 0xffffffff) == (0x80000000 | order.index(late)), f"(d) error word {int(err.item()) & 0xffffffff:#x}"
        assert dt < 2.0, f"(d) the bounded wait took {dt:.2f} s"


@pytest.mark.parametrize("Sq,Skv,H", [(300, 257, 2), (1, 1, 1), (513, 64, 3)])
def test_attention_add_into_output(hip_ops, Sq, Skv, H):
    """icv_attention_fwd_add: o += softmax(q k^T) v (the i2v image cross-attention; 257 = CLIP tokens)."""
    d = H * 128
    q, k, v = (rnd((Sq, d), 331).to(torch.bfloat16), rnd((Skv, d), 332).to(torch.bfloat16), rnd((Skv, d), 333).to(torch.bfloat16))
    prev = rnd((Sq, d), 334).to(torch.bfloat16)
    ref = prev.float() + R.attention(q.float(), k.float(), v.float(), H)
    o = torch.full((Sq + 2, d), 9.0, dtype=torch.bfloat16, device=DEV)
    o[:Sq] = prev.to(DEV)
    hip_ops.attention_add(q.to(DEV), k.to(DEV), v.to(DEV), o[:Sq], H, 1.0 / math.sqrt(128))
    assert_bf16_close(o[:Sq], ref, f"attention_add Sq={Sq} Skv={Skv}", abs_floor=2.0 ** -5, rms_bound=2.0 ** -7)
    assert bool((o[Sq:] == 9.0).all()), "wrote past the last query row"


GEMM_VARIANT_CASES = [(256, 256, 64, "f32"), (300, 512, 192, "f32"), (1000, 768, 1536, "bf16"), (513, 1024, 512, "gelu"),
                      (640, 512, 1280, "resid"), (515, 768, 384, "split")]


@pytest.mark.parametrize("M,N,K,epi", GEMM_VARIANT_CASES)
@pytest.mark.experiments
@pytest.mark.parametrize("kernel", [3, 4])
def test_gemm_4wave_variant(hip_ops, M, N, K, epi, kernel):
    """gemm256w.hip (option gemm256 = 3): 4 waves x 128x128 wave tiles, accumulators pinned to AGPRs, fragments read one
    half-phase ahead; gemm256x.hip (= 4): the same wave tiles with whole-tile double buffering and one barrier per K-tile.
    Same results as the default kernels for every epilogue and for ragged M."""
    need_experiments(hip_ops)
    _gemm_variant_case(hip_ops, M, N, K, epi, kernel)


@pytest.mark.parametrize("M,N,K,epi", GEMM_VARIANT_CASES + [(5000, 2560, 128, "resid"), (6000, 2304, 192, "split"), (30000, 5120, 64, "resid")])
@pytest.mark.parametrize("kernel", [5, 6])
def test_gemm_persistent_forced_for_every_epilogue(hip_ops, M, N, K, epi, kernel):
    """gemm256p.hip forced through the A/B switch (gemm256 = 5 static stride / 6 per-XCD work counter) for EVERY epilogue and for
    launches smaller than the chip (the default uses it for the bf16 / GELU epilogues of large launches only): same results as
    the fp32 reference for every epilogue, ragged M, the split-plane layout, one tile and several tiles per work-group."""
    _gemm_variant_case(hip_ops, M, N, K, epi, kernel)


def _gemm_variant_case(hip_ops, M, N, K, epi, kernel):
    a = rnd((M, K), 431).to(torch.bfloat16)
    w = rnd((N, K), 432, 1.0 / math.sqrt(K)).to(torch.bfloat16)
    bias = rnd((N,), 433, 0.1)
    acc = a.float() @ w.float().t() + bias
    hip_ops.lib.icv_set_option(b"gemm256", kernel)
    try:
        if epi == "f32":
            out = torch.full((M + 1, N), 5.0, device=DEV)
            hip_ops.gemm(a.to(DEV), w.to(DEV), bias.to(DEV), out[:M], EPI_F32)
            assert_f32_close(out[:M], acc, what=f"gemm 4-wave {M}x{N}x{K}")
            assert bool((out[M:] == 5.0).all()), "wrote past the last row"
        elif epi == "bf16":
            out = torch.empty((M, N), dtype=torch.bfloat16, device=DEV)
            hip_ops.gemm(a.to(DEV), w.to(DEV), bias.to(DEV), out, EPI_BF16)
            assert_bf16_close(out, acc, "gemm 4-wave bf16")
        elif epi == "gelu":
            out = torch.empty((M, N), dtype=torch.bfloat16, device=DEV)
            hip_ops.gemm(a.to(DEV), w.to(DEV), bias.to(DEV), out, EPI_GELU_BF16)
            assert_bf16_close(out, torch.nn.functional.gelu(acc, approximate="tanh"), "gemm 4-wave gelu", abs_floor=2.0 ** -8)
        elif epi == "resid":
            resid, gate = rnd((M, N), 434), rnd((N,), 435)
            out = resid.clone().to(DEV)
            hip_ops.gemm(a.to(DEV), w.to(DEV), bias.to(DEV), out, EPI_RESID_F32, resid=out, gate=gate.to(DEV))
            assert_f32_close(out, resid + gate * acc, what="gemm 4-wave resid")
        else:
            ns = N // 3
            out = torch.empty((3, M, ns), dtype=torch.bfloat16, device=DEV)
            hip_ops.gemm(a.to(DEV), w.to(DEV), bias.to(DEV), out, EPI_BF16, nsplit=ns)
            assert_bf16_close(out, acc.reshape(M, 3, ns).permute(1, 0, 2), "gemm 4-wave split planes")
    finally:
        hip_ops.lib.icv_set_option(b"gemm256", 2)


def _persist(hip_ops, on):
    hip_ops.lib.icv_set_option(b"gemm256_persist", int(on))


@pytest.mark.parametrize("M,N,K,epi,split", [(9360, 13824, 256, EPI_GELU_BF16, 0), (18000, 7680, 192, EPI_BF16, 0), (12345, 15360, 128, EPI_BF16, 5120),
                                             (74880, 4608, 64, EPI_BF16, 1536)])
def test_gemm_persistent_default_is_bit_identical_to_one_tile_per_block(hip_ops, M, N, K, epi, split):
    """icv_gemm_bf16 runs the bf16 / GELU epilogues of launches with >= 2 tiles per CU on the persistent kernel (gemm256p.hip:
    per-XCD work counters, next tile's prologue under the current epilogue).  Same MFMA order per accumulator, so the bytes must equal
    the one-tile-per-block launch (gemm256_persist = 0) - for ragged M, the split-plane QKV layout and launch after launch on the same
    stream (the counter block is found zeroed and left zeroed by every launch)."""
    a = rnd((M, K), 441).to(torch.bfloat16).to(DEV)
    w = rnd((N, K), 442, 1.0 / math.sqrt(K)).to(torch.bfloat16).to(DEV)
    bias = rnd((N,), 443, 0.1).to(DEV)
    shape = (N // split, M, split) if split else (M, N)
    ref = torch.empty(shape, dtype=torch.bfloat16, device=DEV)
    _persist(hip_ops, 0)
    try:
        hip_ops.gemm(a, w, bias, ref, epi, nsplit=split or None)
    finally:
        _persist(hip_ops, 1)
    for rep in range(3):
        out = torch.full(shape, 7.0, dtype=torch.bfloat16, device=DEV)
        hip_ops.gemm(a, w, bias, out, epi, nsplit=split or None)
        assert torch.equal(out, ref), f"persistent launch {rep} differs from the one-tile-per-block launch"
    acc = a[:512].float() @ w.float().t() + bias
    if epi == EPI_GELU_BF16:
        acc = torch.nn.functional.gelu(acc, approximate="tanh")
    got = (ref.permute(1, 0, 2).reshape(M, N) if split else ref)[:512]
    assert_bf16_close(got, acc.cpu(), "persistent-default gemm vs fp32", abs_floor=2.0 ** -8)


def test_gemm_persistent_under_graph_capture_and_on_two_streams(hip_ops):
    """The persistent kernel's work counters are stateless between launches (zero at launch, zeroed by the last work-group to leave)
    and come from a per-(device, stream) pool: (a) a hipGraph captured on a stream that never launched the kernel eagerly replays
    correctly any number of times (a launch inside a capture that finds no pool falls back to the one-tile-per-block kernel);
    (b) two streams launching at the same time do not share counters."""
    M, N, K = 20000, 7680, 128
    a = rnd((M, K), 451).to(torch.bfloat16).to(DEV)
    w = rnd((N, K), 452, 1.0 / math.sqrt(K)).to(torch.bfloat16).to(DEV)
    bias = rnd((N,), 453, 0.1).to(DEV)
    ref = torch.empty((M, N), dtype=torch.bfloat16, device=DEV)
    _persist(hip_ops, 0)
    try:
        hip_ops.gemm(a, w, bias, ref, EPI_BF16)
    finally:
        _persist(hip_ops, 1)
    out = torch.zeros_like(ref)
    hip_ops.gemm(a, w, bias, out, EPI_BF16)          # an eager launch first: the counter pool exists before the capture starts
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        hip_ops.gemm(a, w, bias, out, EPI_BF16)
        hip_ops.gemm(a, w, bias, out, EPI_GELU_BF16)
        hip_ops.gemm(a, w, bias, out, EPI_BF16)
    for rep in range(3):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ref), f"graph replay {rep}"
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    o1, o2 = torch.zeros_like(ref), torch.zeros_like(ref)
    for rep in range(4):
        with torch.cuda.stream(s1):
            hip_ops.gemm(a, w, bias, o1, EPI_BF16)
        with torch.cuda.stream(s2):
            hip_ops.gemm(a, w, bias, o2, EPI_BF16)
    torch.cuda.synchronize()
    assert torch.equal(o1, ref) and torch.equal(o2, ref), "concurrent persistent launches on two streams"


def test_gemm_a_operand_of_more_than_4_gib(hip_ops):
    """A lane's A-row position is a 32-bit byte offset from the operand base: icv_gemm_bf16 runs an A operand of >= 4 GiB (here 160 256 rows x
    13 824 = 4.43 GB: FFN2 of both CFG forwards of a long 720p clip) as row ranges cut on the 256-row tile grid.  Rows on both sides of the cut
    (155 136) and the ragged tail against fp32 torch, for the gated-residual and the bf16 epilogue."""
    M, N, K = 160256, 256, 13824
    g = torch.Generator(device=DEV).manual_seed(77)
    a = torch.empty((M, K), dtype=torch.bfloat16, device=DEV)
    for r0 in range(0, M, 20032):                                                  # filled in slabs: no fp32 copy of the whole operand
        a[r0:r0 + 20032] = torch.randn((min(20032, M - r0), K), device=DEV, generator=g).to(torch.bfloat16)
    w = (torch.randn((N, K), device=DEV, generator=g) / math.sqrt(K)).to(torch.bfloat16)
    bias = torch.randn((N,), device=DEV, generator=g) * 0.1
    gate = torch.randn((N,), device=DEV, generator=g)
    resid = torch.randn((M, N), device=DEV, generator=g)
    rows = torch.cat([torch.arange(0, 300), torch.arange(155136 - 300, 155136 + 300), torch.arange(M - 300, M)]).to(DEV)
    want = a[rows].float() @ w.float().t() + bias
    out = resid.clone()
    hip_ops.gemm(a, w, bias, out, EPI_RESID_F32, resid=out, gate=gate)
    assert_f32_close(out[rows], resid[rows] + gate * want, rtol=3e-4, what="gemm, A > 4 GiB, gated residual")
    ob = torch.empty((M, N), dtype=torch.bfloat16, device=DEV)
    hip_ops.gemm(a, w, bias, ob, EPI_BF16)
    assert_bf16_close(ob[rows], want, "gemm, A > 4 GiB, bf16 epilogue")


@pytest.mark.parametrize("M,N,K", [(1, 4, 64), (3, 68, 64), (255, 252, 192), (257, 260, 128), (513, 256, 64)])
def test_gemm_ragged_shapes(hip_ops, M, N, K):
    a = rnd((M, K), 311).to(torch.bfloat16)
    w = rnd((N, K), 312, 1.0 / math.sqrt(K)).to(torch.bfloat16)
    bias = rnd((N,), 313, 0.1)
    out = torch.full((M + 1, N), 5.0, device=DEV)
    hip_ops.gemm(a.to(DEV), w.to(DEV), bias.to(DEV), out[:M], EPI_F32)
    assert_f32_close(out[:M], a.float() @ w.float().t() + bias, what=f"gemm ragged {M}x{N}x{K}")
    assert bool((out[M:] == 5.0).all()), "wrote past the last row"


def test_norm_kernels_single_row(hip_ops):
    x = rnd((1, 1536), 321, 3.0)
    out = torch.empty((1, 1536), dtype=torch.bfloat16, device=DEV)
    hip_ops.ln_modulate(x.to(DEV), out, eps=1e-6)
    assert_bf16_close(out, R.layer_norm(x, None, None, 1e-6), "ln single row")
    q = rnd((1, 1536), 322).to(torch.bfloat16)
    w = 1 + rnd((1536,), 323, 0.1)
    rope = RopeTable.build(2, 2, 2, DEV)
    g = q.clone().to(DEV)
    hip_ops.rmsnorm_rope(g, w.to(DEV), eps=1e-6, rope=rope, tok0=7)        # last token of the grid
    ref = R.rope_apply(R.rms_norm(q.float(), w, 1e-6), R.rope_freqs_3d(128, 2, 2, 2)[7:8], 12)
    assert_bf16_close(g, ref, "rmsnorm+rope single row at the last token")


def test_single_frame_generation_grid(hip_ops):
    """num_frames = 1 (T = 1) is legal (1 mod 4): the whole forward must work on a 1-frame token grid."""
    from infinicube_amd.videogen import synthetic as syn
    from infinicube_amd.videogen.config import TokenGrid, preset
    from infinicube_amd.videogen.dit import WanDiT
    cfg, grid = preset("tiny"), TokenGrid(1, 32, 48)
    sd, bsd = syn.make_dit_state_dict(cfg), syn.make_buffer_embedder_state_dict(cfg)
    noise, ctx, bl = syn.make_latent_noise(grid), syn.make_text_context(cfg, 1), syn.make_buffer_latents(cfg, grid)
    m = WanDiT(cfg, sd, hip_ops, bsd).prepare(grid)
    m.forward_tokens(noise.to(DEV), m.encode_context(ctx), 500.0, m.embed_buffers(bl), m.head_out[0])
    torch.cuda.synchronize()
    v = R.unpatchify(m.head_out[0].cpu(), (grid.T, grid.Hp, grid.Wp), cfg.out_dim)
    ref = R.dit_forward(R.round_state_dict_to_bf16(sd), cfg, noise, ctx, 500.0, R.buffer_embed(R.round_state_dict_to_bf16(bsd), bl))
    assert float((v - ref).norm() / ref.norm()) < 2e-2


def test_fuzz_gemm_and_attention_fixed_sequence():
    """tools/fuzz_kernels.py, 6000 cases of seed 7 (a fixed sequence, a few seconds): random ragged shapes, strides, epilogues, tile families, schedules, key
    chunks of both MFMA entry points against stock PyTorch fp32 on the GPU, every launch repeated bit-identically.
    (A 240 s + 150 s run of the same tool is recorded in profiles/r02/fuzz_kernels.txt.)"""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_kernels.py"), "0", "7", "6000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " 0 failures" in r.stdout


def test_randomised_token_local_kernels(hip_ops):
    """Seeded random sweep of the token-local entry points against the oracle (the GEMM / attention counterpart is
    tools/fuzz_kernels.py): LayerNorm + modulate over ragged row counts at four widths (256, 512, 1536, 5120; every
    width instantiation of the norm kernels is walked by tests/test_token_local_widths_gpu.py), RMSNorm + 3-D RoPE on
    random (T, Hp, Wp) grids with a random shard [tok0, tok0 + n), the e4m3 GEMM on ragged M / N, and the image-branch
    attention that ADDS into an existing output."""
    import random
    rng = random.Random(2024)
    dv = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    for case in range(40):
        # --- K3 / K8 ---
        d = rng.choice([256, 512, 1536, 5120])
        rows = rng.choice([1, 2, 31, 64, 65, 257, rng.randint(1, 700)])
        x = rnd((rows, d), 1000 + case, rng.choice([0.5, 2.0, 8.0])) + rng.choice([0.0, 0.5, -3.0])
        affine, mod = rng.random() < 0.5, rng.random() < 0.7
        w = 1 + rnd((d,), 2000 + case, 0.1) if affine else None
        b = rnd((d,), 3000 + case, 0.1) if affine else None
        sh = rnd((d,), 4000 + case, 0.3) if mod else None
        sc = rnd((d,), 5000 + case, 0.3) if mod else None
        ref = R.layer_norm(x, w, b, 1e-6)
        if mod:
            ref = R.modulate(ref, sh, sc)
        out = torch.full((rows + 1, d), 3.0, dtype=torch.bfloat16, device=DEV)
        hip_ops.ln_modulate(x.to(DEV), out[:rows], dv(w), dv(b), dv(sh), dv(sc), 1e-6)
        assert_bf16_close(out[:rows], ref, f"ln rows={rows} d={d} affine={affine} mod={mod}")
        assert bool((out[rows:] == 3.0).all()), "ln_modulate wrote past the last row"
        # --- K5 ---
        T, Hp, Wp = rng.randint(1, 6), rng.randint(1, 9), rng.randint(1, 11)
        S = T * Hp * Wp
        n = rng.randint(1, S)
        tok0 = rng.randint(0, S - n)
        d = rng.choice([256, 512, 1536, 5120])
        planes = rnd((2, n, d), 6000 + case).to(torch.bfloat16)
        w0, w1 = 1 + rnd((d,), 7000 + case, 0.1), 1 + rnd((d,), 8000 + case, 0.1)
        freqs = R.rope_freqs_3d(128, T, Hp, Wp)[tok0: tok0 + n]
        g = planes.to(DEV)
        hip_ops.rmsnorm_rope(g[0], w0.to(DEV), g[1], w1.to(DEV), 1e-6, RopeTable.build(T, Hp, Wp, DEV), tok0)
        what = f"rms+rope grid=({T},{Hp},{Wp}) tok0={tok0} n={n} d={d}"
        assert_bf16_close(g[0], R.rope_apply(R.rms_norm(planes[0].float(), w0, 1e-6), freqs, d // 128), what + " q")
        assert_bf16_close(g[1], R.rope_apply(R.rms_norm(planes[1].float(), w1, 1e-6), freqs, d // 128), what + " k")
    for case in range(12):
        # --- e4m3 GEMM, ragged M / N ---
        M, N, K = rng.choice([1, 63, 257, 300, 777, 1030]), 4 * rng.choice([1, 33, 64, 65, 192, 260]), 128 * rng.choice([1, 2, 3, 12])
        a = rnd((M, K), 9000 + case, 1.5)
        w = rnd((N, K), 9100 + case, 1.0 / math.sqrt(K))
        bias = rnd((N,), 9200 + case, 0.1)
        aq, asc = R.quantize_rows_fp8(a)
        wq, wsc = R.quantize_rows_fp8(w)
        acc = (aq.double() @ wq.double().t()).float() * asc[:, None] * wsc[None, :] + bias
        out = torch.full((M + 1, N), 5.0, device=DEV)
        hip_ops.gemm_fp8(aq.to(FP8).to(DEV), asc.to(DEV), wq.to(FP8).to(DEV), wsc.to(DEV), bias.to(DEV), out[:M], EPI_F32)
        assert_f32_close(out[:M], acc, rtol=1e-4, what=f"gemm_fp8 {M}x{N}x{K}")
        assert bool((out[M:] == 5.0).all()), "gemm_fp8 wrote past the last row"
        # --- K9 image branch: o += attention(q, k_img, v_img) ---
        H, Sq, Skv = rng.choice([1, 2, 3]), rng.choice([1, 33, 257, 300, 640]), rng.choice([1, 64, 65, 257])
        dd = H * 128
        q, k, v = (rnd((Sq, dd), 9300 + case).to(torch.bfloat16), rnd((Skv, dd), 9400 + case).to(torch.bfloat16),
                   rnd((Skv, dd), 9500 + case).to(torch.bfloat16))
        prev = rnd((Sq, dd), 9600 + case).to(torch.bfloat16)
        o = prev.clone().to(DEV)
        hip_ops.attention_add(q.to(DEV), k.to(DEV), v.to(DEV), o, H, 1.0 / math.sqrt(128))
        assert_bf16_close(o, prev.float() + R.attention(q.float(), k.float(), v.float(), H), f"attention_add Sq={Sq} Skv={Skv} H={H}",
                          abs_floor=2.0 ** -5, rms_bound=2.0 ** -7)


def test_copy_path_probe_controls(hip_ops):
    """icv_probe_copy_path - the first-contact instrument that says whether a copy needs compute units (an occupier kernel holds every wave
    slot of the device; a copy that completes meanwhile was moved by a copy engine) - against its two controls in ONE process:
    a same-device device-to-device copy is a blit KERNEL on this runtime (profiles/r05/stream_ops_probe.txt: __amd_rocclr_copyBuffer) and
    must answer 2; a pinned-host-to-device copy is executed by an SDMA engine and must answer 1.  (Between ranks that SHARE a GPU the
    hardware scheduler time-slices the processes' queues and the probe may answer 0 = inconclusive: it is built for one rank per device.)"""
    import ctypes
    from infinicube_amd import native
    n = 8 << 20
    src_dev = torch.randint(0, 255, (n,), dtype=torch.uint8, device=DEV)
    src_pin = torch.randint(0, 255, (n,), dtype=torch.uint8).pin_memory()
    dst = torch.zeros((n,), dtype=torch.uint8, device=DEV)
    got = {}
    for name, src in (("device->device", src_dev), ("pinned host->device", src_pin)):
        kinds = []
        for _ in range(3):
            kind, ms = ctypes.c_int(-1), ctypes.c_double(0.0)
            native.check(hip_ops.lib.icv_probe_copy_path(src.data_ptr(), dst.data_ptr(), n, ctypes.byref(kind), ctypes.byref(ms)), "icv_probe_copy_path")
            kinds.append(kind.value)
            assert torch.equal(dst.cpu(), src.cpu())
        got[name] = kinds
    print(f"copy-path probe: {got} (1 = copy engine, 2 = blit kernel, 0 = inconclusive)")
    assert all(k == 2 for k in got["device->device"]), got
    assert all(k == 1 for k in got["pinned host->device"]), got
