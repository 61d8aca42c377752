"""Every GEMM kernel and epilogue, bit for bit, on exact-integer inputs (constructions and expected values: tests/gemm_exact.py; their
premise is checked on the CPU by tests/test_gemm_exact_cpu.py).

No tolerance anywhere: operands are small integers, scales and gates powers of two, so every partial sum is exact in f32 whatever the
summation order, and the expected output is known to the bit.  The one exception is the GELU epilogue, whose INPUT is exact and whose
stored bf16 must be a faithful rounding of the float64 activation (gemm_exact.gelu_bad, derived there).

Layouts are chosen so that a stray access shows: every output is a view into a sentinel-filled allocation (ldo = N + 8, two guard rows
behind row M, a gap between split planes), A is a view with lda = K + 64 whose padding holds a huge value, the residual is read in place
and through ldr = N + 16 != ldo.  After two launches back to back into two fresh buffers: interior equal to the expectation, every
sentinel intact, every read-only operand unchanged, both buffers bit-identical.
"""
import contextlib
import functools
from types import SimpleNamespace

import pytest
import torch

import gemm_exact as G
from gemm_exact import BF16, F32, FP8, EPI_BF16, EPI_GELU_BF16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = {BF16: -12288.0, F32: -12345.0}      # both exact in their type; no expected value comes near
OPTION_DEFAULTS = {"gemm256": 2, "gemm256_sched": 3, "gemm256_mfma": 16, "gemm_fp8_sched": 3}
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


@contextlib.contextmanager
def options(lib, **kw):
    try:
        for k, v in kw.items():
            assert lib.icv_set_option(k.encode(), v) == 0
        yield
    finally:
        for k in kw:
            lib.icv_set_option(k.encode(), OPTION_DEFAULTS[k])


def same_bits(a, b):
    return torch.equal(a.view(_INT_VIEW[a.element_size()]), b.view(_INT_VIEW[b.element_size()]))


def _fp8_to_dev(t):
    return t.contiguous().view(torch.uint8).to(DEV).view(FP8)


@functools.lru_cache(maxsize=2)
def operands(fmt, M, N, K, kind):
    """Device copies of one case's read-only operands (+ a pristine clone of each, to show that a launch left them alone)."""
    inp = G.make(fmt, M, N, K, kind)
    d = SimpleNamespace(inp=inp, fmt=fmt)
    if fmt == "bf16":
        d.a_buf = torch.full((M, K + 64), 32768.0, dtype=BF16, device=DEV)        # padding: a value that would wreck any sum it entered
        d.a_buf[:, :K] = inp.a.to(DEV)
        d.w = inp.w.to(DEV)
        ro = {}
    else:
        raw = torch.full((M, K + 64), 0x7E, dtype=torch.uint8, device=DEV)         # 0x7E = 448, the largest e4m3
        raw[:, :K] = inp.a.view(torch.uint8).to(DEV)
        d.a_buf = raw.view(FP8)
        d.w = _fp8_to_dev(inp.w)
        d.a_scale, d.w_scale = inp.a_scale.to(DEV), inp.w_scale.to(DEV)
        ro = {"a_scale": d.a_scale, "w_scale": d.w_scale}
    d.a = d.a_buf[:, :K]                                                           # lda = K + 64
    d.bias, d.gate = inp.bias.to(DEV), inp.gate.to(DEV)
    ro.update(A=d.a_buf, W=d.w, bias=d.bias, gate=d.gate)
    d.read_only = {k: (t, t.clone()) for k, t in ro.items()}
    return d


def out_buffer(M, N, dtype, nsplit):
    """(flat allocation, the view the kernel writes, mask of the view's elements in the allocation)."""
    planes, width = (1, N) if nsplit is None else (N // nsplit, nsplit)
    ldo = width + 8
    sstride = (M + 2) * ldo + 24                  # split planes: a gap between planes (split_stride > M * ldo)
    flat = torch.full((planes * sstride,), SENTINEL[dtype], dtype=dtype, device=DEV)
    size, stride = ((M, N), (ldo, 1)) if nsplit is None else ((planes, M, width), (sstride, ldo, 1))
    interior = torch.zeros(flat.numel(), dtype=torch.bool, device=DEV)
    interior.as_strided(size, stride).fill_(True)
    return SimpleNamespace(flat=flat, view=flat.as_strided(size, stride), interior=interior, ldo=ldo, sstride=sstride)


def _where(mask, n=4):
    return [tuple(i) for i in mask.nonzero()[:n].tolist()]


def run_case(ops, fmt, shape, case, tag, launches=2):
    """One (kernel, epilogue, shape): `launches` launches back to back on the current stream, then every check.  Returns the failures."""
    name, epi, kind, use_bias, use_gate, resid_mode, split = case
    M, N, K = shape
    d = operands(fmt, M, N, K, kind)
    inp = d.inp
    odt = BF16 if epi in (EPI_BF16, EPI_GELU_BF16) else F32
    nsplit = N // 3 if split else None
    exp = G.expected(inp, epi, use_bias, use_gate)
    what = f"{tag} [{name}] {M}x{N}x{K}"
    resid = resid_buf = resid_keep = None
    if resid_mode == "ldr":
        resid_buf = torch.full((M, N + 16), SENTINEL[F32], device=DEV)
        resid_buf[:, :N] = inp.resid.to(DEV)
        resid, resid_keep = resid_buf[:, :N], resid_buf.clone()
    outs = [out_buffer(M, N, odt, nsplit) for _ in range(launches)]
    if resid_mode == "inplace":
        for o in outs:
            o.view.copy_(inp.resid.to(DEV))
    bias, gate = (d.bias if use_bias else None), (d.gate if use_gate else None)
    for o in outs:
        r = o.view if resid_mode == "inplace" else resid
        if fmt == "bf16":
            ops.gemm(d.a, d.w, bias, o.view, epi, resid=r, gate=gate, nsplit=nsplit)
        else:
            ops.gemm_fp8(d.a, d.a_scale, d.w, d.w_scale, bias, o.view, epi, resid=r, gate=gate, nsplit=nsplit)
    torch.cuda.synchronize()

    fails = []
    if epi == EPI_GELU_BF16:
        ref, tol = exp.to(DEV), G.gelu_tol(exp).to(DEV)
        rne = exp.to(F32).to(BF16).to(DEV)
    else:
        want = (exp if nsplit is None else G.split_planes(exp, nsplit)).to(DEV)
    for i, o in enumerate(outs):
        if epi == EPI_GELU_BF16:
            bad = G.gelu_bad(o.view, ref, tol)
            if i == 0:      # information only, no cap: how often the faithful rounding is not the nearest one
                print(f"{what}: {float((o.view != rne).double().mean()):.4%} of the stored elements are not the RNE neighbour of gelu")
            if bool(bad.any()):
                at = _where(bad)
                fails.append(f"{what} launch {i}: {int(bad.sum())} elements are no faithful rounding of gelu, first (m, n) {at}: got "
                             f"{[float(o.view[p]) for p in at]}, reference {[float(ref[p]) for p in at]}")
        elif not torch.equal(o.view, want):
            bad = o.view != want
            at = _where(bad)
            fails.append(f"{what} launch {i}: {int(bad.sum())} of {bad.numel()} elements differ, first {'(plane, m, n)' if split else '(m, n)'} {at}: got "
                         f"{[float(o.view[p]) for p in at]}, expected {[float(want[p]) for p in at]}")
        hit = ~o.interior & (o.flat != SENTINEL[odt])
        if bool(hit.any()):
            offs = [int(x) for x in hit.nonzero()[:4, 0].tolist()]
            fails.append(f"{what} launch {i}: {int(hit.sum())} sentinels overwritten, first (plane, row, column) "
                         f"{[(x // o.sstride, x % o.sstride // o.ldo, x % o.sstride % o.ldo) for x in offs]} (ldo {o.ldo}, M {M})")
    for nm, (t, keep) in d.read_only.items():
        if not same_bits(t, keep):
            fails.append(f"{what}: read-only operand {nm} was written")
    if resid_buf is not None and not same_bits(resid_buf, resid_keep):
        fails.append(f"{what}: read-only operand resid was written")
    for i in range(1, launches):
        if not same_bits(outs[0].flat, outs[i].flat):
            fails.append(f"{what}: launch {i} into a fresh buffer is not bit-identical to launch 0")
    return fails


def run_shape(ops, fmt, shape, tag, only=None, launches=2):
    fails = []
    for case in G.epi_cases(shape[1]):
        if only is None or case[0] in only:
            fails += run_case(ops, fmt, shape, case, tag, launches)
    assert not fails, "\n".join(fails)


# ---- the 128 x 128 kernel (gemm.hip): forced, and as the default dispatch picks it (N % 256 != 0 or M < 256) ----
@pytest.mark.parametrize("gemm256", [0, 2], ids=["forced", "default"])
@pytest.mark.parametrize("shape", G.G128_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gemm128(hip_ops, shape, gemm256):
    with options(hip_ops.lib, gemm256=gemm256):
        run_shape(hip_ops, "bf16", shape, f"gemm128 (gemm256={gemm256})")


# ---- gemm256.hip: default schedule, the k-split schedule (67), and 32x32x16 MFMAs (also: the non-batched residual epilogue, the 32x32 C layout) ----
G256_VARIANTS = {"sched3": {}, "sched67": {"gemm256_sched": 67}, "mfma32": {"gemm256_mfma": 32}}


@pytest.mark.parametrize("variant", list(G256_VARIANTS))
@pytest.mark.parametrize("shape", G.G256_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gemm256(hip_ops, shape, variant):
    with options(hip_ops.lib, gemm256=1, **G256_VARIANTS[variant]):
        run_shape(hip_ops, "bf16", shape, f"gemm256 ({variant})")


# ---- gemm256p.hip: the persistent kernel forced for every epilogue (5 = static stride, 6 = per-XCD work counter) ----
@pytest.mark.parametrize("mode", [5, 6])
@pytest.mark.parametrize("shape", G.G256_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gemm256p(hip_ops, shape, mode):
    with options(hip_ops.lib, gemm256=mode):
        run_shape(hip_ops, "bf16", shape, f"gemm256p (gemm256={mode})")


def test_gemm256p_default_dispatch_with_several_tiles_per_work_group(hip_ops):
    """130 x 4 = 520 tiles: at least two per CU, so the default dispatch takes the persistent kernel for the BF16 / GELU epilogues and
    its work-groups loop over several tiles; ragged M."""
    M, N, K = G.G256P_BIG
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert (M + 255) // 256 * (N // 256) >= 2 * cus, f"{cus} CUs: this shape no longer reaches the persistent kernel by default"
    run_shape(hip_ops, "bf16", G.G256P_BIG, "gemm256p (default dispatch)", only=("bf16+bias", "gelu+bias"))


def test_gemm256p_counter_block_is_found_zeroed_by_the_next_launch(hip_ops):
    """Three launches back to back on one (fresh) stream under the work-counter mode: the counter block a launch leaves must be the
    zeroed block the next one needs, or that one skips or repeats tiles."""
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    try:
        with options(hip_ops.lib, gemm256=6), torch.cuda.stream(side):
            run_shape(hip_ops, "bf16", (2305, 512, 64), "gemm256p (gemm256=6, side stream)", only=("bf16+bias", "resid inplace+gate+bias", "f32"), launches=3)
    finally:
        torch.cuda.synchronize()


# ---- gemm_fp8.hip: two-phase loop + batched residual epilogue (3, default) and the four-phase loop (0) ----
@pytest.mark.parametrize("sched", [3, 0])
@pytest.mark.parametrize("shape", G.FP8_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gemm_fp8(hip_ops, shape, sched):
    """(257, 260, 256) with RESID under sched 3: column block 0 takes the batched residual epilogue, the edge block the per-fragment one."""
    with options(hip_ops.lib, gemm_fp8_sched=sched):
        run_shape(hip_ops, "fp8", shape, f"gemm_fp8 (sched={sched})")


# ---- GEMV (elementwise.hip): all eight M instantiations; N = 6 leaves two of a block's four waves without a column, K = 264 gives 33
# sixteen-byte steps for 64 lanes ----
@pytest.mark.parametrize("M", G.GEMV_M)
def test_gemv(hip_ops, M):
    fails = []
    for N in G.GEMV_N:
        for K in G.GEMV_K:
            inp = G.make_gemv(M, N, K)
            x, w, bias = inp.x.to(DEV), inp.w.to(DEV), inp.bias.to(DEV)
            keep = [t.clone() for t in (x, w, bias)]
            for use_bias in (True, False):
                what = f"gemv M={M} N={N} K={K} bias={use_bias}"
                want = G.expected_gemv(inp, use_bias).to(DEV)
                flats = [torch.full((M * N + 64,), SENTINEL[F32], device=DEV) for _ in range(2)]
                for f in flats:
                    hip_ops.gemv(x, w, bias if use_bias else None, f[: M * N].view(M, N))
                torch.cuda.synchronize()
                for i, f in enumerate(flats):
                    got = f[: M * N].view(M, N)
                    if not torch.equal(got, want):
                        at = _where(got != want)
                        fails.append(f"{what} launch {i}: first (m, n) {at}: got {[float(got[p]) for p in at]}, expected {[float(want[p]) for p in at]}")
                    if not bool((f[M * N:] == SENTINEL[F32]).all()):
                        fails.append(f"{what} launch {i}: wrote behind the output")
                if not same_bits(flats[0], flats[1]):
                    fails.append(f"{what}: second launch is not bit-identical")
            if not all(same_bits(t, k) for t, k in zip((x, w, bias), keep)):
                fails.append(f"gemv M={M} N={N} K={K}: a read-only operand was written")
    assert not fails, "\n".join(fails)
