"""CFG-Zero* guidance on the HIP path (csrc/guidance.hip, icv_cfg_zero_scale_f32): the kernel against float64 at the shapes where its
grid, its sweeps and its two load paths change (bound derived from the arithmetic), its write guard, sum u^2 = 0, reference rounding,
the loop of tests/test_cfg_zero_cpu.py in every driver mode, the two exact cases, the compositions (TeaCache, UniPC, the e4m3 mode)
and the pipeline.

Shapes are (rows, cols, ldh, hu offset in floats).  The kernel's unit of work is a quad of 4 consecutive elements, 256 threads per
block and at most 256 blocks, so one sweep of the grid covers 262 144 elements = 4096 rows of 64."""
import math

import pytest
import torch

from infinicube_amd.videogen import synthetic as syn
from infinicube_amd.videogen import teacache
from infinicube_amd.videogen.dit import WanDiT
from oracle import wan_ref as R
from test_cfg_zero_cpu import CFG, ENV, GRID, LOOP_STEPS, cfg_zero_twin, check_loop, engine_loop, reference, solver_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
SENTINEL = -7.0
PAD = 64                     # floats behind every allocation's last row
EXTRA_ROWS = 2               # rows beyond ``rows`` inside the allocation
WORKSPACE = 512

SHAPES = [
    (1, 64, 64, 0),          # one block, mostly idle
    (23, 64, 72, 0),         # ragged rows, pad columns
    (4099, 64, 64, 0),       # every block busy, a second sweep with a ragged tail
    (4099, 64, 64, 1),       # hu one float past a 16-byte boundary: the scalar path
    (8200, 64, 68, 0),       # two full sweeps and a tail, ldh a multiple of 4 (16-byte loads)
    (8200, 64, 65, 0),       # the same with an odd ldh: the scalar path
]

_DATA = {}


def data(rows, cols):
    """u = randn, c = 0.7 u + 0.5 randn (s ~ 0.7, no cancellation) and the float64 reference, once per (rows, cols)."""
    if (rows, cols) not in _DATA:
        g = torch.Generator().manual_seed(1000 + rows)
        u = torch.randn((rows, cols), generator=g)
        c = 0.7 * u + 0.5 * torch.randn((rows, cols), generator=g)
        _DATA[(rows, cols)] = (c, u) + moments(c, u)
    return _DATA[(rows, cols)]


def moments(c, u):
    """-> (s_ref, bound) in float64 from f32 inputs.

    The bound.  Every product c_j u_j and u_j u_j of two f32 values is exact in fp64, so the kernel's only errors are those of its
    fp64 additions and of the final f32 quotient.  Any summation order of n terms has an error of at most (n - 1) 2^-53 sum |terms|
    to first order; n 2^-52 sum |terms| covers the higher orders, the rounding of den + 1e-8 and of the fp64 division with room to
    spare.  With N = sum c u and D = sum u u + 1e-8:  |dN| <= n 2^-52 sum |c u|,  |dD| <= n 2^-52 sum u u,  so
    |d(N / D)| <= (|dN| + |s| |dD|) / D = n 2^-52 (sum |c u| + |s| sum u u) / sum u u.  The quotient is then rounded to f32 once:
    2^-24 |s| (2^-23 |s| is asserted: a second rounding's worth of room, as the issue sets it)."""
    c64, u64 = c.double(), u.double()
    uu = float((u64 * u64).sum())
    s_ref = float((c64 * u64).sum() / (uu + 1e-8))
    n = c.numel()
    bound = 2.0 ** -23 * abs(s_ref) + n * 2.0 ** -52 * (float((c64 * u64).abs().sum()) + abs(s_ref) * uu) / uu
    return s_ref, bound


def device_rows(values, ldh, offset=0):
    """[rows, cols] values -> (view [rows + EXTRA_ROWS, ldh] of a sentinel-filled allocation that starts ``offset`` floats in, the
    whole allocation).  PAD sentinel floats follow the last row."""
    rows, cols = values.shape
    body = (rows + EXTRA_ROWS) * ldh
    flat = torch.full((offset + body + PAD,), SENTINEL, dtype=F32, device=DEV)
    view = flat[offset: offset + body].view(rows + EXTRA_ROWS, ldh)
    view[:rows, :cols] = values.to(DEV)
    assert (view.data_ptr() % 16 == 0) == (offset % 4 == 0)
    return view, flat


def guard_ok(view, flat, rows, cols, offset):
    """Pad columns, rows beyond ``rows``, the floats in front of and behind the rows: all still the sentinel."""
    host = view.cpu()
    return bool((host[:rows, cols:] == SENTINEL).all() and (host[rows:] == SENTINEL).all()
                and (flat[:offset] == SENTINEL).all() and (flat[-PAD:] == SENTINEL).all())


def run_kernel(hip_ops, c, u, ldh, offset, round_bf16=False):
    rows, cols = u.shape
    (hc, hc_flat), (hu, hu_flat) = device_rows(c, ldh), device_rows(u, ldh, offset)
    work = torch.full((WORKSPACE + 8,), float(SENTINEL), dtype=F64, device=DEV)
    out = torch.full((3,), SENTINEL, dtype=F32, device=DEV)
    hip_ops.cfg_zero_scale(hc[:, :cols], hu[:, :cols], rows, work[:WORKSPACE], out[1:2], round_bf16=round_bf16)
    torch.cuda.synchronize()
    assert torch.equal(hc[:rows, :cols].cpu(), c), "hc was written"
    assert guard_ok(hc, hc_flat, rows, cols, 0) and guard_ok(hu, hu_flat, rows, cols, offset), "written outside [rows, cols]"
    assert (work[WORKSPACE:] == SENTINEL).all() and out[0] == SENTINEL and out[2] == SENTINEL, "written outside the workspace / the scale slot"
    return out[1:2].cpu(), hu[:rows, :cols].cpu()


# ---- 1. the kernel against float64 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols,ldh,offset", SHAPES)
def test_kernel_matches_float64(hip_ops, rows, cols, ldh, offset):
    c, u, s_ref, bound = data(rows, cols)
    s, hu = run_kernel(hip_ops, c, u, ldh, offset)
    err = abs(float(s) - s_ref)
    print(f"{(rows, cols, ldh, offset)}: s = {float(s):.9f}, float64 {s_ref:.9f}, |err| {err:.2e}, bound {bound:.2e}")
    assert abs(s_ref - 0.7) < 0.2 and err <= bound, f"|s - s_ref| = {err:.3e} > {bound:.3e}"
    assert torch.equal(hu, s * u), "hu must be fl32(s * u): one f32 multiply per element"
    # the same bits on a second run, in fresh allocations
    s2, hu2 = run_kernel(hip_ops, c, u, ldh, offset)
    assert torch.equal(s2, s) and torch.equal(hu2, hu)


def test_alignment_and_stride_do_not_change_the_bits(hip_ops):
    """The assignment of elements to threads is a function of (rows, cols) alone: the 16-byte path and the scalar path sum in the
    same order."""
    for rows, cols, variants in ((4099, 64, ((64, 0), (64, 1), (68, 0), (65, 3))), (23, 64, ((64, 0), (72, 2)))):
        c, u, _, _ = data(rows, cols)
        got = [run_kernel(hip_ops, c, u, ldh, off) for ldh, off in variants]
        assert all(torch.equal(s, got[0][0]) and torch.equal(hu, got[0][1]) for s, hu in got[1:])


# ---- 2. sum u^2 = 0 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("round_bf16", [False, True])
def test_zero_unconditional_output(hip_ops, round_bf16):
    c = data(23, 64)[0]
    s, hu = run_kernel(hip_ops, c, torch.zeros_like(c), 72, 0, round_bf16=round_bf16)
    assert float(s) == 0.0 and torch.equal(hu, torch.zeros_like(c)) and not torch.isnan(hu).any()


# ---- 3. reference rounding ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols,ldh,offset", [(23, 64, 72, 0), (4099, 64, 64, 0), (4099, 64, 64, 1)])
def test_reference_rounding(hip_ops, rows, cols, ldh, offset):
    """The moments on the bf16-rounded inputs (bound: moments(), the products of bf16 values are exact as well), s rounded to bf16:
    half a bf16 ulp of the reference on top.  hu: the twin's bf16(s * bf16(u)) on the kernel's own s, bit for bit."""
    rb = lambda t: t.to(torch.bfloat16).to(F32)                                  # noqa: E731
    c, u, _, _ = data(rows, cols)
    s_ref, bound = moments(rb(c), rb(u))
    s, hu = run_kernel(hip_ops, c, u, ldh, offset, round_bf16=True)
    half_ulp = 2.0 ** (math.floor(math.log2(abs(s_ref))) - 8)
    assert torch.equal(s, rb(s)), "s must be a bf16 value"
    assert abs(float(s) - s_ref) <= bound + half_ulp, f"s = {float(s)}, reference {s_ref}"
    assert torch.equal(hu, rb(s * rb(u)))
    out, twin_u = torch.zeros(1), u.clone()
    cfg_zero_twin(c, twin_u, rows, out, round_bf16=True)
    assert torch.equal(out, s) and torch.equal(twin_u, hu), "the CPU twin and the kernel disagree"


def test_operator_layer_checks(hip_ops):
    c, u, _, _ = data(23, 64)
    hc, hu = c.to(DEV), u.to(DEV)
    work, out = torch.zeros(WORKSPACE, dtype=F64, device=DEV), torch.zeros(1, device=DEV)
    with pytest.raises(TypeError):
        hip_ops.cfg_zero_scale(hc, hu.double(), 23, work, out)
    with pytest.raises(TypeError):
        hip_ops.cfg_zero_scale(hc, hu, 23, work.float(), out)
    with pytest.raises(ValueError, match="fewer rows than n_tok"):
        hip_ops.cfg_zero_scale(hc, hu, 24, work, out)
    with pytest.raises(ValueError, match="row stride"):
        hip_ops.cfg_zero_scale(hc, torch.zeros((23, 72), device=DEV)[:, :64], 23, work, out)
    with pytest.raises(ValueError, match="workspace must hold"):
        hip_ops.cfg_zero_scale(hc, hu, 23, work[:100], out)
    with pytest.raises(Exception, match="hc and hu must differ"):
        hip_ops.cfg_zero_scale(hu, hu, 23, work, out)
    torch.cuda.synchronize()
    assert torch.equal(hu.cpu(), u), "a refused call must not launch"


# ---- 4. the loop, in every driver mode ------------------------------------------------------------------------------------------------
def _sequential(m):
    m.cfg_batch = False


@pytest.mark.parametrize("mode", ["per-op", "pair", "pair-no-stem", "native", "graphs", "dual-stream"])
def test_loop_matches_restated_cfg_zero_star(hip_ops, mode, monkeypatch):
    """The loop of test_cfg_zero_cpu on HipOps (tiny preset, 5 latent frames, CFG 5, Euler, 6 steps, the gains of that file): the scale
    runs in front of the update, outside captured graphs, on the update's stream.  The same three conditions in every mode."""
    prep, setup = dict(graphs=False), None
    if mode == "per-op":
        setup = _sequential
    elif mode == "pair-no-stem":
        setup = lambda m: setattr(m, "share_stem", False)                        # noqa: E731
    elif mode == "native":
        setup = lambda m: setattr(m, "native_forward", True)                     # noqa: E731
    elif mode == "graphs":
        prep = dict(graphs=True)
    elif mode == "dual-stream":
        monkeypatch.setenv("ICV_DUAL_STREAM", "1")
    m, lat = engine_loop(hip_ops, setup=setup, prep=prep, dev=DEV)
    torch.cuda.synchronize()
    assert torch.isfinite(lat).all()
    if mode == "per-op":
        assert m._pair is None
    if mode in ("pair", "pair-no-stem"):
        assert m._pair is not None
    if mode == "native":
        assert m.native_forward and m._native_eligible()
    if mode == "graphs":
        assert m._graphs_on and m._graphs
    if mode == "dual-stream":
        assert m.dual_stream and m._twin is not None
    assert len(m.guidance_scales) == LOOP_STEPS
    check_loop(lat, m.guidance_scales, mode)
    _, plain = engine_loop(hip_ops, zero_star=False, setup=setup, prep=prep, dev=DEV)
    torch.cuda.synchronize()
    assert not torch.equal(plain, lat)
    p = R.psnr(plain.cpu(), reference(False)[0])
    assert p >= 40.0, f"{mode}: the plain loop on the same inputs vs restated plain CFG: {p:.1f} dB"


def test_identical_branches_are_the_plain_path_bit_for_bit(hip_ops):
    """Both branches on one context, sequential forwards: c == u bit for bit, sum u^2 > 1 on every step, so s rounds to exactly 1.0f
    and the latent is the plain call's."""
    box, dens = [], []

    def on_step(i, latent):
        m = box[0]
        dens.append(float((m.head_out[1][: m.plan.n_tok].double() ** 2).sum()))     # u after the scale: 1.0f * u

    setup = lambda m: (_sequential(m), box.append(m))                            # noqa: E731
    m, lat = engine_loop(hip_ops, setup=setup, prep=dict(graphs=False), dev=DEV, same_context=True, data=solver_inputs(), on_step=on_step)
    torch.cuda.synchronize()
    assert len(dens) == LOOP_STEPS and all(d > 1.0 for d in dens), dens
    assert m.guidance_scales == [1.0] * LOOP_STEPS, m.guidance_scales
    m0, lat0 = engine_loop(hip_ops, zero_star=False, setup=_sequential, prep=dict(graphs=False), dev=DEV, same_context=True, data=solver_inputs())
    torch.cuda.synchronize()
    assert m0.guidance_scales is None and m0._guidance_state is None and torch.equal(lat, lat0)


@pytest.mark.parametrize("solver", ["euler", "unipc"])
@pytest.mark.parametrize("k", [1, 2])
def test_zero_init_is_a_later_start(hip_ops, solver, k):
    seen = []
    m, lat = engine_loop(hip_ops, zero_star=False, k=k, solver=solver, dev=DEV, data=solver_inputs(), on_step=lambda i, x: seen.append(x.clone()))
    m0, lat0 = engine_loop(hip_ops, zero_star=False, solver=solver, dev=DEV, data=solver_inputs(), loop_steps=range(k, LOOP_STEPS))
    torch.cuda.synchronize()
    noise = solver_inputs()[2]
    assert torch.equal(lat, lat0) and len(seen) == LOOP_STEPS
    assert all(torch.equal(x.cpu(), noise) for x in seen[:k]) and not torch.equal(seen[k].cpu(), noise)
    assert m.guidance_scales == [None] * LOOP_STEPS and m._guidance_state is None


# ---- 5. compositions ------------------------------------------------------------------------------------------------------------------
def test_with_teacache_one_forced_skip(hip_ops):
    """Step 3 of 6 runs no blocks: the scale is taken on the skipped step's head outputs like on any other."""
    computed = (0, 1, 2, 4, 5)
    plan = lambda m, sch: teacache.TeaCachePlan("test-linear", 0.0, tuple(range(LOOP_STEPS)), (0.0,) * LOOP_STEPS, computed)      # noqa: E731
    m, lat = engine_loop(hip_ops, dev=DEV, tea=plan)
    torch.cuda.synchronize()
    ref = reference(True, tea_skipped=(3,))
    p = R.psnr(lat.cpu(), ref[0])
    print(f"CFG-Zero* + TeaCache (step 3 skipped) vs its restatement: {p:.1f} dB; scales {m.guidance_scales} vs {ref[1]}")
    assert p >= 40.0, f"{p:.1f} dB"
    assert m._tc_res is not None and not torch.equal(ref[0], reference(True)[0]), "the skip must change the restated result"


def test_with_unipc(hip_ops):
    m, lat = engine_loop(hip_ops, solver="unipc", dev=DEV)
    torch.cuda.synchronize()
    ref = reference(True, solver="unipc")
    p, p_plain = R.psnr(lat.cpu(), ref[0]), R.psnr(reference(False, solver="unipc")[0], ref[0])
    print(f"CFG-Zero* + UniPC vs its restatement: {p:.1f} dB (restated plain CFG + UniPC: {p_plain:.1f} dB); scales {m.guidance_scales} vs {ref[1]}")
    assert p >= 40.0, f"{p:.1f} dB"
    assert m._solver_state is not None and len(m.guidance_scales) == LOOP_STEPS


def test_with_the_e4m3_mode(hip_ops):
    """The six per-layer projections on the fp8 MFMA: the e4m3 mode's loop bar, >= 40 dB against the oracle run with the same e4m3 row
    quantisation (tests/test_dit_gpu.py test_fp8_gemm_mode_forward_and_loop), here with both combined by CFG-Zero*."""
    m, lat = engine_loop(hip_ops, dev=DEV, kw=dict(gemm_dtype="fp8", fp8_weights=WanDiT.FP8_WEIGHTS))
    torch.cuda.synchronize()
    ref8 = reference(True, fp8=True)
    p8, p = R.psnr(lat.cpu(), ref8[0]), R.psnr(lat.cpu(), reference(True)[0])
    print(f"CFG-Zero* e4m3 loop: vs fake-quant restatement {p8:.1f} dB, vs unquantised restatement {p:.1f} dB; scales {m.guidance_scales} vs {ref8[1]}")
    assert p8 >= 40.0, f"{p8:.1f} dB"


# ---- 6. the pipeline ------------------------------------------------------------------------------------------------------------------
def _pipe():
    from infinicube_amd.videogen.ops import HipOps
    from infinicube_amd.videogen.pipeline import DiTHolder, WanVideoPipeline
    from standins import HashTextEncoder, PoolVAE
    return WanVideoPipeline(DEV, torch.bfloat16, DiTHolder(syn.make_dit_state_dict(CFG), CFG), HashTextEncoder(CFG), PoolVAE(), ops=HipOps(DEV))


def test_pipeline(monkeypatch):
    for key in ENV:
        monkeypatch.delenv(key, raising=False)
    kw = dict(prompt="a street", negative_prompt="bad", height=GRID.height, width=GRID.width, num_frames=GRID.num_frames, seed=3,
              num_inference_steps=6, return_latents=True)
    p = _pipe()
    n, k = 6, 2
    lat = p(**kw, cfg_zero_star=True, cfg_zero_init_steps=k).cpu()
    rec = p.guidance_record
    assert rec["optimized_scale"] is True and rec["zero_init_steps"] == k and rec["scales"][:k] == [None] * k
    assert len(rec["scales"]) == n and len(rec["scales"][k:]) == n - k and all(math.isfinite(s) for s in rec["scales"][k:])
    plain = p(**kw).cpu()                                                        # the keywords do not outlive their call
    assert p.guidance_record is None
    fresh = _pipe()(**kw).cpu()
    assert torch.equal(plain, fresh), "a call without the keywords must give a fresh pipeline's bits"
    assert torch.isfinite(lat).all() and not torch.equal(lat, fresh)
