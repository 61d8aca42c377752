"""EasyCache on the HIP path (csrc/easycache.hip): icv_l1_change_f64 against float64 at the shapes where its grid, its sweeps and its
two load paths change (bound derived from the arithmetic), its write guards and its determinism; icv_easycache_predict_f32 bit for bit
against the torch twin; the operator layer's checks; the loop of tests/test_easycache_cpu.py in every driver mode against the float64
restatement (same decisions, the loop bar), the head outputs of a forced skip bit for bit; the compositions and the pipeline.

icv_l1_change_f64's shapes are (rows, cols, ld of both operands, b's offset in floats): the six of tests/test_cfg_zero_gpu.py (the same
quad / 256 threads / at most 256 blocks geometry: one sweep covers 262 144 elements), the tiny latent as one row and a ragged row of
more than one sweep."""
import pytest
import torch

from infinicube_amd.videogen import easycache as E
from infinicube_amd.videogen import synthetic as syn
from infinicube_amd.videogen import teacache
from infinicube_amd.videogen.dit import WanDiT
from infinicube_amd.videogen.scheduler import FlowMatchScheduler
from oracle import wan_ref as R
from test_cfg_zero_gpu import PAD, SENTINEL, SHAPES, device_rows, guard_ok
from test_easycache_cpu import (CASES, CFG, CFG_SCALE, ENV, GRID, STEPS, WARMUP, check_loop, check_trace, engine_loop, forced_reference,
                                head_layout, inputs, predict_twin, reference)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
WORKSPACE = 512
L1_SHAPES = SHAPES + [
    (1, 4608, 4608, 0),      # the tiny latent [16, 3, 8, 12] as one row
    (1, 70001, 70001, 0),    # one ragged row (a last quad of one element): the scalar path, 69 blocks
    (1, 300004, 300004, 0),  # one row of more than one sweep on the 16-byte path (75 001 quads > 65 536 threads)
]

_DATA = {}


def data(rows, cols):
    """a = randn, b = a + 0.3 randn, and the two float64 sums with their bounds, once per (rows, cols).

    The bound.  |a_j| is exact in fp64; a_j - b_j is formed in fp64 from two f32 values with at most one rounding (2^-53 relative).
    Any summation order of n terms then has an error of at most (n - 1) 2^-53 sum |terms| to first order - the kernel's order and the
    reference's each - so n 2^-52 sum |terms| per sum covers both and the terms' own rounding (the argument of moments(),
    tests/test_cfg_zero_gpu.py)."""
    if (rows, cols) not in _DATA:
        g = torch.Generator().manual_seed(2000 + rows + cols)
        a = torch.randn((rows, cols), generator=g)
        b = a + 0.3 * torch.randn((rows, cols), generator=g)
        d, s = float((a.double() - b.double()).abs().sum()), float(a.double().abs().sum())
        n = a.numel()
        _DATA[(rows, cols)] = (a, b, (d, s), (n * 2.0 ** -52 * d, n * 2.0 ** -52 * s))
    return _DATA[(rows, cols)]


def run_l1(hip_ops, a, b, ld, offset, update_b):
    rows, cols = a.shape
    (av, a_flat), (bv, b_flat) = device_rows(a, ld), device_rows(b, ld, offset)
    work = torch.full((WORKSPACE + 8,), float(SENTINEL), dtype=F64, device=DEV)
    out = torch.full((4,), float(SENTINEL), dtype=F64, device=DEV)
    hip_ops.l1_change(av[:rows, :cols], bv[:rows, :cols], work[:WORKSPACE], out[1:3], update_b=update_b)
    torch.cuda.synchronize()
    assert torch.equal(av[:rows, :cols].cpu(), a), "a was written"
    assert guard_ok(av, a_flat, rows, cols, 0) and guard_ok(bv, b_flat, rows, cols, offset), "written outside [rows, cols]"
    assert (work[WORKSPACE:] == SENTINEL).all() and out[0] == SENTINEL and out[3] == SENTINEL, "written outside the workspace / the output slot"
    return out[1:3].cpu(), bv[:rows, :cols].cpu()


# ---- 1. icv_l1_change_f64 against float64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols,ld,offset", L1_SHAPES)
def test_l1_change_matches_float64(hip_ops, rows, cols, ld, offset):
    a, b, ref, bound = data(rows, cols)
    got, b_after = run_l1(hip_ops, a, b, ld, offset, update_b=False)
    for name, g, r, bd in zip(("sum|a - b|", "sum|a|"), got.tolist(), ref, bound):
        print(f"{(rows, cols, ld, offset)}: {name} = {g:.12e}, float64 {r:.12e}, |err| {abs(g - r):.2e}, bound {bd:.2e}")
        assert abs(g - r) <= bd, f"{name}: |err| = {abs(g - r):.3e} > {bd:.3e}"
    assert torch.equal(b_after, b), "without update_b, b is read only"
    got_u, b_upd = run_l1(hip_ops, a, b, ld, offset, update_b=True)
    assert torch.equal(got_u, got), "update_b must not change the sums"
    assert torch.equal(b_upd, a), "with update_b, b ends bit-equal to a inside [rows, cols]"
    # the same bits on a second run, in fresh allocations
    again, _ = run_l1(hip_ops, a, b, ld, offset, update_b=False)
    assert torch.equal(again, got)


def test_l1_change_alignment_and_stride_do_not_change_the_bits(hip_ops):
    """The assignment of elements to threads is a function of (rows, cols) alone: the 16-byte path and the scalar path add in the
    same order."""
    for rows, cols, variants in ((4099, 64, ((64, 0), (64, 1), (68, 0), (65, 3))), (23, 64, ((64, 0), (72, 2))), (1, 4608, ((4608, 0), (4608, 1)))):
        a, b, _, _ = data(rows, cols)
        got = [run_l1(hip_ops, a, b, ld, off, update_b=upd)[0] for ld, off in variants for upd in (False, True)]
        assert all(torch.equal(g, got[0]) for g in got[1:])


def test_l1_change_equal_operands(hip_ops):
    a = data(23, 64)[0]
    got, _ = run_l1(hip_ops, a, a.clone(), 72, 0, update_b=False)
    assert float(got[0]) == 0.0 and float(got[1]) > 0.0


# ---- 2. icv_easycache_predict_f32 bit-equal to the torch twin --------------------------------------------------------------------------
PREDICT = [((3, 8, 12), 0, 72), ((3, 8, 12), 5, 50), ((2, 6, 10), 0, 30)]


@pytest.mark.parametrize("two", [True, False])
@pytest.mark.parametrize("ldh", [64, 72])
@pytest.mark.parametrize("grid,tok0,n_tok", PREDICT)
def test_predict_is_the_twin_bit_for_bit(hip_ops, grid, tok0, n_tok, ldh, two):
    C, (T, H8, W8) = 16, grid
    g = torch.Generator().manual_seed(31 + T + tok0)
    x, x_last = torch.randn((C, T, H8, W8), generator=g), torch.randn((C, T, H8, W8), generator=g)
    rows = n_tok + 3                                             # rows behind the range, pad columns where ldh > 64

    def head(fill=None):
        t = torch.full((rows, ldh), SENTINEL, dtype=F32)
        if fill is not None:
            t[:n_tok, :64] = torch.randn((n_tok, 64), generator=fill)
        return t

    hcl, hul, hc, hu = head(g), head(g), head(), head()
    want_c, want_u = hc.clone(), hu.clone()
    predict_twin(x, x_last, hcl, hul if two else None, want_c, want_u if two else None, tok0, n_tok)
    dev = [t.to(DEV) for t in (x, x_last, hcl, hul, hc, hu)]
    hip_ops.easycache_predict(dev[0], dev[1], dev[2], dev[3] if two else None, dev[4], dev[5] if two else None, tok0, n_tok)
    torch.cuda.synchronize()
    assert torch.equal(dev[4].cpu(), want_c) and torch.equal(dev[5].cpu(), want_u), "h = h_last + P(x - x_last), sentinels elsewhere"
    assert bool((want_c[:n_tok, :64] != SENTINEL).all()) and bool((want_c[n_tok:] == SENTINEL).all()) and bool((want_c[:, 64:] == SENTINEL).all())
    for t, host in zip(dev[:4], (x, x_last, hcl, hul)):
        assert torch.equal(t.cpu(), host), "x, x_last and h_last are read only"
    # the twin's layout is unpatchify_cfg_euler's, read in the other direction
    assert torch.equal(R.unpatchify(head_layout(x - x_last), (T, H8 // 2, W8 // 2), C), x - x_last)


def test_predict_unaligned_heads_take_the_scalar_path_with_the_same_bits(hip_ops):
    C, T, H8, W8 = 16, 3, 8, 12
    g = torch.Generator().manual_seed(5)
    x, x_last, hcl = torch.randn((C, T, H8, W8), generator=g), torch.randn((C, T, H8, W8), generator=g), torch.randn((72, 64), generator=g)
    outs = []
    for off, ldh in ((0, 64), (1, 64), (0, 65)):
        flat_l = torch.zeros((off + 72 * ldh + PAD,), device=DEV)
        flat_o = torch.full((off + 72 * ldh + PAD,), SENTINEL, device=DEV)
        hl, ho = flat_l[off: off + 72 * ldh].view(72, ldh), flat_o[off: off + 72 * ldh].view(72, ldh)
        hl[:, :64] = hcl.to(DEV)
        hip_ops.easycache_predict(x.to(DEV), x_last.to(DEV), hl, None, ho, None, 0, 72)
        torch.cuda.synchronize()
        assert bool((flat_o[:off] == SENTINEL).all()) and bool((flat_o[-PAD:] == SENTINEL).all()) and bool((ho[:, 64:] == SENTINEL).all())
        outs.append(ho[:, :64].cpu())
    assert torch.equal(outs[0], hcl + head_layout(x - x_last)) and all(torch.equal(o, outs[0]) for o in outs[1:])


# ---- 3. the operator layer's argument checks --------------------------------------------------------------------------------------------
def test_operator_layer_checks(hip_ops):
    a, b, _, _ = data(23, 64)
    da, db = a.to(DEV), b.to(DEV)
    work, out = torch.zeros(WORKSPACE, dtype=F64, device=DEV), torch.full((2,), float(SENTINEL), dtype=F64, device=DEV)
    with pytest.raises(TypeError):
        hip_ops.l1_change(da, db.double(), work, out)
    with pytest.raises(TypeError):
        hip_ops.l1_change(da, db, work.float(), out)
    with pytest.raises(TypeError):
        hip_ops.l1_change(da, db, work, out.float())
    with pytest.raises(ValueError, match="one non-empty shape"):
        hip_ops.l1_change(da, db[:22], work, out)
    with pytest.raises(ValueError, match="one non-empty shape"):
        hip_ops.l1_change(da.view(-1), db.view(-1), work, out)
    with pytest.raises(ValueError, match="workspace must hold"):
        hip_ops.l1_change(da, db, work[:100], out)
    with pytest.raises(ValueError, match="workspace must hold"):
        hip_ops.l1_change(da, db, work, torch.zeros(3, dtype=F64, device=DEV))
    with pytest.raises(Exception, match="must not overlap"):
        hip_ops.l1_change(da, da, work, out, update_b=True)
    with pytest.raises(Exception, match="out2 lies inside the workspace"):
        hip_ops.l1_change(da, db, work, work[10:12])
    x = torch.zeros((16, 3, 8, 12), device=DEV)
    h = [torch.full((72, 64), SENTINEL, device=DEV) for _ in range(4)]
    with pytest.raises(TypeError):
        hip_ops.easycache_predict(x, x.double(), h[0], None, h[2], None, 0, 72)
    with pytest.raises(ValueError, match="contiguous"):
        hip_ops.easycache_predict(x, x[:, :2], h[0], None, h[2], None, 0, 48)
    with pytest.raises(ValueError, match="given together"):
        hip_ops.easycache_predict(x, x.clone(), h[0], h[1], h[2], None, 0, 72)
    with pytest.raises(ValueError, match="fewer rows than n_tok"):
        hip_ops.easycache_predict(x, x.clone(), h[0][:70], None, h[2], None, 0, 72)
    with pytest.raises(ValueError, match="buffers of their own"):
        hip_ops.easycache_predict(x, x.clone(), h[0], None, h[0], None, 0, 72)
    with pytest.raises(Exception, match="token range"):
        hip_ops.easycache_predict(x, x.clone(), h[0], None, h[2], None, 1, 72)
    with pytest.raises(ValueError, match="at most 8"):
        hip_ops.read_doubles(work[:9])
    torch.cuda.synchronize()
    assert torch.equal(db.cpu(), b) and bool((out == SENTINEL).all()) and all(bool((t == SENTINEL).all()) for t in h), "a refused call must not launch"
    assert hip_ops.read_doubles(out) == [SENTINEL, SENTINEL]


# ---- 4. the loop, in every driver mode --------------------------------------------------------------------------------------------------
def _sequential(m):
    m.cfg_batch = False


def _mode(mode, monkeypatch):
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
    return prep, setup


@pytest.mark.parametrize("mode", ["per-op", "pair", "pair-no-stem", "native", "graphs", "dual-stream"])
def test_loop_matches_restatement(hip_ops, mode, monkeypatch):
    """The loop of test_easycache_cpu on HipOps: the same inputs and threshold, the restatement's decisions, the loop bar.  The GPU's
    sums are printed next to the restatement's (check_loop)."""
    ref = reference("plain")
    check_trace(ref, CASES["plain"]["thresh"], "plain")
    prep, setup = _mode(mode, monkeypatch)
    reads, raw = [], hip_ops.read_doubles
    monkeypatch.setattr(hip_ops, "read_doubles", lambda t: (reads.append(t.numel() * 8), raw(t))[1])
    m, lat, plan = engine_loop(hip_ops, dev=DEV, setup=setup, prep=prep)
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
    check_loop(lat, plan, ref, mode)
    assert reads == [64] * STEPS, "one blocking read of at most 64 bytes per executed step"
    # a computed step is today's computed step: with a threshold nothing stays under, the plain loop's bits in the same mode
    m2, every, p2 = engine_loop(hip_ops, dev=DEV, setup=setup, prep=prep, thresh=1e-12)
    cfg, sd, bsd, noise, c1, c2, bl, _, _ = inputs()
    m3 = WanDiT(cfg, sd, hip_ops, bsd).prepare(GRID, **prep)
    if setup is not None:
        setup(m3)
    plain = noise.clone().to(DEV)
    m3.denoise(plain, m3.encode_context(c1), m3.encode_context(c2), m3.embed_buffers(bl), FlowMatchScheduler(STEPS), CFG_SCALE)
    torch.cuda.synchronize()
    assert p2.skipped == [] and m3._easy_state is None and torch.equal(every, plain) and not torch.equal(lat, plain)


def test_force_skip_head_outputs_bit_for_bit(hip_ops, monkeypatch):
    """Steps 3 and 5 skip whatever the sums say.  Around each predict launch the device tensors are cloned: the head outputs are
    h_last + P(x - x_last) formed in torch on the device, bit for bit, for both branches."""
    raw, seen = hip_ops.easycache_predict, []

    def spy(x, x_last, hc_last, hu_last, hc, hu, tok0, n_tok):
        raw(x, x_last, hc_last, hu_last, hc, hu, tok0, n_tok)
        d = head_layout(x - x_last)[tok0: tok0 + n_tok]
        seen.append((torch.equal(hc[:n_tok], hc_last[:n_tok] + d), torch.equal(hu[:n_tok], hu_last[:n_tok] + d), bool(d.abs().max() > 0)))

    monkeypatch.setattr(hip_ops, "easycache_predict", spy)
    m, lat, plan = engine_loop(hip_ops, dev=DEV, prep=dict(graphs=False), force_skip=(3, 5), thresh=1e-12)
    torch.cuda.synchronize()
    want = forced_reference()
    assert plan.skipped == [3, 5] == want["skipped"] and seen == [(True, True, True)] * 2
    p = R.psnr(lat.cpu(), want["lat"])
    print(f"force_skip (3, 5): engine vs restatement {p:.1f} dB")
    assert p >= 40.0, f"{p:.1f} dB"


# ---- 5. compositions ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["unipc", "zero", "mask", "nag", "i2v", "subrange"])
def test_with(hip_ops, case):
    ref = reference(case)
    check_trace(ref, CASES[case]["thresh"], case)
    m, lat, plan = engine_loop(hip_ops, case, dev=DEV)
    torch.cuda.synchronize()
    check_loop(lat, plan, ref, case)
    if case == "unipc":
        assert m._solver_state is not None
    if case == "zero":
        assert m.guidance_scales[0] is None and len(m.guidance_scales) == STEPS


def test_with_the_e4m3_mode(hip_ops):
    """The six per-layer projections on the fp8 MFMA, against the restatement run with the same e4m3 row quantisation."""
    ref = reference("plain", fp8=True)
    check_trace(ref, CASES["plain"]["thresh"], "plain, e4m3")
    m, lat, plan = engine_loop(hip_ops, dev=DEV, kw=dict(gemm_dtype="fp8", fp8_weights=WanDiT.FP8_WEIGHTS))
    torch.cuda.synchronize()
    check_loop(lat, plan, ref, "e4m3")


def test_teacache_together_with_easy_cache_raises(hip_ops):
    cfg, sd, bsd, noise, c1, c2, bl, _, _ = inputs()
    m = WanDiT(cfg, sd, hip_ops, bsd).prepare(GRID, graphs=False)
    lat = noise.clone().to(DEV)
    tea = teacache.TeaCachePlan("test-linear", 0.0, tuple(range(STEPS)), (0.0,) * STEPS, tuple(range(STEPS)))
    with pytest.raises(ValueError, match=r"easy_cache=\) cannot be combined with TeaCache"):
        m.denoise(lat, m.encode_context(c1), m.encode_context(c2), m.embed_buffers(bl), FlowMatchScheduler(STEPS), CFG_SCALE,
                  tea_cache=tea, easy_cache=E.EasyCachePlan(0.5, WARMUP))
    torch.cuda.synchronize()
    assert torch.equal(lat.cpu(), noise) and m._easy_state is None and m._tc_res is None


# ---- 6. the pipeline ----------------------------------------------------------------------------------------------------------------------
def _pipe(vae=None):
    from infinicube_amd.videogen.ops import HipOps
    from infinicube_amd.videogen.pipeline import DiTHolder, WanVideoPipeline
    from standins import HashTextEncoder, PoolVAE
    return WanVideoPipeline(DEV, torch.bfloat16, DiTHolder(syn.make_dit_state_dict(CFG), CFG), HashTextEncoder(CFG), vae or PoolVAE(), ops=HipOps(DEV))


def test_pipeline(monkeypatch):
    for key in ENV:
        monkeypatch.delenv(key, raising=False)
    kw = dict(prompt="a street", negative_prompt="bad", height=GRID.height, width=GRID.width, num_frames=GRID.num_frames, seed=3,
              num_inference_steps=6, return_latents=True)
    p = _pipe()
    lat = p(**kw, easy_cache_thresh=1e9, easy_cache_warmup_steps=2).cpu()
    rec = p.easy_cache_record
    assert rec["computed"] == [0, 1, 5] and rec["skipped"] == [2, 3, 4] and rec["thresh"] == 1e9 and rec["warmup_steps"] == 2
    assert rec["k"][:2] == [None, None] and all(k > 0 for k in rec["k"][2:]) and rec["accumulated"][5] is None
    assert all(a is not None and a > 0 for a in rec["accumulated"][2:5]) and rec["accumulated"][2] < rec["accumulated"][3] < rec["accumulated"][4]
    plain = p(**kw).cpu()                                                        # the keywords do not outlive their call
    assert p.easy_cache_record is None
    fresh = _pipe()(**kw).cpu()
    assert torch.equal(plain, fresh), "a call without the keywords must give a fresh pipeline's bits"
    assert torch.isfinite(lat).all() and not torch.equal(lat, fresh)
    p.easy_cache_thresh, p.easy_cache_warmup_steps = 1e9, 3                      # the attributes; a keyword wins over its attribute
    by_attr = p(**kw).cpu()
    assert p.easy_cache_record["computed"] == [0, 1, 2, 5] and not torch.equal(by_attr, lat)
    by_kw = p(**kw, easy_cache_warmup_steps=2).cpu()
    assert p.easy_cache_record["computed"] == [0, 1, 5] and torch.equal(by_kw, lat)


def test_generator_attribute_route(tmp_path, monkeypatch):
    """The caller of the unchanged WanVideoGenerator: gen.pipe.easy_cache_thresh."""
    from test_solver_cpu import CountingVAE, generator_through_env
    for key in ENV:
        monkeypatch.delenv(key, raising=False)
    vae = CountingVAE()
    g, sem, co = generator_through_env(lambda torch_dtype, device, model_configs: _pipe(vae), tmp_path, monkeypatch, GRID, DEV, ICV_SAMPLE_STEPS="6")
    plain = vae.last_decoded
    assert g.pipe.easy_cache_record is None
    g.pipe.easy_cache_thresh, g.pipe.easy_cache_warmup_steps = 1e9, 2
    video = g.generate(sem, co, prompt="a street", negative_prompt="bad", seed=3)
    assert len(video) == GRID.num_frames and g.pipe.easy_cache_record["skipped"] == [2, 3, 4] and not torch.equal(vae.last_decoded, plain)
