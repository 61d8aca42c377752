"""Normalized Attention Guidance on the HIP path (csrc/nag.hip, icv_nag_combine_bf16): the kernel against the float64 restatement
(tests/nag_ref.py) at every wave layout it has and at a width icv_ln_modulate has no kernel for, its write guard, in place, the exact
and the zero-row cases, the refused calls; the loop of tests/test_nag_cpu.py on the per-op, graph and one-call drivers, a second graph
key, the compositions (UniPC, a forced TeaCache skip, the frame window, the e4m3 mode, an image-to-video DiT), and the pipeline.

Kernel shapes are (rows, d, ld).  A row is owned by 1 wave up to d = 2048, by 2 up to 4096, by 4 above; a lane holds at most four
16-byte vectors per input, so d = 256 (half a wave live), 1536 and 2304 (a dead vector slot), 5120 (a half-live slot, waves of one row
with different loads) and 8192 (every slot full) are the distinct cases; 4099 rows leave the last work-group one live row of four."""
import pytest
import torch

from infinicube_amd.videogen import synthetic as syn
from infinicube_amd.videogen import teacache
from infinicube_amd.videogen.config import TokenGrid, preset
from infinicube_amd.videogen.dit import WanDiT
from infinicube_amd.videogen.nag import NagPlan
from infinicube_amd.videogen.scheduler import FlowMatchScheduler, flow_match_sigmas
from nag_ref import BF16, NagForward, nag_rule, nag_velocity
from oracle import wan_ref as R
from test_nag_cpu import CFG, ENV, GAINS, GRID, LOOP_STEPS, NAG, check_loop, engine_loop, reference
from test_solver_cpu import restated_sample

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
SENTINEL = -7.0
PAD = 64                     # elements in front of and behind every allocation's rows
SHAPES = [(1, 256, 256), (5, 1536, 1536), (7, 2304, 2304), (67, 5120, 5136), (3, 8192, 8192), (4099, 1536, 1544)]
NOISE_CYCLE = (0.0, 0.05, 0.25, 1.0)

_DATA = {}


def data(rows, d):
    """p bf16 normal, n = p + e_r noise with e_r cycling through NOISE_CYCLE by row, and the float64 rule on them, once per shape."""
    if (rows, d) not in _DATA:
        g = torch.Generator().manual_seed(2000 + rows + d)
        p = torch.randn((rows, d), generator=g).to(BF16)
        e = torch.tensor([NOISE_CYCLE[r % 4] for r in range(rows)])[:, None]
        n = (p.float() + e * torch.randn((rows, d), generator=g)).to(BF16)
        _DATA[(rows, d)] = (p, n) + nag_rule(p, n, *NAG)
    return _DATA[(rows, d)]


def device_rows(values, ld):
    """[rows, d] bf16 -> (view [rows, d] with row stride ld inside a sentinel-filled allocation, the allocation)."""
    rows, d = values.shape
    flat = torch.full((PAD + rows * ld + PAD,), SENTINEL, dtype=BF16, device=DEV)
    view = flat[PAD: PAD + rows * ld].view(rows, ld)[:, :d]
    view.copy_(values.to(DEV))
    assert view.data_ptr() % 16 == 0
    return view, flat


def guard_ok(view, flat, ld):
    rows, d = view.shape
    body = flat[PAD: PAD + rows * ld].view(rows, ld)
    return bool((body[:, d:] == SENTINEL).all() and (flat[:PAD] == SENTINEL).all() and (flat[-PAD:] == SENTINEL).all())


def run_kernel(hip_ops, p, n, ld, in_place=False, nag=NAG):
    (zp, fp), (zn, fn) = device_rows(p, ld), device_rows(n, ld)
    out, fo = (zp, fp) if in_place else device_rows(torch.full_like(p, SENTINEL), ld)
    hip_ops.nag_combine(zp, zn, out, *nag)
    torch.cuda.synchronize()
    assert guard_ok(zp, fp, ld) and guard_ok(zn, fn, ld) and guard_ok(out, fo, ld), "written outside [rows, d]"
    assert torch.equal(zn.cpu(), n) and (in_place or torch.equal(zp.cpu(), p)), "an input was written"
    return out.cpu()


# ---- 1. the kernel against float64 ----------------------------------------------------------------------------------------------------
def test_inputs_are_clipped_and_unclipped():
    """At least a quarter of the rows clipped and at least a quarter not - per shape where it has more than one row (one row cannot be
    both: (1, 256) draws e = 0 and is not clipped), and over all shapes' rows together."""
    clipped = total = 0
    for rows, d, _ in SHAPES:
        c = data(rows, d)[3]
        k = int((c < 1.0).sum())
        print(f"{(rows, d)}: {k} of {rows} rows clipped")
        clipped, total = clipped + k, total + rows
        if rows > 1:
            assert 4 * k >= rows and 4 * (rows - k) >= rows, (rows, d, k)
    assert 4 * clipped >= total and 4 * (total - clipped) >= total


@pytest.mark.parametrize("rows,d,ld", SHAPES)
def test_kernel_matches_float64(hip_ops, rows, d, ld):
    """|got - r| <= 2^-8 |r| + 2^-10 (alpha c |g| + (1 - alpha) |p|) per element against the unrounded float64 value r: one bf16
    rounding, plus twice the worst-case f32 error of an 8192-term L1 sum (2^-11) carried into each addend - the blend can cancel, so
    a bound in ulps of r alone would be wrong."""
    p, n, ref, c, g = data(rows, d)
    _, _, alpha = NAG
    got = run_kernel(hip_ops, p, n, ld).double()
    tol = 2.0 ** -8 * ref.abs() + 2.0 ** -10 * (alpha * c * g.abs() + (1.0 - alpha) * p.double().abs())
    err = (got - ref).abs()
    worst = float((err / tol.clamp_min(1e-300)).max())
    print(f"{(rows, d, ld)}: max |err| / tolerance = {worst:.3f}, max |err| = {float(err.max()):.3e}")
    assert bool((err <= tol).all()), f"{(rows, d, ld)}: max |err| / tolerance = {worst:.3f}"
    # in place gives the same bits
    assert torch.equal(run_kernel(hip_ops, p, n, ld, in_place=True).double(), got)


def test_equal_inputs_and_zero_rows(hip_ops):
    for rows, d, ld in ((5, 1536, 1536), (67, 5120, 5136)):
        p, n = data(rows, d)[:2]
        assert torch.equal(run_kernel(hip_ops, p, p.clone(), ld), p), "z_neg == z_pos must give z_pos bit for bit"
        pz = p.clone()
        pz[1] = 0
        got = run_kernel(hip_ops, pz, n, ld)
        assert torch.equal(got[1], torch.zeros_like(got[1])) and torch.isfinite(got.float()).all()
        both = run_kernel(hip_ops, torch.zeros_like(p), torch.zeros_like(p), ld)
        assert torch.equal(both, torch.zeros_like(p))


def test_refused_calls_leave_the_output_untouched(hip_ops):
    from infinicube_amd import native
    lib = native.lib()
    rows = 5
    good = torch.zeros((rows, 512), dtype=BF16, device=DEV)
    out = torch.full((rows, 512), SENTINEL, dtype=BF16, device=DEV)
    st = hip_ops._stream()
    with pytest.raises(ValueError, match="d % 256 == 0"):                        # a bad d
        hip_ops.nag_combine(good[:, :264], good[:, :264], out[:, :264], *NAG)
    assert lib.icv_nag_combine_bf16(good.data_ptr(), 512, good.data_ptr(), 512, out.data_ptr(), 512, rows, 264, 11.0, 2.5, 0.25, st) != 0
    assert b"d=264" in lib.icv_last_error()
    odd = torch.zeros((rows, 260), dtype=BF16, device=DEV)                       # a bad ld
    with pytest.raises(ValueError, match="multiples of 8"):
        hip_ops.nag_combine(good[:, :256], odd[:, :256], out[:, :256], *NAG)
    assert lib.icv_nag_combine_bf16(good.data_ptr(), 512, good.data_ptr(), 260, out.data_ptr(), 512, rows, 256, 11.0, 2.5, 0.25, st) != 0
    assert b"multiples of 8" in lib.icv_last_error()
    for bad in (dict(zp=good.float()), dict(zn=good.to(torch.float16)), dict(out=out.float())):      # wrong dtypes
        a = dict(zp=good, zn=good, out=out)
        a.update(bad)
        with pytest.raises(TypeError, match="nag_combine"):
            hip_ops.nag_combine(a["zp"], a["zn"], a["out"], *NAG)
    with pytest.raises(ValueError, match="one shape"):
        hip_ops.nag_combine(good, good[:4], out, *NAG)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()), "a refused call must not launch"


# ---- 2. the loop, per driver ----------------------------------------------------------------------------------------------------------
_PER_OP = {}


def per_op(hip_ops):
    if "v" not in _PER_OP:
        m, lat = engine_loop(hip_ops, prep=dict(graphs=False), dev=DEV)
        torch.cuda.synchronize()
        assert not m._graphs_on and m._nag_buf is not None and m._nag is None
        _PER_OP["v"] = lat.cpu()
    return _PER_OP["v"]


@pytest.mark.parametrize("mode", ["per-op", "graphs", "native"])
def test_loop_matches_restated_nag_loop(hip_ops, mode, monkeypatch):
    """The loop of test_nag_cpu on HipOps (tiny preset, 5 latent frames, cfg_scale 1, Euler, 6 steps, that file's gains)."""
    if mode == "per-op":
        lat = per_op(hip_ops)
    elif mode == "graphs":
        m, lat = engine_loop(hip_ops, prep=dict(graphs=True), dev=DEV)
        torch.cuda.synchronize()
        assert m._graphs_on and m._graphs
    else:
        monkeypatch.setenv("ICV_NATIVE_FORWARD", "1")
        m, lat = engine_loop(hip_ops, prep=dict(graphs=False), dev=DEV)
        torch.cuda.synchronize()
        assert m.native_forward and m._native is None, "the one-call driver does not know the launches: the per-op driver runs"
        assert torch.equal(lat.cpu(), per_op(hip_ops)), "... with the per-op driver's bits"
    assert torch.isfinite(lat).all()
    check_loop(lat, mode)
    p_plain = R.psnr(reference(None), reference())
    assert p_plain < 30.0, f"plain vs NAG {p_plain:.1f} dB: the bar could pass with the feature ignored"


def test_two_graph_keys(hip_ops):
    """One engine under graphs, the same contexts, buffer tokens and latent tensor in every call: a plain call, a NAG call and a NAG call
    with another nag_scale each match their own restatement - a graph captured for one is never replayed for another."""
    m, plain = engine_loop(hip_ops, nag=None, prep=dict(graphs=True), dev=DEV)
    torch.cuda.synchronize()
    assert m._graphs_on and len(m._graphs) == 1 and m._nag_buf is None
    check_loop(plain, "graphs, plain", ref=reference(None))
    _, first = engine_loop(hip_ops, engine=m)
    torch.cuda.synchronize()
    assert len(m._graphs) == 2
    check_loop(first, "graphs, nag_scale 11")
    other = (3.0, 2.5, 0.25)                 # restated: 30.9 dB from the default setting's loop, 28.7 dB from the plain loop
    _, second = engine_loop(hip_ops, nag=other, engine=m)
    torch.cuda.synchronize()
    assert len(m._graphs) == 3
    check_loop(second, "graphs, nag_scale 3", ref=reference(other))
    assert max(R.psnr(reference(other), reference()), R.psnr(reference(other), reference(None))) < 35.0, "a stale graph must miss the bar"
    _, again = engine_loop(hip_ops, engine=m)                                    # replayed
    torch.cuda.synchronize()
    assert len(m._graphs) == 3 and torch.equal(again, first)


def test_same_prompts_give_the_plain_call(hip_ops):
    _, lat = engine_loop(hip_ops, same_context=True, prep=dict(graphs=False), dev=DEV)
    m0, lat0 = engine_loop(hip_ops, nag=None, prep=dict(graphs=False), dev=DEV)
    torch.cuda.synchronize()
    assert m0._nag_buf is None and torch.equal(lat, lat0)
    assert not torch.equal(lat0.cpu(), per_op(hip_ops))


# ---- 3. compositions ------------------------------------------------------------------------------------------------------------------
def test_with_unipc(hip_ops):
    m, lat = engine_loop(hip_ops, solver="unipc", dev=DEV)
    torch.cuda.synchronize()
    check_loop(lat, "NAG + UniPC", ref=reference(solver="unipc"))
    assert m._solver_state is not None


def test_with_teacache_one_forced_skip(hip_ops):
    """Step 3 of 6 runs no blocks, so no cross-attention and no combine: the residual of step 2 (computed with NAG) is added."""
    computed = (0, 1, 2, 4, 5)
    plan = lambda m, sch: teacache.TeaCachePlan("test-linear", 0.0, tuple(range(LOOP_STEPS)), (0.0,) * LOOP_STEPS, computed)      # noqa: E731
    m, lat = engine_loop(hip_ops, dev=DEV, tea=plan)
    torch.cuda.synchronize()
    ref = reference(tea_skipped=(3,))
    check_loop(lat, "NAG + TeaCache (step 3 skipped)", ref=ref)
    assert m._tc_res is not None and not torch.equal(ref, reference()), "the skip must change the restated result"


def test_with_the_frame_window(hip_ops):
    """Window 1 + 1 anchor frame (tests/test_attn_window_gpu.py's setting and bar): the masked restatement with the NAG step."""
    m, lat = engine_loop(hip_ops, dev=DEV, prep=dict(graphs=False), setup=lambda m: m.set_attention_window(1, 1))
    torch.cuda.synchronize()
    assert m._framewin() == (1, 1)
    check_loop(lat, "NAG + frame window", ref=reference(window=(1, 1)))
    assert not torch.equal(lat.cpu(), per_op(hip_ops))


def test_with_the_e4m3_mode(hip_ops):
    """The six per-layer projections on the fp8 MFMA: the e4m3 mode's loop bar, >= 40 dB against the restatement run with the same e4m3
    row quantisation (tests/test_dit_gpu.py test_fp8_gemm_mode_forward_and_loop).  The combine's output is what cross-o quantises."""
    m, lat = engine_loop(hip_ops, dev=DEV, kw=dict(gemm_dtype="fp8", fp8_weights=WanDiT.FP8_WEIGHTS))
    torch.cuda.synchronize()
    p = R.psnr(lat.cpu(), reference())
    print(f"NAG e4m3 loop vs the unquantised restatement: {p:.1f} dB")
    check_loop(lat, "NAG + e4m3", ref=reference(fp8=True))


def test_with_an_image_to_video_dit(hip_ops):
    """tiny-i2v (tests/test_dit_gpu.py test_i2v_forward_and_loop_parity's config, steps and bar): the CLIP-token softmax is added after
    the combine, in the engine and in the restatement."""
    cfg, grid = preset("tiny-i2v"), TokenGrid(9, 64, 96)
    sd, bsd = syn.make_dit_state_dict(cfg), syn.make_buffer_embedder_state_dict(cfg)
    for k in [k for k in sd if k.endswith("cross_attn.o.weight")]:
        sd[k] = sd[k] * GAINS["cross_attn_o"]
    noise, c1 = syn.make_latent_noise(grid), syn.make_text_context(cfg, 1)
    cp = c1 * GAINS["cond_context"]
    cn = (torch.randn(c1.shape, generator=torch.Generator().manual_seed(5)) * float(c1.std()) * GAINS["neg_context"]).to(c1.dtype)
    bl, clip, y = syn.make_buffer_latents(cfg, grid), syn.make_clip_features(cfg), syn.make_cond_latents(cfg, grid)
    m = WanDiT(cfg, sd, hip_ops, bsd).prepare(grid, graphs=False)
    ck, ckn = m.encode_context(cp, clip), m.encode_context(cn, clip)
    add = m.embed_cond_latents(y, add_to=m.embed_buffers(bl))
    steps = 6
    lat = noise.to(DEV)
    m.denoise(lat, ck, None, add, FlowMatchScheduler(steps), 1.0, nag=NagPlan(ckn, *NAG))
    torch.cuda.synchronize()
    sdr, bsdr = R.round_state_dict_to_bf16(sd), R.round_state_dict_to_bf16(bsd)
    sigmas = flow_match_sigmas(steps)
    refs = [restated_sample(nag_velocity(NagForward(sdr, cfg, cp, cn, nag, R.buffer_embed(bsdr, bl), clip_fea=clip, y=y), sigmas),
                            noise.double(), sigmas, "euler").float() for nag in (NAG, None)]
    p, p_plain = R.psnr(lat.cpu(), refs[0]), R.psnr(refs[1], refs[0])
    print(f"NAG i2v loop vs its restatement: {p:.1f} dB; restated plain i2v loop vs restated NAG i2v loop: {p_plain:.1f} dB")
    assert p >= 40.0, f"{p:.1f} dB"
    assert p_plain <= p - 10.0, f"the bar cannot tell NAG from the plain loop here: plain {p_plain:.1f} dB, engine {p:.1f} dB"


# ---- 4. the pipeline ------------------------------------------------------------------------------------------------------------------
def _pipe():
    from infinicube_amd.videogen.ops import HipOps
    from infinicube_amd.videogen.pipeline import DiTHolder, WanVideoPipeline
    from standins import HashTextEncoder, PoolVAE
    return WanVideoPipeline(DEV, torch.bfloat16, DiTHolder(syn.make_dit_state_dict(CFG), CFG), HashTextEncoder(CFG), PoolVAE(), ops=HipOps(DEV))


def test_pipeline(monkeypatch):
    for key in ENV:
        monkeypatch.delenv(key, raising=False)
    kw = dict(prompt="a street", negative_prompt="bad", height=GRID.height, width=GRID.width, num_frames=GRID.num_frames, seed=3,
              num_inference_steps=4, return_latents=True, cfg_scale=1.0)
    p = _pipe()
    lat = p(**kw, nag_scale=11.0).cpu()
    assert p.nag_record == dict(scale=11.0, tau=2.5, alpha=0.25)
    plain = p(**kw).cpu()                                                        # the keyword does not outlive its call
    assert p.nag_record is None
    fresh = _pipe()(**kw).cpu()
    assert torch.equal(plain, fresh), "a call without the keywords must give a fresh pipeline's bits"
    assert torch.isfinite(lat).all() and not torch.equal(lat, fresh), "nag_scale must not be swallowed"
    same = p(**dict(kw, negative_prompt=kw["prompt"]), nag_scale=11.0).cpu()
    assert torch.equal(same, fresh), "negative_prompt == prompt gives the plain call's bits"
