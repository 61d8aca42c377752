"""Coarse-to-fine sampling (infinicube_amd/videogen/coarse.py: ``coarse_steps`` / ``coarse_size``) on CPU: the rule's validation
and every refused combination before an operator runs, the TEST-ONLY torch twin of icv_latent_resize_noise_f32 against
``torch.nn.functional.interpolate`` under a derived bound, the pipeline on the oracle operator set against the two stages driven by
hand on fresh engines (bits; Euler, UniPC, CFG-Zero*) and against the rule restated on ``oracle.wan_ref`` (>= 40 dB), off = the
parent's calls, bits and ONE generator draw, and the kernel's host-side argument checks."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from infinicube_amd.videogen import coarse, guidance, solver
from infinicube_amd.videogen import synthetic as syn
from infinicube_amd.videogen.config import TokenGrid, preset
from infinicube_amd.videogen.dit import WanDiT
from infinicube_amd.videogen.pipeline import _video_to_tensor
from infinicube_amd.videogen.scheduler import FlowMatchScheduler
from oracle import wan_ref as R
from standins import HashImageEncoder
from test_cfg_zero_cpu import ZeroOps
from test_v2v_cpu import CFG, ENV, SHORT, TILES, CountingVAE, V2VOps, _call_kw, _pipe, add_noise_twin, make_clip, pil, rb, strength_sigmas

F32 = torch.float32
FINE = TokenGrid(9, 128, 192)          # latent planes 16 x 24, 288 tokens
SIZES = ((64, 96), (96, 128))          # exactly 2x (weights 0.25 / 0.75); ratios 4/3 and 3/2 (fractional weights, clamps at both borders)
SHORT_SIZE = (SHORT.height, SHORT.width)
U = 2.0 ** -24                         # the relative error of one f32 rounding


# ---- the TEST-ONLY twin of icv_latent_resize_noise_f32 -------------------------------------------------------------------------------
def axis_source(n_out, n_in, device="cpu", align_corners=False):
    """(i0, i1, l) per output index along one axis, one tensor op per rounding (include/icvideo.h): scale divided in f32,
    s = max((o + 0.5) * scale - 0.5, 0).  ``align_corners``: the deliberately mis-centred coordinates s = o * (n_in - 1) / (n_out - 1)."""
    o = torch.arange(n_out, dtype=F32, device=device)
    if align_corners:
        s = o * float(torch.tensor(float(n_in - 1), dtype=F32) / torch.tensor(float(max(n_out - 1, 1)), dtype=F32))
    else:
        scale = float(torch.tensor(float(n_in), dtype=F32) / torch.tensor(float(n_out), dtype=F32))
        s = ((o + 0.5) * scale - 0.5).clamp_min(0.0)
    i0 = s.floor().long().clamp_max(n_in - 1)
    i1 = (i0 + 1).clamp_max(n_in - 1)
    return i0, i1, s - i0.to(F32)


def resize_twin(x0, h_out, w_out, align_corners=False):
    """up(x0): f32 [..., h_in, w_in] -> [..., h_out, w_out], v = (1 - ly) ((1 - lx) a + lx b) + ly ((1 - lx) c + lx d)."""
    y0, y1, ly = axis_source(h_out, x0.shape[-2], x0.device, align_corners)
    c0, c1, lx = axis_source(w_out, x0.shape[-1], x0.device, align_corners)
    ly = ly[:, None]
    wy0, wx0 = 1.0 - ly, 1.0 - lx
    top, bot = x0[..., y0, :], x0[..., y1, :]
    t = wx0 * top[..., c0] + lx * top[..., c1]
    b = wx0 * bot[..., c0] + lx * bot[..., c1]
    return wy0 * t + ly * b


def resize_noise_twin(x0, noise_out, sigma, round_bf16=False, align_corners=False):
    """Torch twin of icv_latent_resize_noise_f32: noise_out <- add_noise(up(x0), noise_out, sigma), in place."""
    add_noise_twin(resize_twin(x0, *noise_out.shape[-2:], align_corners=align_corners), noise_out, noise_out, sigma, round_bf16)


class CoarseOps(V2VOps, ZeroOps):
    """The counting operator set of the video-to-video tests + the multistep and CFG-Zero* twins + the twin of this feature's kernel."""

    def latent_resize_noise(self, x0, noise_out, sigma, round_bf16=False):
        assert x0.dtype == noise_out.dtype == F32 and x0.shape[:-2] == noise_out.shape[:-2] and x0.data_ptr() != noise_out.data_ptr()
        resize_noise_twin(x0, noise_out, sigma, round_bf16)


def _env(monkeypatch):
    for k in ENV + ("ICV_GRAPHS", "ICV_DUAL_STREAM", "ICV_NATIVE_FORWARD", "ICV_CFG_BATCH", "ICV_SHARE_STEM"):
        monkeypatch.delenv(k, raising=False)


# ---- 1. the rule -----------------------------------------------------------------------------------------------------------------------
def test_validate():
    v = coarse.validate
    assert v(None, None, 50, 480, 832) is None and v(0, None, 50, 480, 832) is None
    assert v(25, None, 50, 480, 832) == (25, (240, 416))
    assert v(1, None, 2, 720, 1280) == (1, (352, 640))                 # 360 rounds DOWN to a multiple of 16
    assert v(49, (480, 416), 50, 480, 832) == (49, (480, 416))         # one dimension may stay
    assert v(3, [96, 128], 4, 128, 192) == (3, (96, 128))
    for bad in (True, False, 1.0, "2", -1, 50, 51):
        with pytest.raises(ValueError, match="coarse_steps must be an integer in"):
            v(bad, None, 50, 480, 832)
    with pytest.raises(ValueError, match="coarse_steps must be an integer in"):
        v(1, None, 1, 480, 832)                                        # N = 1 leaves no fine step
    for bad in (240, (240,), (240, 416, 1), (240.0, 416), (True, 416), "ab", (None, 416)):
        with pytest.raises(ValueError, match="coarse_size must be two integers"):
            v(2, bad, 50, 480, 832)
    for bad in ((250, 416), (240, 420), (0, 416), (-16, 416)):
        with pytest.raises(ValueError, match="multiples of 16"):
            v(2, bad, 50, 480, 832)
    for bad in ((496, 416), (240, 848)):
        with pytest.raises(ValueError, match="at most the call's size"):
            v(2, bad, 50, 480, 832)
    with pytest.raises(ValueError, match="strictly smaller"):
        v(2, (480, 832), 50, 480, 832)
    with pytest.raises(ValueError, match="multiples of 16"):
        v(2, None, 50, 16, 16)                                         # the default of a 16 x 16 call would be 0 x 0
    for off in (None, 0):
        with pytest.raises(ValueError, match="coarse_size given without coarse_steps"):
            v(off, (240, 416), 50, 480, 832)
    assert coarse.record(2, (64, 96), 0.5, (72, 288)) == dict(steps=2, size=(64, 96), sigma=0.5, tokens=(72, 288))


def test_refused_combinations_raise_before_any_operator(monkeypatch):
    _env(monkeypatch)
    ops = CoarseOps()
    p = _pipe(ops)
    kw = _call_kw(FINE, num_inference_steps=4)
    clip = pil(make_clip(FINE, 1))
    mask = np.ones((FINE.num_frames, FINE.height, FINE.width), dtype=np.uint8)
    cases = ((dict(tea_cache_l1_thresh=0.1), "coarse_steps cannot be combined with TeaCache"),
             (dict(easy_cache_thresh=0.05, easy_cache_warmup_steps=2), "coarse_steps cannot be combined with EasyCache"),
             (dict(input_video=clip, denoising_strength=0.6), "coarse_steps cannot be combined with input_video / input_mask"),
             (dict(input_video=clip, input_mask=mask), "coarse_steps cannot be combined with input_video / input_mask"),
             (dict(cfg_zero_init_steps=2), "cfg_zero_init_steps=2 must be less than coarse_steps=2"),
             (dict(coarse_size=(128, 192)), "strictly smaller"), (dict(coarse_size=(64, 100)), "multiples of 16"))
    for extra, msg in cases:
        with pytest.raises(ValueError, match=msg):
            p(**kw, coarse_steps=2, **extra)
    for bad in (4, True, 1.5):
        with pytest.raises(ValueError, match="coarse_steps must be an integer in"):
            p(**kw, coarse_steps=bad)
    with pytest.raises(ValueError, match="coarse_size given without coarse_steps"):
        p(**kw, coarse_size=(64, 96))
    long = TokenGrid(33, 128, 192)
    with pytest.raises(ValueError, match=r"coarse_steps cannot be combined with sliding_window_size \(more than one window\)"):
        p(**_call_kw(long, num_inference_steps=4), coarse_steps=2, sliding_window_size=4, sliding_window_stride=2)
    import torch.distributed as dist
    with monkeypatch.context() as mp:
        mp.setattr(dist, "is_initialized", lambda: True)
        mp.setattr(dist, "get_world_size", lambda *a: 2)
        mp.setattr(dist, "get_rank", lambda *a: 0)
        with pytest.raises(ValueError, match="coarse_steps cannot be combined with a process group of 2 ranks"):
            p(**kw, coarse_steps=2)
    assert p._engine is None and p.coarse_record is None and not ops.calls, dict(ops.calls)
    # the attributes are the keywords' fallback; a keyword of 0 switches an attribute off
    p.coarse_steps = 4
    with pytest.raises(ValueError, match="coarse_steps must be an integer in"):
        p(**kw)
    assert not ops.calls
    p(**kw, coarse_steps=0)
    assert p.coarse_record is None


def test_engine_refuses_what_it_can_observe():
    m = WanDiT(CFG, syn.make_dit_state_dict(CFG), CoarseOps(), syn.make_buffer_embedder_state_dict(CFG))
    with pytest.raises(ValueError, match="prepare"):
        m.coarse_engine(64, 96)
    m.prepare(FINE, force_sp=True)
    with pytest.raises(ValueError, match="cannot be combined with sequence / CFG-branch parallelism"):
        m.coarse_engine(64, 96)
    m.prepare(FINE)
    with pytest.raises(ValueError, match="not a coarser grid"):
        m.coarse_engine(128, 192)
    lo = m.coarse_engine(64, 96)
    assert lo.grid == TokenGrid(9, 64, 96) and lo is not m and lo.layers is m.layers and lo.x is not m.x
    m.prepare(FINE)                                                   # the next call's prepare: the twin stays
    assert m.coarse_engine(64, 96) is lo and m.coarse_engine(96, 128) is not lo


def test_scheduler_over_an_explicit_list():
    for rounding in (False, True):
        full = FlowMatchScheduler(7, 5.0, rounding)
        lo = FlowMatchScheduler.from_sigmas(full.sigmas[:3], rounding)
        assert lo.sigmas == full.sigmas[:3] and lo.timesteps == full.timesteps[:3] and lo.reference_rounding == rounding
        assert [lo.dsigma(i) for i in range(3)] == [full.dsigma(0), full.dsigma(1), -full.sigmas[2]]      # the last step goes to 0
    with pytest.raises(ValueError, match="empty"):
        FlowMatchScheduler.from_sigmas([])


# ---- 2. the twin against torch's bilinear resize -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=["2x", "fractional"])
def test_twin_against_interpolate(size):
    """Bound, from the formula: the twin and ``F.interpolate(mode="bilinear", align_corners=False)`` evaluate the same convex
    combination of four inputs; the value takes at most eight f32 roundings (1 - lx, 1 - ly, four products and two sums along the
    longest path), each relative 2^-24 on a term bounded by max|x0|; and the two may place the source coordinate one f32 ulp apart -
    an ulp at the largest output index times the largest neighbour difference of the input moves the value by at most that product.
    With sigma = 0 the noising is the identity (1 * v + 0 * z), so the bound is asserted bare; with sigma > 0 both sides run the SAME
    add-noise twin on values that differ by at most the bound, which scales it by (1 - sigma) and adds that twin's own three
    roundings on terms bounded by max|x0| + max|noise|.
    A wrong tap is off by a neighbour difference times a weight - O(1) on unit-variance planes, seven orders of magnitude above
    the bound - and a half-pixel convention off by one cell or centred on corners shifts every interior coordinate by up to a
    quarter to a half cell: the same order.  The mis-centred twin below shows it."""
    g = torch.Generator().manual_seed(size[0])
    h_in, w_in = size[0] // 8, size[1] // 8
    h_out, w_out = FINE.latent_hw
    x0 = torch.randn((16, 3, h_in, w_in), generator=g)
    noise = torch.randn((16, 3, h_out, w_out), generator=g)
    ref = F.interpolate(x0, size=(h_out, w_out), mode="bilinear", align_corners=False)
    m = float(x0.abs().max())
    nd = max(float((x0[..., 1:, :] - x0[..., :-1, :]).abs().max()), float((x0[..., :, 1:] - x0[..., :, :-1]).abs().max()))
    s_max = max(float((i0.to(F32) + l).max()) for i0, _, l in (axis_source(h_out, h_in), axis_source(w_out, w_in)))      # at the largest output index
    coord_ulp = float(torch.tensor(s_max, dtype=F32).nextafter(torch.tensor(float("inf"))) - s_max)
    bound = 8 * U * m + coord_ulp * nd
    for sigma in (0.0, 0.5, FlowMatchScheduler(4, 5.0).sigmas[2], 1.0):
        got, want, wrong = noise.clone(), torch.empty_like(noise), noise.clone()
        resize_noise_twin(x0, got, sigma)
        add_noise_twin(ref, noise, want, sigma)
        b = bound if sigma == 0.0 else (1.0 - sigma) * bound + 3 * U * (m + float(noise.abs().max()))
        err = float((got - want).abs().max())
        print(f"{size} sigma={sigma:.4f}: max |twin - interpolate| {err:.3e}, bound {b:.3e}")
        assert err <= b, (sigma, err, b)
        if sigma < 1.0:
            resize_noise_twin(x0, wrong, sigma, align_corners=True)
            assert float((wrong - want).abs().max()) > 1e3 * b, "a mis-centred resize must exceed the bound by orders of magnitude"
    # the weights of the exact 2x case, and the clamps at both borders of the fractional one
    y0, y1, ly = axis_source(h_out, h_in)
    if size == (64, 96):
        assert ly.tolist() == [0.0] + [0.25, 0.75] * (h_in - 1) + [0.25] and y0.tolist()[:4] == [0, 0, 0, 1]
    else:
        assert 0.0 < float(ly[2]) < 1.0 and float(ly[2]) not in (0.25, 0.5, 0.75)
    assert int(y0[0]) == int(y1[0] - 1) == 0 and float(ly[0]) == 0.0 and int(y0[-1]) == int(y1[-1]) == h_in - 1


@pytest.mark.parametrize("rounding", [False, True])
def test_same_size_twin_is_the_add_noise_twin(rounding):
    g = torch.Generator().manual_seed(5)
    x0, noise = torch.randn((3, 16, 24), generator=g), torch.randn((3, 16, 24), generator=g)
    for sigma in (0.0, 0.5, 0.8333333, 1.0):
        got, want = noise.clone(), torch.empty_like(noise)
        resize_noise_twin(x0, got, sigma, rounding)
        add_noise_twin(x0, noise, want, sigma, rounding)
        assert torch.equal(got, want)
    _, _, l = axis_source(24, 24)
    assert float(l.abs().max()) == 0.0                                 # ly = lx = 0 exactly


# ---- 3. the pipeline against the two stages driven by hand -------------------------------------------------------------------------------
def truncated(sch, k):
    """The first ``k`` steps of ``sch`` as a scheduler of their own, without the feature's constructor: the last step goes to 0."""
    lo = FlowMatchScheduler(len(sch.sigmas), 5.0, sch.reference_rounding)
    lo.sigmas, lo.timesteps = sch.sigmas[:k], sch.timesteps[:k]
    return lo


def drive_coarse_by_hand(pipe, ops, kw, k, size, solver_name=None, gd=None, resize_op=None, setup=None, prep=None, engine_kw=None,
                         stage_kw=None, cfg_scale=5.0, twin=False, seen=None):
    """What a coarse-to-fine call must amount to, spelled out on fresh engines over the pipeline's components: the two generator
    draws in order, the buffers (and an image-to-video DiT's conditioning) resized and encoded per stage, ``denoise`` over the
    truncated scheduler on an engine built for the coarse grid, the TWIN (or ``resize_op``), ``denoise(steps=range(K, N))``.
    ``stage_kw(engine)``: more ``denoise`` keywords per stage (NAG, Enhance-A-Video).  ``twin``: take the coarse engine from
    ``WanDiT.coarse_engine`` instead of building a second one.  -> (latent, guidance scales of both stages in step order)."""
    cfg, rr = pipe.dit.cfg, pipe.reference_rounding
    h, w, n = kw["height"], kw["width"], kw["num_inference_steps"]
    grids = (TokenGrid(kw["num_frames"], *size), TokenGrid(kw["num_frames"], h, w))
    bsd = pipe.buffer_embedder.state_dict() if pipe.buffer_embedder else None
    hi = WanDiT(cfg, pipe.dit.state_dict(), ops, bsd, **(engine_kw or {}))
    hi.prepare(grids[1], **(prep or {}))
    if setup is not None:
        setup(hi)
    if twin:
        lo = hi.coarse_engine(*size)
    else:
        lo = WanDiT(cfg, pipe.dit.state_dict(), ops, bsd, **(engine_kw or {}))
        lo.prepare(grids[0], **(prep or {}))
        if setup is not None:
            setup(lo)
    if seen is not None:
        seen.update(hi=hi, lo=lo)
    image = kw.get("input_image")
    clip_fea = pipe.image_encoder.encode_image(image) if image is not None else None
    ck = hi.encode_context(pipe.text_encoder.encode(kw["prompt"]), clip_fea)
    cu = hi.encode_context(pipe.text_encoder.encode(kw["negative_prompt"]), clip_fea) if cfg_scale != 1.0 else None
    g = torch.Generator().manual_seed(kw["seed"])
    lats = []
    for grid in grids:                                                  # the coarse noise is the FIRST draw
        z = torch.randn((1, 16) + grid.latent_shape()[1:], generator=g, dtype=F32)[0]
        lats.append(ops.to_device(rb(z) if rr else z, F32))
    bts = []
    for m, grid in zip((lo, hi), grids):
        enc = lambda fr: pipe.vae.encode(_video_to_tensor(fr, grid.height, grid.width), tiled=True, **TILES).to(F32)   # noqa: E731
        bt = None
        if "semantic_buffer_video" in kw:
            bt = m.embed_buffers(torch.cat([enc(kw["semantic_buffer_video"]), enc(kw["coordinate_buffer_video"])], dim=0))
        if image is not None:
            bt = m.embed_cond_latents(pipe._image_cond_latents(image, grid, True, TILES["tile_size"], TILES["tile_stride"]), add_to=bt)
        bts.append(bt)
    sch = FlowMatchScheduler(n, 5.0, rr)
    sch_lo = truncated(sch, k)
    plans = (lambda s: dict(solver=solver.MultistepPlan(solver_name, s.sigmas))) if solver_name else (lambda s: {})
    more = stage_kw or (lambda m: {})
    lo.denoise(lats[0], ck, cu, bts[0], sch_lo, cfg_scale, round_bf16=rr, guidance=gd, **plans(sch_lo), **more(lo))
    scales = list(lo.guidance_scales or [])
    (resize_op or resize_noise_twin)(lats[0], lats[1], sch.sigmas[k], rr)
    hi.denoise(lats[1], ck, cu, bts[1], sch, cfg_scale, steps=range(k, n), round_bf16=rr, guidance=gd, **plans(sch), **more(hi))
    return lats[1], scales + list(hi.guidance_scales or [])


@pytest.mark.parametrize("rounding", [False, True], ids=["exact", "reference-rounding"])
@pytest.mark.parametrize("size", SIZES, ids=["2x", "fractional"])
def test_pipeline_equals_the_stages_driven_by_hand(size, rounding, monkeypatch):
    _env(monkeypatch)
    ops, vae = CoarseOps(), CountingVAE()
    p = _pipe(ops, vae=vae)
    p.reference_rounding = rounding
    kw = _call_kw(FINE, num_inference_steps=4)
    plain = p(**kw)
    assert p.coarse_record is None and vae.encodes == 2 and ops.calls["latent_resize_noise"] == 0
    got = p(**kw, coarse_steps=2, coarse_size=size)
    assert vae.encodes == 6 and ops.calls["latent_resize_noise"] == 1            # one more encode of the two buffers, one launch
    s_lo = 3 * (size[0] // 16) * (size[1] // 16)                                 # 3 latent frames
    assert p.coarse_record == dict(steps=2, size=size, sigma=FlowMatchScheduler(4, 5.0).sigmas[2], tokens=(s_lo, 288))
    want, _ = drive_coarse_by_hand(p, CoarseOps(), kw, 2, size)
    assert torch.equal(got, want), f"max |d| {float((got - want).abs().max())}"
    assert tuple(got.shape) == FINE.latent_shape() and torch.isfinite(got).all() and not torch.equal(got, plain)
    assert not torch.equal(got, p(**kw, coarse_steps=1, coarse_size=size)) and p.coarse_record["steps"] == 1
    if size == SHORT_SIZE:                                                       # None = half of each dimension
        assert torch.equal(p(**kw, coarse_steps=2), got) and p.coarse_record["size"] == SHORT_SIZE
        p.coarse_steps, p.coarse_size = 2, SHORT_SIZE                            # the attributes, for the unchanged generator's caller
        assert torch.equal(p(**kw), got)
        p.coarse_steps = p.coarse_size = None
    # the twin engine is kept: a second call builds none
    twins = dict(p._engine._coarse_engines)
    assert set(twins) == {size + (9,)}
    again = p(**kw, coarse_steps=2, coarse_size=size)
    assert torch.equal(again, got) and all(p._engine._coarse_engines[k_] is e for k_, e in twins.items())
    if rounding:
        p.reference_rounding = False
        assert not torch.equal(got, p(**kw, coarse_steps=2, coarse_size=size)), "reference rounding must differ from the exact path"


def test_unipc_builds_one_plan_per_stage(monkeypatch):
    _env(monkeypatch)
    ops = CoarseOps()
    p = _pipe(ops)
    kw = _call_kw(FINE, num_inference_steps=4)
    got = p(**kw, coarse_steps=2, coarse_size=SHORT_SIZE, sample_solver="unipc")
    hand = CoarseOps()
    want, _ = drive_coarse_by_hand(p, hand, kw, 2, SHORT_SIZE, solver_name="unipc")
    assert torch.equal(got, want)
    assert p.coarse_record["steps"] == 2 and p.solver_record == dict(name="unipc", steps=4, orders=[1, 1, 1, 1])      # each stage's last step is a first-order one
    # the history starts anew at step K: no corrector there, and the coarse stage's last step predicts to sigma = 0 at order 1
    assert [a is None for _, a, _ in ops.multistep_calls] == [True, False, True, False]
    assert [s for s, _, _ in ops.multistep_calls] == FlowMatchScheduler(4, 5.0).sigmas
    assert not torch.equal(got, p(**kw, coarse_steps=2, coarse_size=SHORT_SIZE))


def test_cfg_zero_star_acts_in_both_stages_and_zero_init_in_the_coarse_one(monkeypatch):
    _env(monkeypatch)
    ops = CoarseOps()
    p = _pipe(ops)
    kw = _call_kw(FINE, num_inference_steps=4)
    got = p(**kw, coarse_steps=2, coarse_size=(96, 128), cfg_zero_star=True, cfg_zero_init_steps=1)
    want, scales = drive_coarse_by_hand(p, CoarseOps(), kw, 2, (96, 128), gd=guidance.GuidancePlan(True, 1))
    assert torch.equal(got, want)
    rec = p.guidance_record
    assert rec["optimized_scale"] and rec["zero_init_steps"] == 1 and rec["scales"] == scales
    assert len(scales) == 4 and scales[0] is None and all(isinstance(s, float) for s in scales[1:])
    assert len(ops.zero_calls) == 3 and p.coarse_record["size"] == (96, 128)


def test_image_to_video_conditions_once_per_grid(monkeypatch):
    _env(monkeypatch)
    from PIL import Image
    cfg = preset("tiny-i2v")
    p = _pipe(CoarseOps(), cfg=cfg, image_encoder=HashImageEncoder(cfg))
    kw = _call_kw(FINE, num_inference_steps=3, input_image=Image.fromarray(make_clip(FINE, 1)[0], mode="RGB"))
    got = p(**kw, coarse_steps=1, coarse_size=(96, 128))
    want, _ = drive_coarse_by_hand(p, CoarseOps(), kw, 1, (96, 128))
    assert torch.equal(got, want) and not torch.equal(got, p(**kw))


def test_progress_bar_wraps_the_range_once(monkeypatch):
    _env(monkeypatch)
    p = _pipe(CoarseOps())
    kw = _call_kw(FINE, num_inference_steps=4)
    seen, wrapped = [], []

    def bar(it):
        wrapped.append(it)
        for i in it:
            seen.append(i)
            yield i

    got = p(**kw, coarse_steps=3, coarse_size=SHORT_SIZE, progress_bar_cmd=bar)
    assert wrapped == [range(4)] and seen == [0, 1, 2, 3]
    assert torch.equal(got, p(**kw, coarse_steps=3, coarse_size=SHORT_SIZE))


# ---- 4. the pipeline against an independent restatement ------------------------------------------------------------------------------------
def coarse_reference(p, kw, k, size, shift=5.0, cfg_scale=5.0):
    """The rule restated on oracle.wan_ref in plain fp32: float64 sigmas, the oracle's own forwards at both grids, F.interpolate."""
    n = kw["num_inference_steps"]
    sd = R.round_state_dict_to_bf16(p.dit.state_dict())
    bsd = R.round_state_dict_to_bf16(p.buffer_embedder.state_dict())
    c1, c2 = p.text_encoder.encode(kw["prompt"]), p.text_encoder.encode(kw["negative_prompt"])
    grids = (TokenGrid(kw["num_frames"], *size), TokenGrid(kw["num_frames"], kw["height"], kw["width"]))
    g = torch.Generator().manual_seed(kw["seed"])
    noises = [torch.randn((1, 16) + gr.latent_shape()[1:], generator=g, dtype=F32)[0] for gr in grids]
    bufs = []
    for gr in grids:
        enc = lambda fr: p.vae.encode(_video_to_tensor(fr, gr.height, gr.width)).float()      # noqa: E731
        bufs.append(R.buffer_embed(bsd, torch.cat([enc(kw["semantic_buffer_video"]), enc(kw["coordinate_buffer_video"])], dim=0), F32))
    sig = [float(s) for s in strength_sigmas(n, shift, 1.0)]

    def step(x, i, buf, nxt):
        v_c = R.dit_forward(sd, CFG, x, c1, sig[i] * 1000.0, buf, F32)
        v_u = R.dit_forward(sd, CFG, x, c2, sig[i] * 1000.0, buf, F32)
        return x + (v_u + cfg_scale * (v_c - v_u)) * (nxt - sig[i])

    x = noises[0].clone()
    for i in range(k):
        x = step(x, i, bufs[0], sig[i + 1] if i + 1 < k else 0.0)               # the coarse stage's last step goes to 0: x0-prediction
    up = F.interpolate(x, size=grids[1].latent_hw, mode="bilinear", align_corners=False)      # [16, T, h, w]: planes (c, t), frames untouched
    x = (1.0 - sig[k]) * up + sig[k] * noises[1]
    for i in range(k, n):
        x = step(x, i, bufs[1], sig[i + 1] if i + 1 < n else 0.0)
    return x


@pytest.mark.parametrize("size", SIZES, ids=["2x", "fractional"])
def test_pipeline_matches_the_restated_rule(size, monkeypatch):
    """Bar: the one tests/test_v2v_cpu.py holds its pipeline to against its restated loop (>= 40 dB latent PSNR)."""
    _env(monkeypatch)
    p = _pipe(CoarseOps())
    kw = _call_kw(FINE, num_inference_steps=4)
    got = p(**kw, coarse_steps=2, coarse_size=size)
    ref = coarse_reference(p, kw, 2, size)
    db = R.psnr(got, ref)
    print(f"coarse-to-fine pipeline (K = 2 of 4, {size}) vs the restated rule: {db:.1f} dB")
    assert db >= 40.0, f"{db:.1f} dB"
    # the result provably went through the coarse stage: the plain call and another K are far away
    assert R.psnr(p(**kw), ref) < db - 10.0 and R.psnr(got, coarse_reference(p, kw, 1, size)) < db - 10.0


# ---- 5. off is off ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [None, 0])
def test_off_is_the_call_without_the_keyword(off, monkeypatch):
    _env(monkeypatch)
    kw = _call_kw(FINE, num_inference_steps=3)
    base_ops, base_vae = CoarseOps(), CountingVAE()
    base = _pipe(base_ops, vae=base_vae)(**kw)
    ops, vae = CoarseOps(), CountingVAE()
    p = _pipe(ops, vae=vae)
    draws = []
    raw = torch.randn
    spy = lambda *a, **k: (draws.append(a[0]) if len(a[0]) == 5 else None, raw(*a, **k))[1]      # noqa: E731  (latent-shaped draws only)
    monkeypatch.setattr(torch, "randn", spy)
    got = p(**kw, coarse_steps=off)
    monkeypatch.setattr(torch, "randn", raw)
    assert torch.equal(got, base) and p.coarse_record is None
    assert dict(ops.calls) == dict(base_ops.calls) and vae.encodes == base_vae.encodes == 2
    assert ops.calls["latent_resize_noise"] == 0 and p._engine._coarse_engines == {}
    assert draws == [(1, 16) + FINE.latent_shape()[1:]]                          # ONE draw, at the call's shape
    # ... so a generator seeded and advanced the same way continues alike: the draw is the first of the seed's stream
    g = torch.Generator().manual_seed(kw["seed"])
    first = torch.randn((1, 16) + FINE.latent_shape()[1:], generator=g, dtype=F32)
    assert torch.equal(torch.randn(4, generator=g), torch.randn(4, generator=_advanced(kw["seed"], first.shape)))
    # on, for contrast: two draws, the coarse one first
    monkeypatch.setattr(torch, "randn", spy)
    p(**kw, coarse_steps=1)
    monkeypatch.setattr(torch, "randn", raw)
    assert draws[1:] == [(1, 16, 3, 8, 12), (1, 16, 3, 16, 24)]


def _advanced(seed, shape):
    g = torch.Generator().manual_seed(seed)
    torch.randn(shape, generator=g, dtype=F32)
    return g


# ---- 6. the contract -------------------------------------------------------------------------------------------------------------------------
def test_kernel_argument_validation_without_gpu():
    from infinicube_amd import native
    lib = native.lib()
    assert "icv_latent_resize_noise_f32" in native.SIGNATURES
    f = lib.icv_latent_resize_noise_f32
    assert f(None, None, 0, 8, 12, 16, 24, 0.5, 0, None) == 0                    # zero planes: nothing to do, whatever the pointers
    for args, msg in (((None, 16, 3, 8, 12, 16, 24), b"null argument"), ((16, None, 3, 8, 12, 16, 24), b"null argument"),
                      ((16, 16, -1, 8, 12, 16, 24), b"negative plane count -1"),
                      ((16, 32, 3, 8, 12, 7, 24), b"must be at least the input plane 8 x 12"),
                      ((16, 32, 3, 8, 12, 16, 11), b"must be at least the input plane 8 x 12"),
                      ((16, 32, 3, 0, 12, 16, 24), b"at least 1 x 1"), ((16, 32, 3, 8, 0, 16, 24), b"at least 1 x 1"),
                      ((18, 32, 3, 8, 12, 16, 24), b"4-byte aligned"), ((16, 33, 3, 8, 12, 16, 24), b"4-byte aligned"),
                      ((16, 32, 1 << 20, 8, 12, 64, 64), b"too many for one launch"),
                      ((16, 32, 1, 8, 12, 1 << 31, 24), b"too many for one launch"),
                      ((16, 32, 3, 8, 12, 1 << 40, 1 << 40), b"too many for one launch")):
        assert f(*args, 0.5, 0, None) != 0 and msg in lib.icv_last_error(), (args, lib.icv_last_error())
