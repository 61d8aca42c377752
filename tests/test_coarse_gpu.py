"""Coarse-to-fine sampling on the HIP path: icv_latent_resize_noise_f32 against its torch twin bit for bit (ragged widths, one-row
and one-column planes, every pointer-misalignment pair, both rounding modes, between guard bands, x0 untouched), same-size against
icv_add_noise_f32, its contract, the HIP pipeline against the two stages driven by hand on fresh engines (text-to-video and
image-to-video), every driver mode against the sequential per-op two-stage call, one composed call (NAG + Enhance-A-Video + radial
attention) and the unchanged generator through the pipeline's attributes."""
import contextlib
import io

import numpy as np
import pytest
import torch

from infinicube_amd.videogen import enhance, nag
from infinicube_amd.videogen import synthetic as syn
from infinicube_amd.videogen.config import preset
from infinicube_amd.videogen.pipeline import DiTHolder, WanVideoPipeline
from infinicube_amd.videogen.scheduler import FlowMatchScheduler
from standins import HashImageEncoder, HashTextEncoder, PoolVAE
from test_buffer_edges_gpu import Arena
from test_coarse_cpu import FINE, SHORT_SIZE, SIZES, _env, drive_coarse_by_hand, resize_noise_twin
from test_v2v_cpu import CFG, _call_kw, make_clip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SIGMAS = (0.0, 1.0, 0.5, FlowMatchScheduler(50, 5.0).sigmas[25])          # the ends, the middle, a shifted schedule value
# (w_out, input widths): each output width with inputs at ratio 1, 2 and a fractional one where the width has them
WIDTHS = ((1, (1,)), (2, (2, 1)), (3, (3, 2, 1)), (5, (5, 3, 2)), (7, (7, 4, 3)), (13, (13, 7, 6)), (24, (24, 12, 16)), (104, (104, 52, 78)),
          (160, (160, 80, 104)))
HEIGHTS = ((1, (1,)), (2, (2, 1)), (16, (16, 8, 12)), (90, (90, 45, 60)))


def run_resize(hip_ops, planes, h_in, w_in, h_out, w_out, offs, sigma, rounding):
    """One launch on buffers carved out of a sentinel-filled arena, against the twin on the host."""
    g = torch.Generator().manual_seed(1000 * w_out + 10 * h_out + planes)
    x0, noise = torch.randn((planes, h_in, w_in), generator=g), torch.randn((planes, h_out, w_out), generator=g)
    want = noise.clone()
    resize_noise_twin(x0, want, sigma, rounding)
    ar = Arena(nbytes=4 * (x0.numel() + noise.numel()) + 4096)
    bx, bo = ar.carve(np.float32, x0.numel(), offs[0]), ar.carve(np.float32, noise.numel(), offs[1])
    tx, to = bx.tensor(tuple(x0.shape)), bo.tensor(tuple(noise.shape))
    tx.copy_(x0)
    to.copy_(noise)
    assert tx.data_ptr() % 16 == 4 * offs[0] and to.data_ptr() % 16 == 4 * offs[1]
    before = ar.snapshot()
    hip_ops.latent_resize_noise(tx, to, sigma, round_bf16=rounding)
    ar.check(before, [bo])                         # the guard bands, and x0 is not written
    got = to.cpu()
    assert torch.equal(got, want), (f"planes={planes} {h_in}x{w_in} -> {h_out}x{w_out} offsets={offs} sigma={sigma} round_bf16={rounding}: "
                                    f"{int((got != want).sum())} of {got.numel()} differ, first at {(got != want).nonzero()[0].tolist()}, "
                                    f"max |d| {float((got - want).abs().max())}")
    return got


@pytest.mark.parametrize("rounding", [False, True], ids=["exact", "round-bf16"])
@pytest.mark.parametrize("planes", [1, 3, 48])
def test_kernel_matches_twin(hip_ops, planes, rounding):
    """Every output width x its input widths x every output height (input heights in turn); the pointer offsets of (x0, noise_out)
    from a 256-byte boundary walk all 16 pairs and the sigmas all four values as the cases go by, so every output width meets every
    head length of the vector body."""
    case = 0
    for w_out, w_ins in WIDTHS:
        for w_in in w_ins:
            for hi, (h_out, h_ins) in enumerate(HEIGHTS):
                h_in = h_ins[(case + hi) % len(h_ins)]
                offs = (case // 4 % 4, case % 4)
                run_resize(hip_ops, planes, h_in, w_in, h_out, w_out, offs, SIGMAS[(case // 16 + case) % 4], rounding)
                case += 1
    # the two modes differ where there is something to round
    a = run_resize(hip_ops, planes, 8, 12, 16, 24, (0, 0), 0.5, False)
    b = run_resize(hip_ops, planes, 8, 12, 16, 24, (0, 0), 0.5, True)
    assert not torch.equal(a, b)


@pytest.mark.parametrize("offs", [(0, 0), (1, 3), (2, 1), (3, 2)], ids=lambda o: f"{o[0]}{o[1]}")
def test_every_sigma_and_height_at_one_offset_pair(hip_ops, offs):
    """The cross product the walk above thins out, at the sizes of the pipeline tests and one ragged pair."""
    for rounding in (False, True):
        for sigma in SIGMAS:
            for (h_in, w_in, h_out, w_out) in ((8, 12, 16, 24), (12, 16, 16, 24), (3, 5, 4, 7), (1, 1, 2, 13), (2, 3, 2, 3)):
                run_resize(hip_ops, 3, h_in, w_in, h_out, w_out, offs, sigma, rounding)


@pytest.mark.parametrize("rounding", [False, True], ids=["exact", "round-bf16"])
def test_same_size_is_add_noise_bit_for_bit(hip_ops, rounding):
    g = torch.Generator().manual_seed(3)
    for shape in ((3, 16, 24), (48, 1, 7), (1, 90, 13)):
        x0, noise = torch.randn(shape, generator=g).to(DEV), torch.randn(shape, generator=g).to(DEV)
        for sigma in SIGMAS:
            want = torch.empty_like(noise)
            hip_ops.add_noise(x0, noise, want, sigma, round_bf16=rounding)
            got = noise.clone()
            hip_ops.latent_resize_noise(x0, got, sigma, round_bf16=rounding)
            assert torch.equal(got, want), (shape, sigma)


def test_contract(hip_ops):
    from infinicube_amd import native
    lib, st = native.lib(), torch.cuda.current_stream().cuda_stream
    ar = Arena(nbytes=1 << 14)
    bx, bo = ar.carve(np.float32, 3 * 2 * 3, 0), ar.carve(np.float32, 3 * 4 * 6, 0)
    bx.tensor((18,)).copy_(torch.ones(18))
    bo.tensor((72,)).copy_(torch.ones(72))
    before = ar.snapshot()
    f = lib.icv_latent_resize_noise_f32
    assert f(bx.ptr, bo.ptr, 0, 2, 3, 4, 6, 0.5, 0, st) == 0 and f(None, None, 0, 2, 3, 4, 6, 0.5, 0, st) == 0      # zero planes: no launch
    for args, msg in (((None, bo.ptr, 3, 2, 3, 4, 6), b"null argument"), ((bx.ptr, None, 3, 2, 3, 4, 6), b"null argument"),
                      ((bx.ptr, bo.ptr, -3, 2, 3, 4, 6), b"negative plane count"), ((bx.ptr, bo.ptr, 3, 4, 6, 2, 3), b"must be at least the input plane"),
                      ((bx.ptr, bo.ptr, 3, 2, 3, 4, 2), b"must be at least the input plane"), ((bx.ptr, bo.ptr, 3, 0, 3, 4, 6), b"at least 1 x 1"),
                      ((bx.ptr + 2, bo.ptr, 3, 2, 3, 4, 6), b"4-byte aligned"), ((bx.ptr, bo.ptr + 1, 3, 2, 3, 4, 6), b"4-byte aligned"),
                      ((bx.ptr, bo.ptr, 1 << 20, 2, 3, 64, 64), b"too many for one launch")):
        assert f(*args, 0.5, 0, st) != 0 and msg in lib.icv_last_error(), args
    ar.check(before, [])
    # the operator's own checks
    x, o = torch.zeros((3, 2, 3), device=DEV), torch.zeros((3, 4, 6), device=DEV)
    with pytest.raises(TypeError, match="latent_resize_noise.x0"):
        hip_ops.latent_resize_noise(x.to(torch.bfloat16), o, 0.5)
    with pytest.raises(TypeError, match="latent_resize_noise.noise_out"):
        hip_ops.latent_resize_noise(x, o.double(), 0.5)
    with pytest.raises(ValueError, match="same leading dimensions"):
        hip_ops.latent_resize_noise(x[:2], o, 0.5)
    with pytest.raises(ValueError, match="must be at least the input plane"):
        hip_ops.latent_resize_noise(o, x, 0.5)
    hip_ops.latent_resize_noise(x[:0], o[:0], 0.5)                       # no planes: nothing to do


# ---- the pipeline --------------------------------------------------------------------------------------------------------------------
def _pipe(hip_ops, cfg=CFG, vae=None, buffers=True, **kw):
    p = WanVideoPipeline(DEV, torch.bfloat16, DiTHolder(syn.make_dit_state_dict(cfg), cfg), HashTextEncoder(cfg), vae or PoolVAE(), ops=hip_ops, **kw)
    if buffers:
        p.initialize_buffer_embedder(16, zero_init=False)
    return p


@pytest.mark.parametrize("rounding", [False, True], ids=["exact", "reference-rounding"])
@pytest.mark.parametrize("size", SIZES, ids=["2x", "fractional"])
def test_hip_pipeline_equals_the_stages_driven_by_hand(hip_ops, size, rounding, monkeypatch):
    """The hand-driven switch is the torch TWIN on the device, so this also pins the kernel inside the call."""
    _env(monkeypatch)
    p = _pipe(hip_ops)
    p.reference_rounding = rounding
    kw = _call_kw(FINE, num_inference_steps=4)
    plain = p(**kw)
    assert p.coarse_record is None
    got = p(**kw, coarse_steps=2, coarse_size=size)
    assert p.coarse_record == dict(steps=2, size=size, sigma=FlowMatchScheduler(4, 5.0).sigmas[2], tokens=(3 * size[0] * size[1] // 256, 288))
    want, _ = drive_coarse_by_hand(p, hip_ops, kw, 2, size)
    torch.cuda.synchronize()
    assert torch.equal(got, want), f"max |d| {float((got - want).abs().max())}"
    assert torch.isfinite(got).all() and not torch.equal(got, plain)
    twin = p._engine._coarse_engines[size + (9,)]
    assert torch.equal(p(**kw, coarse_steps=2, coarse_size=size), got) and p._engine._coarse_engines[size + (9,)] is twin      # kept between calls


def test_hip_pipeline_image_to_video(hip_ops, monkeypatch):
    """``synthetic`` has an image-to-video preset at this width ("tiny-i2v"): the conditioning latent is encoded and embedded once per
    stage's grid."""
    _env(monkeypatch)
    from PIL import Image
    cfg = preset("tiny-i2v")
    p = _pipe(hip_ops, cfg=cfg, image_encoder=HashImageEncoder(cfg))
    kw = _call_kw(FINE, num_inference_steps=3, input_image=Image.fromarray(make_clip(FINE, 1)[0], mode="RGB"))
    got = p(**kw, coarse_steps=1, coarse_size=(96, 128))
    want, _ = drive_coarse_by_hand(p, hip_ops, kw, 1, (96, 128))
    torch.cuda.synchronize()
    assert torch.equal(got, want) and not torch.equal(got, p(**kw))


MODES = {"per-op": dict(ICV_CFG_BATCH="0"), "pair": {}, "pair-no-stem": dict(ICV_SHARE_STEM="0"), "dual-stream": dict(ICV_DUAL_STREAM="1"),
         "graphs": dict(ICV_GRAPHS="1"), "native": dict(ICV_NATIVE_FORWARD="1")}
_SEQ = {}


def _sequential(m):
    m.cfg_batch = False


@pytest.mark.parametrize("mode", list(MODES))
def test_driver_modes_match_the_sequential_two_stage_call(hip_ops, mode, monkeypatch):
    """The pipeline under each driver mode's switch - both stages take it, the coarse twin through ``coarse_engine`` - against the
    sequential per-op two-stage call driven by hand from the same noise with the kernel as the switch."""
    _env(monkeypatch)
    kw = _call_kw(FINE, num_inference_steps=4)
    if "ref" not in _SEQ:
        ref, _ = drive_coarse_by_hand(_pipe(hip_ops), hip_ops, kw, 2, SHORT_SIZE, resize_op=hip_ops.latent_resize_noise, setup=_sequential,
                                      prep=dict(graphs=False))
        _SEQ["ref"] = ref.clone()
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    p = _pipe(hip_ops)
    got = p(**kw, coarse_steps=2, coarse_size=SHORT_SIZE)
    torch.cuda.synchronize()
    hi = p._engine
    lo = hi._coarse_engines[SHORT_SIZE + (9,)]
    for m in (lo, hi):
        if mode in ("pair", "pair-no-stem"):
            assert m._pair is not None and m.share_stem == (mode == "pair")
        if mode == "per-op":
            assert m._pair is None and not m._graphs and m._twin is None and m._native is None
        if mode == "dual-stream":
            assert m.dual_stream and m._twin is not None
        if mode == "graphs":
            assert m._graphs_on and m._graphs
        if mode == "native":
            assert m.native_forward and m._native is not None
    assert torch.equal(got, _SEQ["ref"]), f"{mode}: max |d| {float((got - _SEQ['ref']).abs().max())}"
    # a second call with the same sizes builds no new twin
    assert torch.equal(p(**kw, coarse_steps=2, coarse_size=SHORT_SIZE), got) and hi._coarse_engines[SHORT_SIZE + (9,)] is lo


def test_composition_nag_enhance_radial(hip_ops, monkeypatch):
    """One call with NAG (cfg_scale = 1) + Enhance-A-Video + radial attention (1, 1) + coarse_steps against the hand-driven sequence
    with the same plans on both stages; the records of NAG, Enhance and the window are the fine stage's."""
    _env(monkeypatch)
    p = _pipe(hip_ops)
    kw = _call_kw(FINE, num_inference_steps=3)
    on = dict(cfg_scale=1.0, nag_scale=4.0, enhance_weight=2.0, attention_window_frames=1, attention_sink_frames=1, attention_radial=True)
    got = p(**kw, **on, coarse_steps=2, coarse_size=(96, 128))
    rec = dict(nag=p.nag_record, enhance=p.enhance_record, window=p.attention_window_record)
    assert rec["nag"]["scale"] == 4.0 and rec["enhance"]["weight"] == 2.0 and rec["enhance"]["frames"] == 3 and rec["window"]["radial"] is True
    seen = {}

    def plans(m):
        return dict(nag=nag.NagPlan(m.encode_context(p.text_encoder.encode(kw["negative_prompt"])), 4.0, nag.DEFAULT_TAU, nag.DEFAULT_ALPHA),
                    enhance=enhance.EnhancePlan(2.0))

    want, _ = drive_coarse_by_hand(p, hip_ops, kw, 2, (96, 128), resize_op=hip_ops.latent_resize_noise, cfg_scale=1.0, stage_kw=plans,
                                   setup=lambda m: m.set_attention_window(1, 1, radial=True), seen=seen)
    torch.cuda.synchronize()
    assert torch.equal(got, want), f"max |d| {float((got - want).abs().max())}"
    assert rec["enhance"]["scores"] == enhance.EnhancePlan(2.0).record(3, seen["hi"].enhance_scores)["scores"]      # the fine stage's
    off = p(**kw, **on)
    assert p.coarse_record is None and not torch.equal(got, off)


# ---- the unchanged generator -----------------------------------------------------------------------------------------------------------
def test_generator_through_the_attributes(hip_ops, tmp_path, monkeypatch):
    _env(monkeypatch)
    from safetensors.torch import save_file
    from infinicube.videogen import WanVideoGenerator
    ck = str(tmp_path / "step-1.safetensors")
    save_file({"buffer_embedder." + k: v for k, v in syn.make_buffer_embedder_state_dict(CFG).items()}, ck)
    sem, co = syn.make_dummy_buffers(FINE)
    with contextlib.redirect_stdout(io.StringIO()):
        g = WanVideoGenerator(ck, device=DEV, use_wan_1pt3b=True, pipeline_factory=lambda torch_dtype, device, model_configs: _pipe(hip_ops, buffers=False))
        g.pipe.num_inference_steps = 3
        plain = g.generate(sem, co, prompt="a street", negative_prompt="bad", seed=3)
        assert g.pipe.coarse_record is None
        g.pipe.coarse_steps, g.pipe.coarse_size = 2, (96, 128)
        video = g.generate(sem, co, prompt="a street", negative_prompt="bad", seed=3)
    assert g.pipe.coarse_record["steps"] == 2 and g.pipe.coarse_record["size"] == (96, 128) and g.pipe.coarse_record["tokens"] == (144, 288)
    assert len(video) == FINE.num_frames and video[0].size == (FINE.width, FINE.height)
    a, b = (np.stack([np.asarray(f) for f in v]) for v in (plain, video))
    assert b.std() > 0 and not np.array_equal(a, b)
    # ICV_WORLD = 2: refused in the client, before a request reaches a rank (the pool stand-in has no methods to call)
    g._pool = object()
    with contextlib.redirect_stdout(io.StringIO()), pytest.raises(ValueError, match="pipe.coarse_steps cannot be combined with ICV_WORLD > 1"):
        g.generate(sem, co, seed=3)
