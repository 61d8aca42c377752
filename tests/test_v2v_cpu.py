"""Video-to-video (infinicube_amd/videogen/v2v.py: ``input_video`` / ``denoising_strength``) on CPU: the strength-aware sigma
list against today's floats and a float64 ``torch.linspace`` restatement, every validation error before an engine exists, the
pipeline on the TEST-ONLY oracle operator set against the engine driven by hand from the twin's noised latent (bits) and against
upstream's loop restated on ``oracle.wan_ref.dit_forward`` (>= 40 dB), off = the parent's calls and bits, the compositions
(sliding windows, TeaCache, an image-to-video DiT, reference rounding), and the unchanged generator through the environment."""
import collections
import contextlib
import io
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from infinicube_amd.videogen import sliding_window as SW
from infinicube_amd.videogen import synthetic as syn
from infinicube_amd.videogen import options, teacache, v2v
from infinicube_amd.videogen.config import TokenGrid, preset
from infinicube_amd.videogen.dit import WanDiT
from infinicube_amd.videogen.pipeline import DiTHolder, WanVideoPipeline, _video_to_tensor, _video_to_uint8
from infinicube_amd.videogen.scheduler import FlowMatchScheduler, flow_match_sigmas, round_through_bf16
from oracle import wan_ref as R
from oracle_ops import OracleOps
from standins import HashImageEncoder, HashTextEncoder, PoolVAE
from test_sliding_window_cpu import window_euler_twin
from test_teacache_cpu import LINEAR, TeaOps

CFG, GRID = preset("tiny"), TokenGrid(33, 64, 96)        # the sliding-window tests' preset: 9 latent frames of 4 x 6 tokens
SHORT = TokenGrid(9, 64, 96)                             # 3 latent frames: everything that needs no second window
ENV = options.ENV_NAMES + ("ICV_REFERENCE_ROUNDING",)
TILES = dict(tile_size=(30, 52), tile_stride=(15, 26))   # the pipeline's defaults


def rb(t):
    return t.to(torch.bfloat16).to(torch.float32)


def add_noise_twin(x0, noise, out, sigma, round_bf16=False):
    """Torch twin of icv_add_noise_f32, one tensor op per rounding point (include/icvideo.h): 1 - sigma formed in f32, two
    products, one sum.  ``out`` may be ``noise`` or ``x0``."""
    s = torch.tensor(float(sigma), dtype=torch.float32)
    one_minus = float(torch.tensor(1.0, dtype=torch.float32) - s)
    a, b = x0 * one_minus, noise * float(s)
    out.copy_(rb(rb(a) + rb(b)) if round_bf16 else a + b)


class V2VOps(TeaOps):
    """OracleOps + the CPU twins of the TeaCache kernels, of the window kernel and of icv_add_noise_f32; counts every public
    operator by name (``calls``)."""

    def __init__(self, device="cpu"):
        super().__init__(device)
        self.calls = collections.Counter()

    def __getattribute__(self, name):
        v = object.__getattribute__(self, name)
        if not name.startswith("_") and callable(v):
            object.__getattribute__(self, "calls")[name] += 1
        return v

    def unpatchify_cfg_euler_window(self, latent_next, hc, hu, cfg_scale, dsigma, frame_coef, frame0, tok0, n_tok, round_bf16=False):
        window_euler_twin(latent_next, hc, hu, cfg_scale, dsigma, frame_coef, frame0, tok0, n_tok, round_bf16)

    def add_noise(self, x0, noise, out, sigma, round_bf16=False):
        assert x0.dtype == noise.dtype == out.dtype == torch.float32 and x0.shape == noise.shape == out.shape
        add_noise_twin(x0, noise, out, sigma, round_bf16)


assert issubclass(V2VOps, OracleOps)


class CountingVAE(PoolVAE):
    """PoolVAE that counts its encodes and keeps the last latent it was asked to decode."""

    def __init__(self):
        super().__init__()
        self.encodes, self.last_decoded = 0, None

    def encode(self, video, **kw):
        self.encodes += 1
        return super().encode(video, **kw)

    def decode(self, latent, **kw):
        self.last_decoded = latent.detach().clone().cpu()
        return super().decode(latent, **kw)


def make_clip(grid, seed):
    """A seeded uint8 clip [F, H, W, 3] with structure at the scale the pooling VAE keeps."""
    g = np.random.default_rng(seed)
    coarse = g.integers(0, 256, (grid.num_frames, grid.height // 8, grid.width // 8, 3), dtype=np.uint8)
    return np.ascontiguousarray(coarse.repeat(8, axis=1).repeat(8, axis=2))


def pil(clip):
    return [Image.fromarray(f, mode="RGB") for f in clip]


# ---- 1. the scheduler -----------------------------------------------------------------------------------------------------------
def strength_sigmas(num_steps, shift, strength):
    """Upstream's rule in float64: linspace(s, 0, N + 1)[:-1], then the shift warp."""
    s = torch.linspace(strength, 0.0, num_steps + 1, dtype=torch.float64)[:-1]
    return shift * s / (1.0 + (shift - 1.0) * s)


def _todays_lists(n, shift, rounding):
    """FlowMatchScheduler as it stood before the argument existed, restated."""
    sig = []
    for i in range(n):
        s = 1.0 + (0.0 - 1.0) * (i / n)
        sig.append(shift * s / (1.0 + (shift - 1.0) * s))
    ts = [s * 1000.0 for s in sig]
    return sig, [round_through_bf16(t) for t in ts] if rounding else ts


@pytest.mark.parametrize("rounding", [False, True])
def test_strength_one_is_todays_scheduler(rounding):
    for n, shift in ((50, 5.0), (2, 5.0), (7, 3.0), (10, 1.0)):
        sig, ts = _todays_lists(n, shift, rounding)
        for sch in (FlowMatchScheduler(n, shift, rounding), FlowMatchScheduler(n, shift, rounding, denoising_strength=1.0)):
            assert sch.sigmas == sig and sch.timesteps == ts and sch.denoising_strength == 1.0
            assert [sch.dsigma(i) for i in range(n)] == [(sig[i + 1] if i + 1 < n else 0.0) - sig[i] for i in range(n)]
        assert flow_match_sigmas(n, shift) == sig


@pytest.mark.parametrize("strength", [0.6, 0.05])
def test_strength_matches_linspace_restatement(strength):
    for n, shift in ((50, 5.0), (2, 5.0), (7, 3.0), (10, 1.0)):
        sch = FlowMatchScheduler(n, shift, denoising_strength=strength)
        want = strength_sigmas(n, shift, strength)
        assert len(sch.sigmas) == n
        assert float((torch.tensor(sch.sigmas, dtype=torch.float64) - want).abs().max()) <= 1e-12
        assert sch.timesteps == [s * 1000.0 for s in sch.sigmas]
        assert sch.sigmas[0] < 1.0 and sch.dsigma(n - 1) == -sch.sigmas[-1]          # all N steps, the last one to sigma = 0
    assert FlowMatchScheduler(4, 1.0, denoising_strength=strength).sigmas[0] == strength


def test_strength_one_starts_at_sigma_one_exactly():
    for shift in (1.0, 3.0, 5.0, 17.0):
        for n in (1, 2, 50):
            assert FlowMatchScheduler(n, shift, denoising_strength=1.0).sigmas[0] == 1.0


# ---- 2. validation and settings ---------------------------------------------------------------------------------------------------
def _pipe(ops=None, cfg=CFG, vae=None, buffers=True, **kw):
    p = WanVideoPipeline("cpu", torch.bfloat16, DiTHolder(syn.make_dit_state_dict(cfg), cfg), HashTextEncoder(cfg), vae or PoolVAE(),
                         ops=ops or V2VOps(), **kw)
    if buffers:
        p.initialize_buffer_embedder(16, zero_init=False)
    return p


def _call_kw(grid=SHORT, buffers=True, **extra):
    kw = dict(prompt="a street", negative_prompt="bad", height=grid.height, width=grid.width, num_frames=grid.num_frames, seed=3,
              num_inference_steps=2, return_latents=True)
    if buffers:
        sem, co = syn.make_dummy_buffers(grid)
        kw.update(semantic_buffer_video=pil(sem), coordinate_buffer_video=pil(co))
    kw.update(extra)
    return kw


def test_validation_errors_come_before_the_engine(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    clip = pil(make_clip(SHORT, 1))
    p = _pipe()
    for bad in (0, 0.0, -0.1, 1.5, "0.5", float("nan"), True):
        with pytest.raises(ValueError, match=r"denoising_strength must be a number in \(0, 1\]"):
            p(**_call_kw(input_video=clip, denoising_strength=bad))
        assert p._engine is None
    with pytest.raises(ValueError, match="needs an input_video"):                    # upstream would denoise pure noise over a short range
        p(**_call_kw(denoising_strength=0.6))
    assert p._engine is None
    for wrong in (clip[:8], clip + clip[:1]):
        with pytest.raises(ValueError, match=f"input_video has {len(wrong)} frames, num_frames=9"):
            p(**_call_kw(input_video=wrong, denoising_strength=0.6))
        assert p._engine is None
    with pytest.raises(ValueError, match="uint8 frames"):
        p(**_call_kw(input_video=np.zeros((9, 64, 96, 3), dtype=np.float32)))
    assert p._engine is None
    # one process only: a process group of more than one rank raises, naming the combination
    import torch.distributed as dist
    with monkeypatch.context() as mp:
        mp.setattr(dist, "is_initialized", lambda: True)
        mp.setattr(dist, "get_world_size", lambda *a: 2)
        mp.setattr(dist, "get_rank", lambda *a: 0)
        with pytest.raises(ValueError, match="cannot be combined with a process group of 2 ranks"):
            p(**_call_kw(input_video=clip, denoising_strength=0.6))
    assert p._engine is None and p.v2v_record is None
    monkeypatch.setenv("ICV_DENOISING_STRENGTH", "strong")
    with pytest.raises(ValueError, match="ICV_DENOISING_STRENGTH must be a number"):
        _pipe()


def test_worker_pool_combination_raises(monkeypatch):
    """ICV_WORLD > 1 behind the unchanged generator: refused in the client before a request reaches the ranks."""
    from infinicube_amd.videogen.inference import WanVideoGenerator
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    sem, co = syn.make_dummy_buffers(SHORT)
    for attr, value in (("input_video", "/clips/drive.npy"), ("denoising_strength", 0.6)):
        g = WanVideoGenerator.__new__(WanVideoGenerator)
        g._pool, g.pipe = object(), _pipe()
        setattr(g.pipe, attr, value)
        with contextlib.redirect_stdout(io.StringIO()), pytest.raises(ValueError, match="ICV_WORLD > 1"):
            g.generate(sem, co, seed=0)


def test_settings_precedence_and_record(monkeypatch, tmp_path):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    p = _pipe()
    assert (p.input_video, p.denoising_strength, p.v2v_record) == (None, None, None)
    a, b = make_clip(SHORT, 1), make_clip(SHORT, 2)
    np.save(tmp_path / "a.npy", a)
    monkeypatch.setenv("ICV_INPUT_VIDEO", str(tmp_path / "a.npy"))
    monkeypatch.setenv("ICV_DENOISING_STRENGTH", "0.6")
    p = _pipe()
    assert (p.input_video, p.denoising_strength) == (str(tmp_path / "a.npy"), 0.6)      # environment -> attributes
    from_env = p(**_call_kw())
    assert p.v2v_record == dict(denoising_strength=0.6, sigma_0=FlowMatchScheduler(2, 5.0, denoising_strength=0.6).sigmas[0])
    assert torch.equal(from_env, _pipe()(**_call_kw(input_video=pil(a), denoising_strength=0.6)))
    kw_wins = p(**_call_kw(input_video=pil(b), denoising_strength=0.3))                  # keywords win, each on its own
    assert p.v2v_record["denoising_strength"] == 0.3 and not torch.equal(kw_wins, from_env)
    assert torch.equal(p(**_call_kw(input_video=pil(b))), _pipe()(**_call_kw(input_video=pil(b), denoising_strength=0.6)))
    p.input_video, p.denoising_strength = pil(b), None                                    # attributes set after construction
    assert torch.equal(p(**_call_kw(denoising_strength=0.3)), kw_wins)
    p.input_video = None
    p(**_call_kw())
    assert p.v2v_record is None
    # an input video without a strength: upstream's default of 1.0
    p(**_call_kw(input_video=a))
    assert p.v2v_record == dict(denoising_strength=1.0, sigma_0=1.0)


# ---- 3. the pipeline against the engine driven by hand and against upstream's loop -------------------------------------------------
def drive_by_hand(pipe, ops, kw, frames=None, strength=1.0, sw=None, tea=None, prep=None, setup=None, engine_kw=None, noise_op=None):
    """What the call must amount to, spelled out on a fresh engine over the pipeline's components: CPU-generator noise, the input
    clip through the VAE, the start latent from the TWIN (or ``noise_op``), a strength-aware scheduler, then ``engine.denoise``
    exactly as the plain loop (or the windowed / TeaCache loop) is driven."""
    cfg, rr = pipe.dit.cfg, pipe.reference_rounding
    h, w, n = kw["height"], kw["width"], kw["num_inference_steps"]
    grid = TokenGrid(kw["num_frames"], h, w)
    m = WanDiT(cfg, pipe.dit.state_dict(), ops, pipe.buffer_embedder.state_dict() if pipe.buffer_embedder else None, **(engine_kw or {}))
    m.prepare(TokenGrid(4 * (sw[0] - 1) + 1, h, w) if sw else grid, **(prep or {}))
    if setup is not None:
        setup(m)
    image = kw.get("input_image")
    clip_fea = pipe.image_encoder.encode_image(image) if image is not None else None
    ck = m.encode_context(pipe.text_encoder.encode(kw["prompt"]), clip_fea)
    cu = m.encode_context(pipe.text_encoder.encode(kw["negative_prompt"]), clip_fea)
    noise = torch.randn((1, 16) + grid.latent_shape()[1:], generator=torch.Generator().manual_seed(kw["seed"]), dtype=torch.float32)[0]
    lat = ops.to_device(rb(noise) if rr else noise, torch.float32)

    def enc(fr):
        clip = _video_to_uint8(fr, h, w) if getattr(pipe.vae, "accepts_uint8", False) else _video_to_tensor(fr, h, w)
        return pipe.vae.encode(clip, tiled=True, **TILES).to(torch.float32)

    bt = None
    if "semantic_buffer_video" in kw:
        bl = torch.cat([enc(kw["semantic_buffer_video"]), enc(kw["coordinate_buffer_video"])], dim=0)
        bt = m.embed_buffers(bl, **(dict(whole_clip=True) if sw else {}))
    if image is not None:
        bt = m.embed_cond_latents(pipe._image_cond_latents(image, grid, True, TILES["tile_size"], TILES["tile_stride"]), add_to=bt)
    sch = FlowMatchScheduler(n, 5.0, rr, denoising_strength=strength)
    if frames is not None:
        x0 = enc(frames)
        x0 = ops.to_device(rb(x0) if rr else x0, torch.float32)
        (noise_op or add_noise_twin)(x0, lat, lat, sch.sigmas[0], rr)
    tc = teacache.plan(m, sch, tea[0], tea[1], range(n)) if tea else None
    m.denoise(lat, ck, cu, bt, sch, 5.0, round_bf16=rr, tea_cache=tc, **(dict(sliding_window=SW.plan(grid.T, *sw)) if sw else {}))
    return lat


def v2v_reference(sd, bsd, cfg, x0, noise, c1, c2, bl, num_steps, strength, shift=5.0, cfg_scale=5.0, dtype=torch.float32):
    """Upstream's video-to-video loop restated on oracle.wan_ref.dit_forward: the strength-aware sigma list in float64,
    latent = (1 - sigma_0) x0 + sigma_0 noise, then CFG and Euler over ALL num_steps steps (oracle.wan_ref.denoise_loop
    hard-codes the full range)."""
    sig = strength_sigmas(num_steps, shift, strength)
    buf = R.buffer_embed(bsd, bl, dtype) if bl is not None else None
    x = noise.to(dtype).clone() if x0 is None else (1.0 - float(sig[0])) * x0.to(dtype) + float(sig[0]) * noise.to(dtype)
    for i in range(num_steps):
        ts = float(sig[i]) * 1000.0
        v_c = R.dit_forward(sd, cfg, x, c1, ts, buf, dtype)
        v_u = R.dit_forward(sd, cfg, x, c2, ts, buf, dtype)
        v = v_u + cfg_scale * (v_c - v_u)
        nxt = float(sig[i + 1]) if i + 1 < num_steps else 0.0
        x = x + v * (nxt - float(sig[i]))
    return x


def oracle_inputs(pipe, kw, frames, dev="cpu"):
    """The tensors the restated loop needs, from the pipeline's own components (bf16-rounded weights, as the engine stores them)."""
    grid = TokenGrid(kw["num_frames"], kw["height"], kw["width"])
    enc = lambda fr: pipe.vae.encode(_video_to_tensor(fr, grid.height, grid.width)).float()     # noqa: E731
    noise = torch.randn((1, 16) + grid.latent_shape()[1:], generator=torch.Generator().manual_seed(kw["seed"]), dtype=torch.float32)[0]
    to = lambda t: t.to(dev)                                                                    # noqa: E731
    return dict(sd={k: to(v) for k, v in R.round_state_dict_to_bf16(pipe.dit.state_dict()).items()},
                bsd={k: to(v) for k, v in R.round_state_dict_to_bf16(pipe.buffer_embedder.state_dict()).items()},
                x0=to(enc(frames)), noise=to(noise), c1=to(pipe.text_encoder.encode(kw["prompt"])),
                c2=to(pipe.text_encoder.encode(kw["negative_prompt"])),
                bl=to(torch.cat([enc(kw["semantic_buffer_video"]), enc(kw["coordinate_buffer_video"])], dim=0)))


def test_strength_one_with_input_video_is_the_plain_call(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    ops = V2VOps()
    p = _pipe(ops)
    base = p(**_call_kw())
    assert ops.calls["add_noise"] == 0 and p.v2v_record is None
    clip = pil(make_clip(SHORT, 1))
    for kw in (dict(input_video=clip), dict(input_video=clip, denoising_strength=1.0)):
        got = p(**_call_kw(**kw))
        assert torch.equal(got, base)
        assert p.v2v_record == dict(denoising_strength=1.0, sigma_0=1.0)
    assert ops.calls["add_noise"] == 2                      # the clip IS encoded and noised: sigma_0 = 1 returns the noise


@pytest.mark.parametrize("rounding", [False, True])
def test_pipeline_equals_engine_driven_by_hand(rounding, monkeypatch):
    """Pins the wiring: three clips through the VAE, x0 rounded like the noise under reference rounding, the noised latent in
    place of the noise, the scheduler of the call."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    vae = CountingVAE()
    p = _pipe(vae=vae)
    p.reference_rounding = rounding
    clip = pil(make_clip(SHORT, 1))
    kw = _call_kw()
    got = p(**kw, input_video=clip, denoising_strength=0.6)
    assert vae.encodes == 3 and p._ops.calls["add_noise"] == 1
    assert p.scheduler.denoising_strength == 0.6 and p.v2v_record["sigma_0"] == p.scheduler.sigmas[0] < 1.0
    want = drive_by_hand(p, V2VOps(), kw, clip, 0.6)
    assert torch.equal(got, want), f"max |d| {float((got - want).abs().max())}"
    # ... and it is neither the text-to-video result nor independent of the clip
    assert not torch.equal(got, p(**kw))
    other = p(**kw, input_video=pil(make_clip(SHORT, 2)), denoising_strength=0.6)
    assert torch.isfinite(other).all() and not torch.equal(got, other)
    if rounding:
        p.reference_rounding = False
        assert not torch.equal(got, p(**kw, input_video=clip, denoising_strength=0.6)), "reference rounding must differ from the exact path"


def test_pipeline_matches_restated_upstream_loop(monkeypatch):
    """Bar: the one the TeaCache and window tests hold their host loops to against their restatements (>= 40 dB latent PSNR)."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    p = _pipe()
    clip = pil(make_clip(SHORT, 1))
    kw = _call_kw()
    got = p(**kw, input_video=clip, denoising_strength=0.6)
    o = oracle_inputs(p, kw, clip)
    ref = v2v_reference(o["sd"], o["bsd"], CFG, o["x0"], o["noise"], o["c1"], o["c2"], o["bl"], 2, 0.6)
    db = R.psnr(got, ref)
    print(f"v2v pipeline (strength 0.6, 2 steps) vs restated loop: {db:.1f} dB")
    assert db >= 40.0, f"{db:.1f} dB"
    # the result provably starts from the encoded clip: the restatement from pure noise, and from another clip, are far away
    t2v = v2v_reference(o["sd"], o["bsd"], CFG, None, o["noise"], o["c1"], o["c2"], o["bl"], 2, 1.0)
    other = v2v_reference(o["sd"], o["bsd"], CFG, oracle_inputs(p, kw, pil(make_clip(SHORT, 2)))["x0"], o["noise"], o["c1"], o["c2"], o["bl"], 2, 0.6)
    assert R.psnr(got, t2v) < db - 10.0 and R.psnr(got, other) < db - 10.0
    # strength 1.0 without a clip restates oracle.wan_ref.denoise_loop (the restatement's own anchor)
    full = R.denoise_loop(o["sd"], o["bsd"], CFG, o["noise"], o["c1"], o["c2"], o["bl"], 2)
    assert torch.equal(t2v, full)


# ---- 4. off ------------------------------------------------------------------------------------------------------------------------
def test_off_calls_nothing_new(monkeypatch):
    """Without the keywords: no new launch, no allocation, no VAE work, the parent's bits - the operator calls of the pipeline are
    those of the engine driven by hand from pure noise with the scheduler as it was before the argument existed."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    ops, vae = V2VOps(), CountingVAE()
    p = _pipe(ops, vae=vae)
    kw = _call_kw()
    allocs = []
    raw = ops.alloc
    monkeypatch.setattr(ops, "alloc", lambda shape, dtype: (allocs.append(tuple(shape)), raw(shape, dtype))[1])
    got = p(**kw)
    assert p.v2v_record is None and ops.calls["add_noise"] == 0 and vae.encodes == 2
    assert tuple(got.shape) not in allocs, "off: no second latent"
    assert p.scheduler.sigmas == _todays_lists(2, 5.0, False)[0]
    hand_ops = V2VOps()
    want = drive_by_hand(p, hand_ops, kw)
    assert torch.equal(got, want)
    plumbing = ("alloc", "to_device")
    assert {k: v for k, v in ops.calls.items() if k not in plumbing} == {k: v for k, v in hand_ops.calls.items() if k not in plumbing}
    # on, for contrast: one more encode, one add_noise, nothing else
    before, encodes = collections.Counter(ops.calls), vae.encodes
    p(**kw, input_video=pil(make_clip(SHORT, 1)), denoising_strength=0.6)
    new = {k: v - before[k] for k, v in ops.calls.items() if k not in plumbing}
    assert vae.encodes - encodes == 3 and new == {**{k: v for k, v in hand_ops.calls.items() if k not in plumbing}, "add_noise": 1}


# ---- 5. composition ------------------------------------------------------------------------------------------------------------------
def test_with_sliding_windows_the_whole_clip_is_noised_once(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    ops = V2VOps()
    p = _pipe(ops)
    clip = pil(make_clip(GRID, 1))
    kw = _call_kw(GRID)
    got = p(**kw, input_video=clip, denoising_strength=0.6, sliding_window_size=4, sliding_window_stride=2)
    assert p.sliding_window_record == [(0, 4), (2, 6), (4, 8), (6, 9)] and ops.calls["add_noise"] == 1
    want = drive_by_hand(p, V2VOps(), kw, clip, 0.6, sw=(4, 2))
    assert torch.equal(got, want), f"max |d| {float((got - want).abs().max())}"
    assert not torch.equal(got, p(**kw, sliding_window_size=4, sliding_window_stride=2))


def test_with_teacache_the_plan_reads_the_shortened_range(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setitem(teacache.COEFFICIENTS, "test-linear", LINEAR)
    p = _pipe()
    clip = pil(make_clip(SHORT, 1))
    kw = _call_kw(num_inference_steps=6)
    got = p(**kw, input_video=clip, denoising_strength=0.6, tea_cache_l1_thresh=1e9, tea_cache_model_id="test-linear")
    assert p.tea_cache_record["computed"] == [0, 5]
    d_v2v = p.tea_cache_record["distances"]
    want = drive_by_hand(p, V2VOps(), kw, clip, 0.6, tea=(1e9, "test-linear"))
    assert torch.equal(got, want), f"max |d| {float((got - want).abs().max())}"
    assert not torch.equal(got, p(**kw, input_video=clip, denoising_strength=0.6))
    p(**kw, tea_cache_l1_thresh=1e9, tea_cache_model_id="test-linear")
    assert p.tea_cache_record["distances"] != d_v2v, "the plan must read the call's timesteps"


def test_with_an_image_to_video_dit_only_the_start_latent_changes(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    cfg = preset("tiny-i2v")
    p = _pipe(cfg=cfg, image_encoder=HashImageEncoder(cfg))
    clip = make_clip(SHORT, 1)
    kw = _call_kw(input_image=Image.fromarray(clip[0], mode="RGB"))
    got = p(**kw, input_video=pil(clip), denoising_strength=0.6)
    want = drive_by_hand(p, V2VOps(), kw, pil(clip), 0.6)
    assert torch.equal(got, want), f"max |d| {float((got - want).abs().max())}"
    assert not torch.equal(got, p(**kw))


# ---- 6. the unchanged generator, through the environment ---------------------------------------------------------------------------
def generator_through_env(factory, tmp_path, monkeypatch, form, clip, grid, device, strength="0.6"):
    """WanVideoGenerator built with ICV_INPUT_VIDEO (``form``: "npy" | "dir") + ICV_DENOISING_STRENGTH set; -> (generator, frames)."""
    from safetensors.torch import save_file
    from infinicube.videogen import WanVideoGenerator
    ck = str(tmp_path / "step-1.safetensors")
    save_file({"buffer_embedder." + k: v for k, v in syn.make_buffer_embedder_state_dict(CFG).items()}, ck)
    if form == "npy":
        path = tmp_path / "clip.npy"
        np.save(path, clip)
    else:
        path = tmp_path / "frames"
        path.mkdir()
        for i in np.random.default_rng(0).permutation(len(clip)):          # written out of order: the NAMES decide the order
            Image.fromarray(clip[i], mode="RGB").save(path / f"frame_{i:04d}.png")
    monkeypatch.setenv("ICV_INPUT_VIDEO", str(path))
    monkeypatch.setenv("ICV_DENOISING_STRENGTH", strength)
    sem, co = syn.make_dummy_buffers(grid)
    with contextlib.redirect_stdout(io.StringIO()):
        g = WanVideoGenerator(ck, device=device, use_wan_1pt3b=True, pipeline_factory=factory)
        g.pipe.num_inference_steps = 2
        video = g.generate(sem, co, prompt="a street", negative_prompt="bad", seed=3)
    return g, video


@pytest.mark.parametrize("form", ["npy", "dir"])
def test_generator_through_the_environment(form, tmp_path, monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    clip = make_clip(SHORT, 1)
    p = _pipe()
    p.buffer_embedder.load_state_dict(syn.make_buffer_embedder_state_dict(CFG))
    want = p(**_call_kw(), input_video=pil(clip), denoising_strength=0.6)
    vae = CountingVAE()
    g, video = generator_through_env(lambda torch_dtype, device, model_configs: _pipe(vae=vae, buffers=False), tmp_path, monkeypatch,
                                     form, clip, SHORT, "cpu")
    assert len(video) == SHORT.num_frames and g.pipe.v2v_record["denoising_strength"] == 0.6
    assert torch.equal(vae.last_decoded, want)


def test_other_paths_need_imageio(tmp_path, monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    path = tmp_path / "drive.mp4"
    path.write_bytes(b"not a video")
    monkeypatch.setitem(sys.modules, "imageio", None)             # `import imageio` raises ImportError
    monkeypatch.setenv("ICV_INPUT_VIDEO", str(path))
    p = _pipe()
    with pytest.raises(ValueError, match=r"\.npy file of uint8 \[N, H, W, 3\] frames, or a directory of image files"):
        p(**_call_kw())
    assert p._engine is None
    with pytest.raises(ValueError, match="imageio"):
        v2v.load_clip(str(path))
    bad = tmp_path / "f32.npy"
    np.save(bad, np.zeros((9, 64, 96, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="uint8 frames"):
        v2v.load_clip(str(bad))
    (tmp_path / "empty").mkdir()
    with pytest.raises(ValueError, match="holds no files"):
        v2v.load_clip(str(tmp_path / "empty"))


# ---- 7. the kernel's argument checks run on the host, before any launch ---------------------------------------------------------------
def test_kernel_argument_validation_without_gpu():
    from infinicube_amd import native
    lib = native.lib()
    assert lib.icv_add_noise_f32(None, None, None, 0, 0.5, 0, None) == 0                 # n == 0: nothing to do, whatever the pointers
    for args, msg in (((16, 16, 16, -1), b"negative element count -1"), ((None, 16, 16, 64), b"null argument"),
                      ((16, None, 16, 64), b"null argument"), ((16, 16, None, 64), b"null argument"),
                      ((18, 16, 16, 32), b"4-byte aligned"), ((16, 16, 17, 32), b"4-byte aligned")):
        assert lib.icv_add_noise_f32(*args, 0.5, 0, None) != 0 and msg in lib.icv_last_error(), args
