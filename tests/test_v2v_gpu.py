"""Video-to-video on the HIP path: icv_add_noise_f32 against its torch restatement bit for bit (every size class, every
pointer-misalignment class, both rounding modes, in place over either input, between guard bands), its contract, the HIP
pipeline against the engine driven by hand and against upstream's loop restated in fp32 on the GPU, every driver mode from the
same noised latent, 125 frames in two windows through the Wan-VAE architecture with the unchanged generator, and the kernel's
time at the 14B 480p latent size next to a device copy of the same bytes."""

import numpy as np
import pytest
import torch

from infinicube_amd.videogen import synthetic as syn
from infinicube_amd.videogen.config import TokenGrid
from infinicube_amd.videogen.dit import WanDiT
from infinicube_amd.videogen.pipeline import DiTHolder, WanVideoPipeline
from infinicube_amd.videogen.scheduler import FlowMatchScheduler
from oracle import wan_ref as R
from standins import HashTextEncoder, PoolVAE
from test_buffer_edges_gpu import Arena
from test_v2v_cpu import (CFG, ENV, SHORT, _call_kw, add_noise_twin, drive_by_hand, generator_through_env, make_clip, oracle_inputs, pil,
                          v2v_reference)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SIZES = (1, 2, 3, 4, 5, 63, 64, 65, 257, 4099)       # below one vector, around one wave of vectors, more than one block, ragged
# float offsets of (x0, noise, out) from a 256-byte boundary: all equal (the vector body with a head of 0, 3, 2, 1 elements),
# all different, and two equal with the third off (each pointer in turn) - the scalar path
OFFSETS = ((0, 0, 0), (1, 1, 1), (2, 2, 2), (3, 3, 3), (0, 1, 2), (1, 2, 3), (3, 0, 1), (2, 3, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (2, 2, 3))
SIGMAS = (0.0, 1.0, 0.5, FlowMatchScheduler(50, 5.0, denoising_strength=0.05).sigmas[0], FlowMatchScheduler(50, 5.0, denoising_strength=0.6).sigmas[0])


def _data(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g), torch.randn(n, generator=g)


def run_add_noise(hip_ops, n, offs, sigma, rounding, alias=None):
    """One launch on buffers carved out of a sentinel-filled arena.  ``alias``: None | "noise" | "x0" = the input ``out`` is."""
    x0, noise = _data(n, 1000 * n + 7)
    want = torch.empty(n)
    add_noise_twin(x0, noise, want, sigma, rounding)
    ar = Arena(nbytes=1 << 16)
    bx = ar.carve(np.float32, n, offs[0])
    bn = ar.carve(np.float32, n, offs[1])
    bo = {None: None, "noise": bn, "x0": bx}[alias] or ar.carve(np.float32, n, offs[2])
    tx, tn, to = bx.tensor((n,)), bn.tensor((n,)), bo.tensor((n,))
    tx.copy_(x0)
    tn.copy_(noise)
    assert tx.data_ptr() % 16 == 4 * offs[0] and tn.data_ptr() % 16 == 4 * offs[1]
    before = ar.snapshot()
    hip_ops.add_noise(tx, tn, to, sigma, round_bf16=rounding)
    ar.check(before, [bo])                         # guard bands and everything that is not ``out`` (the other inputs included)
    got = to.cpu()
    assert torch.equal(got, want), (f"n={n} offsets={offs} sigma={sigma} round_bf16={rounding} out={alias or 'own'}: "
                                    f"{int((got != want).sum())} of {n} differ, first at {int((got != want).nonzero()[0])}")
    return got


@pytest.mark.parametrize("alias", [None, "noise", "x0"], ids=["out", "out-is-noise", "out-is-x0"])
@pytest.mark.parametrize("offs", OFFSETS, ids=["".join(map(str, o)) for o in OFFSETS])
def test_kernel_matches_twin(hip_ops, offs, alias):
    for n in SIZES:
        for sigma in SIGMAS:
            exact = run_add_noise(hip_ops, n, offs, sigma, False, alias)
            rounded = run_add_noise(hip_ops, n, offs, sigma, True, alias)
            if n >= 63 and 0.0 < sigma < 1.0:
                assert not torch.equal(exact, rounded), "reference rounding must differ from the exact path"


def test_sigma_one_returns_the_noise_and_sigma_zero_the_clip(hip_ops):
    """sigma = 1: (1 - 1) * x0 is 0 for any finite x0 (1e30 here), so the output is the noise; sigma = 0 likewise gives x0.  This
    is what makes denoising_strength = 1.0 with an input video the plain call."""
    n = 4099
    _, noise = _data(n, 5)
    big = torch.full((n,), 1e30)
    big[::2] = -1e30
    for rounding in (False, True):
        src = noise.to(torch.bfloat16).float() if rounding else noise      # what the pipeline hands over under reference rounding
        for offs in ((0, 0, 0), (1, 2, 3)):
            ar = Arena(nbytes=1 << 16)
            tx, tn, to = (ar.carve(np.float32, n, o).tensor((n,)) for o in offs)
            tx.copy_(big)
            tn.copy_(src)
            hip_ops.add_noise(tx, tn, to, 1.0, round_bf16=rounding)
            assert torch.equal(to.cpu(), src)
            hip_ops.add_noise(tn, tx, to, 0.0, round_bf16=rounding)       # x0 = src, noise = 1e30
            assert torch.equal(to.cpu(), src)


def test_contract(hip_ops):
    from infinicube_amd import native
    lib, st = native.lib(), torch.cuda.current_stream().cuda_stream
    ar = Arena(nbytes=1 << 14)
    bx, bn, bo = (ar.carve(np.float32, 64, 0) for _ in range(3))
    bx.tensor((64,)).copy_(torch.ones(64))
    bn.tensor((64,)).copy_(torch.ones(64))
    before = ar.snapshot()
    # n == 0: nothing is launched, nothing is written - through the C ABI (null pointers included) and through the operator
    assert lib.icv_add_noise_f32(bx.ptr, bn.ptr, bo.ptr, 0, 0.5, 0, st) == 0
    assert lib.icv_add_noise_f32(None, None, None, 0, 0.5, 0, st) == 0
    e = torch.empty(0, device=DEV)
    hip_ops.add_noise(e, e, e, 0.5)
    # bad arguments: an icv_last_error message and no launch
    for args, msg in (((bx.ptr, bn.ptr, bo.ptr, -1), b"negative element count"), ((None, bn.ptr, bo.ptr, 64), b"null argument"),
                      ((bx.ptr, None, bo.ptr, 64), b"null argument"), ((bx.ptr, bn.ptr, None, 64), b"null argument"),
                      ((bx.ptr + 2, bn.ptr, bo.ptr, 32), b"4-byte aligned"), ((bx.ptr, bn.ptr, bo.ptr + 1, 32), b"4-byte aligned")):
        assert lib.icv_add_noise_f32(*args, 0.5, 0, st) != 0 and msg in lib.icv_last_error(), args
    ar.check(before, [])
    # the operator's own checks
    f = torch.zeros(8, device=DEV)
    with pytest.raises(TypeError, match="add_noise.x0"):
        hip_ops.add_noise(f.to(torch.bfloat16), f, f, 0.5)
    with pytest.raises(TypeError, match="add_noise.out"):
        hip_ops.add_noise(f, f, f.double(), 0.5)
    with pytest.raises(ValueError, match="must have one shape"):
        hip_ops.add_noise(f[:4], f, f, 0.5)
    with pytest.raises(ValueError, match="innermost dimension must be contiguous"):
        hip_ops.add_noise(f[::2], f[::2], f[::2], 0.5)


# ---- the pipeline --------------------------------------------------------------------------------------------------------------------
def _pipe(hip_ops, vae=None, buffers=True):
    p = WanVideoPipeline(DEV, torch.bfloat16, DiTHolder(syn.make_dit_state_dict(CFG), CFG), HashTextEncoder(CFG), vae or PoolVAE(), ops=hip_ops)
    if buffers:
        p.initialize_buffer_embedder(16, zero_init=False)
    return p


@pytest.mark.parametrize("rounding", [False, True])
def test_hip_pipeline_equals_engine_driven_by_hand(hip_ops, rounding, monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    p = _pipe(hip_ops)
    p.reference_rounding = rounding
    clip, kw = pil(make_clip(SHORT, 1)), _call_kw()
    base = p(**kw)
    assert p.v2v_record is None
    one = p(**kw, input_video=clip, denoising_strength=1.0)
    assert torch.equal(one, base) and p.v2v_record == dict(denoising_strength=1.0, sigma_0=1.0)
    got = p(**kw, input_video=clip, denoising_strength=0.6)
    want = drive_by_hand(p, hip_ops, kw, clip, 0.6)                       # start latent from the torch twin, on the device
    torch.cuda.synchronize()
    assert torch.equal(got, want), f"max |d| {float((got - want).abs().max())}"
    assert torch.isfinite(got).all() and not torch.equal(got, base)
    assert not torch.equal(got, p(**kw, input_video=pil(make_clip(SHORT, 2)), denoising_strength=0.6))


def test_hip_pipeline_matches_restated_upstream_loop(hip_ops, monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    p = _pipe(hip_ops)
    clip, kw = pil(make_clip(SHORT, 1)), _call_kw()
    got = p(**kw, input_video=clip, denoising_strength=0.6)
    o = oracle_inputs(p, kw, clip, dev=DEV)
    ref = v2v_reference(o["sd"], o["bsd"], CFG, o["x0"], o["noise"], o["c1"], o["c2"], o["bl"], 2, 0.6)
    db = R.psnr(got.cpu(), ref.cpu())
    print(f"HIP v2v pipeline (strength 0.6, 2 steps) vs the loop restated in fp32 on the GPU: {db:.1f} dB")
    assert db >= 40.0, f"{db:.1f} dB"
    t2v = v2v_reference(o["sd"], o["bsd"], CFG, None, o["noise"], o["c1"], o["c2"], o["bl"], 2, 1.0)
    assert R.psnr(got.cpu(), t2v.cpu()) < db - 10.0, "the result must start from the encoded clip, not from pure noise"


FP8 = dict(gemm_dtype="fp8", attn_dtype="fp8", fp8_weights=WanDiT.FP8_WEIGHTS)


def _sequential(m):
    m.cfg_batch = False


@pytest.mark.parametrize("mode", ["pair", "pair-no-stem", "native", "graphs", "dual-stream", "fp8-pair", "reference-rounding"])
def test_driver_modes_match_sequential_loop(hip_ops, mode, monkeypatch):
    """Nothing inside denoise knows about the feature: from the same noised latent (the kernel's) every driver mode the window
    tests enumerate gives the sequential loop's bits over the shortened range."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    p = _pipe(hip_ops)
    p.reference_rounding = mode == "reference-rounding"
    clip, kw = pil(make_clip(SHORT, 1)), _call_kw(num_inference_steps=4)
    ekw = FP8 if mode.startswith("fp8") else None
    run = lambda **more: drive_by_hand(p, hip_ops, kw, clip, 0.6, engine_kw=ekw, noise_op=hip_ops.add_noise, **more)   # noqa: E731
    ref = run(setup=_sequential, prep=dict(graphs=False))
    prep, setup, seen = dict(graphs=False), None, {}

    def look(check):
        return lambda m: (seen.update(m=m), check(m))[1]

    if mode == "pair-no-stem":
        setup = lambda m: setattr(m, "share_stem", False)                        # noqa: E731
    elif mode == "native":
        setup = lambda m: setattr(m, "native_forward", True)                     # noqa: E731
    elif mode == "graphs":
        prep = dict(graphs=True)
    elif mode == "dual-stream":
        monkeypatch.setenv("ICV_DUAL_STREAM", "1")
    got = run(setup=look(setup or (lambda m: None)), prep=prep)
    torch.cuda.synchronize()
    m = seen["m"]
    assert torch.isfinite(got).all()
    if mode in ("pair", "pair-no-stem", "fp8-pair", "reference-rounding"):
        assert m._pair is not None
    if mode == "native":
        assert m.native_forward
    if mode == "graphs":
        assert m._graphs_on and m._graphs
    if mode == "dual-stream":
        assert m.dual_stream and m._twin is not None
    assert torch.equal(got, ref), f"{mode}: max |d| {float((got - ref).abs().max())}"
    if mode == "reference-rounding":
        p.reference_rounding = False
        assert not torch.equal(got, run(setup=_sequential, prep=dict(graphs=False)))


# ---- 125 frames, two windows, the Wan-VAE architecture, the unchanged generator ---------------------------------------------------------
LONG = TokenGrid(125, 64, 96)          # 32 latent frames
LONG_TILES = dict(tile_size=(8, 8), tile_stride=(4, 4))


def _tiny_vae_net():
    """tests/test_sliding_window_gpu.py's tiny Wan-VAE (the real architecture at width 32, bf16-representable weights), restated."""
    from infinicube_amd.videogen import vae as V
    torch.manual_seed(4)
    net = V.WanVAENet(dim=32, z_dim=16).eval()
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(p.to(torch.bfloat16).float())
    return net


def _long_pipe(hip_ops, captured=None):
    from infinicube_amd.videogen import vae as V
    vae = V.WanVAE(_tiny_vae_net(), torch.device(DEV))
    if captured is not None:
        decode = vae.decode
        vae.decode = lambda latent, *a, **k: (captured.append(latent.detach().clone()), decode(latent, *a, **k))[1]
    p = _pipe(hip_ops, vae=vae, buffers=False)
    p.num_inference_steps = 2
    return p


def test_long_clip_two_windows_and_generator(hip_ops, tmp_path, monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    clip = make_clip(LONG, 1)
    sem, co = syn.make_dummy_buffers(LONG)
    p = _long_pipe(hip_ops)
    p.initialize_buffer_embedder(16, zero_init=True)
    p.buffer_embedder.load_state_dict(syn.make_buffer_embedder_state_dict(CFG))
    kw = dict(prompt="a street", negative_prompt="bad", semantic_buffer_video=pil(sem), coordinate_buffer_video=pil(co), height=LONG.height,
              width=LONG.width, num_frames=125, seed=3, return_latents=True, sliding_window_size=24, sliding_window_stride=8, **LONG_TILES)
    got = p(**kw, input_video=pil(clip), denoising_strength=0.6)
    assert p.sliding_window_record == [(0, 24), (8, 32)] and p.v2v_record["denoising_strength"] == 0.6
    assert tuple(got.shape) == LONG.latent_shape() and torch.isfinite(got).all()
    t2v = p(**kw)
    assert p.v2v_record is None and not torch.equal(got, t2v)
    # strength 1.0: three clips through the tiled VAE instead of two, the same latent bits as without the clip
    assert torch.equal(p(**kw, input_video=pil(clip)), t2v)
    # the unchanged generator: the two variables (and the window pair) in the environment give the keyword call's latent
    monkeypatch.setenv("ICV_SLIDING_WINDOW_SIZE", "24")
    monkeypatch.setenv("ICV_SLIDING_WINDOW_STRIDE", "8")
    captured = []
    g, video = generator_through_env(lambda torch_dtype, device, model_configs: _long_pipe(hip_ops, captured), tmp_path, monkeypatch, "npy",
                                     clip, LONG, DEV)
    assert len(video) == 125 and video[0].size == (LONG.width, LONG.height)
    assert g.pipe.sliding_window_record == [(0, 24), (8, 32)] and g.pipe.v2v_record["denoising_strength"] == 0.6
    assert np.stack([np.asarray(f) for f in video]).std() > 0


def test_long_clip_generator_latent_equals_keyword_call(hip_ops, tmp_path, monkeypatch):
    """Default tiles (the generator passes none): the latent the generator decodes is the keyword call's."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    grid = TokenGrid(33, 64, 96)
    clip = make_clip(grid, 2)
    sem, co = syn.make_dummy_buffers(grid)
    p = _long_pipe(hip_ops)
    p.initialize_buffer_embedder(16, zero_init=True)
    p.buffer_embedder.load_state_dict(syn.make_buffer_embedder_state_dict(CFG))
    want = p(prompt="a street", negative_prompt="bad", semantic_buffer_video=pil(sem), coordinate_buffer_video=pil(co), height=grid.height,
             width=grid.width, num_frames=grid.num_frames, seed=3, return_latents=True, input_video=pil(clip), denoising_strength=0.6)
    captured = []
    g, video = generator_through_env(lambda torch_dtype, device, model_configs: _long_pipe(hip_ops, captured), tmp_path, monkeypatch, "dir",
                                     clip, grid, DEV)
    assert len(video) == grid.num_frames and len(captured) == 1
    assert torch.equal(captured[0], want)


# ---- the kernel at the 14B 480p latent size ------------------------------------------------------------------------------------------
def test_kernel_at_the_14b_480p_latent_size(hip_ops):
    """16 x 24 x 60 x 104 floats in place over the noise, bit-equal to the twin run on the device, and its time next to a device
    copy of the same bytes (HIP events, median of 5 after a warm-up).  No threshold on the time (DESIGN.md §12 records it)."""
    shape = (16, 24, 60, 104)
    g = torch.Generator(device=DEV).manual_seed(11)
    x0, noise = torch.randn(shape, generator=g, device=DEV), torch.randn(shape, generator=g, device=DEV)
    sigma = SIGMAS[4]
    for rounding in (False, True):
        want = torch.empty_like(noise)
        add_noise_twin(x0, noise, want, sigma, rounding)
        got = noise.clone()
        hip_ops.add_noise(x0, got, got, sigma, round_bf16=rounding)
        assert torch.equal(got, want)

    def timed(fn, reps=5):
        fn()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        return sorted(ts)[reps // 2]

    lat, dst = noise.clone(), torch.empty_like(noise)
    t_kernel = timed(lambda: hip_ops.add_noise(x0, lat, lat, sigma))
    t_copy = timed(lambda: dst.copy_(noise))
    mb = noise.numel() * 4 / 1e6
    print(f"icv_add_noise_f32 on {shape} ({mb:.1f} MB per tensor; reads two, writes one): {t_kernel * 1e3:.1f} us; a device copy of one "
          f"tensor (reads one, writes one): {t_copy * 1e3:.1f} us; kernel / copy {t_kernel / t_copy:.2f}")
