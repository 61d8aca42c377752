"""Sliding temporal windows on the HIP path: icv_unpatchify_cfg_euler_window against its torch twin (exact and reference
rounding), its write guard and the partition-of-unity check against icv_unpatchify_cfg_euler, the windowed loop against the
torch restatement of upstream's loop and against the loop spelled out with plain forwards, every driver mode, one window = the
plain loop, the pipeline and the unchanged generator on a 125-frame clip through the Wan-VAE architecture, and one step at the
product's per-window token count against the fp32 oracle."""
import contextlib
import io
import time

import numpy as np
import pytest
import torch

from infinicube_amd.videogen import sliding_window as SW
from infinicube_amd.videogen import synthetic as syn
from infinicube_amd.videogen.config import TokenGrid, preset
from infinicube_amd.videogen.dit import WanDiT
from infinicube_amd.videogen.scheduler import FlowMatchScheduler
from oracle import wan_ref as R
from test_sliding_window_cpu import (CFG, ENV, GRID, _inputs, _window_loop, manual_window_loop, sliding_window_reference,
                                     window_euler_twin)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---- 6. the kernel against its twin ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_hu", [True, False])
def test_window_kernel_matches_twin(hip_ops, with_hu):
    """Non-zero frame0, a token sub-range that starts and ends inside a frame, head outputs with a row stride.  Exact path:
    atol 1e-5 on unit-variance inputs (the bar of test_patchify_and_unpatchify_euler); reference rounding: the twin's bits."""
    torch.manual_seed(5)
    C, T, H8, W8 = 16, 7, 12, 20
    per_frame = (H8 // 2) * (W8 // 2)
    frame0, frames, tok0, n_tok = 2, 4, 37, 150
    lat = torch.randn(C, T, H8, W8, device=DEV)
    hcb, hub = torch.randn(n_tok, 4 * C + 32, device=DEV), torch.randn(n_tok, 4 * C + 32, device=DEV)
    hc, hu = hcb[:, : 4 * C], (hub[:, : 4 * C] if with_hu else None)
    coef = torch.rand(frames, device=DEV)
    assert tok0 + n_tok <= frames * per_frame
    outs = {}
    for rounding in (False, True):
        got, want = lat.clone(), lat.clone()
        hip_ops.unpatchify_cfg_euler_window(got, hc, hu, 5.0, -0.07, coef, frame0, tok0, n_tok, round_bf16=rounding)
        torch.cuda.synchronize()
        window_euler_twin(want, hc, hu, 5.0, -0.07, coef, frame0, tok0, n_tok, round_bf16=rounding)
        d = float((got - want).abs().max())
        print(f"window kernel vs twin (hu={with_hu}, round_bf16={rounding}): max |d| {d:.3g}")
        if rounding:
            assert torch.equal(got, want), f"reference rounding: max |d| {d}"
        else:
            assert d <= 1e-5
        assert not torch.equal(got, lat)
        outs[rounding] = got
    assert not torch.equal(outs[True], outs[False]), "reference rounding must differ from the exact path"
    # argument checks happen on the host, before any launch
    with pytest.raises(Exception, match="outside the 7-frame latent"):
        hip_ops.unpatchify_cfg_euler_window(lat.clone(), hc, hu, 5.0, -0.07, torch.rand(6, device=DEV), 5, 0, 150)
    with pytest.raises(ValueError, match="frame coefficients do not cover"):
        hip_ops.unpatchify_cfg_euler_window(lat.clone(), hc, hu, 5.0, -0.07, coef[:2], frame0, tok0, n_tok)


# ---- 7. guard and partition of unity ----------------------------------------------------------------------------------------------
def test_window_kernel_writes_only_its_tokens(hip_ops):
    torch.manual_seed(6)
    C, T, H8, W8 = 16, 7, 12, 20
    Hp, Wp = H8 // 2, W8 // 2
    frame0, tok0, n_tok = 3, 61, 100
    lat = torch.randn(C, T, H8, W8, device=DEV)
    hc, hu = torch.randn(n_tok, 4 * C, device=DEV) + 3.0, torch.randn(n_tok, 4 * C, device=DEV)
    got = lat.clone()
    hip_ops.unpatchify_cfg_euler_window(got, hc, hu, 5.0, -0.1, torch.ones(4, device=DEV), frame0, tok0, n_tok)
    torch.cuda.synchronize()
    mine = torch.zeros((T * Hp * Wp, 4 * C))
    mine[frame0 * Hp * Wp + tok0: frame0 * Hp * Wp + tok0 + n_tok] = 1.0
    mine = (R.unpatchify(mine, (T, Hp, Wp), C) > 0).to(DEV)
    assert torch.equal(got[~mine], lat[~mine]), "elements outside the window's token range were written"
    assert (got[mine] != lat[mine]).float().mean() > 0.99


@pytest.mark.parametrize("size,stride", [(4, 2), (4, 1), (3, 3)])
def test_windows_reproduce_the_plain_euler_step(hip_ops, size, stride):
    """Windows whose coefficients sum to 1, fed the same velocity on shared frames, give icv_unpatchify_cfg_euler on the whole latent
    to f32 rounding.  Bound, per element, u = 2^-24, k = ceil(size / stride) = the most addends a frame gets, vd = v * dsigma:
      * each c_w carries one rounding (f64 -> f32) and each product c_w * vd one more, and sum c_w = 1 to k u: 3 k u |vd|;
      * k accumulations here against one in the plain kernel, each rounding a partial sum no larger than |l| + |vd|: (k + 1) u (|l| + |vd|);
      * the plain kernel may contract u + cfg * (c - u) and l + v * dsigma into fused multiply-adds, this one's last two operations
        are not contracted: 2 u (|dsigma cfg (c - u)| + |vd|).
    Together <= (4 k + 5) u (|l| + |vd| + |dsigma cfg (c - u)|)."""
    torch.manual_seed(7)
    C, T, H8, W8 = 16, 9, 8, 12
    Hp, Wp = H8 // 2, W8 // 2
    pf, S = Hp * Wp, T * Hp * Wp
    plan = SW.plan(T, size, stride)
    lat = torch.randn(C, T, H8, W8, device=DEV)
    hc, hu = torch.randn(S, 4 * C, device=DEV), torch.randn(S, 4 * C, device=DEV)
    cfg, dsigma = 5.0, -0.0625
    want = lat.clone()
    hip_ops.unpatchify_cfg_euler(want, hc, hu, cfg, dsigma, 0, S)
    got = lat.clone()
    coef = torch.from_numpy(plan.coef).float().to(DEV)
    for w, (f0, f1) in enumerate(plan.windows):
        hip_ops.unpatchify_cfg_euler_window(got, hc[f0 * pf: f1 * pf], hu[f0 * pf: f1 * pf], cfg, dsigma, coef[w], f0, 0, (f1 - f0) * pf)
    torch.cuda.synchronize()
    k = -(-size // stride)
    cd, ud = hc.double().cpu(), hu.double().cpu()
    scale_tok = (dsigma * (ud + cfg * (cd - ud))).abs() + (dsigma * cfg * (cd - ud)).abs()
    mag = lat.double().cpu().abs() + R.unpatchify(scale_tok, (T, Hp, Wp), C)
    err = (got.double().cpu() - want.double().cpu()).abs()
    ulps = float((err / (2.0 ** -24 * mag)).max())
    print(f"windows {size}/{stride} vs plain Euler step: worst error {ulps:.2f} u * magnitude, bound {4 * k + 5}")
    assert (err <= (4 * k + 5) * 2.0 ** -24 * mag).all(), f"worst {ulps:.2f} u"


# ---- 8. the loop -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,stride", [(4, 2), (4, 1)])
def test_hip_loop_matches_restatement(hip_ops, size, stride):
    """Test 3's shape on the GPU (9 latent frames, CFG, 6 steps): latent PSNR >= 40 dB against the torch restatement of upstream's
    loop (the project's loop bar), and the same bits as the loop spelled out with plain forwards on the cut-out windows."""
    sd, bsd, noise, c1, c2, bl = _inputs()
    m, lat = _window_loop(hip_ops, size, stride, dev=DEV)
    torch.cuda.synchronize()
    assert m._pair is not None, "the default driver is the CFG-batched pair"
    assert sorted(m._win_engines) == ([3] if stride == 2 else [])
    ref = sliding_window_reference(R.round_state_dict_to_bf16(sd), R.round_state_dict_to_bf16(bsd), CFG, noise, c1, c2, bl, 6, size, stride)
    p = R.psnr(lat.cpu(), ref)
    print(f"HIP sliding-window loop {size}/{stride} vs restatement: {p:.1f} dB")
    assert p >= 40.0, f"{p:.1f} dB"
    engines = {}

    def m_of(frames):
        if frames not in engines:
            engines[frames] = WanDiT(CFG, sd, hip_ops, bsd).prepare(TokenGrid(4 * (frames - 1) + 1, GRID.height, GRID.width), graphs=False)
        return engines[frames]

    ck, cu = m_of(size).encode_context(c1), m_of(size).encode_context(c2)
    want = manual_window_loop(m_of, hip_ops, noise, ck, cu, bl, 6, size, stride, hip_ops.unpatchify_cfg_euler_window, dev=DEV)
    torch.cuda.synchronize()
    assert torch.equal(lat, want), f"max |d| vs the spelled-out loop {float((lat - want).abs().max())}"


FP8 = dict(gemm_dtype="fp8", attn_dtype="fp8", fp8_weights=WanDiT.FP8_WEIGHTS)


def _sequential(m):
    m.cfg_batch = False


@pytest.mark.parametrize("mode", ["pair", "pair-no-stem", "native", "graphs", "dual-stream", "fp8-pair", "reference-rounding"])
def test_driver_modes_match_sequential_loop(hip_ops, mode, monkeypatch):
    """Every driver mode runs the windows: bit-identical to the sequential windowed loop (ICV_CFG_BATCH=0), as the existing tests
    demand between those modes of the plain loop.  The one-call C driver does not cover a window offset: the per-op driver runs."""
    kw = FP8 if mode.startswith("fp8") else None
    _, ref = _window_loop(hip_ops, 4, 2, setup=_sequential, prep=dict(graphs=False), kw=kw, dev=DEV)
    prep, setup = dict(graphs=False), None
    if mode == "pair-no-stem":
        setup = lambda m: setattr(m, "share_stem", False)                        # noqa: E731
    elif mode == "native":
        setup = lambda m: setattr(m, "native_forward", True)                     # noqa: E731
    elif mode == "graphs":
        prep = dict(graphs=True)
    elif mode == "dual-stream":
        monkeypatch.setenv("ICV_DUAL_STREAM", "1")
    m, got = _window_loop(hip_ops, 4, 2, setup=setup, prep=prep, kw=kw, dev=DEV)
    torch.cuda.synchronize()
    assert torch.isfinite(got).all()
    if mode in ("pair", "pair-no-stem", "fp8-pair"):
        assert m._pair is not None and m._win_engines[3]._pair is not None
    if mode == "native":
        assert m.native_forward and m._native is None and m._win_engines[3]._native is None
    if mode == "graphs":
        assert m._graphs_on and m._win_engines[3]._graphs_on
        assert {k[6] for k in m._graphs} == {0, 2 * 24, 4 * 24}, "one graph per window offset"
    if mode == "dual-stream":
        assert m.dual_stream and m._twin is not None
    if mode == "reference-rounding":
        sd, bsd, noise, c1, c2, bl = _inputs()
        outs = []
        for batch in (False, True):
            e = WanDiT(CFG, sd, hip_ops, bsd).prepare(TokenGrid(13, GRID.height, GRID.width), graphs=False)
            e.cfg_batch = batch
            lat = noise.clone().to(DEV)
            e.denoise(lat, e.encode_context(c1), e.encode_context(c2), e.embed_buffers(bl, whole_clip=True), FlowMatchScheduler(6), 5.0,
                      round_bf16=True, sliding_window=SW.plan(GRID.T, 4, 2))
            outs.append(lat)
        torch.cuda.synchronize()
        assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], ref)
        return
    assert torch.equal(got, ref), f"{mode}: max |d| {float((got - ref).abs().max())}"


# ---- 9. one window -----------------------------------------------------------------------------------------------------------------
def test_one_window_is_the_plain_hip_loop(hip_ops):
    sd, bsd, noise, c1, c2, bl = _inputs()
    lats = []
    for kw in ({}, dict(sliding_window=None), dict(sliding_window=SW.plan(GRID.T, 9, 4)), dict(sliding_window=SW.plan(GRID.T, 24, 12))):
        m = WanDiT(CFG, sd, hip_ops, bsd).prepare(GRID)
        lat = noise.clone().to(DEV)
        m.denoise(lat, m.encode_context(c1), m.encode_context(c2), m.embed_buffers(bl), FlowMatchScheduler(6), 5.0, **kw)
        torch.cuda.synchronize()
        assert m._win_next is None and not m._win_engines, "one window must allocate nothing"
        lats.append(lat.cpu())
    assert all(torch.equal(lats[0], x) for x in lats[1:])


# ---- 10. pipeline and generator, 125 frames through the Wan-VAE architecture -------------------------------------------------------
LONG = TokenGrid(125, 64, 96)          # 32 latent frames
TILES = dict(tile_size=(8, 8), tile_stride=(4, 4))


def _tiny_vae_net():
    from infinicube_amd.videogen import vae as V
    torch.manual_seed(4)
    net = V.WanVAENet(dim=32, z_dim=16).eval()
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(p.to(torch.bfloat16).float())
    return net


def _pipe(vae=None):
    from infinicube_amd.videogen import vae as V
    from infinicube_amd.videogen.ops import HipOps
    from infinicube_amd.videogen.pipeline import DiTHolder, WanVideoPipeline
    from standins import HashTextEncoder
    p = WanVideoPipeline(DEV, torch.bfloat16, DiTHolder(syn.make_dit_state_dict(CFG), CFG), HashTextEncoder(CFG),
                         vae or V.WanVAE(_tiny_vae_net(), torch.device(DEV)), ops=HipOps(DEV))
    p.num_inference_steps = 2
    return p


def long_factory(torch_dtype, device, model_configs):
    return _pipe()


def _net_close(got, ref, what, rel_bound=2e-2):
    """The bar of tests/test_vae_hip_gpu.py::test_hip_path_equals_miopen_path_within_bf16 (its _net_close)."""
    got, ref = got.float().cpu(), ref.float().cpu()
    rel = float((got - ref).norm() / ref.norm())
    cos = float(torch.nn.functional.cosine_similarity(got.flatten(), ref.flatten(), dim=0))
    print(f"{what}: rel-L2 {rel:.3g}, cosine {cos:.6f}")
    assert rel <= rel_bound and cos >= 0.999, f"{what}: rel-L2 {rel}, cosine {cos}"


def test_long_clip_vae_hip_equals_miopen(monkeypatch):
    """The Wan-VAE path has no 93-frame cap but had never been run longer: 125-frame encode / decode on libicvideo's convolutions
    against the same modules on stock PyTorch."""
    import copy
    from infinicube_amd.videogen import vae as V
    net = _tiny_vae_net()
    a = V.WanVAE(copy.deepcopy(net), torch.device(DEV))
    monkeypatch.setenv("ICV_VAE_CONV", "miopen")
    b = V.WanVAE(copy.deepcopy(net), torch.device(DEV))
    assert a.hip is not None and b.hip is None
    torch.manual_seed(9)
    clip = torch.rand(3, LONG.num_frames, LONG.height, LONG.width) * 2 - 1
    ea, eb = a.encode(clip, tiled=True, **TILES), b.encode(clip, tiled=True, **TILES)
    assert tuple(ea.shape) == LONG.latent_shape()
    _net_close(ea, eb, "125-frame tiled encode: HIP convolutions vs MIOpen")
    lat = torch.randn(LONG.latent_shape())
    va, vb = a.decode(lat, tiled=True, **TILES), b.decode(lat, tiled=True, **TILES)
    assert tuple(va.shape) == (3, LONG.num_frames, LONG.height, LONG.width)
    _net_close(va, vb, "125-frame tiled decode: HIP convolutions vs MIOpen")


def test_pipeline_and_generator_long_clip(tmp_path, monkeypatch):
    from safetensors.torch import save_file
    from infinicube.videogen import WanVideoGenerator
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    sem, co = syn.make_dummy_buffers(LONG)
    assert sem.shape[0] == 125
    from PIL import Image
    p = _pipe()
    p.initialize_buffer_embedder(16, zero_init=False)
    kw = dict(prompt="a street", negative_prompt="bad", semantic_buffer_video=[Image.fromarray(f) for f in sem],
              coordinate_buffer_video=[Image.fromarray(f) for f in co], height=LONG.height, width=LONG.width, num_frames=125, seed=3, **TILES)
    frames = p(**kw, sliding_window_size=24, sliding_window_stride=8)
    assert len(frames) == 125 and frames[0].size == (LONG.width, LONG.height)
    assert p.sliding_window_record == [(0, 24), (8, 32)]
    assert p._engine.grid.T == 24 and sorted(p._engine._win_engines) == []
    win = p(**kw, sliding_window_size=24, sliding_window_stride=8, return_latents=True).cpu()
    full = p(**kw, return_latents=True).cpu()
    assert p.sliding_window_record is None and p._engine.grid.T == 32
    assert torch.isfinite(win).all() and win.shape == full.shape and not torch.equal(win, full)
    # the unchanged generator: a caller that stops cutting to 93 frames and sets the two variables gets the long clip
    path = str(tmp_path / "step-1.safetensors")
    save_file({"buffer_embedder." + k: v for k, v in syn.make_buffer_embedder_state_dict(CFG).items()}, path)
    monkeypatch.setenv("ICV_SLIDING_WINDOW_SIZE", "24")
    monkeypatch.setenv("ICV_SLIDING_WINDOW_STRIDE", "16")
    import test_sliding_window_gpu as me
    with contextlib.redirect_stdout(io.StringIO()):
        g = WanVideoGenerator(path, device=DEV, use_wan_1pt3b=True, pipeline_factory=me.long_factory)
        video = g.generate(sem, co, seed=3)
    assert len(video) == 125 and g.pipe.sliding_window_record == [(0, 24), (16, 32)]
    assert sorted(g.pipe._engine._win_engines) == [16], "the shorter last window has a workspace of its own"
    assert np.stack([np.asarray(f) for f in video]).std() > 0


# ---- 11. the product's per-window token count ----------------------------------------------------------------------------------------
def test_wan_1p3b_480p_125_frames_two_windows_one_step(hip_ops):
    """Wan2.1-1.3B, 480x832, 125 frames = 32 latent frames, size 24 / stride 8 -> two windows of config #2's grid (S = 37 440 each), ONE
    step with CFG, against the restatement run in fp32 on the GPU by stock PyTorch: latent PSNR >= 40 dB."""
    cfg, grid = preset("1.3b"), TokenGrid(125, 480, 832)
    sd = syn.make_dit_state_dict(cfg, seed=0, dtype=torch.bfloat16)
    bsd = syn.make_buffer_embedder_state_dict(cfg, dtype=torch.bfloat16)
    noise, bl = syn.make_latent_noise(grid), syn.make_buffer_latents(cfg, grid)
    c1, c2 = syn.make_text_context(cfg, 1), syn.make_text_context(cfg, 2)
    plan = SW.plan(grid.T, 24, 8)
    assert plan.windows == ((0, 24), (8, 32))
    m = WanDiT(cfg, sd, hip_ops, bsd).prepare(TokenGrid(93, 480, 832))
    lat = noise.clone().to(DEV)
    t0 = time.time()
    m.denoise(lat, m.encode_context(c1), m.encode_context(c2), m.embed_buffers(bl, whole_clip=True), FlowMatchScheduler(1), 5.0,
              sliding_window=plan)
    torch.cuda.synchronize()
    t_hip = time.time() - t0
    assert not m._win_engines
    lat = lat.cpu()
    del m
    torch.cuda.empty_cache()
    sdr = {k: v.float().to(DEV) for k, v in sd.items()}
    bsdr = {k: v.float().to(DEV) for k, v in bsd.items()}
    t0 = time.time()
    ref = sliding_window_reference(sdr, bsdr, cfg, noise.to(DEV), c1.to(DEV), c2.to(DEV), bl.to(DEV), 1, 24, 8)
    torch.cuda.synchronize()
    t_ref = time.time() - t0
    p = R.psnr(lat, ref.cpu())
    cos = float(torch.nn.functional.cosine_similarity((lat - noise).flatten().double(), (ref.cpu() - noise).flatten().double(), dim=0))
    line = (f"1.3B 480x832 125 frames, two windows of S = 37 440, one step: HIP {t_hip:.1f}s, fp32 torch restatement on GPU {t_ref:.1f}s; "
            f"latent PSNR {p:.1f} dB, update cosine {cos:.5f}")
    print(line)
    assert p >= 40.0, line
