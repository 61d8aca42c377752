"""Sliding temporal windows (infinicube_amd/videogen/sliding_window.py) on CPU: the window plan and its blend coefficients
against a line-by-line restatement of upstream DiffSynth's ``TemporalTiler_BCTHW``, validation and where the settings come
from, the host loop (dit.WanDiT.denoise(sliding_window=)) on the TEST-ONLY oracle operator set against an independent torch
restatement built from oracle.wan_ref pieces, one window = the plain loop (bits and launches), and off = nothing new."""
import numpy as np
import pytest
import torch

from dit_launch_trace import Trace, TracedOps
from infinicube_amd.videogen import options
from infinicube_amd.videogen import sliding_window as SW
from infinicube_amd.videogen import synthetic as syn
from infinicube_amd.videogen.config import TokenGrid, preset
from infinicube_amd.videogen.dit import WanDiT
from infinicube_amd.videogen.pipeline import DiTHolder, WanVideoPipeline
from infinicube_amd.videogen.scheduler import FlowMatchScheduler
from oracle import wan_ref as R
from oracle_ops import OracleOps

CFG, GRID = preset("tiny"), TokenGrid(33, 64, 96)        # 9 latent frames of 4 x 6 tokens
CASES = [(9, 4, 2), (48, 24, 12), (48, 24, 18), (30, 24, 12), (47, 24, 12), (27, 8, 8), (9, 4, 1), (20, 24, 12)]
ENV = options.ENV_NAMES


def window_euler_twin(latent_next, hc, hu, cfg_scale, dsigma, frame_coef, frame0, tok0, n_tok, round_bf16=False):
    """Torch twin of icv_unpatchify_cfg_euler_window, one tensor op per rounding point (include/icvideo.h)."""
    C, T, H8, W8 = latent_next.shape
    Hp, Wp = H8 // 2, W8 // 2
    hc = hc[:n_tok]
    hu = None if hu is None else hu[:n_tok]
    if round_bf16:
        rb = lambda t: t.to(torch.bfloat16).to(torch.float32)   # noqa: E731
        v = rb(hc) if hu is None else rb(rb(hu) + rb(cfg_scale * rb(rb(hc) - rb(hu))))
        vd = rb(v * dsigma)
    else:
        v = hc if hu is None else hu + cfg_scale * (hc - hu)
        vd = v * dsigma
    tok = torch.arange(tok0, tok0 + n_tok, device=hc.device)
    f, hp, wp = tok // (Hp * Wp), (tok // Wp) % Hp, tok % Wp
    upd = frame_coef[f][:, None] * vd                                  # [n_tok, (y z c)]
    upd = upd.reshape(n_tok, 2, 2, C)
    for y in range(2):
        for z in range(2):
            idx = (frame0 + f, 2 * hp + y, 2 * wp + z)
            latent_next[:, idx[0], idx[1], idx[2]] = latent_next[:, idx[0], idx[1], idx[2]] + upd[:, y, z, :].t()


class WindowOps(OracleOps):
    """OracleOps + the CPU twin of the window kernel; counts its calls."""

    def __init__(self):
        super().__init__()
        self.window_calls = 0

    def unpatchify_cfg_euler_window(self, latent_next, hc, hu, cfg_scale, dsigma, frame_coef, frame0, tok0, n_tok, round_bf16=False):
        self.window_calls += 1
        window_euler_twin(latent_next, hc, hu, cfg_scale, dsigma, frame_coef, frame0, tok0, n_tok, round_bf16)


# ---- 1. the plan against upstream's tiler --------------------------------------------------------------------------------------
class TemporalTiler_BCTHW:
    """Upstream's tiler, restated line by line (einops' repeat written as a reshape; float64 so that the sums can be checked)."""

    def build_1d_mask(self, length, left_bound, right_bound, border_width):
        x = torch.ones((length,), dtype=torch.float64)
        if border_width == 0:
            return x
        shift = 0.5
        if not left_bound:
            x[:border_width] = (torch.arange(border_width, dtype=torch.float64) + shift) / border_width
        if not right_bound:
            x[-border_width:] = torch.flip((torch.arange(border_width, dtype=torch.float64) + shift) / border_width, dims=(0,))
        return x

    def build_mask(self, data, is_bound, border_width):
        _, _, T, _, _ = data.shape
        t = self.build_1d_mask(T, is_bound[0], is_bound[1], border_width[0])
        return t.reshape(1, 1, T, 1, 1)

    def run(self, model_fn, sliding_window_size, sliding_window_stride, latents):
        B, C, T, H, W = latents.shape
        value = torch.zeros((B, C, T, H, W), dtype=latents.dtype, device=latents.device)
        weight = torch.zeros((1, 1, T, 1, 1), dtype=torch.float64, device=latents.device)
        self.windows, self.masks = [], []
        for t in range(0, T, sliding_window_stride):
            if t - sliding_window_stride >= 0 and t - sliding_window_stride + sliding_window_size >= T:
                continue
            t_ = min(t + sliding_window_size, T)
            model_output = model_fn(latents[:, :, t:t_], t)
            mask = self.build_mask(model_output, is_bound=(t == 0, t_ == T), border_width=(sliding_window_size - sliding_window_stride,)).to(latents.device)
            value[:, :, t:t_] += model_output * mask.to(value.dtype)
            weight[:, :, t:t_] += mask
            self.windows.append((t, t_))
            self.masks.append(mask.reshape(-1).cpu())
        self.weight = weight.reshape(-1).cpu()
        value /= weight.to(value.dtype)
        return value


@pytest.mark.parametrize("T,size,stride", CASES)
def test_plan_matches_upstream_tiler(T, size, stride):
    g = torch.Generator().manual_seed(T * 100 + size + stride)
    plan = SW.plan(T, size, stride)
    outs = {f0: torch.randn((1, 3, f1 - f0, 2, 2), generator=g) for f0, f1 in plan.windows}
    tiler = TemporalTiler_BCTHW()
    want = tiler.run(lambda x, t: outs[t], size, stride, torch.zeros((1, 3, T, 2, 2)))
    assert tuple(tiler.windows) == plan.windows
    # the coefficients of the windows over a frame sum to 1 (float64), and each equals mask / weight
    total = np.zeros(T)
    for w, (f0, f1) in enumerate(plan.windows):
        total[f0:f1] += plan.coef[w, : f1 - f0]
        assert np.abs(plan.coef[w, : f1 - f0] - (tiler.masks[w] / tiler.weight[f0:f1]).numpy()).max() <= 1e-12
        assert not plan.coef[w, f1 - f0:].any()
    assert np.abs(total - 1.0).max() <= 1e-12
    # blended result of the per-window outputs = upstream's value / weight to f32 rounding: per element at most three addends
    # c_w * out_w (here: 4 with stride 1), each with the rounding of c_w to f32, of the product and of the running sum
    got = torch.zeros((1, 3, T, 2, 2))
    mag = torch.zeros((1, 3, T, 2, 2))
    coef = torch.from_numpy(plan.coef).float()
    for w, (f0, f1) in enumerate(plan.windows):
        got[:, :, f0:f1] += coef[w, : f1 - f0].reshape(1, 1, -1, 1, 1) * outs[f0]
        mag[:, :, f0:f1] += outs[f0].abs()
    n_add = max(1, -(-size // stride))
    assert ((got - want).abs() <= (3 * n_add + 2) * 2.0 ** -24 * mag + 1e-30).all()
    if T <= size:
        assert len(plan.windows) == 1 and np.array_equal(plan.coef[0, :T], np.ones(T))


def test_plain_weights_need_the_division_with_three_fold_overlap():
    """With two windows over a frame the two ramps already sum to 1; with more (9/4/1) they do not: the division stays."""
    for T, size, stride in CASES[:6]:
        p = SW.plan(T, size, stride)
        w = np.zeros(T)
        for f0, f1 in p.windows:
            w[f0:f1] += SW.mask(f0, f1, T, size - stride)
        assert np.abs(w - 1.0).max() <= 1e-12 and (w > 0).all()
    p = SW.plan(9, 4, 1)
    w = np.zeros(9)
    for f0, f1 in p.windows:
        w[f0:f1] += SW.mask(f0, f1, 9, 3)
    assert np.abs(w - 1.0).max() > 0.1


# ---- 2. validation and settings ------------------------------------------------------------------------------------------------
def _pipe(ops=None, cfg=CFG):
    from standins import HashTextEncoder, PoolVAE
    return WanVideoPipeline("cpu", torch.bfloat16, DiTHolder(syn.make_dit_state_dict(cfg), cfg), HashTextEncoder(cfg), PoolVAE(),
                            ops=ops or WindowOps())


def _call_kw(**extra):
    return dict(prompt="a street", negative_prompt="bad", height=GRID.height, width=GRID.width, num_frames=GRID.num_frames, seed=3,
                num_inference_steps=2, return_latents=True, **extra)


def test_validation_errors(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    assert SW.validate(None, None) is None
    for size, stride, msg in ((4, None, "together"), (None, 2, "together"), (4.0, 2, "integer"), (4, "2", "integer"), (True, 1, "integer"),
                              (0, 1, ">= 1"), (4, 0, ">= 1"), (-3, -4, ">= 1"), (4, 5, "must not exceed")):
        with pytest.raises(ValueError, match=msg):
            SW.validate(size, stride)
        with pytest.raises(ValueError, match=msg):
            _pipe()(**_call_kw(sliding_window_size=size, sliding_window_stride=stride))
    assert SW.validate(np.int64(4), 4) == (4, 4)
    monkeypatch.setenv("ICV_SLIDING_WINDOW_SIZE", "four")
    with pytest.raises(ValueError, match="ICV_SLIDING_WINDOW_SIZE must be an integer"):
        _pipe()
    monkeypatch.delenv("ICV_SLIDING_WINDOW_SIZE")
    # first-version scope: each combination raises and names itself
    p = _pipe()
    with pytest.raises(ValueError, match="cannot be combined with TeaCache"):
        p(**_call_kw(sliding_window_size=4, sliding_window_stride=2, tea_cache_l1_thresh=0.1, tea_cache_model_id="Wan2.1-T2V-1.3B"))
    with pytest.raises(ValueError, match="cannot be combined with an image-to-video DiT"):
        _pipe(cfg=preset("tiny-i2v"))(**_call_kw(sliding_window_size=4, sliding_window_stride=2))
    import torch.distributed as dist
    with monkeypatch.context() as mp:
        mp.setattr(dist, "is_initialized", lambda: True)
        mp.setattr(dist, "get_world_size", lambda *a: 2)
        mp.setattr(dist, "get_rank", lambda *a: 0)
        with pytest.raises(ValueError, match="cannot be combined with a process group of 2 ranks"):
            p(**_call_kw(sliding_window_size=4, sliding_window_stride=2))
    # the engine says the same when it is driven directly
    sd, bsd = syn.make_dit_state_dict(CFG), syn.make_buffer_embedder_state_dict(CFG)
    m = WanDiT(CFG, sd, WindowOps(), bsd).prepare(TokenGrid(13, 64, 96), force_sp=True)
    with pytest.raises(ValueError, match="world > 1"):
        m.denoise(syn.make_latent_noise(GRID), None, None, None, FlowMatchScheduler(2), 5.0, sliding_window=SW.plan(9, 4, 2))


def test_worker_pool_combination_raises(monkeypatch):
    """ICV_WORLD > 1 behind the unchanged generator: refused in the client before a request reaches the ranks."""
    from infinicube_amd.videogen.inference import WanVideoGenerator
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    g = WanVideoGenerator.__new__(WanVideoGenerator)
    g._pool, g.pipe = object(), _pipe()
    g.pipe.sliding_window_size, g.pipe.sliding_window_stride = 4, 2
    sem, co = syn.make_dummy_buffers(TokenGrid(9, 64, 96))
    with pytest.raises(ValueError, match="ICV_WORLD > 1"):
        g.generate(sem, co, seed=0)


def _settings(p, size, stride):
    """What WanVideoPipeline.__call__ does with its two keywords: keyword or attribute, then the feature's validation."""
    opt = options.resolve(p, dict(sliding_window_size=size, sliding_window_stride=stride))
    return SW.validate(opt.sliding_window_size, opt.sliding_window_stride)


def test_settings_precedence_and_record(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    p = _pipe()
    assert (p.sliding_window_size, p.sliding_window_stride, p.sliding_window_record) == (None, None, None)
    assert _settings(p, None, None) is None                          # off by default
    assert _settings(p, 4, 2) == (4, 2)
    monkeypatch.setenv("ICV_SLIDING_WINDOW_SIZE", "6")
    monkeypatch.setenv("ICV_SLIDING_WINDOW_STRIDE", "3")
    p = _pipe()
    assert (p.sliding_window_size, p.sliding_window_stride) == (6, 3)              # environment -> attributes
    assert _settings(p, None, None) == (6, 3)
    assert _settings(p, 4, 2) == (4, 2)                              # keywords win
    assert _settings(p, 4, None) == (4, 3)                           # ... each on its own
    p.sliding_window_size, p.sliding_window_stride = 5, 5                          # attributes set after construction
    assert _settings(p, None, None) == (5, 5)
    monkeypatch.delenv("ICV_SLIDING_WINDOW_STRIDE")
    with pytest.raises(ValueError, match="together"):                              # only one of the two variables
        _pipe()(**_call_kw())
    monkeypatch.delenv("ICV_SLIDING_WINDOW_SIZE")
    # the record of a call: the windows, None when off or when the clip fits one window
    p = _pipe()
    base = p(**_call_kw())
    assert p.sliding_window_record is None
    win = p(**_call_kw(sliding_window_size=4, sliding_window_stride=2))
    assert p.sliding_window_record == [(0, 4), (2, 6), (4, 8), (6, 9)]
    assert win.shape == base.shape and torch.isfinite(win).all() and not torch.equal(win, base)
    one = p(**_call_kw(sliding_window_size=9, sliding_window_stride=5))
    assert p.sliding_window_record is None and torch.equal(one, base)
    p(**_call_kw())
    assert p.sliding_window_record is None


# ---- 3. the loop against a restatement -----------------------------------------------------------------------------------------
def _inputs():
    sd, bsd = syn.make_dit_state_dict(CFG), syn.make_buffer_embedder_state_dict(CFG)
    return sd, bsd, syn.make_latent_noise(GRID), syn.make_text_context(CFG, 1), syn.make_text_context(CFG, 2), syn.make_buffer_latents(CFG, GRID)


def sliding_window_reference(sd, bsd, cfg, noise, c1, c2, bl, num_steps, size, stride, cfg_scale=5.0, dtype=torch.float32):
    """Upstream's loop with the tiler, restated on oracle.wan_ref pieces: per step and window, the oracle's forward on
    latent[:, f0:f1] as a clip of its own (its own grid, RoPE from 0) with that window's buffer-latent slice, CFG on the blended
    predictions, value / weight, Euler."""
    sig = R.flow_match_sigmas(num_steps)
    x = noise.clone().to(dtype)
    for i in range(num_steps):
        ts = float(sig[i]) * 1000.0
        preds = []
        for ctx in (c1, c2):
            def model_fn(lat, f0, ctx=ctx):
                buf = R.buffer_embed(bsd, bl[:, f0: f0 + lat.shape[2]], dtype)
                return R.dit_forward(sd, cfg, lat[0], ctx, ts, buf, dtype)[None]
            preds.append(TemporalTiler_BCTHW().run(model_fn, size, stride, x[None])[0])
        v = preds[1] + cfg_scale * (preds[0] - preds[1])
        nxt = float(sig[i + 1]) if i + 1 < num_steps else 0.0
        x = x + v * (nxt - float(sig[i]))
    return x


def _window_loop(ops, size, stride, steps=6, setup=None, prep=None, kw=None, dev="cpu"):
    sd, bsd, noise, c1, c2, bl = _inputs()
    m = WanDiT(CFG, sd, ops, bsd, **(kw or {})).prepare(TokenGrid(4 * (size - 1) + 1, GRID.height, GRID.width), **(prep or {}))
    if setup is not None:
        setup(m)
    ck, cu, bt = m.encode_context(c1), m.encode_context(c2), m.embed_buffers(bl, whole_clip=True)
    assert tuple(bt.shape) == (GRID.S, CFG.dim)
    lat = noise.clone().to(dev)
    out = m.denoise(lat, ck, cu, bt, FlowMatchScheduler(steps), 5.0, sliding_window=SW.plan(GRID.T, size, stride))
    assert out is lat                                      # the caller's tensor holds the result
    return m, lat


@pytest.mark.parametrize("size,stride,cfg_batch", [(4, 2, True), (4, 2, False), (4, 1, True)])
def test_host_loop_matches_restatement(size, stride, cfg_batch):
    """9 latent frames, size 4 / stride 2 -> four windows, the last one shorter (a second workspace); 4 / 1 -> three-fold overlap.
    Bar: the one tests/test_teacache_cpu.py holds its host loop to against its restatement (>= 40 dB)."""
    sd, bsd, noise, c1, c2, bl = _inputs()
    ops = WindowOps()
    m, lat = _window_loop(ops, size, stride, setup=lambda m: setattr(m, "cfg_batch", cfg_batch))
    n_win = len(SW.windows(GRID.T, size, stride))
    assert ops.window_calls == 6 * n_win
    assert (m._pair is not None) == cfg_batch
    assert sorted(m._win_engines) == ([3] if stride == 2 else []), "one extra workspace, for the shorter last window only"
    ref = sliding_window_reference(R.round_state_dict_to_bf16(sd), R.round_state_dict_to_bf16(bsd), CFG, noise, c1, c2, bl, 6, size, stride)
    p = R.psnr(lat, ref)
    assert p >= 40.0, f"sliding-window loop {size}/{stride} vs restatement: {p:.1f} dB"
    # ... and it is not the single full-length forward the swallowed keywords used to give
    full = R.denoise_loop(R.round_state_dict_to_bf16(sd), R.round_state_dict_to_bf16(bsd), CFG, noise, c1, c2, bl, 6)
    assert R.psnr(full, ref) < p, "the windows must actually change the result"


def manual_window_loop(m_of, ops, noise, ck, cu, bl, steps, size, stride, twin, dev="cpu", round_bf16=False):
    """The windowed loop spelled out with the engine's PLAIN forward: every window is cut out of the latent as a contiguous clip of
    its own and run by an engine prepared for exactly that clip (no offset anywhere), with buffer tokens embedded from that
    window's buffer-latent slice.  denoise(sliding_window=) must give the same bits: same kernels on the same rows."""
    plan, sch = SW.plan(GRID.T, size, stride), FlowMatchScheduler(steps)
    coef = torch.from_numpy(plan.coef).float().to(dev)
    cur = noise.clone().to(dev)
    for i in range(steps):
        nxt = cur.clone()
        for w, (f0, f1) in enumerate(plan.windows):
            m = m_of(f1 - f0)
            bt = m.embed_buffers(bl[:, f0:f1])
            clip = cur[:, f0:f1].contiguous()
            m.forward_tokens(clip, ck, sch.timesteps[i], bt, m.head_out[0])
            m.forward_tokens(clip, cu, sch.timesteps[i], bt, m.head_out[1])
            twin(nxt, m.head_out[0], m.head_out[1], 5.0, sch.dsigma(i), coef[w], f0, 0, m.plan.n_tok, round_bf16)
        cur = nxt
    return cur


@pytest.mark.parametrize("size,stride", [(4, 2), (4, 1)])
def test_window_forward_is_a_plain_forward_on_the_slice(size, stride):
    """Sharper than a PSNR against fp32 (this preset's update is dominated by token-local terms, so 40 dB cannot tell a wrong RoPE
    origin or attention scope): bit equality with the spelled-out loop, in both CFG driver modes."""
    sd, bsd, noise, c1, c2, bl = _inputs()
    ops, engines = WindowOps(), {}

    def m_of(frames):
        if frames not in engines:
            engines[frames] = WanDiT(CFG, sd, ops, bsd).prepare(TokenGrid(4 * (frames - 1) + 1, GRID.height, GRID.width))
        return engines[frames]

    m0 = m_of(size)
    ck, cu = m0.encode_context(c1), m0.encode_context(c2)
    want = manual_window_loop(m_of, ops, noise, ck, cu, bl, 2, size, stride, window_euler_twin)
    for cfg_batch in (False, True):
        _, got = _window_loop(WindowOps(), size, stride, steps=2, setup=lambda m: setattr(m, "cfg_batch", cfg_batch))
        assert torch.equal(got, want), f"cfg_batch={cfg_batch}: max |d| {float((got - want).abs().max())}"


# ---- 4. one window = the plain loop ----------------------------------------------------------------------------------------------
def _traced(sliding_window):
    sd, bsd, noise, c1, c2, bl = _inputs()
    tr = Trace()
    m = WanDiT(CFG, sd, TracedOps(tr), bsd).prepare(GRID)
    bt = m.embed_buffers(bl)
    tr.on = True
    ck, cu = m.encode_context(c1), m.encode_context(c2)
    lat = noise.clone()
    m.denoise(lat, ck, cu, bt, FlowMatchScheduler(3), 5.0, **sliding_window)
    tr.on = False
    assert m._win_next is None and not m._win_engines
    return tr.log, lat


def test_one_window_is_the_plain_loop():
    log0, lat0 = _traced({})
    for size, stride in ((9, 4), (24, 12)):
        plan = SW.plan(GRID.T, size, stride)
        assert plan.windows == ((0, 9),)
        log1, lat1 = _traced(dict(sliding_window=plan))
        assert torch.equal(lat1, lat0)
        assert log1 == log0, "a one-window plan must issue the plain loop's launches"
    assert not any(e[0] == "unpatchify_cfg_euler_window" for e in log0)


# ---- 5. off -----------------------------------------------------------------------------------------------------------------------
def test_off_calls_nothing_new(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    ops = WindowOps()
    p = _pipe(ops)
    allocs = []
    raw = ops.alloc
    monkeypatch.setattr(ops, "alloc", lambda shape, dtype: (allocs.append(tuple(shape)), raw(shape, dtype))[1])
    lat = p(**_call_kw())
    assert ops.window_calls == 0 and p.sliding_window_record is None
    eng = p._engine
    assert eng._win_next is None and not eng._win_engines and eng._lat_tok0 is None
    assert tuple(lat.shape) not in allocs, "off: no second latent"
    assert eng.grid == GRID
    # on, for contrast: the second latent and the window calls appear
    p(**_call_kw(sliding_window_size=4, sliding_window_stride=2))
    assert ops.window_calls == 2 * 4 and tuple(lat.shape) in allocs and p._engine._lat_tok0 is None
