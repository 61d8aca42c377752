"""Frame-windowed self-attention (infinicube_amd/videogen/attn_window.py) on CPU: the per-frame key ranges against a
brute-force T x T mask, validation and where the settings come from, the three first-version scope errors, the host loop
(dit.WanDiT with set_attention_window) on the TEST-ONLY oracle operator set against a masked restatement built from
oracle.wan_ref pieces, a window that covers the clip = the plain loop (bits and launches), off = nothing new, and the C entry
point's argument checks (they run on the host, before any launch)."""
import numpy as np
import pytest
import torch

from dit_launch_trace import Trace, TracedOps
from infinicube_amd.videogen import attn_window as AW
from infinicube_amd.videogen import options
from infinicube_amd.videogen import synthetic as syn
from infinicube_amd.videogen.config import TokenGrid, preset
from infinicube_amd.videogen.dit import WanDiT
from infinicube_amd.videogen.pipeline import DiTHolder, WanVideoPipeline
from infinicube_amd.videogen.scheduler import FlowMatchScheduler
from oracle import wan_ref as R
from oracle_ops import OracleOps

CFG, GRID = preset("tiny"), TokenGrid(17, 64, 96)        # 5 latent frames of 4 x 6 tokens
ENV = options.ENV_NAMES
BF16 = torch.bfloat16


# ---- the restatement: a mask, never ranges() ---------------------------------------------------------------------------------------
def frame_mask(T, window, sink):
    """mask[f, g]: a query of frame f reads the keys of frame g."""
    f, g = np.arange(T)[:, None], np.arange(T)[None, :]
    return (np.abs(g - f) <= window) | (g < sink)


def masked_attention(q, k, v, heads, T, F, window, sink, scale=None):
    """softmax over the allowed keys only, per query frame, on oracle.wan_ref.attention: q, k, v [T * F, heads * hd] -> same."""
    mask = torch.from_numpy(frame_mask(T, window, sink))
    out = torch.empty_like(q)
    for f in range(T):
        keys = mask[f].repeat_interleave(F).to(k.device)
        out[f * F: (f + 1) * F] = R.attention(q[f * F: (f + 1) * F], k[keys], v[keys], heads, scale=scale)
    return out


def windowed_dit_forward(sd, cfg, latent, context, timestep, buf_tokens, window, sink, dtype=torch.float32):
    """oracle.wan_ref.dit_forward (text-to-video, unquantised) with the self-attention of every block masked; everything else is
    that function's own pieces in its own order."""
    C, T, H8, W8 = latent.shape
    grid = (T // cfg.patch[0], H8 // cfg.patch[1], W8 // cfg.patch[2])
    F = grid[1] * grid[2]
    t, t_mod = R.time_embed(sd, cfg, timestep, dtype)
    ctx = R.text_embed(sd, context, dtype)
    x = R.patchify_tokens(latent.to(dtype), sd["patch_embedding.weight"].to(dtype), sd["patch_embedding.bias"].to(dtype))
    if buf_tokens is not None:
        x = x + buf_tokens.to(dtype)
    freqs = R.rope_freqs_3d(cfg.head_dim, *grid).to(x.device)
    H, eps = cfg.num_heads, cfg.eps
    lin = R._lin
    for i in range(cfg.num_layers):
        p = f"blocks.{i}"
        sh1, sc1, g1, sh2, sc2, g2 = (sd[f"{p}.modulation"].to(dtype).reshape(6, cfg.dim) + t_mod).unbind(0)
        h = R.modulate(R.layer_norm(x, None, None, eps), sh1, sc1)
        q = R.rope_apply(R.rms_norm(lin(sd, f"{p}.self_attn.q", h, dtype), sd[f"{p}.self_attn.norm_q.weight"].to(dtype), eps), freqs, H)
        k = R.rope_apply(R.rms_norm(lin(sd, f"{p}.self_attn.k", h, dtype), sd[f"{p}.self_attn.norm_k.weight"].to(dtype), eps), freqs, H)
        v = lin(sd, f"{p}.self_attn.v", h, dtype)
        x = x + g1 * lin(sd, f"{p}.self_attn.o", masked_attention(q, k, v, H, grid[0], F, window, sink), dtype)
        h = R.layer_norm(x, sd[f"{p}.norm3.weight"].to(dtype), sd[f"{p}.norm3.bias"].to(dtype), eps)
        q = R.rms_norm(lin(sd, f"{p}.cross_attn.q", h, dtype), sd[f"{p}.cross_attn.norm_q.weight"].to(dtype), eps)
        k = R.rms_norm(lin(sd, f"{p}.cross_attn.k", ctx, dtype), sd[f"{p}.cross_attn.norm_k.weight"].to(dtype), eps)
        x = x + lin(sd, f"{p}.cross_attn.o", R.attention(q, k, lin(sd, f"{p}.cross_attn.v", ctx, dtype), H), dtype)
        h = R.modulate(R.layer_norm(x, None, None, eps), sh2, sc2)
        h = torch.nn.functional.gelu(lin(sd, f"{p}.ffn.0", h, dtype), approximate="tanh")
        x = x + g2 * lin(sd, f"{p}.ffn.2", h, dtype)
    return R.unpatchify(R.head(sd, cfg, x, t, dtype), grid, cfg.out_dim, cfg.patch)


def windowed_denoise_loop(sd, bsd, cfg, noise, c1, c2, bl, num_steps, window, sink, cfg_scale=5.0, dtype=torch.float32):
    """oracle.wan_ref.denoise_loop with the masked forward."""
    sig = R.flow_match_sigmas(num_steps)
    buf = R.buffer_embed(bsd, bl, dtype) if bl is not None else None
    x = noise.to(dtype).clone()
    for i in range(num_steps):
        ts = float(sig[i]) * 1000.0
        v_c = windowed_dit_forward(sd, cfg, x, c1, ts, buf, window, sink, dtype)
        v_u = windowed_dit_forward(sd, cfg, x, c2, ts, buf, window, sink, dtype)
        nxt = float(sig[i + 1]) if i + 1 < num_steps else 0.0
        x = x + (v_u + cfg_scale * (v_c - v_u)) * (nxt - float(sig[i]))
    return x


class FramewinOps(OracleOps):
    """OracleOps + the CPU twin of icv_attention_fwd_framewin; counts its calls."""

    def __init__(self):
        super().__init__()
        self.framewin_calls = []

    def attention_framewin(self, q, k, v, o, heads, scale, frames, frame_rows, window, sink):
        self.framewin_calls.append((frames, frame_rows, window, sink))
        o.copy_(masked_attention(q.float(), k.float(), v.float(), heads, frames, frame_rows, window, sink, scale=scale).to(BF16))


# ---- 1. ranges against a brute-force mask -------------------------------------------------------------------------------------------
def _runs(row):
    """Maximal runs of True in a boolean vector -> [(a, b), ...] ascending."""
    edges = np.flatnonzero(np.diff(np.concatenate(([0], row.astype(np.int8), [0]))))
    return [(int(a), int(b)) for a, b in zip(edges[::2], edges[1::2])]


def test_ranges_equal_the_brute_force_mask():
    for T in range(1, 13):
        for window in range(0, T + 1):
            for sink in range(0, T + 1):
                got = AW.ranges(T, window, sink)
                mask = frame_mask(T, window, sink)
                assert len(got) == T
                for f in range(T):
                    assert got[f] == _runs(mask[f]), f"T={T} window={window} sink={sink} frame {f}: {got[f]} vs mask {_runs(mask[f])}"
                    assert 1 <= len(got[f]) <= 2
                    assert all(0 <= a < b <= T for a, b in got[f])
                    assert all(r0[1] < r1[0] for r0, r1 in zip(got[f][:-1], got[f][1:])), "disjoint, ascending, not touching"
                assert abs(AW.key_fraction(T, window, sink) - mask.mean()) <= 1e-15
                if AW.dense(T, window):
                    assert mask.all()
    # the 14B / 480p example of DESIGN.md §13: 169 pairs inside the windows + frame 0 for the 16 frames whose window starts behind it
    assert frame_mask(21, 4, 0).sum() == 169 and frame_mask(21, 4, 1).sum() == 185
    assert AW.record(21, 4, 1) == dict(window=4, sink=1, key_fraction=185 / 441)


# ---- 2. validation and settings -----------------------------------------------------------------------------------------------------
def _pipe(ops=None, cfg=CFG, dtype=torch.bfloat16):
    from standins import HashTextEncoder, PoolVAE
    return WanVideoPipeline("cpu", dtype, DiTHolder(syn.make_dit_state_dict(cfg), cfg), HashTextEncoder(cfg), PoolVAE(),
                            ops=ops or FramewinOps())


def _call_kw(**extra):
    return dict(prompt="a street", negative_prompt="bad", height=GRID.height, width=GRID.width, num_frames=GRID.num_frames, seed=3,
                num_inference_steps=2, return_latents=True, **extra)


def test_validation_errors(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    assert AW.validate(None, None, 5) is None and AW.validate(None, 0, 5) is None
    assert AW.validate(2, None, 5) == (2, 0) and AW.validate(np.int64(2), 1, 5) == (2, 1) and AW.validate(0, 0, 5) == (0, 0)
    assert AW.validate(2, 9, 5) == (2, 5), "an anchor longer than the clip is the whole clip"
    for window, sink, msg in ((-1, 0, ">= 0"), (1, -2, ">= 0"), (1.0, 0, "integer"), (1, "1", "integer"), (True, 0, "integer"),
                              (1, False, "integer"), (None, 2, "needs attention_window_frames")):
        with pytest.raises(ValueError, match=msg):
            AW.validate(window, sink, 5)
        with pytest.raises(ValueError, match=msg):
            _pipe()(**_call_kw(attention_window_frames=window, attention_sink_frames=sink))
    monkeypatch.setenv("ICV_ATTN_WINDOW_FRAMES", "two")
    with pytest.raises(ValueError, match="ICV_ATTN_WINDOW_FRAMES must be an integer"):
        _pipe()
    monkeypatch.setenv("ICV_ATTN_WINDOW_FRAMES", "1")
    monkeypatch.setenv("ICV_ATTN_SINK_FRAMES", "x")
    with pytest.raises(ValueError, match="ICV_ATTN_SINK_FRAMES must be an integer"):
        _pipe()


def test_settings_are_checked_before_any_gpu_work(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    p = _pipe()
    monkeypatch.setattr(p, "_get_engine", lambda: pytest.fail("the engine was built before the settings were validated"))
    with pytest.raises(ValueError, match=">= 0"):
        p(**_call_kw(attention_window_frames=-1))
    with pytest.raises(ValueError, match="sliding_window_size"):
        p(**_call_kw(attention_window_frames=1, sliding_window_size=4, sliding_window_stride=2))


def _settings(p, window, sink, T):
    """What WanVideoPipeline.__call__ does with its two keywords: keyword or attribute, the feature's validation, dense = off."""
    opt = options.resolve(p, dict(attention_window_frames=window, attention_sink_frames=sink))
    aw = AW.validate(opt.attention_window_frames, opt.attention_sink_frames, T)
    return None if aw is None or AW.dense(T, aw[0]) else aw


def test_settings_precedence_and_record(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    T = GRID.T
    p = _pipe()
    assert (p.attention_window_frames, p.attention_sink_frames, p.attention_window_record) == (None, None, None)
    assert _settings(p, None, None, T) is None                         # off by default
    assert _settings(p, 1, 1, T) == (1, 1)
    monkeypatch.setenv("ICV_ATTN_WINDOW_FRAMES", "2")
    monkeypatch.setenv("ICV_ATTN_SINK_FRAMES", "1")
    p = _pipe()
    assert (p.attention_window_frames, p.attention_sink_frames) == (2, 1)             # environment -> attributes
    assert _settings(p, None, None, T) == (2, 1)
    assert _settings(p, 1, 0, T) == (1, 0)                             # keywords win
    assert _settings(p, 1, None, T) == (1, 1)                          # ... each on its own
    p.attention_window_frames, p.attention_sink_frames = 0, 2                          # attributes set after construction
    assert _settings(p, None, None, T) == (0, 2)
    monkeypatch.delenv("ICV_ATTN_WINDOW_FRAMES")
    with pytest.raises(ValueError, match="needs attention_window_frames"):            # the anchor variable alone
        _pipe()(**_call_kw())
    monkeypatch.delenv("ICV_ATTN_SINK_FRAMES")
    # the record of a call
    ops = FramewinOps()
    p = _pipe(ops)
    base = p(**_call_kw())
    assert p.attention_window_record is None and not ops.framewin_calls
    win = p(**_call_kw(attention_window_frames=1, attention_sink_frames=1))
    assert p.attention_window_record == dict(window=1, sink=1, key_fraction=float(frame_mask(T, 1, 1).mean()))
    assert set(ops.framewin_calls) == {(T, GRID.tokens_per_frame, 1, 1)}
    assert win.shape == base.shape and torch.isfinite(win).all() and not torch.equal(win, base)
    again = p(**_call_kw())                                                            # the setting does not outlive its call
    assert p.attention_window_record is None and p._engine.attn_window is None and torch.equal(again, base)


# ---- 3. first-version scope -----------------------------------------------------------------------------------------------------------
def test_scope_errors(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    on = dict(attention_window_frames=1, attention_sink_frames=1)
    p = _pipe()
    with pytest.raises(ValueError, match="cannot be combined with sliding_window_size"):
        p(**_call_kw(sliding_window_size=4, sliding_window_stride=2, **on))
    with pytest.raises(ValueError, match="cannot be combined with the e4m3 self-attention mode"):
        _pipe(dtype=torch.float8_e4m3fn)(**_call_kw(**on))
    import torch.distributed as dist
    with monkeypatch.context() as mp:
        mp.setattr(dist, "is_initialized", lambda: True)
        mp.setattr(dist, "get_world_size", lambda *a: 2)
        mp.setattr(dist, "get_rank", lambda *a: 0)
        with pytest.raises(ValueError, match="cannot be combined with a process group of 2 ranks"):
            p(**_call_kw(**on))
    # the engine says the same when it is driven directly
    sd, bsd = syn.make_dit_state_dict(CFG), syn.make_buffer_embedder_state_dict(CFG)
    with pytest.raises(ValueError, match="sequence parallelism"):
        WanDiT(CFG, sd, FramewinOps(), bsd).prepare(GRID, force_sp=True).set_attention_window(1, 1)
    with pytest.raises(ValueError, match="e4m3 self-attention mode"):
        WanDiT(CFG, sd, FramewinOps(), bsd, gemm_dtype="fp8", attn_dtype="fp8", fp8_weights=WanDiT.FP8_WEIGHTS).prepare(GRID).set_attention_window(1, 1)
    from infinicube_amd.videogen import sliding_window as SW
    m = WanDiT(CFG, sd, FramewinOps(), bsd).prepare(TokenGrid(9, 64, 96)).set_attention_window(0, 0)
    with pytest.raises(ValueError, match="sliding_window_size"):
        m.denoise(syn.make_latent_noise(GRID), None, None, None, FlowMatchScheduler(2), 5.0, sliding_window=SW.plan(GRID.T, 3, 2))


def test_what_is_no_combination_does_not_raise(monkeypatch):
    """Pipeline and engine agree on 'in the same call': a clip that fits ONE sliding window is the plain loop, and an attention
    window that covers the clip is dense attention - neither is a combination, in the pipeline or on an engine driven directly."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    T = GRID.T
    on = dict(attention_window_frames=1, attention_sink_frames=1)
    ops = FramewinOps()
    p = _pipe(ops)
    win = p(**_call_kw(**on))
    one = p(**_call_kw(sliding_window_size=T, sliding_window_stride=T, **on))            # one sliding window: today's loop, windowed attention
    assert p.sliding_window_record is None and p.attention_window_record["window"] == 1 and torch.equal(one, win)
    # the engine: a covering window is off for the graph key, the C driver's eligibility and the sliding-window check alike
    sd, bsd = syn.make_dit_state_dict(CFG), syn.make_buffer_embedder_state_dict(CFG)
    m = WanDiT(CFG, sd, FramewinOps(), bsd).prepare(GRID).set_attention_window(T - 1, 0)
    assert m.attn_window == (T - 1, 0) and m._framewin() is None
    m.set_attention_window(1, 1)
    assert m._framewin() == (1, 1) and not m._native_eligible()
    from infinicube_amd.videogen import sliding_window as SW
    m3 = WanDiT(CFG, sd, FramewinOps(), bsd).prepare(TokenGrid(9, 64, 96)).set_attention_window(2, 0)   # 3 latent frames: window 2 covers them
    assert m3.grid.T == 3 and m3._framewin() is None
    reached = []
    monkeypatch.setattr(m3, "_denoise_windows", lambda *a, **k: reached.append(1))     # past the scope checks: the windowed loop itself
    m3.denoise(syn.make_latent_noise(GRID), None, None, None, FlowMatchScheduler(1), 1.0, sliding_window=SW.plan(T, 3, 2))
    assert reached == [1]


def test_worker_pool_combination_raises(monkeypatch):
    """ICV_WORLD > 1 behind the unchanged generator: refused in the client before a request reaches the ranks."""
    from infinicube_amd.videogen.inference import WanVideoGenerator
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    g = WanVideoGenerator.__new__(WanVideoGenerator)
    g._pool, g.pipe = object(), _pipe()
    g.pipe.attention_window_frames = 1
    sem, co = syn.make_dummy_buffers(TokenGrid(9, 64, 96))
    with pytest.raises(ValueError, match="ICV_ATTN_WINDOW_FRAMES.*ICV_WORLD > 1"):
        g.generate(sem, co, seed=0)


# ---- 4. the loop against the masked restatement ------------------------------------------------------------------------------------
def _inputs():
    sd, bsd = syn.make_dit_state_dict(CFG), syn.make_buffer_embedder_state_dict(CFG)
    return sd, bsd, syn.make_latent_noise(GRID), syn.make_text_context(CFG, 1), syn.make_text_context(CFG, 2), syn.make_buffer_latents(CFG, GRID)


def _loop(ops, window, sink, steps=3, setup=None, prep=None, dev="cpu"):
    sd, bsd, noise, c1, c2, bl = _inputs()
    m = WanDiT(CFG, sd, ops, bsd).prepare(GRID, **(prep or {}))
    m.set_attention_window(window, sink)
    if setup is not None:
        setup(m)
    lat = noise.clone().to(dev)
    m.denoise(lat, m.encode_context(c1), m.encode_context(c2), m.embed_buffers(bl), FlowMatchScheduler(steps), 5.0)
    return m, lat


_REFS = {}


def reference(window, sink, steps=3):
    """The masked restatement's latent (bf16-rounded weights, fp32 arithmetic), computed once per setting."""
    key = (window, sink, steps)
    if key not in _REFS:
        sd, bsd, noise, c1, c2, bl = _inputs()
        rsd, rbsd = R.round_state_dict_to_bf16(sd), R.round_state_dict_to_bf16(bsd)
        _REFS[key] = (windowed_denoise_loop(rsd, rbsd, CFG, noise, c1, c2, bl, steps, window, sink) if window is not None
                      else R.denoise_loop(rsd, rbsd, CFG, noise, c1, c2, bl, steps))
    return _REFS[key]


@pytest.mark.parametrize("cfg_batch", [True, False])
def test_host_loop_matches_masked_restatement(cfg_batch):
    """5 latent frames, window 1 + 1 anchor frame: single-range, merged and two-range frames.  Bar: the project's loop bar (>= 40 dB)."""
    ops = FramewinOps()
    m, lat = _loop(ops, 1, 1, setup=lambda m: setattr(m, "cfg_batch", cfg_batch))
    assert (m._pair is not None) == cfg_batch
    # per step: layer 0's self-attention once (shared stem) + the other layers per branch
    assert len(ops.framewin_calls) == 3 * (1 + 2 * (CFG.num_layers - 1))
    assert set(ops.framewin_calls) == {(GRID.T, GRID.tokens_per_frame, 1, 1)}
    ref = reference(1, 1)
    p = R.psnr(lat, ref)
    assert p >= 40.0, f"frame-windowed loop vs masked restatement: {p:.1f} dB"
    # at this preset's depth the window moves the latent by about as much as bf16 rounding does (the update is dominated by token-local
    # terms), so the PSNR cannot tell the two apart; what pins the scope is the launch's arguments above and the kernel's own tests
    _, dense = _loop(FramewinOps(), None, None, setup=lambda m: setattr(m, "cfg_batch", cfg_batch))
    assert not torch.equal(lat, dense), "the window must actually change the result"
    assert not torch.equal(ref, reference(None, None))


def test_restatement_with_a_full_window_is_the_oracle():
    """The restated forward is oracle.wan_ref.dit_forward when the mask is all-True: the restatement adds the mask and nothing else."""
    sd, bsd, noise, c1, _, bl = _inputs()
    buf = R.buffer_embed(bsd, bl)
    a = windowed_dit_forward(sd, CFG, noise, c1, 500.0, buf, GRID.T, 0)
    b = R.dit_forward(sd, CFG, noise, c1, 500.0, buf)
    assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())      # SDPA per query frame vs over all rows: fp32 rounding only


# ---- 5. a window that covers the clip = the plain loop -----------------------------------------------------------------------------
def _traced(window, sink):
    sd, bsd, noise, c1, c2, bl = _inputs()
    tr = Trace()
    m = WanDiT(CFG, sd, TracedOps(tr), bsd).prepare(GRID)
    if window is not None:
        m.set_attention_window(window, sink)
    bt = m.embed_buffers(bl)
    tr.on = True
    lat = noise.clone()
    m.denoise(lat, m.encode_context(c1), m.encode_context(c2), bt, FlowMatchScheduler(2), 5.0)
    tr.on = False
    return tr.log, lat


def test_window_that_covers_the_clip_is_the_plain_loop(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    log0, lat0 = _traced(None, None)
    for window, sink in ((GRID.T - 1, 0), (GRID.T, 2), (100, 1)):
        assert AW.dense(GRID.T, window)
        assert AW.ranges(GRID.T, window, sink) == [[(0, GRID.T)]] * GRID.T
        log1, lat1 = _traced(window, sink)      # TracedOps has no attention_framewin: calling it would raise
        assert torch.equal(lat1, lat0)
        assert log1 == log0, "a window that covers the clip must issue the plain loop's launches"
    assert not AW.dense(GRID.T, GRID.T - 2)
    # ... and through the pipeline: same bits, no record, nothing left on the engine
    ops = FramewinOps()
    p = _pipe(ops)
    base = p(**_call_kw())
    full = p(**_call_kw(attention_window_frames=GRID.T, attention_sink_frames=1))
    assert torch.equal(full, base) and p.attention_window_record is None and not ops.framewin_calls and p._engine.attn_window is None
    edge = p(**_call_kw(attention_window_frames=GRID.T - 1))
    assert torch.equal(edge, base) and not ops.framewin_calls


# ---- 6. off ---------------------------------------------------------------------------------------------------------------------------
def test_off_calls_and_allocates_nothing_new(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)

    def run(**kw):
        ops = FramewinOps()
        p = _pipe(ops)
        allocs = []
        raw = ops.alloc
        monkeypatch.setattr(ops, "alloc", lambda shape, dtype: (allocs.append((tuple(shape), dtype)), raw(shape, dtype))[1])
        lat = p(**_call_kw(**kw))
        return p, ops, allocs, lat

    p, ops, allocs_off, _ = run()
    assert not ops.framewin_calls and p.attention_window_record is None and p._engine.attn_window is None
    assert not p._engine._native_eligible()
    p2, ops2, allocs_on, _ = run(attention_window_frames=1)
    assert ops2.framewin_calls and allocs_on == allocs_off, "the window is scalars in a launch: no workspace of its own"
    # the one-call C driver does not know the window: it is refused while the setting is on
    eng = p2._engine
    eng.native_forward, eng._is_gpu, eng.ops.lib = True, (lambda: True), object()
    assert not eng._native_eligible()
    eng.set_attention_window(None, None)
    assert eng._native_eligible()


# ---- 7. the C entry point's argument checks ------------------------------------------------------------------------------------------
def test_argument_errors_without_gpu():
    from infinicube_amd import native
    lib = native.lib()

    def call(**kw):
        a = dict(q=256, ldq=256, k=256, ldk=256, v=256, ldv=256, o=256, ldo=256, frames=5, frame_rows=300, heads=2, window=1, sink=1)
        a.update(kw)
        rc = lib.icv_attention_fwd_framewin(a["q"], a["ldq"], a["k"], a["ldk"], a["v"], a["ldv"], a["o"], a["ldo"], a["frames"], a["frame_rows"],
                                            a["heads"], a["window"], a["sink"], 1.0, None)
        return rc, lib.icv_last_error()

    for kw, msg in ((dict(sink=6), b"sink (6) exceeds the 5 frames"), (dict(frame_rows=0), b"empty problem"), (dict(frames=0), b"empty problem"),
                    (dict(ldk=260), b"16-byte row alignment"), (dict(window=-1), b"must be >= 0"), (dict(sink=-1), b"must be >= 0"),
                    (dict(q=None), b"null pointer"), (dict(frames=1 << 13, frame_rows=1 << 13), b"key axis too large")):
        rc, err = call(**kw)
        assert rc != 0 and msg in err, (kw, rc, err)
