"""Radial self-attention (infinicube_amd/videogen/attn_window.py) on CPU: ``radial_ranges`` against a brute-force mask
built straight from the rule, the table of DESIGN.md, validation / precedence / record / scope (all before any GPU work), off =
exactly the frame window's calls and allocations, and the host loop (dit.WanDiT with set_attention_window(radial=True)) on the
TEST-ONLY oracle operator set against a masked restatement of the oracle's loop."""
import math

import numpy as np
import pytest
import torch

from infinicube_amd.videogen import attn_window as AW
from infinicube_amd.videogen import options
from infinicube_amd.videogen import synthetic as syn
from infinicube_amd.videogen.config import TokenGrid, preset
from infinicube_amd.videogen.dit import WanDiT
from infinicube_amd.videogen.scheduler import FlowMatchScheduler
from oracle import wan_ref as R
import test_attn_window_cpu as W
from test_attn_window_cpu import FramewinOps, _pipe, _runs

CFG, GRID = preset("tiny"), TokenGrid(33, 256, 384)       # 9 latent frames of 16 x 24 = 384 tokens: q-blocks of 256 and 128 rows
ENV = options.ENV_NAMES
BF16 = torch.bfloat16
QBLOCK = 256


# ---- the restatement: a boolean mask per key row, never radial_ranges() ---------------------------------------------------------------
def half_band(F, e):
    """h of the rule for e = |g - f| - W >= 1, with the level from the logarithm itself."""
    level = int(math.floor(math.log2(e))) + 1
    return F // (2 ** (level + 1))


def block_mask(T, F, window, sink, f, p0):
    """bool [T * F]: the key rows that query block [p0, min(F, p0 + 256)) of frame f reads - every key row judged on its own."""
    p1 = min(F, p0 + QBLOCK)
    idx = np.arange(T * F)
    g, r = idx // F, idx % F
    dist = np.abs(g - f)
    whole = (g < sink) | (dist <= window)
    e = np.maximum(dist - window, 1)
    h = F // (2 ** (np.floor(np.log2(e)).astype(np.int64) + 2))
    return whole | ((r >= p0 - h) & (r < p1 + h))


def blocks(T, F):
    return [(f, p0) for f in range(T) for p0 in range(0, F, QBLOCK)]


def radial_masked_attention(q, k, v, heads, T, F, window, sink, scale=None):
    """softmax over the allowed keys only, per query block, on oracle.wan_ref.attention: q, k, v [T * F, heads * hd] -> same."""
    out = torch.empty_like(q)
    for f, p0 in blocks(T, F):
        keys = torch.from_numpy(block_mask(T, F, window, sink, f, p0)).to(k.device)
        rows = slice(f * F + p0, f * F + min(F, p0 + QBLOCK))
        out[rows] = R.attention(q[rows], k[keys], v[keys], heads, scale=scale)
    return out


def radial_denoise_loop(sd, bsd, cfg, noise, c1, c2, bl, num_steps, window, sink):
    """test_attn_window_cpu's restated oracle loop with the radial mask in place of the frame mask: that loop reaches its masked
    attention through its module's name, which is swapped for the duration of the call - everything else is the same code."""
    orig = W.masked_attention
    W.masked_attention = radial_masked_attention
    try:
        return W.windowed_denoise_loop(sd, bsd, cfg, noise, c1, c2, bl, num_steps, window, sink)
    finally:
        W.masked_attention = orig


class RadialOps(FramewinOps):
    """FramewinOps + the CPU twin of icv_attention_fwd_radial: fp32 softmax per (frame, block) over the pieces of radial_ranges (the
    production rule; the restatement above is the other side of the comparison); counts its calls."""

    def __init__(self):
        super().__init__()
        self.radial_calls = []

    def attention_radial(self, q, k, v, o, heads, scale, frames, frame_rows, window, sink):
        self.radial_calls.append((frames, frame_rows, window, sink))
        qf, kf, vf = q.float(), k.float(), v.float()
        for (f, p0), pieces in zip(blocks(frames, frame_rows), AW.radial_ranges(frames, frame_rows, window, sink)):
            keys = torch.cat([torch.arange(a, b) for a, b in pieces])
            rows = slice(f * frame_rows + p0, f * frame_rows + min(frame_rows, p0 + QBLOCK))
            o[rows] = R.attention(qf[rows], kf[keys], vf[keys], heads, scale=scale).to(BF16)


# ---- 1. radial_ranges against the brute-force mask ------------------------------------------------------------------------------------
def _fraction_and_pieces(T, F, window, sink):
    read, most = 0, 0
    for f, p0 in blocks(T, F):
        m = block_mask(T, F, window, sink, f, p0)
        read += (min(F, p0 + QBLOCK) - p0) * int(m.sum())
        most = max(most, len(_runs(m)))
    return read / float(T * F) ** 2, most


def test_ranges_equal_the_brute_force_mask():
    assert AW.RADIAL_QBLOCK == QBLOCK and AW.RADIAL_MAX_FRAMES == 64
    for T in range(1, 13):
        for F in (40, 257, 384, 600):
            for window in range(4):
                for sink in range(4):
                    got = AW.radial_ranges(T, F, window, sink)
                    bl = blocks(T, F)
                    assert len(got) == len(bl)
                    tiles = 0
                    for (f, p0), pieces in zip(bl, got):
                        what = f"T={T} F={F} window={window} sink={sink} frame {f} block at {p0}"
                        mask = block_mask(T, F, window, sink, f, p0)
                        assert pieces == _runs(mask), f"{what}: {pieces} vs mask {_runs(mask)}"
                        assert 1 <= len(pieces) <= T, what
                        assert all(0 <= a < b <= T * F for a, b in pieces), what
                        assert all(r0[1] < r1[0] for r0, r1 in zip(pieces[:-1], pieces[1:])), f"{what}: ascending, disjoint, not adjacent"
                        tiles += sum(-(-(b - a) // 64) for a, b in pieces)
                        # every query row's own position +- h (clipped to the frame) lies inside its band, in every key frame
                        p1 = min(F, p0 + QBLOCK)
                        for g in range(T):
                            e = abs(g - f) - window
                            h = F if (g < min(sink, T) or e <= 0) else half_band(F, e)
                            for qrow in (p0, p1 - 1):
                                assert mask[g * F + max(0, qrow - h)] and mask[g * F + min(F - 1, qrow + h)], f"{what} key frame {g}"
                    assert AW.radial_tiles(T, F, window, sink) == tiles
                    frac, most = _fraction_and_pieces(T, F, window, sink)
                    assert abs(AW.radial_key_fraction(T, F, window, sink) - frac) <= 1e-15
                    assert AW.radial_record(T, F, window, sink) == dict(window=window, sink=sink, radial=True, key_fraction=frac, max_pieces=most)
                    if AW.dense(T, window):
                        assert got == [[(0, T * F)]] * len(bl)


@pytest.mark.parametrize("T,F,window,sink,fraction,pieces", [
    (21, 1560, 1, 1, 0.422, 20), (9, 600, 0, 0, 0.604, 9), (9, 600, 1, 1, 0.740, 8), (9, 600, 0, 2, 0.696, None), (9, 600, 2, 1, 0.814, 7),
    (5, 257, 0, 0, 0.997, None), (9, 384, 0, 1, 0.751, 9), (9, 40, 0, 0, 1.000, 1), (9, 40, 1, 0, 1.000, 1), (9, 40, 2, 3, 1.000, 1),
    (32, 1560, 1, 1, 0.351, None), (21, 3600, 1, 1, 0.357, None)])
def test_the_table_of_the_design_section(T, F, window, sink, fraction, pieces):
    frac, most = _fraction_and_pieces(T, F, window, sink)           # from the mask ...
    assert round(frac, 3) == fraction and abs(AW.radial_key_fraction(T, F, window, sink) - frac) <= 1e-15      # ... and from the ranges
    if pieces is not None:
        assert most == pieces == max(len(p) for p in AW.radial_ranges(T, F, window, sink))


def test_examples_and_tile_counts():
    assert AW.radial_ranges(5, 257, 0, 0)[2 * 2 + 1] == [(224, 257), (449, 771), (963, 1028), (1252, 1285)]
    assert AW.radial_ranges(9, 40, 1, 2) == [[(0, 360)]] * 9, "a frame of one block: every band is the whole frame"
    # the 14B / 480p shape: radial (1, 1) issues 1.007 x the 64-key tiles of the frame window (4, 1)
    fw = sum(-(-(b - a) * 1560 // 64) for r in AW.ranges(21, 4, 1) for a, b in r) * 7            # 7 q-blocks per frame
    assert AW.framewin_tiles(21, 1560, 4, 1) == fw
    assert round(AW.radial_tiles(21, 1560, 1, 1) / fw, 3) == 1.007
    with pytest.raises(ValueError, match="at most 64"):
        AW.radial_ranges(65, 40, 0, 0)
    assert len(AW.radial_ranges(64, 40, 0, 0)) == 64


# ---- 2. validation, precedence, record, scope -------------------------------------------------------------------------------------------
def _rpipe(ops=None, **kw):
    return _pipe(ops or RadialOps(), **kw)


def _kw(**extra):
    return dict(dict(prompt="a street", negative_prompt="bad", height=GRID.height, width=GRID.width, num_frames=GRID.num_frames, seed=3,
                     num_inference_steps=2, return_latents=True), **extra)


def test_validation_before_any_gpu_work(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    assert AW.validate_radial(None, None) is False and AW.validate_radial(False, None) is False and AW.validate_radial(True, 0, 64) is True
    p = _rpipe()
    monkeypatch.setattr(p, "_get_engine", lambda: pytest.fail("the engine was built before the settings were validated"))
    for bad in (1, 0, "yes", 1.0):
        with pytest.raises(ValueError, match="attention_radial must be a bool"):
            p(**_kw(attention_window_frames=1, attention_radial=bad))
    with pytest.raises(ValueError, match="attention_radial needs attention_window_frames"):
        p(**_kw(attention_radial=True))
    with pytest.raises(ValueError, match="attention_radial needs attention_window_frames"):
        p(**_kw(attention_radial=True, attention_sink_frames=0))
    with pytest.raises(ValueError, match="65 latent frames.*at most 64 pieces"):
        p(**_kw(attention_window_frames=0, attention_radial=True, num_frames=257, height=64, width=96))       # T = 65
    p.attention_radial = "on"                                   # the attribute is checked like the keyword
    with pytest.raises(ValueError, match="attention_radial must be a bool"):
        p(**_kw(attention_window_frames=1))
    # the three scope errors of the attention window are radial's
    p.attention_radial = True
    on = dict(attention_window_frames=1, attention_sink_frames=1)
    with pytest.raises(ValueError, match="cannot be combined with sliding_window_size"):
        p(**_kw(sliding_window_size=4, sliding_window_stride=2, **on))
    p8 = _rpipe(dtype=torch.float8_e4m3fn)
    monkeypatch.setattr(p8, "_get_engine", lambda: pytest.fail("the engine was built before the scope was checked"))
    with pytest.raises(ValueError, match="cannot be combined with the e4m3 self-attention mode"):
        p8(**_kw(attention_radial=True, **on))
    import torch.distributed as dist
    with monkeypatch.context() as mp:
        mp.setattr(dist, "is_initialized", lambda: True)
        mp.setattr(dist, "get_world_size", lambda *a: 2)
        mp.setattr(dist, "get_rank", lambda *a: 0)
        with pytest.raises(ValueError, match="cannot be combined with a process group of 2 ranks"):
            p(**_kw(**on))
    # the engine says the same when it is driven directly
    sd, bsd = syn.make_dit_state_dict(CFG), syn.make_buffer_embedder_state_dict(CFG)
    with pytest.raises(ValueError, match="sequence parallelism"):
        WanDiT(CFG, sd, RadialOps(), bsd).prepare(GRID, force_sp=True).set_attention_window(1, 1, radial=True)
    with pytest.raises(ValueError, match="e4m3 self-attention mode"):
        WanDiT(CFG, sd, RadialOps(), bsd, gemm_dtype="fp8", attn_dtype="fp8", fp8_weights=WanDiT.FP8_WEIGHTS).prepare(GRID).set_attention_window(1, 1, radial=True)
    with pytest.raises(ValueError, match="attention_radial needs attention_window_frames"):
        WanDiT(CFG, sd, RadialOps(), bsd).prepare(GRID).set_attention_window(None, None, radial=True)
    with pytest.raises(ValueError, match="attention_radial must be a bool"):
        WanDiT(CFG, sd, RadialOps(), bsd).prepare(GRID).set_attention_window(1, 1, radial=1)
    from infinicube_amd.videogen import sliding_window as SW
    m = WanDiT(CFG, sd, RadialOps(), bsd).prepare(TokenGrid(9, 256, 384)).set_attention_window(0, 0, radial=True)
    with pytest.raises(ValueError, match="sliding_window_size"):
        m.denoise(syn.make_latent_noise(GRID), None, None, None, FlowMatchScheduler(2), 5.0, sliding_window=SW.plan(GRID.T, 3, 2))
    m65 = WanDiT(CFG, sd, RadialOps(), bsd).prepare(TokenGrid(257, 64, 96)).set_attention_window(0, 0)
    with pytest.raises(ValueError, match="65 latent frames"):
        m65.set_attention_window(0, 0, radial=True)


def test_precedence_record_and_engine_state(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    T, F = GRID.T, GRID.tokens_per_frame
    assert (T, F) == (9, 384)
    ops = RadialOps()
    p = _rpipe(ops)
    assert p.attention_radial is None
    base = p(**_kw())
    assert p.attention_window_record is None and not ops.radial_calls and not ops.framewin_calls
    rad = p(**_kw(attention_window_frames=0, attention_sink_frames=1, attention_radial=True))
    frac, most = _fraction_and_pieces(T, F, 0, 1)
    assert p.attention_window_record == dict(window=0, sink=1, radial=True, key_fraction=frac, max_pieces=most)
    assert round(frac, 3) == 0.751 and most == 9
    assert set(ops.radial_calls) == {(T, F, 0, 1)} and not ops.framewin_calls
    assert p._engine.attn_radial is True and p._engine._framewin() == (0, 1, True)
    assert torch.isfinite(rad).all() and not torch.equal(rad, base)
    n = len(ops.radial_calls)
    win = p(**_kw(attention_window_frames=0, attention_sink_frames=1))                   # the setting does not outlive its call
    assert len(ops.radial_calls) == n and ops.framewin_calls and p._engine.attn_radial is False
    assert p.attention_window_record == dict(window=0, sink=1, key_fraction=float(W.frame_mask(T, 0, 1).mean()))
    assert not torch.equal(win, rad)
    # attribute, and keyword over attribute
    p.attention_radial = True
    ops.framewin_calls.clear()
    assert torch.equal(p(**_kw(attention_window_frames=0, attention_sink_frames=1)), rad) and not ops.framewin_calls
    assert torch.equal(p(**_kw(attention_window_frames=0, attention_sink_frames=1, attention_radial=False)), win) and ops.framewin_calls
    p.attention_radial = False
    assert torch.equal(p(**_kw(attention_window_frames=0, attention_sink_frames=1, attention_radial=True)), rad)
    # a window that covers the clip: the plain path, bit for bit, no record - and nothing left on the engine
    n, ops.framewin_calls[:] = len(ops.radial_calls), []
    full = p(**_kw(attention_window_frames=T - 1, attention_radial=True))
    assert torch.equal(full, base) and p.attention_window_record is None and len(ops.radial_calls) == n and not ops.framewin_calls
    assert p._engine.attn_window is None and p._engine.attn_radial is False and p._engine._framewin() is None
    # the engine: radial is part of what keys a graph and of what the C driver's eligibility reads
    eng = p._engine.set_attention_window(1, 1, radial=True)
    assert eng._framewin() == (1, 1, True) and eng.set_attention_window(1, 1)._framewin() == (1, 1)
    assert eng.set_attention_window(T - 1, 0, radial=True)._framewin() is None


def test_off_is_the_frame_window_as_it_was(monkeypatch):
    """attention_radial None or False: the frame window's launches, allocations, bits and record; True: no launch or allocation
    besides its own (scalars in a launch, no workspace)."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)

    def run(**kw):
        ops = RadialOps()
        p = _rpipe(ops)
        allocs, calls = [], []
        raw = ops.alloc
        monkeypatch.setattr(ops, "alloc", lambda shape, dtype: (allocs.append((tuple(shape), dtype)), raw(shape, dtype))[1])
        lat = p(**_kw(attention_window_frames=1, attention_sink_frames=1, **kw))
        return p, ops, allocs, lat

    p0, ops0, allocs0, lat0 = run()
    for value in (None, False):
        p1, ops1, allocs1, lat1 = run(attention_radial=value)
        assert ops1.framewin_calls == ops0.framewin_calls and not ops1.radial_calls and allocs1 == allocs0 and torch.equal(lat1, lat0)
        assert p1.attention_window_record == p0.attention_window_record == dict(window=1, sink=1, key_fraction=float(W.frame_mask(GRID.T, 1, 1).mean()))
    p2, ops2, allocs2, lat2 = run(attention_radial=True)
    assert ops2.radial_calls == ops0.framewin_calls and not ops2.framewin_calls and allocs2 == allocs0 and not torch.equal(lat2, lat0)
    eng = p2._engine
    eng.native_forward, eng._is_gpu, eng.ops.lib = True, (lambda: True), object()
    assert not eng._native_eligible(), "the one-call C driver does not know the mask"
    eng.set_attention_window(None, None)
    assert eng._native_eligible()


# ---- 3. the host loop against the masked restatement ---------------------------------------------------------------------------------------
STEPS, SETTING = 2, (0, 1)          # window 0 + 1 anchor frame at T = 9: nine pieces for the middle frames, levels 1 .. 4


def _inputs():
    sd, bsd = syn.make_dit_state_dict(CFG), syn.make_buffer_embedder_state_dict(CFG)
    return sd, bsd, syn.make_latent_noise(GRID), syn.make_text_context(CFG, 1), syn.make_text_context(CFG, 2), syn.make_buffer_latents(CFG, GRID)


def _loop(ops, window, sink, radial, steps=STEPS, setup=None, prep=None, dev="cpu"):
    sd, bsd, noise, c1, c2, bl = _inputs()
    m = WanDiT(CFG, sd, ops, bsd).prepare(GRID, **(prep or {}))
    m.set_attention_window(window, sink, radial=radial)
    if setup is not None:
        setup(m)
    lat = noise.clone().to(dev)
    m.denoise(lat, m.encode_context(c1), m.encode_context(c2), m.embed_buffers(bl), FlowMatchScheduler(steps), 5.0)
    return m, lat


_REFS = {}


def reference(kind, window=None, sink=None, steps=STEPS):
    """The restatement's latent (bf16-rounded weights, fp32 arithmetic), once per setting: "radial", "window" or "dense"."""
    key = (kind, window, sink, steps)
    if key not in _REFS:
        sd, bsd, noise, c1, c2, bl = _inputs()
        rsd, rbsd = R.round_state_dict_to_bf16(sd), R.round_state_dict_to_bf16(bsd)
        if kind == "radial":
            _REFS[key] = radial_denoise_loop(rsd, rbsd, CFG, noise, c1, c2, bl, steps, window, sink)
        elif kind == "window":
            _REFS[key] = W.windowed_denoise_loop(rsd, rbsd, CFG, noise, c1, c2, bl, steps, window, sink)
        else:
            _REFS[key] = R.denoise_loop(rsd, rbsd, CFG, noise, c1, c2, bl, steps)
    return _REFS[key]


@pytest.mark.parametrize("cfg_batch", [True, False])
def test_host_loop_matches_masked_restatement(cfg_batch):
    """Bar: the project's loop bar (>= 40 dB)."""
    ops = RadialOps()
    m, lat = _loop(ops, *SETTING, True, setup=lambda m: setattr(m, "cfg_batch", cfg_batch))
    assert (m._pair is not None) == cfg_batch
    # per step: layer 0's self-attention once (shared stem) + the other layers per branch
    assert len(ops.radial_calls) == STEPS * (1 + 2 * (CFG.num_layers - 1)) and not ops.framewin_calls
    assert set(ops.radial_calls) == {(GRID.T, GRID.tokens_per_frame) + SETTING}
    ref = reference("radial", *SETTING)
    psnr = R.psnr(lat, ref)
    print(f"radial loop vs masked restatement: {psnr:.1f} dB")
    assert psnr >= 40.0, f"{psnr:.1f} dB"
    _, dense = _loop(RadialOps(), None, None, False, setup=lambda m: setattr(m, "cfg_batch", cfg_batch))
    _, win = _loop(RadialOps(), *SETTING, False, setup=lambda m: setattr(m, "cfg_batch", cfg_batch))
    assert not torch.equal(lat, dense) and not torch.equal(lat, win), "radial is neither dense attention nor the frame window"
    assert not torch.equal(ref, reference("dense")) and not torch.equal(ref, reference("window", *SETTING))
