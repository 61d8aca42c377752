"""Radial self-attention on the HIP path (csrc/attn7r.hip, icv_attention_fwd_radial): bit identity with the per-(frame, block)
icv_attention_fwd_pieces launches the one launch replaces, parity with fp32 masked attention (spikes on the first and the last row of
a band and on the rows just outside one, at bands two levels apart), a covering window = the plain launch, the write guard under
strided operands, the host-side argument checks, every driver mode of the DiT, and the pipeline / the unchanged generator."""
import contextlib
import io
import math

import pytest
import torch

from infinicube_amd.videogen import attn_window as AW
from infinicube_amd.videogen import synthetic as syn
from oracle import wan_ref as R
from infinicube_amd.videogen.scheduler import FlowMatchScheduler
from test_attn_radial_cpu import (CFG, ENV, GRID, QBLOCK, SETTING, STEPS, _fraction_and_pieces, _inputs, _loop, block_mask, blocks, half_band,
                                  radial_denoise_loop, radial_masked_attention, reference)
from test_kernels_gpu import assert_bf16_close, rnd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALE = 1.0 / math.sqrt(128)
LOG2E = 1.4426950408889634
SETTINGS = [(0, 0), (1, 1), (0, 2), (2, 1)]       # (window, sink) at T = 9
BF16 = torch.bfloat16


def _qkv(T, F, H, seed, unit):
    """q, k, v bf16 [T * F, H * 128] on the CPU and the launch's scale.  ``unit``: the code path the DiT runs - the softmax scale and
    log2(e) folded into K, scale = ln 2."""
    d = H * 128
    q, k, v = (rnd((T * F, d), seed + i).to(BF16) for i in range(3))
    return q, k, v, (math.log(2.0) if unit else SCALE)


def _fold(k, unit):
    return (k.float() * SCALE * LOG2E).to(BF16) if unit else k


def _radial(hip_ops, q, k, v, H, scale, T, F, window, sink):
    o = torch.zeros_like(q)
    hip_ops.attention_radial(q, k, v, o, H, scale, T, F, window, sink)
    return o


# ---- 1. bit identity with the launches it replaces ---------------------------------------------------------------------------------
@pytest.mark.parametrize("unit", [False, True])
def test_bit_identical_to_the_per_block_pieces_launches(hip_ops, unit):
    """T = 9, F = 600: q-blocks of 256, 256 and 88 rows (the last one's waves 3..7 hold no row at all), up to nine pieces per work-group
    that start and end at arbitrary rows, ragged tail tiles in most of them.  Per (frame, block), the existing launch over that block's
    pieces is the reference: same tiles, same order, same bits."""
    T, F, H = 9, 600, 2
    q, k, v, scale = _qkv(T, F, H, 500, unit)
    q, k, v = q.to(DEV), _fold(k, unit).to(DEV), v.to(DEV)
    most = 0
    for window, sink in SETTINGS:
        want = torch.zeros_like(q)
        for (f, p0), pieces in zip(blocks(T, F), AW.radial_ranges(T, F, window, sink)):
            rows = slice(f * F + p0, f * F + min(F, p0 + QBLOCK))
            hip_ops.attention_pieces(q[rows], [(k[a:b], v[a:b], -1, 0) for a, b in pieces], want[rows], H, scale)
            most = max(most, len(pieces))
        got = _radial(hip_ops, q, k, v, H, scale, T, F, window, sink)
        diff = (got != want).any(dim=1)
        assert torch.equal(got, want), f"window={window} sink={sink}: {int(diff.sum())} rows differ, first {int(diff.nonzero()[0]) if diff.any() else -1}"
    assert most == 9


# ---- 2. parity with fp32 masked attention ------------------------------------------------------------------------------------------
def _plan_spikes(T, F, window, sink):
    """[(query row, key row, visible)] for the LAST frame's query block (f, p0), at the key frames with e = 1 (level 1, h = F >> 2)
    and e = 4 (level 3, h = F >> 4): the first row of the level-1 band and the last row of the level-3 band (visible), the row just in
    front of the level-1 band and the row just behind the level-3 band (not visible; a level or an h that is off by one reads or
    misses one of the four).  Edges that coincide with the frame's are left out.  Every spike gets a query row of its own while the
    block has one to give; a one-row block shares its row (one visible spike at the most, then)."""
    f = T - 1
    g1, g4 = f - window - 1, f - window - 4
    if g4 < sink or g4 < 0:
        return None, []
    p0 = QBLOCK if F > QBLOCK else 0
    p1 = min(F, p0 + QBLOCK)
    h1, h4 = half_band(F, 1), half_band(F, 4)
    lo1, hi4 = max(0, p0 - h1), min(F, p1 + h4)
    cand = []
    if lo1 > 0:
        cand += [(g1 * F + lo1, True), (g1 * F + lo1 - 1, False)]
    if hi4 < F:
        cand += [(g4 * F + hi4 - 1, True), (g4 * F + hi4, False)]
    elif max(0, p0 - h4) > 0:             # the level-3 band ends with the frame: take its front edge instead
        lo4 = p0 - h4
        cand += [(g4 * F + lo4, True), (g4 * F + lo4 - 1, False)]
    rows = p1 - p0
    if rows < len(cand):                  # a block of fewer rows than spikes: one visible and one hidden spike, two levels apart, on one row
        vis = [c for c in cand if c[1]][-1:]
        hid = [c for c in cand if not c[1]][:1]
        return (f, p0), [(f * F + p0, key, seen) for key, seen in vis + hid]
    return (f, p0), [(f * F + p0 + 3 + 7 * i, key, seen) for i, (key, seen) in enumerate(cand)]


@pytest.mark.parametrize("unit", [False, True])
@pytest.mark.parametrize("T,F,window,sink", [(9, 600, w, s) for w, s in SETTINGS] + [(5, 257, 0, 0), (9, 40, 1, 0)])
def test_parity_with_fp32_masked_attention(hip_ops, T, F, window, sink, unit):
    """Spikes (key = 5 q: that key takes the whole softmax of that query) as tests/test_attn_window_gpu.py plants them, on the edges
    of two bands two levels apart (_plan_spikes).  Rows whose mask excludes a planted key must come out bit-identical to the launch
    without it; a visible spike owns its row.  (5, 257): the second block holds ONE row; (9, 40): a frame is shorter than a tile,
    every band is the whole frame and the launch is the dense one."""
    H = 2
    q, k, v, scale = _qkv(T, F, H, 510 + T + F, unit)
    block, spikes = _plan_spikes(T, F, window, sink)
    if F == 40:
        assert all(block_mask(T, F, window, sink, f, p0).all() for f, p0 in blocks(T, F)) and not spikes
    else:
        assert sum(seen for _, _, seen in spikes) >= 1 and sum(not seen for _, _, seen in spikes) >= 1
        assert (F != 600) or len(spikes) == 4
    plain = {}
    for row, key, seen in spikes:
        mask = block_mask(T, F, window, sink, *block)
        assert bool(mask[key]) == seen, "the plan must agree with the restated mask"
        plain[key] = k[key].clone()
        k[key] = q[row] * 5.0
    ref = radial_masked_attention(q.float(), _fold(k, unit).float(), v.float(), H, T, F, window, sink, scale=scale)
    qd, kd, vd = q.to(DEV), _fold(k, unit).clone().to(DEV), v.to(DEV)
    got = _radial(hip_ops, qd, kd, vd, H, scale, T, F, window, sink)
    assert_bf16_close(got, ref, f"radial T={T} F={F} window={window} sink={sink} unit={unit}", abs_floor=2.0 ** -5, rms_bound=2.0 ** -7)
    if not spikes:
        return
    f, p0 = block
    mine = slice(f * F + p0, f * F + min(F, p0 + QBLOCK))
    for row, key, seen in spikes:
        if seen:
            continue
        kd[key] = _fold(plain[key], unit).to(DEV)                # the same launch without THIS planted key
        without = _radial(hip_ops, qd, kd, vd, H, scale, T, F, window, sink)
        kd[key] = _fold(k[key], unit).to(DEV)
        assert torch.equal(got[mine], without[mine]), f"the block at row {mine.start} was moved by key row {key}, just outside its band"
        assert not torch.equal(got, without), "the planted key must be visible to the blocks that do read it"
        if len({r for r, _, _ in spikes}) == len(spikes):
            assert float((ref[row] - v[key].float()).abs().max()) > 0.5, "had the row read the planted key, it would be that key's value row"
    for row, key, seen in spikes:                                # the spikes that ARE visible own their rows
        if seen:
            assert float((got[row].float().cpu() - v[key].float()).abs().max()) <= 2.0 ** -5 * float(v[key].float().abs().max()) + 2.0 ** -7


# ---- 3. a window that covers the clip is the plain launch ------------------------------------------------------------------------------
def test_covering_window_is_the_plain_launch(hip_ops):
    T, F, H = 5, 300, 3
    q, k, v, scale = _qkv(T, F, H, 530, False)
    q, k, v = q.to(DEV), k.to(DEV), v.to(DEV)
    want = torch.zeros_like(q)
    hip_ops.attention(q, k, v, want, H, scale)
    for window, sink in ((T - 1, 0), (T, 2), (1 << 40, 1)):
        assert torch.equal(_radial(hip_ops, q, k, v, H, scale, T, F, window, sink), want), f"window={window} sink={sink}"
    assert not torch.equal(_radial(hip_ops, q, k, v, H, scale, T, F, T - 2, 0), want)


# ---- 4. write guard and strides --------------------------------------------------------------------------------------------------------
def test_write_guard_and_strides(hip_ops):
    """q, k, v as column views of one wider [3, S, d + 128] buffer, o as the top-left corner of a larger matrix full of sentinels: only
    o's S x d elements may change, the result must not depend on the strides, and a second run must give the same bits."""
    T, F, H, window, sink = 5, 300, 2, 0, 1
    d, S = H * 128, T * F
    q, k, v, scale = _qkv(T, F, H, 540, False)
    want = _radial(hip_ops, q.to(DEV), k.to(DEV), v.to(DEV), H, scale, T, F, window, sink)
    wide = torch.full((3, S, d + 128), 3.0, dtype=BF16, device=DEV)
    for i, x in enumerate((q, k, v)):
        wide[i, :, :d] = x.to(DEV)
    obuf = torch.full((S + 2, d + 64), -7.0, dtype=BF16, device=DEV)
    o = obuf[:S, :d]
    assert wide[0, :, :d].stride(0) == d + 128 and o.stride(0) == d + 64
    runs = []
    for _ in range(2):
        o.fill_(-7.0)
        hip_ops.attention_radial(wide[0, :, :d], wide[1, :, :d], wide[2, :, :d], o, H, scale, T, F, window, sink)
        torch.cuda.synchronize()
        assert (obuf[S:] == -7.0).all(), "rows behind the last frame were written"
        assert (obuf[:, d:] == -7.0).all(), "padding columns of o were written"
        runs.append(o.clone())
    assert torch.equal(runs[0], runs[1]), "non-deterministic output"
    assert torch.equal(runs[0], want), "the result depends on the operands' strides"
    assert (wide[:, :, d:] == 3.0).all()


# ---- 5. argument errors ------------------------------------------------------------------------------------------------------------------
def test_argument_errors_return_a_status(hip_ops):
    T, F, H = 5, 300, 2
    q, k, v, scale = _qkv(T, F, H, 550, False)
    q, k, v = q.to(DEV), k.to(DEV), v.to(DEV)
    o = torch.full_like(q, -7.0)
    lib, ld = hip_ops.lib, H * 128

    def call(frames=T, frame_rows=F, ldk=ld, ldo=ld, window=1, sink=1):
        rc = lib.icv_attention_fwd_radial(q.data_ptr(), ld, k.data_ptr(), ldk, v.data_ptr(), ld, o.data_ptr(), ldo, frames, frame_rows, H, window, sink,
                                          scale, hip_ops._stream())
        return rc, lib.icv_last_error()

    for kw, msg in ((dict(frames=65, frame_rows=4), b"65 frames"), (dict(window=-1), b"must be >= 0"), (dict(sink=T + 1), b"sink (6) exceeds the 5 frames"),
                    (dict(ldk=ld + 4), b"16-byte row alignment"), (dict(ldo=ld + 2), b"16-byte row alignment"), (dict(frame_rows=0), b"empty problem")):
        rc, err = call(**kw)
        assert rc != 0 and msg in err, (kw, rc, err)
    torch.cuda.synchronize()
    assert (o == -7.0).all(), "a refused call must launch nothing"
    assert call()[0] == 0
    torch.cuda.synchronize()
    assert torch.isfinite(o.float()).all() and not (o == -7.0).all()
    with pytest.raises(ValueError, match="5 frames of 299 rows"):
        hip_ops.attention_radial(q, k, v, o, H, scale, T, F - 1, 1, 1)


# ---- 6. driver modes ---------------------------------------------------------------------------------------------------------------------
def _sequential(m):
    m.cfg_batch = False


_SEQ = {}


def _sequential_latent(hip_ops, radial=True):
    """The sequential per-op loop's latent, once per flag (the driver modes compare against it)."""
    if radial not in _SEQ:
        m, lat = _loop(hip_ops, *SETTING, radial, setup=_sequential, prep=dict(graphs=False), dev=DEV)
        torch.cuda.synchronize()
        assert m._pair is None and m.attn_window == SETTING and m.attn_radial is radial
        _SEQ[radial] = lat.clone()
    return _SEQ[radial]


def test_sequential_forward_matches_masked_restatement_and_differs_from_dense(hip_ops):
    """Tiny DiT, 9 latent frames of 384 tokens (q-blocks of 256 and 128 rows), window 0 + 1 anchor frame, two steps with CFG through the
    sequential per-op driver: latent PSNR >= 40 dB against the masked restatement (the project's loop bar), and neither the dense loop's
    latent nor the frame window's."""
    lat = _sequential_latent(hip_ops)
    p = R.psnr(lat.cpu(), reference("radial", *SETTING))
    print(f"HIP radial loop vs masked restatement: {p:.1f} dB")
    assert p >= 40.0, f"{p:.1f} dB"
    _, dense = _loop(hip_ops, None, None, False, setup=_sequential, prep=dict(graphs=False), dev=DEV)
    torch.cuda.synchronize()
    assert not torch.equal(lat, dense), "the mask must change the result"
    assert not torch.equal(lat, _sequential_latent(hip_ops, radial=False)), "radial is not the frame window"
    _, full = _loop(hip_ops, GRID.T - 1, 1, True, setup=_sequential, prep=dict(graphs=False), dev=DEV)
    torch.cuda.synchronize()
    assert torch.equal(full, dense), "a window that covers the clip is the plain path"


@pytest.mark.parametrize("mode", ["pair", "pair-no-stem", "native", "graphs", "dual-stream"])
def test_driver_modes_match_sequential_loop(hip_ops, mode, monkeypatch):
    """Every driver mode takes the radial launch: bit-identical to the sequential per-op loop.  The one-call C driver does not know the
    mask: the per-op driver runs.  Graphs: two steps = one capture and one replay per graph; another ``radial`` is another key."""
    ref = _sequential_latent(hip_ops)
    prep, setup = dict(graphs=False), None
    if mode == "pair-no-stem":
        setup = lambda m: setattr(m, "share_stem", False)                        # noqa: E731
    elif mode == "native":
        setup = lambda m: setattr(m, "native_forward", True)                     # noqa: E731
    elif mode == "graphs":
        prep = dict(graphs=True)
    elif mode == "dual-stream":
        monkeypatch.setenv("ICV_DUAL_STREAM", "1")
    m, got = _loop(hip_ops, *SETTING, True, setup=setup, prep=prep, dev=DEV)
    torch.cuda.synchronize()
    assert torch.isfinite(got).all()
    if mode in ("pair", "pair-no-stem"):
        assert m._pair is not None
    if mode == "native":
        assert m.native_forward and m._native is None and not m._native_eligible()
    if mode == "dual-stream":
        assert m.dual_stream and m._twin is not None and m._twin[0].attn_window == SETTING and m._twin[0].attn_radial is True
    assert torch.equal(got, ref), f"{mode}: max |d| {float((got - ref).abs().max())}"
    if mode == "graphs":
        radial_key = SETTING + (True,)
        assert m._graphs_on and m._graphs and all(radial_key in key for key in m._graphs), "radial is part of the graph key"
        before = set(m._graphs)
        m.set_attention_window(*SETTING)                                          # the same engine, the flag off: new graphs, the window's bits
        _, _, noise, c1, c2, bl = _inputs()
        lat = noise.clone().to(DEV)
        m.denoise(lat, m.encode_context(c1), m.encode_context(c2), m.embed_buffers(bl), FlowMatchScheduler(STEPS), 5.0)
        torch.cuda.synchronize()
        fresh = set(m._graphs) - before
        assert fresh and all(SETTING in key and radial_key not in key for key in fresh), "a changed radial flag re-keys"
        assert torch.equal(lat, _sequential_latent(hip_ops, radial=False))


# ---- 7. pipeline and generator -------------------------------------------------------------------------------------------------------------
def _pipe():
    from infinicube_amd.videogen.ops import HipOps
    from infinicube_amd.videogen.pipeline import DiTHolder, WanVideoPipeline
    from standins import HashTextEncoder, PoolVAE
    p = WanVideoPipeline(DEV, torch.bfloat16, DiTHolder(syn.make_dit_state_dict(CFG), CFG), HashTextEncoder(CFG), PoolVAE(), ops=HipOps(DEV))
    p.num_inference_steps = 2
    return p


def toy_factory(torch_dtype, device, model_configs):
    return _pipe()


def test_pipeline_and_generator(tmp_path, monkeypatch):
    from PIL import Image
    from safetensors.torch import save_file
    from infinicube.videogen import WanVideoGenerator
    from standins import HashTextEncoder
    for key in ENV:
        monkeypatch.delenv(key, raising=False)
    T, F = GRID.T, GRID.tokens_per_frame
    window, sink = SETTING
    frac, most = _fraction_and_pieces(T, F, window, sink)
    want_record = dict(window=window, sink=sink, radial=True, key_fraction=frac, max_pieces=most)
    sem, co = syn.make_dummy_buffers(GRID)
    p = _pipe()
    p.initialize_buffer_embedder(16, zero_init=False)
    p.buffer_embedder.load_state_dict(syn.make_buffer_embedder_state_dict(CFG))
    kw = dict(prompt="a street", negative_prompt="bad", semantic_buffer_video=[Image.fromarray(f) for f in sem],
              coordinate_buffer_video=[Image.fromarray(f) for f in co], height=GRID.height, width=GRID.width, num_frames=GRID.num_frames, seed=3,
              return_latents=True)
    on = dict(attention_window_frames=window, attention_sink_frames=sink)
    base = p(**kw).cpu()
    assert p.attention_window_record is None
    win = p(**kw, **on).cpu()
    assert "radial" not in p.attention_window_record
    rad = p(**kw, **on, attention_radial=True).cpu()
    assert p.attention_window_record == want_record
    assert torch.isfinite(rad).all() and not torch.equal(rad, base) and not torch.equal(rad, win)
    assert torch.equal(p(**kw, **on, attention_radial=False).cpu(), win)
    # the restated loop on the pipeline's own inputs: its noise, its text contexts, its buffer latents
    enc = HashTextEncoder(CFG)
    g = torch.Generator(device="cpu").manual_seed(3)
    noise = torch.randn((1, 16) + GRID.latent_shape()[1:], generator=g, dtype=torch.float32)[0]
    from infinicube_amd.videogen.pipeline import _video_to_tensor
    bl = torch.cat([p.vae.encode(_video_to_tensor(vid, GRID.height, GRID.width)).float().cpu()
                    for vid in (kw["semantic_buffer_video"], kw["coordinate_buffer_video"])], dim=0)
    sd, bsd = R.round_state_dict_to_bf16(syn.make_dit_state_dict(CFG)), R.round_state_dict_to_bf16(syn.make_buffer_embedder_state_dict(CFG))
    ref = radial_denoise_loop(sd, bsd, CFG, noise, enc.encode("a street").float().cpu(), enc.encode("bad").float().cpu(), bl, 2, window, sink)
    psnr = R.psnr(rad, ref)
    print(f"pipeline, radial window {window} + {sink} anchor frame, vs the restated loop: {psnr:.1f} dB")
    assert psnr >= 40.0, f"{psnr:.1f} dB"
    full = p(**kw, attention_window_frames=T, attention_radial=True).cpu()
    assert torch.equal(full, base) and p.attention_window_record is None
    # the unchanged generator: the window from its two variables, radial from the pipeline's attribute
    path = str(tmp_path / "step-1.safetensors")
    save_file({"buffer_embedder." + key: val for key, val in syn.make_buffer_embedder_state_dict(CFG).items()}, path)
    import test_attn_radial_gpu as me
    monkeypatch.setenv("ICV_ATTN_WINDOW_FRAMES", str(window))
    monkeypatch.setenv("ICV_ATTN_SINK_FRAMES", str(sink))
    with contextlib.redirect_stdout(io.StringIO()):
        gen = WanVideoGenerator(path, device=DEV, use_wan_1pt3b=True, pipeline_factory=me.toy_factory)
        assert gen.pipe.attention_radial is None
        gen.pipe.attention_radial = True
        video = gen.generate(sem, co, prompt="a street", negative_prompt="bad", seed=3)
    assert len(video) == GRID.num_frames
    assert gen.pipe.attention_window_record == want_record
    assert torch.equal(gen.pipe(**kw).cpu(), rad), "the attribute must select what the keyword selects"
    gen.pipe.attention_radial = None
    assert torch.equal(gen.pipe(**kw).cpu(), win) and "radial" not in gen.pipe.attention_window_record
