"""Frame-windowed self-attention on the HIP path (csrc/attn7p.hip, icv_attention_fwd_framewin): bit identity with the per-frame
icv_attention_fwd_pieces launches the one launch replaces, parity with fp32 masked attention (spikes inside the anchor, in the last
window frame and one frame OUTSIDE a row's mask), one frame = the plain launch, the write guard under strided operands, the host-side
argument checks, every driver mode of the DiT, and the pipeline / the unchanged generator."""
import contextlib
import io
import math

import pytest
import torch

from infinicube_amd.videogen import attn_window as AW
from infinicube_amd.videogen import synthetic as syn
from oracle import wan_ref as R
from test_attn_window_cpu import CFG, ENV, GRID, _loop, frame_mask, masked_attention, reference, windowed_denoise_loop
from test_kernels_gpu import assert_bf16_close, rnd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALE = 1.0 / math.sqrt(128)
LOG2E = 1.4426950408889634
SETTINGS = [(1, 1), (1, 0), (0, 2), (2, 1)]       # (window, sink): single-range, merged and two-range frames at T = 5
BF16 = torch.bfloat16


def _qkv(T, F, H, seed, unit):
    """q, k, v bf16 [T * F, H * 128] on the CPU and the launch's scale.  ``unit``: the code path the DiT runs - the softmax scale and
    log2(e) folded into K, scale = ln 2."""
    d = H * 128
    q, k, v = (rnd((T * F, d), seed + i).to(BF16) for i in range(3))
    return q, k, v, (math.log(2.0) if unit else SCALE)


def _fold(k, unit):
    return (k.float() * SCALE * LOG2E).to(BF16) if unit else k


def _framewin(hip_ops, q, k, v, H, scale, T, F, window, sink):
    o = torch.zeros_like(q)
    hip_ops.attention_framewin(q, k, v, o, H, scale, T, F, window, sink)
    return o


# ---- 1. bit identity with the launches it replaces ---------------------------------------------------------------------------------
@pytest.mark.parametrize("unit", [False, True])
def test_bit_identical_to_the_per_frame_pieces_launches(hip_ops, unit):
    """T = 5, F = 300: two q-blocks per frame, the second with 44 rows (its waves 2..7 hold no row at all), and a ragged 44-key tail tile
    in every piece.  Per frame, the existing launch over that frame's pieces is the reference: same tiles, same order, same bits."""
    T, F, H = 5, 300, 2
    q, k, v, scale = _qkv(T, F, H, 400, unit)
    q, k, v = q.to(DEV), _fold(k, unit).to(DEV), v.to(DEV)
    for window, sink in SETTINGS:
        want = torch.zeros_like(q)
        for f, pieces in enumerate(AW.ranges(T, window, sink)):
            rows = slice(f * F, (f + 1) * F)
            hip_ops.attention_pieces(q[rows], [(k[a * F: b * F], v[a * F: b * F], -1, 0) for a, b in pieces], want[rows], H, scale)
        got = _framewin(hip_ops, q, k, v, H, scale, T, F, window, sink)
        diff = (got != want).any(dim=1)
        assert torch.equal(got, want), f"window={window} sink={sink}: {int(diff.sum())} rows differ, first {int(diff.nonzero()[0]) if diff.any() else -1}"
    two = [len(r) for r in AW.ranges(T, 1, 1)]
    assert two == [1, 1, 1, 2, 2], "the settings must cover single-range, merged and two-range frames"


# ---- 2. parity with fp32 masked attention ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unit", [False, True])
@pytest.mark.parametrize("T,F,window,sink", [(5, 300, w, s) for w, s in SETTINGS] + [(9, 40, 2, 0), (9, 40, 1, 3)])
def test_parity_with_fp32_masked_attention(hip_ops, T, F, window, sink, unit):
    """Spikes (key = 5 q: that key takes the whole softmax of that query) planted as tests/test_attn_pieces_gpu.py does: one in frame 0 -
    inside the anchor when there is one - for a query of the last frame, one in the LAST frame of a query's window, and two just
    outside a mask: the last row of the frame in front of a query's window and the first row of the frame behind one.  A `lo` or `hi`
    that is off by one frame reads such a key, and it then owns the row.  Rows whose mask excludes a planted key must come out
    bit-identical to the launch without it.  F = 40: a frame shorter than one 64-key tile."""
    H = 2
    q, k, v, scale = _qkv(T, F, H, 410 + T, unit)
    mask = frame_mask(T, window, sink)
    row_a = (T - 1) * F + 7                                      # query of the last frame -> key in frame 0
    row_b, g_b = 1 * F + 3, min(T - 1, 1 + window)               # query of frame 1 -> key in the last frame of its window
    k[5] = q[row_a] * 5.0
    k[g_b * F + F - 2] = q[row_b] * 5.0
    assert mask[1, g_b] and mask[T - 1, 0] == (sink > 0 or window >= T - 1)
    g_c = T - 2 - window                                         # the frame in front of the last frame's window
    row_c, key_c = (T - 1) * F + F - 1, (g_c + 1) * F - 1        # ... its last row
    g_d = window + 1                                             # the frame behind frame 0's window
    row_d, key_d = 11, g_d * F                                   # ... its first row
    assert g_c >= 0 and g_d < T and not mask[T - 1, g_c]
    plain_c, plain_d = k[key_c].clone(), k[key_d].clone()
    k[key_c] = q[row_c] * 5.0
    k[key_d] = q[row_d] * 5.0
    # the reference reads the K the kernel reads (unit: after the fold's rounding to bf16), at the launch's scale
    ref = masked_attention(q.float(), _fold(k, unit).float(), v.float(), H, T, F, window, sink, scale=scale)
    qd, kd, vd = q.to(DEV), _fold(k, unit).clone().to(DEV), v.to(DEV)
    got = _framewin(hip_ops, qd, kd, vd, H, scale, T, F, window, sink)
    assert_bf16_close(got, ref, f"framewin T={T} F={F} window={window} sink={sink} unit={unit}", abs_floor=2.0 ** -5, rms_bound=2.0 ** -7)
    outside = 0
    for row, g, key, plain in ((row_c, g_c, key_c, plain_c), (row_d, g_d, key_d, plain_d)):
        if mask[row // F, g]:                                    # (0, 2): frame 1 is behind frame 0's window but inside the anchor
            continue
        outside += 1
        kd[key] = _fold(plain, unit).to(DEV)                     # the same launch without THIS planted key (the other stays: a later frame may see it)
        without = _framewin(hip_ops, qd, kd, vd, H, scale, T, F, window, sink)
        kd[key] = _fold(k[key], unit).to(DEV)
        assert torch.equal(got[row], without[row]), f"row {row} (frame {row // F}) was moved by a key of frame {g}, outside its mask"
        assert not torch.equal(got, without), "the planted key must be visible to the frames that do read it"
        assert float((ref[row] - v[key].float()).abs().max()) > 0.5, "had the row read the planted key, it would be that key's value row"
    assert outside >= 1
    # the spikes that ARE visible own their rows: the output is that key's value row
    for row, key in ((row_b, g_b * F + F - 2),) + (((row_a, 5),) if mask[T - 1, 0] else ()):
        assert float((got[row].float().cpu() - v[key].float()).abs().max()) <= 2.0 ** -5 * float(v[key].float().abs().max()) + 2.0 ** -7


# ---- 3. one frame is the plain launch --------------------------------------------------------------------------------------------------
def test_one_frame_is_the_plain_launch(hip_ops):
    T, F, H = 1, 700, 3
    q, k, v, scale = _qkv(T, F, H, 430, False)
    q, k, v = q.to(DEV), k.to(DEV), v.to(DEV)
    want = torch.zeros_like(q)
    hip_ops.attention(q, k, v, want, H, scale)
    for window, sink in ((0, 0), (3, 0), (0, 1), (1 << 40, 1)):
        assert torch.equal(_framewin(hip_ops, q, k, v, H, scale, T, F, window, sink), want), f"window={window} sink={sink}"


# ---- 4. write guard and strides --------------------------------------------------------------------------------------------------------
def test_write_guard_and_strides(hip_ops):
    """q, k, v as column views of one wider [3, S, d + 128] buffer, o as the top-left corner of a larger matrix full of sentinels: only
    o's S x d elements may change, the result must not depend on the strides, and a second run must give the same bits."""
    T, F, H, window, sink = 5, 300, 2, 1, 1
    d, S = H * 128, T * F
    q, k, v, scale = _qkv(T, F, H, 440, False)
    want = _framewin(hip_ops, q.to(DEV), k.to(DEV), v.to(DEV), H, scale, T, F, window, sink)
    wide = torch.full((3, S, d + 128), 3.0, dtype=BF16, device=DEV)
    for i, x in enumerate((q, k, v)):
        wide[i, :, :d] = x.to(DEV)
    obuf = torch.full((S + 2, d + 64), -7.0, dtype=BF16, device=DEV)
    o = obuf[:S, :d]
    assert wide[0, :, :d].stride(0) == d + 128 and o.stride(0) == d + 64
    runs = []
    for _ in range(2):
        o.fill_(-7.0)
        hip_ops.attention_framewin(wide[0, :, :d], wide[1, :, :d], wide[2, :, :d], o, H, scale, T, F, window, sink)
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
    q, k, v, scale = _qkv(T, F, H, 450, False)
    q, k, v = q.to(DEV), k.to(DEV), v.to(DEV)
    o = torch.full_like(q, -7.0)
    lib, ld = hip_ops.lib, H * 128

    def call(frames=T, frame_rows=F, ldk=ld, window=1, sink=1):
        rc = lib.icv_attention_fwd_framewin(q.data_ptr(), ld, k.data_ptr(), ldk, v.data_ptr(), ld, o.data_ptr(), ld, frames, frame_rows, H, window, sink,
                                            scale, hip_ops._stream())
        return rc, lib.icv_last_error()

    for kw, msg in ((dict(sink=T + 1), b"sink (6) exceeds the 5 frames"), (dict(frame_rows=0), b"empty problem"), (dict(ldk=ld + 4), b"16-byte row alignment")):
        rc, err = call(**kw)
        assert rc != 0 and msg in err, (kw, rc, err)
    torch.cuda.synchronize()
    assert (o == -7.0).all(), "a refused call must launch nothing"
    assert call()[0] == 0
    torch.cuda.synchronize()
    assert torch.isfinite(o.float()).all() and not (o == -7.0).all()
    with pytest.raises(ValueError, match="5 frames of 299 rows"):
        hip_ops.attention_framewin(q, k, v, o, H, scale, T, F - 1, 1, 1)


# ---- 6. driver modes ---------------------------------------------------------------------------------------------------------------------
def _sequential(m):
    m.cfg_batch = False


def test_sequential_forward_matches_masked_restatement_and_differs_from_dense(hip_ops):
    """Tiny DiT, 5 latent frames, window 1 + 1 anchor frame, three steps with CFG through the sequential per-op driver: latent PSNR
    >= 40 dB against the masked restatement (the project's loop bar), and not the dense loop's latent."""
    m, lat = _loop(hip_ops, 1, 1, setup=_sequential, prep=dict(graphs=False), dev=DEV)
    torch.cuda.synchronize()
    assert m._pair is None and m.attn_window == (1, 1)
    p = R.psnr(lat.cpu(), reference(1, 1))
    print(f"HIP frame-windowed loop vs masked restatement: {p:.1f} dB")
    assert p >= 40.0, f"{p:.1f} dB"
    _, dense = _loop(hip_ops, None, None, setup=_sequential, prep=dict(graphs=False), dev=DEV)
    torch.cuda.synchronize()
    assert not torch.equal(lat, dense), "the window must change the result"
    _, full = _loop(hip_ops, GRID.T - 1, 1, setup=_sequential, prep=dict(graphs=False), dev=DEV)
    torch.cuda.synchronize()
    assert torch.equal(full, dense), "a window that covers the clip is the plain path"


@pytest.mark.parametrize("mode", ["pair", "pair-no-stem", "native", "graphs", "dual-stream"])
def test_driver_modes_match_sequential_loop(hip_ops, mode, monkeypatch):
    """Every driver mode takes the frame-windowed launch: bit-identical to the sequential per-op loop.  The one-call C driver does not
    know the window: the per-op driver runs."""
    _, ref = _loop(hip_ops, 1, 1, setup=_sequential, prep=dict(graphs=False), dev=DEV)
    prep, setup = dict(graphs=False), None
    if mode == "pair-no-stem":
        setup = lambda m: setattr(m, "share_stem", False)                        # noqa: E731
    elif mode == "native":
        setup = lambda m: setattr(m, "native_forward", True)                     # noqa: E731
    elif mode == "graphs":
        prep = dict(graphs=True)
    elif mode == "dual-stream":
        monkeypatch.setenv("ICV_DUAL_STREAM", "1")
    m, got = _loop(hip_ops, 1, 1, setup=setup, prep=prep, dev=DEV)
    torch.cuda.synchronize()
    assert torch.isfinite(got).all()
    if mode in ("pair", "pair-no-stem"):
        assert m._pair is not None
    if mode == "native":
        assert m.native_forward and m._native is None and not m._native_eligible()
    if mode == "graphs":
        assert m._graphs_on and m._graphs and all((1, 1) in key for key in m._graphs),"the window is part of the graph key"
    if mode == "dual-stream":
        assert m.dual_stream and m._twin is not None and m._twin[0].attn_window == (1, 1)
    assert torch.equal(got, ref), f"{mode}: max |d| {float((got - ref).abs().max())}"


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
    T = GRID.T
    sem, co = syn.make_dummy_buffers(GRID)
    p = _pipe()
    p.initialize_buffer_embedder(16, zero_init=False)
    p.buffer_embedder.load_state_dict(syn.make_buffer_embedder_state_dict(CFG))
    kw = dict(prompt="a street", negative_prompt="bad", semantic_buffer_video=[Image.fromarray(f) for f in sem],
              coordinate_buffer_video=[Image.fromarray(f) for f in co], height=GRID.height, width=GRID.width, num_frames=GRID.num_frames, seed=3,
              return_latents=True)
    base = p(**kw).cpu()
    assert p.attention_window_record is None
    win = p(**kw, attention_window_frames=1, attention_sink_frames=1).cpu()
    assert p.attention_window_record == dict(window=1, sink=1, key_fraction=float(frame_mask(T, 1, 1).mean()))
    assert torch.isfinite(win).all() and not torch.equal(win, base)
    # the restated loop on the pipeline's own inputs: its noise, its text contexts, its buffer latents
    enc = HashTextEncoder(CFG)
    g = torch.Generator(device="cpu").manual_seed(3)
    noise = torch.randn((1, 16) + GRID.latent_shape()[1:], generator=g, dtype=torch.float32)[0]
    from infinicube_amd.videogen.pipeline import _video_to_tensor
    bl = torch.cat([p.vae.encode(_video_to_tensor(vid, GRID.height, GRID.width)).float().cpu()
                    for vid in (kw["semantic_buffer_video"], kw["coordinate_buffer_video"])], dim=0)
    sd, bsd = R.round_state_dict_to_bf16(syn.make_dit_state_dict(CFG)), R.round_state_dict_to_bf16(syn.make_buffer_embedder_state_dict(CFG))
    ref = windowed_denoise_loop(sd, bsd, CFG, noise, enc.encode("a street").float().cpu(), enc.encode("bad").float().cpu(), bl, 2, 1, 1)
    psnr = R.psnr(win, ref)
    print(f"pipeline, window 1 + 1 anchor frame, vs the restated loop: {psnr:.1f} dB")
    assert psnr >= 40.0, f"{psnr:.1f} dB"
    full = p(**kw, attention_window_frames=T).cpu()
    assert torch.equal(full, base) and p.attention_window_record is None
    # the unchanged generator: the two variables switch the same path on
    path = str(tmp_path / "step-1.safetensors")
    save_file({"buffer_embedder." + key: val for key, val in syn.make_buffer_embedder_state_dict(CFG).items()}, path)
    import test_attn_window_gpu as me

    def generator_latents(**env):
        for key, val in env.items():
            monkeypatch.setenv(key, val)
        with contextlib.redirect_stdout(io.StringIO()):
            gen = WanVideoGenerator(path, device=DEV, use_wan_1pt3b=True, pipeline_factory=me.toy_factory)
            video = gen.generate(sem, co, prompt="a street", negative_prompt="bad", seed=3)
        assert len(video) == GRID.num_frames
        record = gen.pipe.attention_window_record
        lat = gen.pipe(**kw).cpu()                  # the generator's pipeline, its settings from the environment
        assert gen.pipe.attention_window_record == record
        for key in env:
            monkeypatch.delenv(key)
        return lat, record

    lat, record = generator_latents(ICV_ATTN_WINDOW_FRAMES="1", ICV_ATTN_SINK_FRAMES="1")
    assert record == dict(window=1, sink=1, key_fraction=float(frame_mask(T, 1, 1).mean()))
    assert torch.equal(lat, win), "the environment must select what the keywords select"
    lat, record = generator_latents(ICV_ATTN_WINDOW_FRAMES=str(T))
    assert record is None and torch.equal(lat, base)
