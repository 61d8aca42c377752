"""Regenerating part of a clip (infinicube_amd/videogen/inpaint.py: ``input_mask``) on CPU: the TEST-ONLY torch twins of
icv_latent_keep_mask_u8 and icv_pin_known_f32 (the keep-mask twin against a brute-force triple loop), every form and refusal of
``validate``, the engine on twin operators (Euler and UniPC: the latent, x_hat and the newest x0-prediction slot at every step; the
zero-init and TeaCache launch counts), the pipeline (an all-regenerate mask is the call without one, the records, the
compositions), ``chain.plan`` and ``chain`` on the pooling VAE."""
import collections

import numpy as np
import pytest
import torch
from PIL import Image

from infinicube_amd.videogen import guidance as G
from infinicube_amd.videogen import inpaint, options, teacache
from infinicube_amd.videogen import solver as S
from infinicube_amd.videogen import synthetic as syn
from infinicube_amd.videogen.config import TokenGrid
from infinicube_amd.videogen.dit import WanDiT
from infinicube_amd.videogen.pipeline import _video_to_tensor
from infinicube_amd.videogen.scheduler import FlowMatchScheduler
from standins import PoolVAE
from test_attn_window_cpu import masked_attention
from test_cfg_zero_cpu import ZeroOps
from test_sliding_window_cpu import window_euler_twin
from test_teacache_cpu import LINEAR
from test_v2v_cpu import CFG, ENV, GRID, SHORT, TILES, _call_kw, _pipe, add_noise_twin, make_clip, pil

F32 = torch.float32
SHAPES = [(n, h, w) for n in (1, 5, 9) for h, w in ((16, 16), (64, 96))]


# ---- the TEST-ONLY twins ----------------------------------------------------------------------------------------------------------------
def keep_mask_twin(mask: torch.Tensor) -> torch.Tensor:
    """Torch twin of icv_latent_keep_mask_u8: mask u8 [N, H, W] (non-zero = regenerate) -> keep u8 [T, H/8, W/8]."""
    n, h, w = mask.shape
    t = (n - 1) // 4 + 1
    m = torch.cat([torch.zeros((3, h, w), dtype=torch.bool, device=mask.device), mask != 0])      # frame 0 alone in its group of four
    touched = m.reshape(t, 4, h // 8, 8, w // 8, 8).permute(0, 2, 4, 1, 3, 5).reshape(t, h // 8, w // 8, -1).any(-1)
    return (~touched).to(torch.uint8)


def keep_mask_brute(mask: np.ndarray) -> np.ndarray:
    n, h, w = mask.shape
    keep = np.zeros(((n - 1) // 4 + 1, h // 8, w // 8), dtype=np.uint8)
    for t in range(keep.shape[0]):
        frames = [0] if t == 0 else list(range(4 * t - 3, 4 * t + 1))
        for y in range(keep.shape[1]):
            for x in range(keep.shape[2]):
                keep[t, y, x] = int(not mask[frames, 8 * y: 8 * y + 8, 8 * x: 8 * x + 8].any())
    return keep


def pin_twin(latent, x0, noise, keep, sigma_next, x_hat=None, sigma_cur=0.0, m_new=None, round_bf16=False):
    """Torch twin of icv_pin_known_f32: add_noise_twin's arithmetic where keep != 0, nothing written elsewhere."""
    k = (keep != 0).expand_as(latent)
    for out, sigma in ((latent, sigma_next), (x_hat, sigma_cur)):
        if out is not None:
            pinned = torch.empty_like(x0)
            add_noise_twin(x0, noise, pinned, sigma, round_bf16)
            out[k] = pinned[k]
    if m_new is not None:
        m_new[k] = x0[k]


def pinned(x0, noise, sigma, round_bf16=False):
    out = torch.empty_like(x0)
    add_noise_twin(x0, noise, out, sigma, round_bf16)
    return out


class InpaintOps(ZeroOps):
    """OracleOps + every CPU twin the compositions need (TeaCache, multistep, CFG-Zero*, the window update, add_noise, the frame
    window) + the twins of the two kernels of this feature; logs every pin (``pins``) and counts the pooling calls."""

    def __init__(self, device="cpu"):
        super().__init__(device)
        self.pins, self.counts = [], collections.Counter()

    def unpatchify_cfg_euler_window(self, latent_next, hc, hu, cfg_scale, dsigma, frame_coef, frame0, tok0, n_tok, round_bf16=False):
        window_euler_twin(latent_next, hc, hu, cfg_scale, dsigma, frame_coef, frame0, tok0, n_tok, round_bf16)

    def add_noise(self, x0, noise, out, sigma, round_bf16=False):
        self.counts["add_noise"] += 1
        add_noise_twin(x0, noise, out, sigma, round_bf16)

    def attention_framewin(self, q, k, v, o, heads, scale, frames, frame_rows, window, sink):
        o.copy_(masked_attention(q.float(), k.float(), v.float(), heads, frames, frame_rows, window, sink, scale=scale).to(torch.bfloat16))

    def unpatchify_cfg_euler(self, *a, **k):
        self.counts["update"] += 1
        return super().unpatchify_cfg_euler(*a, **k)

    def latent_keep_mask(self, mask_u8, keep_u8):
        assert mask_u8.dtype == keep_u8.dtype == torch.uint8
        self.counts["latent_keep_mask"] += 1
        keep_u8.copy_(keep_mask_twin(mask_u8))

    def pin_known(self, latent, x0, noise, keep, sigma_next, x_hat=None, sigma_cur=0.0, m_new=None, round_bf16=False):
        assert latent.dtype == x0.dtype == noise.dtype == F32 and keep.dtype == torch.uint8 and tuple(keep.shape) == tuple(latent.shape[1:])
        assert len({t.data_ptr() for t in (latent, x0, noise, x_hat, m_new) if t is not None}) == 3 + (x_hat is not None) + (m_new is not None)
        self.pins.append(dict(sigma_next=sigma_next, sigma_cur=sigma_cur, state=x_hat is not None and m_new is not None,
                              updates_before=self.counts["update"] + len(self.multistep_calls)))
        pin_twin(latent, x0, noise, keep, sigma_next, x_hat, sigma_cur, m_new, round_bf16)


def corner_masks(n, h, w, cell):
    """One mask per corner of ``cell``'s footprint in time and space, a single byte set in each."""
    t, y, x = cell
    frames = (0,) if t == 0 else (4 * t - 3, 4 * t)
    for f in frames:
        for r in (8 * y, 8 * y + 7):
            for c in (8 * x, 8 * x + 7):
                m = np.zeros((n, h, w), dtype=np.uint8)
                m[f, r, c] = 255
                yield m


def half_mask(grid):
    """Kept: the frames of all latent frames but the last, and the top-left quarter of the last one's."""
    m = np.ones((grid.num_frames, grid.height, grid.width), dtype=np.uint8)
    m[: grid.num_frames - 4] = 0
    m[grid.num_frames - 4:, : grid.height // 2, : grid.width // 2] = 0
    return m


# ---- 1. the keep-mask twin ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_keep_mask_twin_against_the_triple_loop(shape):
    n, h, w = shape
    g = np.random.default_rng(n * 1000 + h)
    for density in (0.0, 1.0, 0.5, 1.0 / 4096):
        mask = (g.random(shape) < density).astype(np.uint8) * g.integers(1, 256, shape, dtype=np.uint8)
        assert np.array_equal(keep_mask_twin(torch.from_numpy(mask)).numpy(), keep_mask_brute(mask))
    t_last, y_last, x_last = (n - 1) // 4, h // 8 - 1, w // 8 - 1
    for cell in {(0, 0, 0), (t_last, y_last, x_last), (t_last, 0, x_last), (min(1, t_last), y_last, 0)}:
        for mask in corner_masks(n, h, w, cell):
            keep = keep_mask_twin(torch.from_numpy(mask)).numpy()
            want = np.ones_like(keep)
            want[cell] = 0
            assert np.array_equal(keep, want) and np.array_equal(keep, keep_mask_brute(mask)), cell
    if n > 1:                                                         # frame 0 belongs to latent frame 0 alone, frame 1 to latent frame 1
        mask = np.zeros(shape, dtype=np.uint8)
        mask[0] = 1
        keep = keep_mask_twin(torch.from_numpy(mask)).numpy()
        assert not keep[0].any() and keep[1:].all()
        mask = np.zeros(shape, dtype=np.uint8)
        mask[1] = 1
        keep = keep_mask_twin(torch.from_numpy(mask)).numpy()
        assert keep[0].all() and not keep[1].any() and keep[2:].all()


# ---- 2. validate and frame_mask -----------------------------------------------------------------------------------------------------------
def test_validate_forms_and_refusals(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    n, h, w = SHORT.num_frames, SHORT.height, SHORT.width
    clip = pil(make_clip(SHORT, 1))
    arr = half_mask(SHORT)
    for form in (arr, arr.astype(bool), arr * 255, [Image.fromarray(f * 255, mode="L") for f in arr], [Image.fromarray(f.astype(bool)) for f in arr]):
        got = inpaint.validate(form, clip, n, h, w)
        assert got.dtype == np.uint8 and got.flags["C_CONTIGUOUS"] and np.array_equal(got, arr)
    flags = [False] * 5 + [True] * 4
    assert np.array_equal(inpaint.validate(flags, clip, n, h, w), inpaint.frame_mask(n, h, w, range(5)))
    assert np.array_equal(inpaint.validate(tuple(np.asarray(flags)), clip, n, h, w), inpaint.frame_mask(n, h, w, slice(0, 5)))
    assert inpaint.validate(None, None, n, h, w) is None and inpaint.validate(None, clip, n, h, w) is None
    with pytest.raises(ValueError, match="outside"):
        inpaint.frame_mask(n, h, w, [9])
    for bad, msg in ((arr[:8], r"input_mask has shape \(8, 64, 96\), the call needs \(9, 64, 96\)"),
                     (arr[:, :32], "masks are not resized"),
                     (arr.astype(np.float32), "expected a uint8 or bool array, got float32"),
                     (arr.astype(np.int64), "expected a uint8 or bool array, got int64"),
                     (flags[:8], "input_mask has 8 frames, num_frames=9"),
                     ([Image.fromarray(f) for f in arr][:5], "input_mask has 5 frames, num_frames=9"),
                     ([Image.new("RGB", (w, h))] * n, "frame 0 is a RGB image, a mask frame has one channel"),
                     ([Image.new("L", (w, h // 2))] * n, "frame 0 is 96x32, the call is 96x64"),
                     ([0, 1] * 4 + [0], "input_mask must be a uint8 / bool array"),
                     (3, "input_mask must be a uint8 / bool array")):
        with pytest.raises(ValueError, match=msg):
            inpaint.validate(bad, clip, n, h, w)
    # through the pipeline: before any encode, any engine
    class NoEncode(PoolVAE):
        def encode(self, *a, **k):
            raise AssertionError("vae.encode was called")
    p = _pipe(InpaintOps(), vae=NoEncode())
    with pytest.raises(ValueError, match="input_mask needs an input_video"):
        p(**_call_kw(input_mask=arr))
    with pytest.raises(ValueError, match="masks are not resized"):
        p(**_call_kw(input_video=clip, input_mask=arr[:, :32]))
    assert p._engine is None and p.inpaint_record is None


# ---- 3. the engine on twin operators ------------------------------------------------------------------------------------------------------
STEPS = 3


def _engine(ops):
    m = WanDiT(CFG, syn.make_dit_state_dict(CFG), ops, syn.make_buffer_embedder_state_dict(CFG)).prepare(SHORT)
    return m, m.encode_context(syn.make_text_context(CFG, 1)), m.encode_context(syn.make_text_context(CFG, 2)), m.embed_buffers(syn.make_buffer_latents(CFG, SHORT))


def _known(keep, seed=5, rounding=False):
    """x0 and the noise through bf16 under reference rounding, as the pipeline hands them over."""
    g = torch.Generator().manual_seed(seed)
    x0, noise = (torch.randn(SHORT.latent_shape(), generator=g) for _ in range(2))
    return inpaint.KnownPlan(*((x0.to(torch.bfloat16).to(F32), noise.to(torch.bfloat16).to(F32)) if rounding else (x0, noise)), keep)


def _run(ops, known, solver=False, on_step=None, rounding=False, **kw):
    m, cc, cu, bt = _engine(ops)
    sch = FlowMatchScheduler(STEPS, 5.0, rounding, denoising_strength=0.8)
    lat = pinned(known.x0, known.noise, sch.sigmas[0], rounding)
    plan = S.MultistepPlan("unipc", sch.sigmas) if solver else None
    m.denoise(lat, cc, cu, bt, sch, 5.0, round_bf16=rounding, solver=plan, on_step=(lambda i, x: on_step(m, sch, i, x)) if on_step else None,
              **(dict(known=known) if known.keep is not None else {}), **kw)
    return m, sch, lat


@pytest.mark.parametrize("rounding", [False, True], ids=["exact", "reference-rounding"])
@pytest.mark.parametrize("solver", [False, True], ids=["euler", "unipc"])
@pytest.mark.parametrize("keep", ["all", "half"])
def test_engine_pins_the_latent_and_the_solver_state(keep, solver, rounding):
    keep_t = torch.ones(SHORT.latent_shape()[1:], dtype=torch.uint8) if keep == "all" else keep_mask_twin(torch.from_numpy(half_mask(SHORT)))
    assert 0 < int(keep_t.sum()) and (keep == "all" or int(keep_t.sum()) < keep_t.numel())
    known = _known(keep_t, rounding=rounding)
    k = (keep_t != 0).expand(SHORT.latent_shape())
    seen = []

    def on_step(m, sch, i, lat):
        nxt = sch.sigmas[i + 1] if i + 1 < STEPS else 0.0
        assert torch.equal(lat[k], pinned(known.x0, known.noise, nxt, rounding)[k]), f"step {i}: latent"
        if solver:
            x_hat, ring = m._solver_buffers(lat)
            assert torch.equal(x_hat[k], pinned(known.x0, known.noise, sch.sigmas[i], rounding)[k]), f"step {i}: x_hat"
            assert torch.equal(ring[i % 3][k], known.x0[k]), f"step {i}: newest x0-prediction"
        seen.append(i)

    ops = InpaintOps()
    _, sch, lat = _run(ops, known, solver, on_step, rounding)
    assert seen == list(range(STEPS)) and torch.equal(lat[k], known.x0[k]) and torch.isfinite(lat).all()
    assert [p["sigma_next"] for p in ops.pins] == sch.sigmas[1:] + [0.0] and [p["updates_before"] for p in ops.pins] == [1, 2, 3]
    assert all(p["state"] == solver for p in ops.pins) and (not solver or [p["sigma_cur"] for p in ops.pins] == sch.sigmas)
    _, _, plain = _run(InpaintOps(), inpaint.KnownPlan(known.x0, known.noise, None), solver, None, rounding)
    if keep == "half":
        assert not torch.equal(lat[~k], plain[~k]), "the kept cells must steer the others"
    assert not torch.equal(plain[k], known.x0[k])


def test_known_none_is_todays_loop():
    known = _known(None)
    ops = InpaintOps()
    _run(ops, known)
    assert ops.pins == [] and ops.counts["latent_keep_mask"] == 0


def test_zero_init_pins_once_before_the_first_executed_step():
    keep_t = keep_mask_twin(torch.from_numpy(half_mask(SHORT)))
    known = _known(keep_t)
    k = (keep_t != 0).expand(SHORT.latent_shape())
    ops, first = InpaintOps(), {}

    def on_step(m, sch, i, lat):
        if i == 0:                                                    # the skipped step: nothing ran, the start latent's bits
            first["ok"] = torch.equal(lat, pinned(known.x0, known.noise, sch.sigmas[0])) and ops.pins == []

    _, sch, lat = _run(ops, known, on_step=on_step, guidance=G.GuidancePlan(False, 1))
    assert first["ok"]
    assert [(p["sigma_next"], p["updates_before"]) for p in ops.pins] == [(sch.sigmas[1], 0), (sch.sigmas[2], 1), (0.0, 2)]
    assert torch.equal(lat[k], known.x0[k])


def test_more_than_one_rank_raises():
    m, cc, cu, bt = _engine(InpaintOps())
    known = _known(torch.ones(SHORT.latent_shape()[1:], dtype=torch.uint8))
    m.sp_on = True
    with pytest.raises(ValueError, match="known cells .* cannot be combined with sequence / CFG-branch parallelism"):
        m.denoise(known.noise.clone(), cc, cu, bt, FlowMatchScheduler(2), 5.0, known=known)
    m.sp_on = False
    with pytest.raises(ValueError, match="do not fit a latent"):
        m.denoise(known.noise.clone(), cc, cu, bt, FlowMatchScheduler(2), 5.0, known=inpaint.KnownPlan(known.x0, known.noise, known.keep[:2]))


# ---- 4. the pipeline on twin operators ----------------------------------------------------------------------------------------------------
def _x0(p, clip, grid=SHORT):
    return p.vae.encode(_video_to_tensor(clip, grid.height, grid.width), tiled=True, **TILES).to(F32)


def test_all_regenerate_mask_is_the_call_without_a_mask(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    ops = InpaintOps()
    p = _pipe(ops)
    clip = pil(make_clip(SHORT, 1))
    kw = _call_kw(input_video=clip, denoising_strength=0.6)
    base = p(**kw)
    assert p.inpaint_record is None
    records = {name: getattr(p, name) for name in options.RECORDS.values()}
    allocs = []
    raw = ops.alloc
    monkeypatch.setattr(ops, "alloc", lambda shape, dtype: (allocs.append(tuple(shape)), raw(shape, dtype))[1])
    got = p(**kw, input_mask=np.ones((9, 64, 96), dtype=np.uint8))
    assert torch.equal(got, base) and ops.pins == [] and ops.counts["latent_keep_mask"] == 1
    assert tuple(got.shape) not in allocs, "nothing kept: no copy of the noise"
    assert p.inpaint_record == dict(cells=288, kept_cells=0, kept_fraction=0.0)
    assert {name: getattr(p, name) for name in options.RECORDS.values()} == records
    # a kept part: the records of every other feature are what they were, the mask's own is set, and a later call resets it
    half = half_mask(SHORT)
    got = p(**kw, input_mask=half)
    kept = int(keep_mask_twin(torch.from_numpy(half)).sum())
    assert kept == 2 * 96 + 24 and p.inpaint_record == dict(cells=288, kept_cells=kept, kept_fraction=kept / 288)
    assert {name: getattr(p, name) for name in options.RECORDS.values()} == records
    assert len(ops.pins) == 2 and not torch.equal(got, base)
    p(**kw)
    assert p.inpaint_record is None


COMPOSE = {
    "plain": (SHORT, {}),
    "strength-1": (SHORT, dict(denoising_strength=1.0)),
    "unipc": (SHORT, dict(sample_solver="unipc", num_inference_steps=3)),
    "cfg-zero": (SHORT, dict(cfg_zero_star=True, cfg_zero_init_steps=1, num_inference_steps=3)),
    "teacache": (SHORT, dict(tea_cache_l1_thresh=1e9, tea_cache_model_id="test-linear", num_inference_steps=6)),
    "attention-window": (SHORT, dict(attention_window_frames=1)),
    "two-sliding-windows": (GRID, dict(sliding_window_size=6, sliding_window_stride=3)),
}


def check_composition(p, name, pins_of, run_plain=True):
    """The mask with one other feature: the call runs, the other feature's record says it ran, the kept cells equal the encoded
    clip, and one pin follows every update (plus the one in front of a zero-init start)."""
    grid, extra = COMPOSE[name]
    clip = pil(make_clip(grid, 1))
    kw = _call_kw(grid, input_video=clip, **{"denoising_strength": 0.6, **extra})
    mask = half_mask(grid)
    got = p(**kw, input_mask=mask).cpu()
    k = (keep_mask_twin(torch.from_numpy(mask)) != 0).expand(grid.latent_shape())
    x0 = _x0(p, clip, grid)
    assert torch.isfinite(got).all() and torch.equal(got[k], x0[k]), name
    steps = kw["num_inference_steps"]
    record = {"unipc": "solver_record", "cfg-zero": "guidance_record", "teacache": "tea_cache_record", "attention-window": "attention_window_record",
              "two-sliding-windows": "sliding_window_record"}.get(name)
    assert record is None or getattr(p, record) is not None
    if name == "two-sliding-windows":
        assert len(p.sliding_window_record) == 2
    if name == "teacache":
        assert p.tea_cache_record["computed"] == [0, 5]
    if pins_of is not None:
        assert len(pins_of()) == steps, name                          # cfg-zero: steps - 1 executed + the one in front
    if run_plain:
        assert not torch.equal(got[~k], p(**kw).cpu()[~k])
    return got, dict(kw, input_mask=mask)


@pytest.mark.parametrize("name", list(COMPOSE))
def test_mask_composes(name, monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setitem(teacache.COEFFICIENTS, "test-linear", LINEAR)
    ops = InpaintOps()
    p = _pipe(ops)
    check_composition(p, name, lambda: ops.pins)
    if name == "cfg-zero":
        assert ops.pins[0]["updates_before"] == 0


# ---- 5. continuing a clip -------------------------------------------------------------------------------------------------------------------
def test_chain_plan():
    for (n, clip, ov), starts, overlaps in (((17, 9, 5), [0, 4, 8], [0, 5, 5]), ((21, 9, 5), [0, 4, 8, 12], [0, 5, 5, 5]),
                                           ((33, 17, 5), [0, 12, 16], [0, 5, 13]), ((93, 93, 9), [0], [0])):
        p = inpaint.chain.plan(n, clip, ov)
        assert (p.starts, p.overlaps) == (starts, overlaps)
        assert all(s % 4 == 0 for s in p.starts) and all(o % 4 == 1 for o in p.overlaps[1:]) and p.starts[-1] + clip == n
    assert inpaint.plan(185)[0] == [0, 84, 92] and inpaint.plan(185)[1] == [0, 9, 85]
    for args, msg in (((16, 9, 5), "num_frames must be an integer 4k"), ((17, 8, 5), "clip_frames must be an integer 4k"),
                      ((17, 9, 4), "overlap_frames must be an integer 4k"), ((17, 9, 9), "must be smaller than clip_frames"),
                      ((17, 9, 13), "must be smaller than clip_frames"), ((5, 9, 5), "fewer than one clip"),
                      ((17.0, 9, 5), "num_frames must be an integer"), ((17, 9, True), "overlap_frames must be an integer")):
        with pytest.raises(ValueError, match=msg):
            inpaint.chain.plan(*args)


class RecordingVAE(PoolVAE):
    """PoolVAE that keeps every latent it was asked to decode."""

    def __init__(self):
        super().__init__()
        self.decoded = []

    def decode(self, latent, **kw):
        self.decoded.append(latent.detach().clone().cpu())
        return super().decode(latent, **kw)


def check_chain(p, vae):
    """N = 17 as clips of 9 frames overlapping by 5: N frames out, clip 0 is the plain call, and the kept latent cells of every
    later call are the encoding of the frames before it - which, the encoder being causal, the overlap alone decides."""
    grid = TokenGrid(17, 64, 96)
    sem, co = syn.make_dummy_buffers(grid)
    sem, co = pil(sem), pil(co)
    kw = dict(prompt="a street", negative_prompt="bad", height=64, width=96, num_inference_steps=2)
    out = inpaint.chain(p, semantic_buffer_video=sem, coordinate_buffer_video=co, clip_frames=9, overlap_frames=5, seed=3, **kw)
    assert len(out) == 17 and all(f.size == (96, 64) for f in out) and len(vae.decoded) == 3
    assert p.inpaint_record == dict(cells=288, kept_cells=192, kept_fraction=192 / 288)
    for j, start in ((1, 4), (2, 8)):
        held = out[start: start + 5]
        for filler in (held[-1], Image.new("RGB", (96, 64))):
            x0 = vae.encode(_video_to_tensor(held + [filler] * 4, 64, 96)).to(F32)
            assert torch.equal(vae.decoded[j][:, :2], x0[:, :2]), f"clip {j}"
        assert not torch.equal(vae.decoded[j][:, 2], x0[:, 2])
    plain = p(**kw, semantic_buffer_video=sem[:9], coordinate_buffer_video=co[:9], num_frames=9, seed=3)
    assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(out[:9], plain))
    assert torch.equal(vae.decoded[3], vae.decoded[0]) and p.inpaint_record is None
    with pytest.raises(ValueError, match="return_latents"):
        inpaint.chain(p, semantic_buffer_video=sem, coordinate_buffer_video=co, clip_frames=9, overlap_frames=5, return_latents=True, **kw)
    with pytest.raises(ValueError, match="chain sets input_mask itself"):
        inpaint.chain(p, semantic_buffer_video=sem, coordinate_buffer_video=co, clip_frames=9, overlap_frames=5, input_mask=[True] * 9, **kw)


def test_chain_on_the_pooling_vae(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    vae = RecordingVAE()
    check_chain(_pipe(InpaintOps(), vae=vae), vae)


# ---- 6. the kernels' argument checks run on the host, before any launch ---------------------------------------------------------------------
def test_kernel_argument_validation_without_gpu():
    from infinicube_amd import native
    lib = native.lib()
    assert lib.icv_pin_known_f32(None, None, None, None, None, None, 0, 64, 0.5, 0.5, 0, None) == 0        # C == 0 / cells == 0: nothing
    assert lib.icv_pin_known_f32(None, None, None, None, None, None, 16, 0, 0.5, 0.5, 0, None) == 0
    for args, msg in (((16, None, None, 16, 16, 16, -1, 4), b"negative size"), ((16, None, None, 16, 16, 16, 4, -1), b"negative size"),
                      ((None, None, None, 16, 16, 16, 4, 4), b"null argument"), ((16, None, None, None, 16, 16, 4, 4), b"null argument"),
                      ((16, None, None, 16, None, 16, 4, 4), b"null argument"), ((16, None, None, 16, 16, None, 4, 4), b"null argument"),
                      ((18, None, None, 16, 16, 16, 4, 4), b"4-byte aligned"), ((16, 17, None, 16, 16, 16, 4, 4), b"4-byte aligned"),
                      ((16, None, 18, 16, 16, 16, 4, 4), b"4-byte aligned"), ((16, None, None, 16, 19, 16, 4, 4), b"4-byte aligned")):
        assert lib.icv_pin_known_f32(*args, 0.5, 0.5, 0, None) != 0 and msg in lib.icv_last_error(), args
    assert lib.icv_latent_keep_mask_u8(None, None, 5, 0, 16, None) == 0
    for args, msg in (((16, 16, 4, 16, 16), b"need 4k + 1"), ((16, 16, 0, 16, 16), b"need 4k + 1"), ((16, 16, 5, 24, 16), b"multiples of 16"),
                      ((16, 16, 5, 16, 8), b"multiples of 16"), ((None, 16, 5, 16, 16), b"null argument"), ((16, None, 5, 16, 16), b"null argument")):
        assert lib.icv_latent_keep_mask_u8(*args, None) != 0 and msg in lib.icv_last_error(), args
