"""Regenerating part of a clip on the HIP path: icv_latent_keep_mask_u8 and icv_pin_known_f32 against their torch twins bit for bit
(every size class, every pointer-offset class, both rounding modes, with and without the solver's state, between guard bands, over
NaN-patterned outputs), their contract, the HIP pipeline against the engine driven by hand with the pins issued by the test, every
driver mode and composition against the sequential loop, upstream's inpainting loop restated in fp32 on the GPU, and ``chain``."""
import itertools

import numpy as np
import pytest
import torch

from infinicube_amd.videogen import inpaint, teacache
from infinicube_amd.videogen.config import TokenGrid
from infinicube_amd.videogen.scheduler import FlowMatchScheduler
from oracle import wan_ref as R
from test_buffer_edges_gpu import Arena
from test_inpaint_cpu import (COMPOSE, SHAPES, RecordingVAE, check_chain, check_composition, corner_masks, half_mask, keep_mask_twin, pin_twin)
from test_teacache_cpu import LINEAR
from test_v2v_cpu import CFG, ENV, SHORT, _call_kw, add_noise_twin, drive_by_hand, make_clip, oracle_inputs, pil, strength_sigmas
from test_v2v_gpu import FP8, OFFSETS, _pipe, _sequential

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

GPU_SHAPES = SHAPES + [(n, 48, 80) for n in (1, 5, 9)]
CELLS = (1, 3, 4, 5, 255, 256, 257, 4 * 260 + 3)     # below one vector, around one wave of vectors, whole and ragged channels, more than one block
SIGMAS = (0.0, 1.0, 0.5, FlowMatchScheduler(50, 5.0, denoising_strength=0.6).sigmas[0])
PATTERNS = ("none", "all", "alternating", "random", "one")
NAN_BITS = 0x7FC00000                                 # a quiet NaN; the payload below it numbers the element


def _abi():
    from infinicube_amd import native
    return native, native.lib(), torch.cuda.current_stream().cuda_stream


# ---- icv_latent_keep_mask_u8 ---------------------------------------------------------------------------------------------------------------
def run_keep_mask(mask, offset=0):
    """One launch through the C ABI on buffers carved out of a sentinel-filled arena; ``offset``: the mask's byte offset."""
    native, lib, st = _abi()
    n, h, w = mask.shape
    t = (n - 1) // 4 + 1
    ar = Arena(nbytes=1 << 17)
    bm = ar.carve(np.uint8, mask.size, offset, mask)
    bk = ar.carve(np.uint8, t * (h // 8) * (w // 8), 1 if offset else 0)
    before = ar.snapshot()
    native.check(lib.icv_latent_keep_mask_u8(bm.ptr, bk.ptr, n, h, w, st), "icv_latent_keep_mask_u8")
    ar.check(before, [bk])
    return bk.read((t, h // 8, w // 8))


@pytest.mark.parametrize("shape", GPU_SHAPES, ids=["x".join(map(str, s)) for s in GPU_SHAPES])
def test_keep_mask_matches_twin(hip_ops, shape):
    n, h, w = shape
    g = np.random.default_rng(n * 1000 + h)
    for k, density in enumerate((0.0, 1.0, 0.5, 1.0 / 4096)):
        mask = (g.random(shape) < density).astype(np.uint8) * g.integers(1, 256, shape, dtype=np.uint8)
        want = keep_mask_twin(torch.from_numpy(mask)).numpy()
        for offset in (0, 1, 4):                                      # 8-byte loads, bytes, bytes
            assert np.array_equal(run_keep_mask(mask, offset), want), (shape, density, offset)
        assert {0.0: want.all(), 1.0: not want.any()}.get(density, True)
    for cell in {(0, 0, 0), ((n - 1) // 4, h // 8 - 1, w // 8 - 1), ((n - 1) // 4, 0, w // 8 - 1), (min(1, (n - 1) // 4), h // 8 - 1, 0)}:
        for i, mask in enumerate(corner_masks(n, h, w, cell)):
            want = np.ones(((n - 1) // 4 + 1, h // 8, w // 8), dtype=np.uint8)
            want[cell] = 0
            assert np.array_equal(run_keep_mask(mask, i % 2), want), (shape, cell, i)
    # the operator, on plain tensors
    mask = torch.from_numpy((g.random(shape) < 0.01).astype(np.uint8)).to(DEV)
    keep = torch.full(((n - 1) // 4 + 1, h // 8, w // 8), 7, dtype=torch.uint8, device=DEV)
    hip_ops.latent_keep_mask(mask, keep)
    assert torch.equal(keep.cpu(), keep_mask_twin(mask.cpu()))


# ---- icv_pin_known_f32 ---------------------------------------------------------------------------------------------------------------------
def keep_pattern(name, cells, seed):
    k = np.zeros(cells, dtype=np.uint8)
    if name == "all":
        k[:] = 1
    elif name == "alternating":
        k[::2] = 1
    elif name == "random":
        g = np.random.default_rng(seed)
        k[:] = (g.random(cells) < 0.5) * g.integers(1, 256, cells)    # any non-zero byte keeps
    elif name == "one":
        k[(seed * 7) % cells] = 255
    return k


def nan_pattern(n, salt):
    return (np.arange(n, dtype=np.int64) * 2654435761 + salt) % (1 << 22) + NAN_BITS


def run_pin(hip_ops, C, cells, offs, keep_off, pattern, sigma_next, sigma_cur, rounding, state, state_offs=None):
    """One launch on buffers carved out of a sentinel-filled arena.  ``offs``: float offsets of (latent, x0, noise) from a 256-byte
    boundary, ``keep_off``: keep's byte offset; ``state``: with x_hat and m_new (at ``state_offs``, default the latent's offset).
    Outputs start as NaNs whose payload numbers the element.  Compared as int32."""
    n = C * cells
    g = torch.Generator().manual_seed(1000 * cells + C)
    x0, noise = torch.randn(n, generator=g), torch.randn(n, generator=g)
    if rounding:
        x0, noise = x0.to(torch.bfloat16).float(), noise.to(torch.bfloat16).float()
    keep = keep_pattern(pattern, cells, cells + C + keep_off)
    ar = Arena(nbytes=1 << 19)
    bl, bx, bn = (ar.carve(np.float32, n, o) for o in offs)
    bk = ar.carve(np.uint8, cells, keep_off, keep)
    so = state_offs or (offs[0], offs[0])
    bh, bm = (ar.carve(np.float32, n, so[0]), ar.carve(np.float32, n, so[1])) if state else (None, None)
    outs = [b for b in (bl, bh, bm) if b is not None]
    start = {}
    for salt, b in enumerate(outs):
        start[b] = torch.from_numpy(nan_pattern(n, salt * 977).astype(np.int32))
        b.tensor((n,)).view(torch.int32).copy_(start[b])
    bx.tensor((n,)).copy_(x0)
    bn.tensor((n,)).copy_(noise)
    bx.is_output = bn.is_output = False                               # carved without data, but inputs: check() must see them unchanged
    assert bk.ptr % 4 == keep_off and bl.ptr % 16 == 4 * offs[0]
    want = {b: start[b].clone().view(torch.float32).view(C, cells) for b in outs}
    pin_twin(want[bl], x0.view(C, cells), noise.view(C, cells), torch.from_numpy(keep), sigma_next, want.get(bh), sigma_cur, want.get(bm), rounding)
    before = ar.snapshot()
    keep_t = ar.flat[bk.start:bk.end]
    hip_ops.pin_known(bl.tensor((C, cells)), bx.tensor((C, cells)), bn.tensor((C, cells)), keep_t, sigma_next,
                      x_hat=bh.tensor((C, cells)) if state else None, sigma_cur=sigma_cur, m_new=bm.tensor((C, cells)) if state else None,
                      round_bf16=rounding)
    ar.check(before, outs)                                            # guard bands, x0, noise, keep and everything else unchanged
    for name, b in (("latent", bl), ("x_hat", bh), ("m_new", bm)):
        if b is None:
            continue
        got, exp = b.tensor((n,)).view(torch.int32).cpu(), want[b].reshape(-1).view(torch.int32)
        assert torch.equal(got, exp), (f"{name}: C={C} cells={cells} offsets={offs} keep+{keep_off} {pattern} sigma={sigma_next}/{sigma_cur} "
                                       f"round_bf16={rounding}: {int((got != exp).sum())} of {n} differ, first at {int((got != exp).nonzero()[0])}")
        unkept = torch.from_numpy(np.repeat((keep == 0)[None], C, 0).reshape(-1))
        assert torch.equal(got[unkept], start[b][unkept]), f"{name}: an element of a cell that is not kept was written"
    return bl.tensor((n,)).cpu()


@pytest.mark.parametrize("state", [False, True], ids=["latent-only", "with-x_hat-and-m_new"])
@pytest.mark.parametrize("offs", OFFSETS, ids=["".join(map(str, o)) for o in OFFSETS])
def test_pin_matches_twin(hip_ops, offs, state):
    """Channel counts x sizes x keep patterns x keep's byte offset x rounding mode in full for every pointer-offset class; the sigma
    pair cycles (every sigma meets every size, pattern and offset; the full sigma product runs in the next test)."""
    s = sum(offs) + state
    for C in (1, 16):
        for cells in CELLS:
            for pattern in PATTERNS:
                s += 1                                                # 40 values per case: every (keep offset, rounding) meets every sigma
                for keep_off in (0, 1, 2, 3):
                    for rounding in (False, True):
                        i = s + keep_off + 3 * rounding
                        so = ((offs[0] + 1) % 4, offs[0]) if (state and C == 1 and cells % 2) else None      # a state tensor off the others' offset
                        run_pin(hip_ops, C, cells, offs, keep_off, pattern, SIGMAS[i % 4], SIGMAS[(i // 4 + 1) % 4], rounding, state, so)


def test_pin_every_sigma_and_keep_offset_on_the_vector_path(hip_ops):
    """The full product the cycling above only samples, at the one size class where it matters: whole channels of vectors."""
    for keep_off, sigma, rounding, state in itertools.product((0, 1, 2, 3), SIGMAS, (False, True), (False, True)):
        for offs in ((0, 0, 0), (3, 3, 3)):
            run_pin(hip_ops, 16, 256, offs, keep_off, "random", sigma, 0.5, rounding, state)


@pytest.mark.parametrize("rounding", [False, True])
def test_all_kept_is_add_noise_bit_for_bit(hip_ops, rounding):
    for cells, offs in ((4 * 260 + 3, (0, 0, 0)), (256, (1, 1, 1)), (256, (0, 1, 2)), (4 * 260, (2, 2, 2))):
        for sigma in SIGMAS:
            got = run_pin(hip_ops, 16, cells, offs, 0, "all", sigma, 0.0, rounding, False)
            n = 16 * cells
            g = torch.Generator().manual_seed(1000 * cells + 16)
            x0, noise = torch.randn(n, generator=g), torch.randn(n, generator=g)
            if rounding:
                x0, noise = x0.to(torch.bfloat16).float(), noise.to(torch.bfloat16).float()
            out = torch.empty(n, device=DEV)
            hip_ops.add_noise(x0.to(DEV), noise.to(DEV), out, sigma, round_bf16=rounding)
            assert torch.equal(got.view(torch.int32), out.cpu().view(torch.int32)), (cells, offs, sigma)


def test_contract(hip_ops):
    native, lib, st = _abi()
    ar = Arena(nbytes=1 << 14)
    bl, bx, bn, bh = (ar.carve(np.float32, 64, 0) for _ in range(4))
    bk = ar.carve(np.uint8, 64, 0, np.ones(64, dtype=np.uint8))
    bmask = ar.carve(np.uint8, 5 * 16 * 16, 0, np.zeros(5 * 16 * 16, dtype=np.uint8))
    for b in (bl, bx, bn, bh):
        b.tensor((64,)).copy_(torch.ones(64))
    before = ar.snapshot()
    # zero sizes: nothing is launched, nothing is written - through the C ABI (null pointers included) and through the operator
    assert lib.icv_pin_known_f32(bl.ptr, None, None, bx.ptr, bn.ptr, bk.ptr, 0, 64, 0.5, 0.5, 0, st) == 0
    assert lib.icv_pin_known_f32(bl.ptr, None, None, bx.ptr, bn.ptr, bk.ptr, 4, 0, 0.5, 0.5, 0, st) == 0
    assert lib.icv_pin_known_f32(None, None, None, None, None, None, 0, 0, 0.5, 0.5, 0, st) == 0
    assert lib.icv_latent_keep_mask_u8(None, None, 5, 16, 0, st) == 0
    e = torch.empty((0, 8), device=DEV)
    hip_ops.pin_known(e, e, e, torch.ones(8, dtype=torch.uint8, device=DEV), 0.5)
    e = torch.empty((4, 0), device=DEV)
    hip_ops.pin_known(e, e, e, torch.ones(0, dtype=torch.uint8, device=DEV), 0.5)
    # bad arguments: an icv_last_error message and no launch
    for args, msg in (((bl.ptr, None, None, bx.ptr, bn.ptr, bk.ptr, -1, 16), b"negative size"), ((bl.ptr, None, None, bx.ptr, bn.ptr, bk.ptr, 4, -16), b"negative size"),
                      ((None, None, None, bx.ptr, bn.ptr, bk.ptr, 4, 16), b"null argument"), ((bl.ptr, None, None, None, bn.ptr, bk.ptr, 4, 16), b"null argument"),
                      ((bl.ptr, None, None, bx.ptr, None, bk.ptr, 4, 16), b"null argument"), ((bl.ptr, None, None, bx.ptr, bn.ptr, None, 4, 16), b"null argument"),
                      ((bl.ptr + 2, None, None, bx.ptr, bn.ptr, bk.ptr, 2, 16), b"4-byte aligned"), ((bl.ptr, bh.ptr + 1, None, bx.ptr, bn.ptr, bk.ptr, 2, 16), b"4-byte aligned"),
                      ((bl.ptr, None, bh.ptr + 3, bx.ptr, bn.ptr, bk.ptr, 2, 16), b"4-byte aligned"), ((bl.ptr, None, None, bx.ptr + 2, bn.ptr, bk.ptr, 2, 16), b"4-byte aligned"),
                      ((bl.ptr, None, None, bx.ptr, bn.ptr + 1, bk.ptr, 2, 16), b"4-byte aligned")):
        assert lib.icv_pin_known_f32(*args, 0.5, 0.5, 0, st) != 0 and msg in lib.icv_last_error(), args
    for args, msg in (((bmask.ptr, bk.ptr, 4, 16, 16), b"need 4k + 1"), ((bmask.ptr, bk.ptr, 0, 16, 16), b"need 4k + 1"), ((bmask.ptr, bk.ptr, 5, 8, 16), b"multiples of 16"),
                      ((bmask.ptr, bk.ptr, 5, 16, 24), b"multiples of 16"), ((None, bk.ptr, 5, 16, 16), b"null argument"), ((bmask.ptr, None, 5, 16, 16), b"null argument")):
        assert lib.icv_latent_keep_mask_u8(*args, st) != 0 and msg in lib.icv_last_error(), args
    ar.check(before, [])
    # the operators' own checks
    f, k = torch.zeros((2, 8), device=DEV), torch.ones(8, dtype=torch.uint8, device=DEV)
    with pytest.raises(TypeError, match="pin_known.latent"):
        hip_ops.pin_known(f.to(torch.bfloat16), f, f, k, 0.5)
    with pytest.raises(TypeError, match="pin_known.keep"):
        hip_ops.pin_known(f, f, f, k.bool(), 0.5)
    with pytest.raises(TypeError, match="pin_known.m_new"):
        hip_ops.pin_known(f, f, f, k, 0.5, m_new=f.double())
    with pytest.raises(ValueError, match="must have one shape"):
        hip_ops.pin_known(f, f[:1], f, k, 0.5)
    with pytest.raises(ValueError, match="must have one shape"):
        hip_ops.pin_known(f, f, f, k, 0.5, x_hat=f[:, :4])
    with pytest.raises(ValueError, match="keep must be"):
        hip_ops.pin_known(f, f, f, k[:4], 0.5)
    with pytest.raises(ValueError, match="innermost dimension must be contiguous"):
        hip_ops.pin_known(f[:, ::2], f[:, ::2], f[:, ::2], k[::2], 0.5)
    m = torch.zeros((5, 16, 16), dtype=torch.uint8, device=DEV)
    kk = torch.zeros((2, 2, 2), dtype=torch.uint8, device=DEV)
    with pytest.raises(TypeError, match="latent_keep_mask.mask"):
        hip_ops.latent_keep_mask(m.float(), kk)
    with pytest.raises(TypeError, match="latent_keep_mask.keep"):
        hip_ops.latent_keep_mask(m, kk.bool())
    with pytest.raises(ValueError, match=r"mask must be \[4k \+ 1, H, W\]"):
        hip_ops.latent_keep_mask(m[:4], kk)
    with pytest.raises(ValueError, match=r"mask must be \[4k \+ 1, H, W\]"):
        hip_ops.latent_keep_mask(m[:, :8], kk)
    with pytest.raises(ValueError, match="keep must be"):
        hip_ops.latent_keep_mask(m, kk[:1])


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------------------
class Hand:
    """Hooks for test_v2v_cpu.drive_by_hand: ``noise_op`` keeps x0 and a copy of the noise before the start latent overwrites it;
    ``setup`` wraps the engine's denoise so that it either is given the plan (``pins="engine"``) or runs step by step with the
    test's own pin - the torch twin, on the device - after every step (``pins="test"``)."""

    def __init__(self, ops, mask, pins, then=None):
        self.ops, self.pins, self.then, self.m = ops, pins, then, None
        self.keep = keep_mask_twin(torch.from_numpy(mask)).to(DEV)

    def noise_op(self, x0, noise, out, sigma, rounding):
        self.x0, self.noise = x0, noise.clone()
        self.ops.add_noise(x0, noise, out, sigma, round_bf16=rounding)

    def setup(self, m):
        self.m, plain = m, m.denoise
        if self.then is not None:
            self.then(m)

        def denoise(lat, cc, cu, bt, sch, cfg_scale, **kw):
            if self.pins == "engine":
                return plain(lat, cc, cu, bt, sch, cfg_scale, known=inpaint.KnownPlan(self.x0, self.noise, self.keep), **kw)
            n = len(sch.sigmas)
            for i in range(n):
                plain(lat, cc, cu, bt, sch, cfg_scale, steps=range(i, i + 1), **kw)
                pin_twin(lat, self.x0, self.noise, self.keep, sch.sigmas[i + 1] if i + 1 < n else 0.0, round_bf16=kw.get("round_bf16", False))
            return lat

        m.denoise = denoise


@pytest.mark.parametrize("rounding", [False, True])
def test_hip_pipeline_equals_engine_driven_by_hand(hip_ops, rounding, monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    p = _pipe(hip_ops)
    p.reference_rounding = rounding
    clip, kw, mask = pil(make_clip(SHORT, 1)), _call_kw(num_inference_steps=3), half_mask(SHORT)
    base = p(**kw, input_video=clip, denoising_strength=0.6)
    assert p.inpaint_record is None
    # an all-regenerate mask: the bits of the call without one
    assert torch.equal(p(**kw, input_video=clip, denoising_strength=0.6, input_mask=np.ones_like(mask)), base)
    assert p.inpaint_record == dict(cells=288, kept_cells=0, kept_fraction=0.0)
    got = p(**kw, input_video=clip, denoising_strength=0.6, input_mask=mask)
    assert p.inpaint_record == dict(cells=288, kept_cells=216, kept_fraction=0.75)
    hand = Hand(hip_ops, mask, "test")
    want = drive_by_hand(p, hip_ops, kw, clip, 0.6, noise_op=hand.noise_op, setup=hand.setup)
    torch.cuda.synchronize()
    assert torch.equal(got, want), f"max |d| {float((got - want).abs().max())}"
    k = (hand.keep != 0).expand_as(got)
    assert torch.equal(got[k], hand.x0[k]) and torch.isfinite(got).all()                 # the kept cells ARE the encoded clip
    assert not torch.equal(got[~k], base[~k]) and not torch.equal(base[k], hand.x0[k])


@pytest.mark.parametrize("mode", ["pair", "pair-no-stem", "native", "graphs", "dual-stream", "fp8-pair", "reference-rounding"])
def test_driver_modes_match_sequential_loop(hip_ops, mode, monkeypatch):
    """test_v2v_gpu's driver modes, each from the same start latent with a half-kept mask and the engine's own pins."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    p = _pipe(hip_ops)
    p.reference_rounding = mode == "reference-rounding"
    clip, kw, mask = pil(make_clip(SHORT, 1)), _call_kw(num_inference_steps=4), half_mask(SHORT)
    ekw = FP8 if mode.startswith("fp8") else None

    def run(then, prep):
        hand = Hand(hip_ops, mask, "engine", then)
        return drive_by_hand(p, hip_ops, kw, clip, 0.6, engine_kw=ekw, noise_op=hand.noise_op, setup=hand.setup, prep=prep), hand

    ref, hand = run(_sequential, dict(graphs=False))
    k = (hand.keep != 0).expand_as(ref)
    assert torch.equal(ref[k], hand.x0[k])
    prep, then = dict(graphs=False), None
    if mode == "pair-no-stem":
        then = lambda m: setattr(m, "share_stem", False)                         # noqa: E731
    elif mode == "native":
        then = lambda m: setattr(m, "native_forward", True)                      # noqa: E731
    elif mode == "graphs":
        prep = dict(graphs=True)
    elif mode == "dual-stream":
        monkeypatch.setenv("ICV_DUAL_STREAM", "1")
    got, hand = run(then, prep)
    torch.cuda.synchronize()
    m = hand.m
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


@pytest.mark.parametrize("name", ["unipc", "cfg-zero", "teacache", "two-sliding-windows"])
def test_compositions_match_sequential_loop(hip_ops, name, monkeypatch):
    """The mask with one other feature through the HIP pipeline: the kept cells equal the encoded clip, and the pipeline's default
    driver mode gives the bits of the sequential loop."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setitem(teacache.COEFFICIENTS, "test-linear", LINEAR)
    p = _pipe(hip_ops)
    got, kw = check_composition(p, name, None, run_plain=False)
    assert p._get_engine().cfg_batch
    p._get_engine().cfg_batch = False                                 # window engines take the setting over at every call
    seq = p(**kw).cpu()
    assert torch.equal(got, seq), f"{name}: max |d| {float((got - seq).abs().max())}"


def inpaint_reference(o, keep, num_steps, strength, shift=5.0, cfg_scale=5.0):
    """test_v2v_cpu.v2v_reference with the inpainting rule: after every step the kept cells go back to (1 - s) x0 + s noise at the
    next sigma (0 after the last step), in fp32 torch."""
    sig = strength_sigmas(num_steps, shift, strength)
    buf = R.buffer_embed(o["bsd"], o["bl"], torch.float32)
    x0, noise = o["x0"].float(), o["noise"].float()
    k = (keep != 0).expand_as(x0)
    x = (1.0 - float(sig[0])) * x0 + float(sig[0]) * noise
    for i in range(num_steps):
        ts = float(sig[i]) * 1000.0
        v_c = R.dit_forward(o["sd"], CFG, x, o["c1"], ts, buf, torch.float32)
        v_u = R.dit_forward(o["sd"], CFG, x, o["c2"], ts, buf, torch.float32)
        nxt = float(sig[i + 1]) if i + 1 < num_steps else 0.0
        x = x + (v_u + cfg_scale * (v_c - v_u)) * (nxt - float(sig[i]))
        x = torch.where(k, (1.0 - nxt) * x0 + nxt * noise, x)
    return x


def test_hip_pipeline_matches_restated_inpainting_loop(hip_ops, monkeypatch):
    """>= 40 dB, test_v2v_gpu's bar for this loop (the pin adds no rounding of its own); the kept cells exactly."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    p = _pipe(hip_ops)
    clip, kw, mask = pil(make_clip(SHORT, 1)), _call_kw(num_inference_steps=3), half_mask(SHORT)
    got = p(**kw, input_video=clip, denoising_strength=0.6, input_mask=mask)
    o = oracle_inputs(p, kw, clip, dev=DEV)
    keep = keep_mask_twin(torch.from_numpy(mask)).to(DEV)
    ref = inpaint_reference(o, keep, 3, 0.6)
    db = R.psnr(got.cpu(), ref.cpu())
    print(f"HIP inpainting pipeline (strength 0.6, 3 steps, 216 of 288 cells kept) vs the loop restated in fp32 on the GPU: {db:.1f} dB")
    assert db >= 40.0, f"{db:.1f} dB"
    k = (keep != 0).expand_as(got)
    assert torch.equal(got[k], ref[k]) and torch.equal(got[k], o["x0"][k])
    plain = inpaint_reference(o, torch.zeros_like(keep), 3, 0.6)
    assert R.psnr(got.cpu(), plain.cpu()) < db - 10.0, "the result must hold the kept cells, not regenerate them"


def test_chain_on_the_gpu(hip_ops, monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    vae = RecordingVAE()
    check_chain(_pipe(hip_ops, vae=vae), vae)
