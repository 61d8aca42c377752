"""The lean body of the 16x16x32 attention tile (option attn_tile16_lean = 1; csrc/attn_common.h: attc::tile16, LEAN) against the
first body (attn_tile16_lean = 0): the same arithmetic in the same order, so every output and every carried (acc, m, l) state must be
EQUAL bit for bit - torch.equal, no tolerance.  Both bodies run in this process on the same operands.

Shapes are the smallest that reach each path of the kernels that share the tile: a single tile, one full trip of the two-tile loop, an
odd tile count (the second tile of a trip skipped), a ragged last tile (the tail mask in both tiles of a trip), a key axis that goes
round the four-stage ring more than twice (the lean body's fragment addresses follow the ring), the lazy-max re-base fired in the
first and in the second 32-key half of a tile, the carried state, a piece boundary that is no multiple of 64, the frame-windowed
launch, and the 4-wave short-key kernel with both epilogues.  Random N(0, 1) bf16 operands, K pre-scaled for unit scale as the DiT
does; 2 heads; Sq = 300 = one full 256-row block and a ragged one with clamped rows."""
import contextlib
import math

import pytest
import torch

import attn_scores as A
from test_kernels_gpu import rnd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H = 2
LN2 = math.log(2.0)
SCALE = 1.0 / math.sqrt(128)
DEFAULTS = {"attn_tile16_lean": -1, "attn_mfma": -1, "attn7_short": -1, "attn7_plain": 0, "attn_unit_scale": 1, "attn_defer_max_log2": 8}


@contextlib.contextmanager
def options(hip_ops, **kv):
    try:
        for k, v in kv.items():
            assert hip_ops.lib.icv_set_option(k.encode(), int(v)) == 0
        yield
    finally:
        for k in kv:
            hip_ops.lib.icv_set_option(k.encode(), DEFAULTS[k])


_RANDOM = {}


def random_qkv():
    """q [300, 256], k, v [577, 256] bf16 on the GPU (made once, never modified; the cases take slices); k carries scale * log2 e."""
    if not _RANDOM:
        _RANDOM["q"] = rnd((300, H * 128), 900).to(torch.bfloat16).to(DEV)
        _RANDOM["k"] = (rnd((64 * 9 + 1, H * 128), 901) * (SCALE * math.log2(math.e))).to(torch.bfloat16).to(DEV)
        _RANDOM["v"] = rnd((64 * 9 + 1, H * 128), 902).to(torch.bfloat16).to(DEV)
    return _RANDOM["q"], _RANDOM["k"], _RANDOM["v"]


def both(hip_ops, launch, **opts):
    """launch() -> tuple of tensors, under attn_tile16_lean = 0 and = 1 (attn_mfma = 16): [(first body's), (lean body's)]."""
    out = []
    for lean in (0, 1):
        with options(hip_ops, attn_mfma=16, attn_tile16_lean=lean, **opts):
            out.append(launch())
    torch.cuda.synchronize()
    return out


def assert_equal(pair, what):
    old, new = pair
    assert len(old) == len(new)
    for i, (a, b) in enumerate(zip(old, new)):
        assert bool(torch.isfinite(a.float()).all()), f"{what}: tensor {i} of the first body is not finite"
        if not torch.equal(a, b):
            bad = (a != b).any(-1).nonzero().flatten()
            d = float((a.float() - b.float()).abs().max())
            raise AssertionError(f"{what}: tensor {i} differs between the bodies on {bad.numel()} rows (first {bad[:6].tolist()}), max |d| {d:.3e}")


def plain(hip_ops, q, k, v, scale=LN2):
    def launch():
        o = torch.zeros_like(q)
        hip_ops.attention(q, k, v, o, H, scale)
        return (o,)
    return launch


@pytest.mark.parametrize("plain7", [0, 1])
@pytest.mark.parametrize("Skv", [64, 128, 192, 321, 64 * 9 + 1])
def test_self_attention_one_piece(hip_ops, Skv, plain7):
    """attn7p.hip's one-piece launch (plain7 = 0) and attn7.hip's 8-wave kernel (attn7_plain = 1); attn7_short = 0 keeps these key
    counts off the short-key kernel.  Skv = 577 crosses the four-stage ring more than twice."""
    q, k, v = random_qkv()
    pair = both(hip_ops, plain(hip_ops, q, k[:Skv], v[:Skv]), attn7_short=0, attn7_plain=plain7)
    assert_equal(pair, f"self-attention Skv={Skv} attn7_plain={plain7}")
    if plain7 == 0:      # and the two kernels still agree with each other under the lean body
        with options(hip_ops, attn_mfma=16, attn_tile16_lean=1, attn7_short=0, attn7_plain=1):
            (o7,) = plain(hip_ops, q, k[:Skv], v[:Skv])()
        assert torch.equal(o7, pair[1][0]), f"Skv={Skv}: attn7.hip and attn7p.hip differ under the lean body"


def rebase_case(Sq, Skv):
    """Peaked scores (tests/attn_scores.py, as tests/test_attn_scores_gpu.py builds them): group 0 climbs by 9 log2 units (> the
    defer-max threshold 8) at key 10 of tiles 1 and 4 - the FIRST 32-key half - and at key 45 of tiles 2 and 5 - the SECOND half -;
    group 1 is flat, so the wave-wide re-base runs with alpha = 1 on its rows; group 2 has one dominant key in a second half."""
    g = torch.Generator().manual_seed(77)
    nt = (Skv + 63) // 64
    rise_at = {64 * 1 + 10, 64 * 4 + 10, 64 * 2 + 45, 64 * 5 + 45}
    cur, top = -A.S_MAX + 2, []
    stair = torch.empty((Skv,), dtype=torch.long)
    for j in range(Skv):
        if j in rise_at:
            cur += 9
            top.append(j)
        stair[j] = cur
    noise = torch.randint(1, 3, (Skv,), generator=g)
    noise[torch.tensor([0] + top)] = 0
    flat = -torch.randint(0, 4, (Skv,), generator=g)
    hot = -torch.randint(0, 65, (Skv,), generator=g) + (A.S_MAX - 80)
    hot[64 * 3 + 50] = A.S_MAX
    assert nt >= 6
    return A.realise(torch.stack([stair - noise, flat, hot]), torch.arange(Sq) % 3, H, 78)


@pytest.mark.parametrize("mode", ["unit", "plain", "scaled"])
def test_rebase_in_either_half(hip_ops, mode):
    """unit: the UNIT instantiation (reference baked into the MFMA's C operand, re-based in place); plain: the same inputs with
    attn_unit_scale = 0 (UNIT = false); scaled: random operands at a non-unit scale (UNIT = false, sc != 1) with the defer-max
    threshold at 2^0, so that every half whose partial row sum exceeds 1 re-bases - with N(0, 1) scores that is most of them.
    That the peaked inputs fire the re-base where the docstring of rebase_case says is the argument of tests/test_attn_scores_gpu.py
    (a rise of 9 > thr = 8 log2 units makes P = 2^9 > p_lim in the half that holds the rising key); equality alone cannot show it,
    since two bodies that both skipped it would agree too - test_attn_scores_gpu.py checks the carried m against those rises, and
    it runs the lean body, the default."""
    if mode == "scaled":
        q, k, v = random_qkv()
        k = (k.float() / (SCALE * math.log2(math.e))).to(torch.bfloat16)
        for short in (0, -1):
            pair = both(hip_ops, plain(hip_ops, q, k[:321], v[:321], SCALE), attn7_short=short, attn_defer_max_log2=0)
            assert_equal(pair, f"non-unit scale, attn7_short={short}")
        return
    c = rebase_case(300, 64 * 6 + 1)
    q, k, v = c["q"].to(DEV), c["k"].to(DEV), c["v"].to(DEV)
    for plain7 in (0, 1):
        pair = both(hip_ops, plain(hip_ops, q, k, v), attn7_short=0, attn7_plain=plain7, attn_unit_scale=1 if mode == "unit" else 0)
        assert_equal(pair, f"re-base {mode} attn7_plain={plain7}")
    assert_equal(both(hip_ops, plain(hip_ops, q, k, v), attn_unit_scale=1 if mode == "unit" else 0), f"re-base {mode}, short-key kernel")


def test_carried_state_128_plus_193(hip_ops):
    q, k, v = random_qkv()
    Sq = q.shape[0]

    def launch():
        acc = torch.zeros((Sq, H * 128), device=DEV)
        ml = torch.zeros((Sq, H, 2), device=DEV)
        o = torch.zeros_like(q)
        hip_ops.attention_chunk(q, k[:128], v[:128], o, acc, ml, H, LN2, first=True, last=False)
        acc1, ml1 = acc.clone(), ml.clone()
        hip_ops.attention_chunk(q, k[128:321], v[128:321], o, acc, ml, H, LN2, first=False, last=True)
        return o, acc1, ml1

    for short in (0, -1):       # the long-key kernel, and the chunks as the default routes them
        assert_equal(both(hip_ops, launch, attn7_short=short), f"chunks 128 + 193, attn7_short={short}")


def test_pieces_100_plus_221(hip_ops):
    q, k, v = random_qkv()

    def launch():
        o = torch.zeros_like(q)
        hip_ops.attention_pieces(q, [(k[:100], v[:100], -1, 0), (k[100:321], v[100:321], -1, 0)], o, H, LN2)
        return (o,)

    assert_equal(both(hip_ops, launch), "pieces 100 | 221")


def test_pieces_odd_tile_count_first(hip_ops):
    """150 rows = 3 tiles, then 171 and 256 rows: the ring position of the next piece is rounded up to an even stage behind an odd
    piece, and the lean body's addresses change ring half once per interval, whatever the piece did with the interval's second tile."""
    q, k, v = random_qkv()
    bounds = [0, 150, 321, 577]

    def launch():
        o = torch.zeros_like(q)
        hip_ops.attention_pieces(q, [(k[a:b], v[a:b], -1, 0) for a, b in zip(bounds[:-1], bounds[1:])], o, H, LN2)
        return (o,)

    pair = both(hip_ops, launch)
    assert_equal(pair, "pieces 150 | 171 | 256")
    with options(hip_ops, attn_mfma=16, attn_tile16_lean=1, attn7_short=0):      # the same keys as one piece: the same tiles but for the cuts
        (one,) = plain(hip_ops, q, k, v)()
    d = (one.float() - pair[1][0].float()).abs().max()
    assert float(d) <= 2.0 ** -5, f"three pieces against one piece: max |d| {float(d):.3e}"


def test_frame_window(hip_ops):
    """5 frames of 70 rows, window 1, sink 1 (the grid of tests/test_attn_mfma16_gpu.py): frame 3 reads two pieces."""
    _, k, v = random_qkv()
    frames, F = 5, 70
    q = rnd((frames * F, H * 128), 903).to(torch.bfloat16).to(DEV)

    def launch():
        o = torch.zeros_like(q)
        hip_ops.attention_framewin(q, k[:frames * F], v[:frames * F], o, H, LN2, frames, F, 1, 1)
        return (o,)

    assert_equal(both(hip_ops, launch), "frame window")


@pytest.mark.parametrize("Skv", [512, 257])
def test_short_key_kernel(hip_ops, Skv):
    """attn7.hip's 4-wave kernel on its two-stage ring (cross-attention), with the store and the add-into-output epilogues."""
    q, k, v = random_qkv()
    q = q[:200]
    prev = A.v_values(200, H, 99).to(DEV)

    def launch():
        o = torch.zeros_like(q)
        hip_ops.attention(q, k[:Skv], v[:Skv], o, H, LN2)
        o2 = prev.clone()
        hip_ops.attention_add(q, k[:Skv], v[:Skv], o2, H, LN2)
        return o, o2

    pair = both(hip_ops, launch)
    assert_equal(pair, f"short-key kernel Skv={Skv}")
    assert not torch.equal(pair[0][1], prev)


def test_an_unknown_body_is_an_error(hip_ops):
    from infinicube_amd import native
    q, k, v = random_qkv()
    o = torch.empty_like(q)
    for short in (0, -1):
        with options(hip_ops, attn_mfma=16, attn_tile16_lean=2, attn7_short=short):
            with pytest.raises(native.NativeError):
                hip_ops.attention(q, k[:128], v[:128], o, H, LN2)
