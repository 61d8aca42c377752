"""The slim key loop of csrc/attn7p.hip (option attn7p_slim = 1: steady intervals without the loop-control tests, their DMA requests
from running tile pointers with one M0 write per K or V pair) against the one loop (attn7p_slim = 0): the same tiles and the same
requests in the same order, so every output and every carried (acc, m, l) state must be EQUAL bit for bit - torch.equal, no
tolerance.  Both loops run in this process on the same operands, under attn_mfma = 16 and attn_tile16_lean = 1 (what the slim loop
is a loop around) and attn7_short = 0, attn7_plain = 0 (so that every key count here goes to attn7p.hip).

A steady interval needs six full tiles ahead of it in its piece, so the key counts are chosen around that: 64 (one tile), 128 (one
interval), 192 (odd tile count), 256 (two intervals) and 449 (seven full tiles and a ragged one: one steady interval) - the issue's
list - and 1 000 and 1 088 keys: five and six steady intervals, the four-stage ring wrapped several times, with an odd ragged tail
and with an even full one.  d = 128; heads 1 and 3; Sq = 32 (one wave's rows, seven waves clamped) and 300 (two work-groups per head,
the second ragged).  Unit scale (K carries scale * log2 e, as the DiT passes it) and a generic scale.  Chunked launches carry the
state through steady intervals in the first, a middle and the last chunk; pieces launches cross piece boundaries with the ring at
either half and steady intervals on either side.  Flags are < 0 or were satisfied before the launch: no work-group ever waits."""
import contextlib
import math

import pytest
import torch

from test_kernels_gpu import rnd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LN2 = math.log(2.0)
SCALE = 1.0 / math.sqrt(128)
DEFAULTS = {"attn7p_slim": -1, "attn_tile16_lean": -1, "attn_mfma": -1, "attn7_short": -1, "attn7_plain": 0}
KEYS_MAX = 1088


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


def random_qkv(heads, unit):
    """q [300, heads * 128], k, v [1088, heads * 128] bf16 on the GPU and the scale to pass (made once per (heads, unit), never
    modified; the cases take row slices).  unit: k carries scale * log2 e and the launch gets ln 2."""
    if (heads, unit) not in _RANDOM:
        q = rnd((300, heads * 128), 910 + heads).to(torch.bfloat16).to(DEV)
        k = rnd((KEYS_MAX, heads * 128), 920 + heads)
        v = rnd((KEYS_MAX, heads * 128), 930 + heads).to(torch.bfloat16).to(DEV)
        k = (k * (SCALE * math.log2(math.e)) if unit else k).to(torch.bfloat16).to(DEV)
        _RANDOM[(heads, unit)] = (q, k, v, LN2 if unit else SCALE)
    return _RANDOM[(heads, unit)]


def both(hip_ops, launch):
    """launch() -> tuple of tensors, under attn7p_slim = 0 and = 1: [(the one loop's), (the slim loop's)]."""
    out = []
    for slim in (0, 1):
        with options(hip_ops, attn_mfma=16, attn_tile16_lean=1, attn7_short=0, attn7_plain=0, attn7p_slim=slim):
            out.append(launch())
    torch.cuda.synchronize()
    return out


def assert_equal(pair, what):
    old, new = pair
    assert len(old) == len(new)
    for i, (a, b) in enumerate(zip(old, new)):
        assert bool(torch.isfinite(a.float()).all()), f"{what}: tensor {i} of the one loop is not finite"
        if not torch.equal(a, b):
            bad = (a != b).flatten(1).any(-1).nonzero().flatten()
            d = float((a.float() - b.float()).abs().max())
            raise AssertionError(f"{what}: tensor {i} differs between the loops on {bad.numel()} rows (first {bad[:6].tolist()}), max |d| {d:.3e}")


@pytest.mark.parametrize("unit", [True, False], ids=["unit", "scaled"])
@pytest.mark.parametrize("heads,Sq", [(1, 32), (1, 300), (3, 32), (3, 300)])
@pytest.mark.parametrize("keys", [64, 128, 192, 256, 449, 1000, 1088])
def test_one_piece(hip_ops, keys, heads, Sq, unit):
    q, k, v, scale = random_qkv(heads, unit)

    def launch():
        o = torch.zeros_like(q[:Sq])
        hip_ops.attention(q[:Sq], k[:keys], v[:keys], o, heads, scale)
        return (o,)

    pair = both(hip_ops, launch)
    assert_equal(pair, f"keys={keys} heads={heads} Sq={Sq} unit={unit}")
    assert bool((pair[1][0] != 0).any())


@pytest.mark.parametrize("unit", [True, False], ids=["unit", "scaled"])
@pytest.mark.parametrize("heads,Sq", [(1, 300), (3, 32)])
def test_chunks_carry_the_state(hip_ops, heads, Sq, unit):
    """448 | 385 | 255 keys: the first chunk (empty state in, state out) and the middle one (state in and out; its last tile is ragged)
    have a steady interval each, the last one (state in, output out) has none; the state behind every chunk is compared."""
    q, k, v, scale = random_qkv(heads, unit)
    q = q[:Sq]
    cuts = [0, 448, 833, 1088]

    def launch():
        acc = torch.zeros((Sq, heads * 128), device=DEV)
        ml = torch.zeros((Sq, heads, 2), device=DEV)
        o = torch.zeros_like(q)
        states = []
        for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            hip_ops.attention_chunk(q, k[a:b], v[a:b], o, acc, ml, heads, scale, first=i == 0, last=i == 2)
            if i < 2:
                states += [acc.clone(), ml.clone()]
        return (o, *states)

    assert_equal(both(hip_ops, launch), f"chunks 448 | 385 | 255, heads={heads} Sq={Sq} unit={unit}")


@pytest.mark.parametrize("flagged", [False, True], ids=["no_flags", "flags_satisfied"])
@pytest.mark.parametrize("rows", [(192, 65, 640), (64, 128), (448, 449), (128, 512)], ids=lambda r: "_".join(map(str, r)))
def test_pieces(hip_ops, rows, flagged):
    """(192, 65, 640): an odd piece, a ragged two-tile piece, then three steady intervals that start with the ring at stage 2 (mod 4);
    (64, 128): the issue's two short pieces, no steady interval; (448, 449): steady intervals on both sides of a boundary the ring runs
    through; (128, 512): the second piece's steady interval starts at stage 2.  flags_satisfied: every piece behind the first names a
    flag whose value was reached before the launch (one of them exactly, one with room), so the kernel polls and never waits."""
    heads, Sq = 3, 300
    q, k, v, scale = random_qkv(heads, True)
    cuts = [0]
    for r in rows:
        cuts.append(cuts[-1] + r)
    flags = torch.tensor([5, 7, 0, 0], dtype=torch.int32, device=DEV)
    err = torch.zeros((1,), dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    pieces = []
    for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        flag, value = (-1, 0) if (i == 0 or not flagged) else (i - 1, 5)
        pieces.append((k[a:b], v[a:b], flag, value))

    def launch():
        o = torch.zeros_like(q)
        hip_ops.attention_pieces(q, pieces, o, heads, scale, flags=flags, err=err, timeout_us=2_000_000)
        return (o,)

    assert_equal(both(hip_ops, launch), f"pieces {rows} flagged={flagged}")
    assert int(err.item()) == 0, "a piece whose flag was satisfied before the launch timed out"


def test_an_unknown_loop_is_an_error(hip_ops):
    from infinicube_amd import native
    q, k, v, scale = random_qkv(1, True)
    o = torch.empty_like(q)
    with options(hip_ops, attn_mfma=16, attn_tile16_lean=1, attn7_short=0, attn7p_slim=2):
        with pytest.raises(native.NativeError):
            hip_ops.attention(q, k[:128], v[:128], o, 1, scale)
