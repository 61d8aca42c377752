"""The staggered long-key kernel of csrc/attn7p.hip (option attn7p_stagger = 1: att7p::attn7ps_kernel - the two waves of a SIMD in
opposite phases of the tile, a barrier per 64 keys, one half of the work-group carrying S^T across it) against the slim loop (attn7p_stagger = 0): every
wave executes the same QK^T / softmax / PV sequence with the same arithmetic, so every output and every carried (acc, m, l) state must
be EQUAL bit for bit - torch.equal, no tolerance.  Both run in this process on the same operands, under attn_mfma = 16,
attn_tile16_lean = 1, attn7p_slim = 1 (the launches the option applies to) and attn7_short = 0, attn7_plain = 0 (so that every key
count here goes to attn7p.hip).

Key counts: 64 (one tile: prologue and drain only), 128, 192 (odd tile count), 256, 320 (five full tiles: the first count with a steady
pair of slots), 449 (seven full tiles and a ragged one) and 1 000 / 1 088 keys: the four-stage ring wrapped several times, with an odd
ragged tail and with an even full one.  d = 128; heads 1 and 3; Sq = 32 (one wave's rows, seven waves clamped) and 300 (two
work-groups per head, the second ragged).  Unit scale (K carries scale * log2 e, as the DiT passes it) and a generic scale.  Chunked
launches carry the state through a first, a middle and a last chunk.  Rising scores (K scaled by a ramp along the key axis) make the
lazy-max re-base run in many tiles and in both halves - S^T and the reference in the MFMA's C operand then change while four waves carry
them across a barrier - and that case is also held against a float64 reference at the suite's bar for bf16 attention
(attn_scores.check_suite_bar).  The kernel's compile-time variants are compared too: with and without the s_setprio window
(attn7p_stagger_setprio), and with either half of the work-group as the one that carries S^T across the barrier (attn7p_stagger_swap).  A two-piece launch and a frame-windowed launch do
not take the new kernel: the option must leave them alone."""
import contextlib
import math

import pytest
import torch

import attn_scores as A
from test_kernels_gpu import rnd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LN2 = math.log(2.0)
SCALE = 1.0 / math.sqrt(128)
DEFAULTS = {"attn7p_stagger": -1, "attn7p_stagger_setprio": -1, "attn7p_stagger_swap": -1, "attn7p_slim": -1, "attn_tile16_lean": -1, "attn_mfma": -1, "attn7_short": -1,
            "attn7_plain": 0}
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


def random_qkv(heads, unit, ramp=False):
    """q [300, heads * 128], k, v [1088, heads * 128] bf16 on the GPU and the scale to pass (made once per key, never modified; the
    cases take row slices).  unit: k carries scale * log2 e and the launch gets ln 2.  ramp: queries and keys share a common direction (3 u) and key row j is
    scaled by 2 (j + 1) / 1088, so that a row's maximum keeps rising along the key axis: by about 12 nats per 64-key tile."""
    key = (heads, unit, ramp)
    if key not in _RANDOM:
        q = rnd((300, heads * 128), 910 + heads)
        k = rnd((KEYS_MAX, heads * 128), 920 + heads)
        v = rnd((KEYS_MAX, heads * 128), 930 + heads).to(torch.bfloat16).to(DEV)
        if ramp:
            u = rnd((1, heads * 128), 940 + heads)
            q = q + 3.0 * u
            k = (k + 3.0 * u) * (2.0 * torch.arange(1, KEYS_MAX + 1, dtype=k.dtype) / KEYS_MAX)[:, None]
        k = (k * (SCALE * math.log2(math.e)) if unit else k).to(torch.bfloat16).to(DEV)
        _RANDOM[key] = (q.to(torch.bfloat16).to(DEV), k, v, LN2 if unit else SCALE)
    return _RANDOM[key]


def both(hip_ops, launch, setprio=-1, swap=-1):
    """launch() -> tuple of tensors, under attn7p_stagger = 0 and = 1: [(the slim loop's), (the staggered kernel's)]."""
    out = []
    for stagger in (0, 1):
        with options(hip_ops, attn_mfma=16, attn_tile16_lean=1, attn7_short=0, attn7_plain=0, attn7p_slim=1, attn7p_stagger=stagger,
                     attn7p_stagger_setprio=setprio, attn7p_stagger_swap=swap):
            out.append(launch())
    torch.cuda.synchronize()
    return out


def assert_equal(pair, what):
    old, new = pair
    assert len(old) == len(new)
    for i, (a, b) in enumerate(zip(old, new)):
        assert bool(torch.isfinite(a.float()).all()), f"{what}: tensor {i} of the slim loop is not finite"
        if not torch.equal(a, b):
            bad = (a != b).flatten(1).any(-1).nonzero().flatten()
            d = float((a.float() - b.float()).abs().max())
            raise AssertionError(f"{what}: tensor {i} differs between the kernels on {bad.numel()} rows (first {bad[:6].tolist()}), max |d| {d:.3e}")


@pytest.mark.parametrize("swap", [1, 0], ids=["swap", "no_swap"])
@pytest.mark.parametrize("unit", [True, False], ids=["unit", "scaled"])
@pytest.mark.parametrize("heads,Sq", [(1, 32), (1, 300), (3, 32), (3, 300)])
@pytest.mark.parametrize("keys", [64, 128, 192, 256, 320, 449, 1000, 1088])
def test_one_piece(hip_ops, keys, heads, Sq, unit, swap):
    q, k, v, scale = random_qkv(heads, unit)

    def launch():
        o = torch.zeros_like(q[:Sq])
        hip_ops.attention(q[:Sq], k[:keys], v[:keys], o, heads, scale)
        return (o,)

    pair = both(hip_ops, launch, swap=swap)
    assert_equal(pair, f"keys={keys} heads={heads} Sq={Sq} unit={unit} swap={swap}")
    assert bool((pair[1][0] != 0).any())


@pytest.mark.parametrize("swap", [1, 0], ids=["swap", "no_swap"])
@pytest.mark.parametrize("unit", [True, False], ids=["unit", "scaled"])
@pytest.mark.parametrize("heads,Sq", [(1, 300), (3, 32)])
def test_chunks_carry_the_state(hip_ops, heads, Sq, unit, swap):
    """448 | 385 | 255 keys: the first chunk (empty state in, state out), the middle one (state in and out; its last tile is ragged)
    and the last one (state in, output out); the state behind every chunk is compared."""
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

    assert_equal(both(hip_ops, launch, swap=swap), f"chunks 448 | 385 | 255, heads={heads} Sq={Sq} unit={unit} swap={swap}")


@pytest.mark.parametrize("swap", [1, 0], ids=["swap", "no_swap"])
@pytest.mark.parametrize("setprio", [1, 0], ids=["setprio", "no_setprio"])
@pytest.mark.parametrize("unit", [True, False], ids=["unit", "scaled"])
@pytest.mark.parametrize("keys", [449, 1088])
def test_rising_scores_rebase_across_the_barrier(hip_ops, keys, unit, setprio, swap):
    """Scores that rise along the key axis: a later tile raises the row maximum again and again, in either 32-key half."""
    heads, Sq = 3, 300
    q, k, v, scale = random_qkv(heads, unit, ramp=True)

    def launch():
        o = torch.zeros_like(q[:Sq])
        hip_ops.attention(q[:Sq], k[:keys], v[:keys], o, heads, scale)
        return (o,)

    what = f"rising scores, keys={keys} unit={unit} setprio={setprio} swap={swap}"
    pair = both(hip_ops, launch, setprio, swap)
    assert_equal(pair, what)
    s, _ = A.scores(q[:Sq], k[:keys], heads, sc=scale / LN2)
    # the premise: in most rows the running maximum rises in at least half of the 64-key tiles
    nt = keys // 64
    tile_max = s[..., :nt * 64].reshape(heads, Sq, nt, 64).amax(-1)
    rises = (tile_max[..., 1:] > tile_max.cummax(-1).values[..., :-1]).sum(-1)
    assert float((rises >= nt // 2).double().mean()) > 0.5, f"{what}: the scores do not rise (median {float(rises.double().median())} rises)"
    fails = A.check_suite_bar(pair[1][0], s, A.heads_v(v[:keys], heads), what=what)
    assert not fails, "\n".join(fails)


def test_a_two_piece_launch_is_left_alone(hip_ops):
    heads, Sq = 3, 300
    q, k, v, scale = random_qkv(heads, True)
    pieces = [(k[:448], v[:448], -1, 0), (k[448:897], v[448:897], -1, 0)]

    def launch():
        o = torch.zeros_like(q)
        hip_ops.attention_pieces(q, pieces, o, heads, scale)
        return (o,)

    assert_equal(both(hip_ops, launch), "pieces 448 | 449")


def test_a_one_piece_pieces_launch(hip_ops):
    """One piece without a flag through the pieces entry point: it takes the staggered kernel."""
    heads, Sq = 3, 300
    q, k, v, scale = random_qkv(heads, True)

    def launch():
        o = torch.zeros_like(q)
        hip_ops.attention_pieces(q, [(k[:897], v[:897], -1, 0)], o, heads, scale)
        return (o,)

    assert_equal(both(hip_ops, launch), "one piece of 897 rows")


def test_a_frame_windowed_launch_is_left_alone(hip_ops):
    heads, frames, frame_rows = 3, 5, 200
    q, k, v, scale = random_qkv(heads, True)
    rows = frames * frame_rows
    qq = torch.cat([q, q, q, q])[:rows].contiguous()

    def launch():
        o = torch.zeros_like(qq)
        hip_ops.attention_framewin(qq, k[:rows], v[:rows], o, heads, scale, frames, frame_rows, 1, 1)
        return (o,)

    assert_equal(both(hip_ops, launch), "frame window 1, sink 1")


@pytest.mark.parametrize("option", ["attn7p_stagger", "attn7p_stagger_setprio", "attn7p_stagger_swap"])
def test_an_unknown_value_is_an_error(hip_ops, option):
    from infinicube_amd import native
    q, k, v, scale = random_qkv(1, True)
    o = torch.empty_like(q)
    with options(hip_ops, attn_mfma=16, attn_tile16_lean=1, attn7_short=0, attn7p_slim=1, **{option: 2}):
        with pytest.raises(native.NativeError):
            hip_ops.attention(q, k[:128], v[:128], o, 1, scale)
