"""attn7.hip and attn7p.hip on 16x16x32 MFMAs (option attn_mfma = 16; csrc/attn_common.h: attc::tile16) against the fp32 oracle.
Nothing is fitted here: the bars are the suite's attention rule (tests/test_kernels_gpu.py: |d| <= 2^-7 |ref| + 2^-5 rms and
rms err <= 2^-7 rms) and the derived bounds of tests/attn_scores.py (check_output, check_suite_bar), which hold for any partition
of a tile's keys among lanes.

Shapes are the smallest at which the tile can go wrong: every key count that crosses a 4-key lane-group edge, a 16-key block and
the two tile edges (1 ... 130 for the short-key kernel, 1025 ... 1089 for the long-key one), query counts around the 16-row
q-block and the 32-row wave, one and three heads; dominant keys on both sides of every lane-group / block / half / tile edge;
a carried state written by one MFMA shape and read by the other."""
import contextlib
import math

import pytest
import torch

import attn_scores as A
from oracle import wan_ref as R
from test_kernels_gpu import assert_bf16_close, rnd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LN2 = math.log(2.0)
SCALE = 1.0 / math.sqrt(128)
GUARD = 9.0
DEFAULTS = {"attn_mfma": -1, "attn_defer_max_log2": 8, "attn_unit_scale": 1, "attn7_plain": 0}
# (name, launch scale, factor folded into K): the DiT's unit-scale path (softmax scale * log2 e in K, scale = ln 2) and the plain one
MODES = [("unit", LN2, SCALE * math.log2(math.e)), ("plain", SCALE, 1.0)]


@contextlib.contextmanager
def options(hip_ops, **kv):
    try:
        for k, v in kv.items():
            assert hip_ops.lib.icv_set_option(k.encode(), int(v)) == 0
        yield
    finally:
        for k in kv:
            hip_ops.lib.icv_set_option(k.encode(), DEFAULTS[k])


_INPUTS = {}


def inputs(Skv_max, seed):
    """q [257, 3 * 128], k, v [Skv_max, 3 * 128] on the GPU, per mode (made once, never modified; smaller cases are slices)."""
    key = (Skv_max, seed)
    if key not in _INPUTS:
        q, k, v = (rnd((257, 384), seed).to(torch.bfloat16), rnd((Skv_max, 384), seed + 1), rnd((Skv_max, 384), seed + 2).to(torch.bfloat16))
        _INPUTS[key] = {m: (q.to(DEV), (k * kf).to(torch.bfloat16).to(DEV), v.to(DEV)) for m, _, kf in MODES}
    return _INPUTS[key]


def heads_of(x, H):
    return x[:, :H * 128].contiguous()


def check(o, q, k, v, H, scale, what, fails, chunks=1, prev=None):
    """o [Sq + 2 guard rows, H * 128] after a launch over q, k, v: guard rows, the suite's rule against the fp32 oracle, the derived bounds."""
    Sq = q.shape[0]
    if not bool((o[Sq:] == GUARD).all()):
        fails.append(what + ": wrote past the last query row")
    ref = R.attention(q.float(), k.float(), v.float(), H, scale=scale)
    if prev is not None:
        ref = ref + prev.float()
    try:
        assert_bf16_close(o[:Sq], ref, what, abs_floor=2.0 ** -5, rms_bound=2.0 ** -7)
    except AssertionError as e:
        fails.append(str(e))
    sc = A.kernel_sc(scale)
    s, ds = A.scores(q, k, H, sc=sc)
    vh = A.heads_v(v, H)
    fails += A.check_output(o[:Sq], s, ds, vh, False, chunks, prev=prev, what=what)
    fails += A.check_suite_bar(o[:Sq], s, vh, prev=prev, what=what)


def finish(fails):
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:12])


@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("Sq", [1, 15, 16, 17, 33, 257])
def test_short_key_kernel_every_key_count_to_130(hip_ops, Sq, H):
    """attn7.hip's 4-wave kernel (Skv <= 1024)."""
    fails = []
    with options(hip_ops, attn_mfma=16):
        for mname, scale, _ in MODES:
            qa, ka, va = inputs(130, 700)[mname]
            q = heads_of(qa[:Sq], H)
            for Skv in range(1, 131):
                k, v = heads_of(ka[:Skv], H), heads_of(va[:Skv], H)
                o = torch.full((Sq + 2, H * 128), GUARD, dtype=torch.bfloat16, device=DEV)
                hip_ops.attention(q, k, v, o[:Sq], H, scale)
                check(o, q, k, v, H, scale, f"attn7 mfma16 {mname} Sq={Sq} Skv={Skv} H={H}", fails)
    finish(fails)


@pytest.mark.parametrize("Sq", [33, 257])
def test_long_key_kernel_every_key_count_1025_to_1089(hip_ops, Sq):
    """attn7p.hip (one piece) and, bit for bit, attn7.hip's 8-wave kernel (attn7_plain = 1): 17 tiles, the last one ragged at every length."""
    H = 2
    fails = []
    for mname, scale, _ in MODES:
        qa, ka, va = inputs(1089, 710)[mname]
        q = heads_of(qa[:Sq], H)
        for Skv in range(1025, 1090):
            k, v = heads_of(ka[:Skv], H), heads_of(va[:Skv], H)
            o = torch.full((Sq + 2, H * 128), GUARD, dtype=torch.bfloat16, device=DEV)
            o_plain = torch.empty((Sq, H * 128), dtype=torch.bfloat16, device=DEV)
            with options(hip_ops, attn_mfma=16):
                hip_ops.attention(q, k, v, o[:Sq], H, scale)
                with options(hip_ops, attn7_plain=1):
                    hip_ops.attention(q, k, v, o_plain, H, scale)
            what = f"attn7p mfma16 {mname} Sq={Sq} Skv={Skv}"
            check(o, q, k, v, H, scale, what, fails)
            if not torch.equal(o[:Sq], o_plain):
                fails.append(what + ": attn7.hip's kernel (attn7_plain) differs from the attn7p launch")
    finish(fails)


@pytest.mark.parametrize("Sq,Skv,H", [(33, 130, 1), (257, 130, 3), (33, 1089, 1), (257, 1089, 2)])
def test_one_hot_rows_are_the_dominant_keys_v_row_bit_for_bit(hip_ops, Sq, Skv, H):
    """Dominant keys on both sides of a 4-key lane-group edge (3 | 4), a 16-key block (15 | 16), a 32-key half (31 | 32), a tile
    (63 | 64) and at the ragged end: a P that meets the wrong V row shows as another row's values."""
    c = A.one_hot(Sq, Skv, H, [0, 3, 4, 15, 16, 31, 32, 63, 64, Skv - 1], seed=Skv + Sq)
    q, k, v = c["q"].to(DEV), c["k"].to(DEV), c["v"].to(DEV)
    want = A.expected_one_hot(c, H)
    fails = []
    for thr in (8, 0):
        for unit in (1, 0):
            with options(hip_ops, attn_mfma=16, attn_defer_max_log2=thr, attn_unit_scale=unit):
                o = torch.full((Sq + 2, H * 128), GUARD, dtype=torch.bfloat16, device=DEV)
                hip_ops.attention(q, k, v, o[:Sq], H, LN2)
                o2 = torch.empty((Sq, H * 128), dtype=torch.bfloat16, device=DEV)
                hip_ops.attention(q, k, v, o2, H, LN2)
            what = f"one-hot mfma16 Sq={Sq} Skv={Skv} H={H} thr={thr} unit={unit}"
            if not bool((o[Sq:] == GUARD).all()):
                fails.append(what + ": wrote past the last query row")
            if not torch.equal(o[:Sq], o2):
                fails.append(what + ": repeat launch differs")
            if not torch.equal(o[:Sq].cpu(), want):
                bad = (o[:Sq].cpu() != want).any(-1).nonzero().flatten()
                fails.append(f"{what}: not bit-exact on {bad.numel()} rows (first {bad[:4].tolist()}, dominant keys {c['dom'][bad[:4]].tolist()})")
    finish(fails)


@pytest.mark.parametrize("split", [[70, 1030], [1030, 70]])
@pytest.mark.parametrize("shapes", [(16, 16), (32, 16), (16, 32)])
def test_carried_state_is_one_memory_format_for_both_mfma_shapes(hip_ops, shapes, split):
    """Two chunks cut at a ragged row; the first writes (acc, m, l) with one MFMA shape, the second reads it with the other."""
    Sq, H = 257, 2
    fails = []
    for mname, scale, _ in MODES:
        qa, ka, va = inputs(1100, 720)[mname]
        q, k, v = heads_of(qa[:Sq], H), heads_of(ka, H), heads_of(va, H)
        acc = torch.empty((Sq, H * 128), device=DEV)
        ml = torch.empty((Sq, H, 2), device=DEV)
        o = torch.full((Sq + 2, H * 128), GUARD, dtype=torch.bfloat16, device=DEV)
        lo = 0
        for j, (n, mf) in enumerate(zip(split, shapes)):
            with options(hip_ops, attn_mfma=mf):
                hip_ops.attention_chunk(q, k[lo:lo + n], v[lo:lo + n], o[:Sq], acc, ml, H, scale, first=j == 0, last=j == 1)
            lo += n
        check(o, q, k, v, H, scale, f"chunks {split} mfma {shapes} {mname}", fails, chunks=2)
    finish(fails)


@pytest.mark.parametrize("thr", [8, 0])
def test_pieces_of_70_1_and_1029_rows(hip_ops, thr):
    Sq, H = 257, 2
    bounds = [0, 70, 71, 1100]
    fails = []
    for mname, scale, _ in MODES:
        qa, ka, va = inputs(1100, 720)[mname]
        q, k, v = heads_of(qa[:Sq], H), heads_of(ka, H), heads_of(va, H)
        plist = [(k[a:b], v[a:b], -1, 0) for a, b in zip(bounds[:-1], bounds[1:])]
        with options(hip_ops, attn_mfma=16, attn_defer_max_log2=thr):
            o = torch.full((Sq + 2, H * 128), GUARD, dtype=torch.bfloat16, device=DEV)
            hip_ops.attention_pieces(q, plist, o[:Sq], H, scale)
            o2 = torch.empty((Sq, H * 128), dtype=torch.bfloat16, device=DEV)
            hip_ops.attention_pieces(q, plist, o2, H, scale)
        what = f"pieces 70 | 1 | 1029 mfma16 {mname} thr={thr}"
        if not torch.equal(o[:Sq], o2):
            fails.append(what + ": repeat launch differs")
        check(o, q, k, v, H, scale, what, fails, chunks=3)
    finish(fails)


def test_attention_add_and_frame_window(hip_ops):
    """The other two epilogues / instantiations that share the tile: o += attention (short-key kernel) and the frame-windowed launch."""
    Sq, H = 33, 2
    fails = []
    qa, ka, va = inputs(130, 700)["unit"]
    q, k, v = heads_of(qa[:Sq], H), heads_of(ka[:77], H), heads_of(va[:77], H)
    prev = A.v_values(Sq, H, 99).to(DEV)
    with options(hip_ops, attn_mfma=16):
        o = torch.full((Sq + 2, H * 128), GUARD, dtype=torch.bfloat16, device=DEV)
        o[:Sq] = prev
        hip_ops.attention_add(q, k, v, o[:Sq], H, LN2)
    check(o, q, k, v, H, LN2, "attention_add mfma16", fails, prev=prev)
    # 5 frames of 70 rows, window 1, sink 1: frame 3 reads the sink piece [0, 70) and the window piece [140, 350)
    frames, F = 5, 70
    _, ka, va = inputs(1100, 720)["unit"]
    q = heads_of(rnd((frames * F, 384), 730).to(torch.bfloat16).to(DEV), H)
    k, v = heads_of(ka[:frames * F], H), heads_of(va[:frames * F], H)
    with options(hip_ops, attn_mfma=16):
        o = torch.full((frames * F + 2, H * 128), GUARD, dtype=torch.bfloat16, device=DEV)
        hip_ops.attention_framewin(q, k, v, o[:frames * F], H, LN2, frames, F, 1, 1)
    if not bool((o[frames * F:] == GUARD).all()):
        fails.append("framewin mfma16: wrote past the last query row")
    for f in range(frames):
        keys = sorted(set(range(0, F)) | set(range(max(f - 1, 0) * F, min(f + 2, frames) * F)))
        idx = torch.tensor(keys, device=DEV)
        of = torch.full((F + 2, H * 128), GUARD, dtype=torch.bfloat16, device=DEV)
        of[:F] = o[f * F:(f + 1) * F]
        check(of, q[f * F:(f + 1) * F], k[idx], v[idx], H, LN2, f"framewin mfma16 frame {f}", fails, chunks=2)
    finish(fails)


def test_an_unknown_mfma_shape_is_an_error(hip_ops):
    from infinicube_amd import native
    q, k, v = (heads_of(x[:16], 1) for x in inputs(130, 700)["unit"])
    o = torch.empty((16, 128), dtype=torch.bfloat16, device=DEV)
    with options(hip_ops, attn_mfma=8):
        with pytest.raises(native.NativeError):
            hip_ops.attention(q, k, v, o, 1, LN2)
