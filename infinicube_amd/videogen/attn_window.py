"""Frame-windowed self-attention: training-free temporal sparsity for the DiT's self-attention.

The DiT's tokens are ordered (frame, row, column), so one latent frame is ``F = Hp * Wp`` contiguous rows.  With
``attention_window_frames = w`` a query of latent frame f attends only to the keys of the frames g with ``|g - f| <= w``, plus -
with ``attention_sink_frames = s`` - the first s frames of the clip as an anchor.  In frames, with T latent frames:

    lo = max(0, f - w),  hi = min(T, f + w + 1)
    s == 0:               one range   [lo, hi)
    s > 0 and lo <= s:    one range   [0, max(hi, s))         (the window touches or overlaps the anchor)
    otherwise:            two ranges  [0, s) then [lo, hi)

One launch (icv_attention_fwd_framewin, csrc/attn7p.hip) computes these ranges per work-group from the four scalars; ``ranges()``
below states the same rule on the host for tests and documentation.  ``w >= T - 1`` makes every range [0, T): dense attention,
for which the engine keeps the plain launch.

This is a change of the MODEL's arithmetic (a trained checkpoint attends densely); what it does to the quality of a trained
checkpoint is not measured in this repository, whose test weights are random - as for TeaCache (teacache.py).

Radial attention (``attention_radial``; the second half of this module) makes the window the dense run of a mask that
keeps every frame in reach and halves the band of in-frame rows with every doubling of the temporal distance.
"""

from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np

ENV_WINDOW, ENV_SINK = "ICV_ATTN_WINDOW_FRAMES", "ICV_ATTN_SINK_FRAMES"


def validate(window, sink, T: Optional[int] = None) -> Optional[Tuple[int, int]]:
    """(window, sink) as ints - sink clamped to the clip's ``T`` latent frames when T is given - or None when the setting is off
    (window None and no sink).  Negatives, non-integers and a sink without a window raise ValueError."""
    for name, v in (("attention_window_frames", window), ("attention_sink_frames", sink)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer))):
            raise ValueError(f"{name} must be an integer number of latent frames, got {v!r}")
        if v is not None and int(v) < 0:
            raise ValueError(f"{name} must be >= 0, got {int(v)}")
    if window is None:
        if sink is not None and int(sink) != 0:
            raise ValueError(f"attention_sink_frames ({int(sink)}) needs attention_window_frames: the anchor frames are an addition to a window")
        return None
    window, sink = int(window), int(sink or 0)
    if T is not None:
        if T < 1:
            raise ValueError(f"frame-windowed attention: T must be >= 1, got {T}")
        sink = min(sink, int(T))
    return window, sink


def dense(T: int, window: int) -> bool:
    """Every query sees every frame: the plain launch computes the same thing."""
    return window >= T - 1


def ranges(T: int, window: int, sink: int) -> List[List[Tuple[int, int]]]:
    """Per latent frame f of T, the key ranges [(frame0, frame1), ...] its queries read, in the order the kernel walks them."""
    window, sink = validate(window, sink, T)
    out = []
    for f in range(T):
        lo, hi = max(0, f - window), min(T, f + window + 1)
        if sink == 0:
            out.append([(lo, hi)])
        elif lo <= sink:
            out.append([(0, max(hi, sink))])
        else:
            out.append([(0, sink), (lo, hi)])
    return out


def key_fraction(T: int, window: int, sink: int) -> float:
    """Share of the T x T (query frame, key frame) pairs that are read: the kernel's key traffic and flops relative to dense."""
    return sum(b - a for r in ranges(T, window, sink) for a, b in r) / float(T * T)


def record(T: int, window: int, sink: int) -> dict:
    return dict(window=int(window), sink=int(sink), key_fraction=key_fraction(T, window, sink))


# ---- radial attention (one launch: icv_attention_fwd_radial, csrc/attn7r.hip) ------------------------------------------
# Every key frame stays in reach; what thins with the temporal distance is the band of in-frame positions a query reads of it: each
# doubling of the distance halves the band.  The mask is defined per QUERY BLOCK of a frame, as the launch's work-groups are.  With T
# frames of F rows, window W >= 0 and sink S, query block b of frame f has the in-frame rows [p0, p1), p0 = 256 b,
# p1 = min(F, p0 + 256), and reads of key frame g the in-frame rows
#
#     g < S or |g - f| <= W:   the whole frame, [0, F)
#     otherwise:               e = |g - f| - W,  l = floor(log2 e) + 1,  h = F >> (l + 1)  (may be 0):
#                              [max(0, p0 - h), min(F, p1 + h))         - never empty
#
# for g ascending.  Two ranges that are adjacent in memory are one piece, so the dense run and the sink stay one piece each; a
# work-group has at most T pieces, hence T <= RADIAL_MAX_FRAMES (the kernel's ICV_ATTN_MAX_PIECES).  Pieces start and end at
# arbitrary rows.  W >= T - 1 is dense attention.  ``radial_ranges`` is the specification; the kernel restates it.
#
# The rule is Radial Attention's (Li et al. 2025) restated and simplified: block granularity 256, no sub-sampled diagonal at large
# distances (ORACLE_RISKS.md).  Like the frame window it changes the MODEL's arithmetic; what it does to a trained checkpoint is not
# measured in this repository, whose test weights are random.
RADIAL_QBLOCK = 256
RADIAL_MAX_FRAMES = 64


def validate_radial(radial, window, T: Optional[int] = None) -> bool:
    """``attention_radial`` as a bool (None = off).  A non-bool raises, True without a window raises (window 0 is a window), and so do
    more than RADIAL_MAX_FRAMES latent frames when ``T`` is given."""
    if radial is None:
        return False
    if not isinstance(radial, (bool, np.bool_)):
        raise ValueError(f"attention_radial must be a bool, got {radial!r}")
    if not radial:
        return False
    if window is None:
        raise ValueError("attention_radial needs attention_window_frames: the dense run around the query's own frame (0 is a valid window)")
    if T is not None and T > RADIAL_MAX_FRAMES and not dense(T, int(window)):
        raise ValueError(f"attention_radial: {T} latent frames, but a work-group walks at most {RADIAL_MAX_FRAMES} pieces, one per frame")
    return True


def radial_ranges(T: int, F: int, window: int, sink: int) -> List[List[Tuple[int, int]]]:
    """Per (frame, query block) - frame-major, ceil(F / 256) blocks per frame - the key pieces [(row0, row1), ...] in GLOBAL rows, in
    the order the kernel walks them."""
    window, sink = validate(window, sink, T)
    if F < 1:
        raise ValueError(f"radial attention: F must be >= 1, got {F}")
    if T > RADIAL_MAX_FRAMES:
        raise ValueError(f"radial attention: {T} frames, at most {RADIAL_MAX_FRAMES}")
    out = []
    for f in range(T):
        for p0 in range(0, F, RADIAL_QBLOCK):
            p1 = min(F, p0 + RADIAL_QBLOCK)
            pieces: List[Tuple[int, int]] = []
            for g in range(T):
                if g < sink or abs(g - f) <= window:
                    lo, hi = 0, F
                else:
                    e = abs(g - f) - window
                    h = F >> (e.bit_length() + 1)          # e.bit_length() = floor(log2 e) + 1
                    lo, hi = max(0, p0 - h), min(F, p1 + h)
                lo, hi = g * F + lo, g * F + hi
                if pieces and pieces[-1][1] == lo:
                    pieces[-1] = (pieces[-1][0], hi)
                else:
                    pieces.append((lo, hi))
            out.append(pieces)
    return out


def radial_key_fraction(T: int, F: int, window: int, sink: int) -> float:
    """Share of the (query row, key row) pairs that are read, of all (T F)^2."""
    read, i = 0, 0
    rr = radial_ranges(T, F, window, sink)
    for f in range(T):
        for p0 in range(0, F, RADIAL_QBLOCK):
            read += (min(F, p0 + RADIAL_QBLOCK) - p0) * sum(b - a for a, b in rr[i])
            i += 1
    return read / float(T * F) ** 2


def radial_tiles(T: int, F: int, window: int, sink: int) -> int:
    """64-key tiles the launch issues per head: sum of ceil(rows / 64) over every work-group's pieces."""
    return sum(-(-(b - a) // 64) for pieces in radial_ranges(T, F, window, sink) for a, b in pieces)


def framewin_tiles(T: int, F: int, window: int, sink: int) -> int:
    """The same count for the frame-windowed launch (its work-groups are the same (frame, block) pairs)."""
    blocks = -(-F // RADIAL_QBLOCK)
    return blocks * sum(-(-(b - a) * F // 64) for r in ranges(T, window, sink) for a, b in r)


def radial_record(T: int, F: int, window: int, sink: int) -> dict:
    return dict(window=int(window), sink=int(sink), radial=True, key_fraction=radial_key_fraction(T, F, window, sink),
                max_pieces=max(len(p) for p in radial_ranges(T, F, window, sink)))
