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
