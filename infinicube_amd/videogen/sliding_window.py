"""Sliding temporal windows for clips longer than one trained forward.

Upstream DiffSynth-Studio's ``WanVideoPipeline.__call__(sliding_window_size=, sliding_window_stride=)`` [EXT] (both in LATENT
frames) runs the DiT, at every denoising step, on overlapping temporal windows of the latent - each window a complete forward
of its own (RoPE positions from 0, full attention inside the window) - and blends the windows' velocity predictions with
linear ramps over the overlap (``TemporalTiler_BCTHW``).  Cost is linear in the clip length and every forward stays at a
trained length.

The rule, restated from upstream as remembered (not read: ORACLE_RISKS.md R18).  T latent frames, ``border = size - stride``:
  * windows: for t in range(0, T, stride): skip if ``t - stride >= 0 and t - stride + size >= T`` (the previous window already
    reached the end); else the window is ``[t, min(t + size, T))``.  A window that is not skipped starts before
    ``T - border``, so every window is longer than ``border``;
  * 1-D mask of a window of length L: ones; not starting at 0 -> its first ``border`` entries are ``(arange(border) + 0.5) / border``;
    not ending at T -> its last ``border`` entries are that ramp reversed; ``border == 0`` -> all ones;
  * upstream accumulates ``value += out * mask``, ``weight += mask`` and returns ``value / weight``.
The weights depend on the window list only, so the per-window, per-frame coefficient ``c_w[f] = mask_w[f] / sum_w' mask_w'[f]``
is computed ONCE per call here in float64 and uploaded as one f32 table; the device then does
``latent_next[:, frame0 + f] += c_w[f] * (v_w * dsigma)`` per window (icv_unpatchify_cfg_euler_window).
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

ENV_SIZE, ENV_STRIDE = "ICV_SLIDING_WINDOW_SIZE", "ICV_SLIDING_WINDOW_STRIDE"


def validate(size, stride) -> Optional[Tuple[int, int]]:
    """(size, stride) as ints, or None when both are None (off).  Everything else raises ValueError."""
    if size is None and stride is None:
        return None
    if size is None or stride is None:
        raise ValueError(f"sliding_window_size and sliding_window_stride must be given together, got size={size!r}, stride={stride!r}")
    for name, v in (("sliding_window_size", size), ("sliding_window_stride", stride)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} must be an integer number of latent frames, got {v!r}")
    size, stride = int(size), int(stride)
    if size < 1 or stride < 1:
        raise ValueError(f"sliding_window_size and sliding_window_stride must be >= 1, got size={size}, stride={stride}")
    if stride > size:
        raise ValueError(f"sliding_window_stride ({stride}) must not exceed sliding_window_size ({size}): the frames between two windows would never be denoised")
    return size, stride


def windows(T: int, size: int, stride: int) -> Tuple[Tuple[int, int], ...]:
    out = []
    for t in range(0, T, stride):
        if t - stride >= 0 and t - stride + size >= T:
            continue
        out.append((t, min(t + size, T)))
    return tuple(out)


def mask(frame0: int, frame1: int, T: int, border: int) -> np.ndarray:
    """Upstream's 1-D blend mask of the window [frame0, frame1) of a T-frame clip (float64)."""
    m = np.ones(frame1 - frame0, dtype=np.float64)
    if border == 0:
        return m
    ramp = (np.arange(border, dtype=np.float64) + 0.5) / border
    if frame0 != 0:
        m[:border] = ramp
    if frame1 != T:
        m[-border:] = ramp[::-1]
    return m


@dataclass(frozen=True)
class WindowPlan:
    """The windows of one call over a T-frame latent and their blend coefficients.  ``coef`` float64 [n_windows, size]:
    row w holds c_w[f] for the window-local frames f of window w (zero beyond a shorter last window)."""
    T: int
    size: int
    stride: int
    windows: Tuple[Tuple[int, int], ...]
    coef: np.ndarray

    def record(self):
        return [(int(a), int(b)) for a, b in self.windows]


def plan(T: int, size: int, stride: int) -> WindowPlan:
    size, stride = validate(size, stride)
    if T < 1:
        raise ValueError(f"sliding window plan: T must be >= 1, got {T}")
    wins = windows(T, size, stride)
    masks = [mask(f0, f1, T, size - stride) for f0, f1 in wins]
    weight = np.zeros(T, dtype=np.float64)
    for (f0, f1), m in zip(wins, masks):
        weight[f0:f1] += m
    coef = np.zeros((len(wins), size), dtype=np.float64)
    for w, ((f0, f1), m) in enumerate(zip(wins, masks)):
        coef[w, : f1 - f0] = m / weight[f0:f1]
    return WindowPlan(int(T), size, stride, wins, coef)
