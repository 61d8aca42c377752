"""Enhance-A-Video: a training-free boost of cross-frame attention, ``enhance_weight``.

Flicker between frames is the usual complaint about Wan2.1 clips.  Enhance-A-Video (Luo et al. 2025, "Enhance-A-Video: Better
Generated Video for Free"; "FETA" in the common Wan wrappers) [EXT: restated from memory of the paper and of the wrappers' code,
ORACLE_RISKS.md R29] measures, in every block, how much the self-attention looks across frames rather than at a token's own frame,
and multiplies that block's self-attention output by one scalar derived from the measurement.  For one self-attention call (one
CFG branch of one forward) on T latent frames x P positions, with q, k the normalised, rotated operands of the attention launch,
per position s and head h, in f32:

    L[t, t']  = scale * <q[(t, s), h], k[(t', s), h]>             the true logit, same position, any two frames
    A[t, .]   = softmax over t' of L[t, .]
    m[s, h]   = (sum over t != t' of A[t, t']) / (T (T - 1))      the mean off-diagonal weight
    E         = max(1, (T + enhance_weight) * mean over (s, h) of m[s, h])
    att      <- bf16(f32(att) * E)                                in front of self_attn.o

Uniform attention gives E = 1 + w / T, the ceiling is (T + w) / (T - 1), and E = 1 gives the plain bits back.  The engine runs it
as two launches per layer and branch (icv_enhance_scores_bf16, icv_enhance_apply_bf16); E never leaves the device inside the loop.
``enhance_weight`` of None is off: today's launches, allocations and bits.  0 is NOT off (E = max(1, T * mean) can exceed 1).

First-version scope, each refused with a ValueError in the pipeline before any GPU work and, where the engine can observe it, in
``WanDiT.denoise``; none falls back:

* more than one rank (the mean over positions would need a cross-rank reduction);
* more than one sliding temporal window;
* fewer than 2 or more than 32 latent frames (one 32-frame tile: 125 frames; longer clips are sliding-window calls).

It composes with CFG pairs (each branch its own E), TeaCache (a skipped step runs no blocks), the multistep solvers, CFG-Zero*,
Normalized Attention Guidance, ``input_video`` / ``input_mask``, LoRA, the frame window (E is still taken over all T frames), the
e4m3 mode (the bf16 q / k exist in front of the e4m3 attention) and an image-to-video DiT.

The setting is a keyword of the call with a pipeline attribute of the same name as its fallback (``pipe.enhance_weight = 4.0`` for
the caller of the unchanged generator).  As for Normalized Attention Guidance there is no environment route and no row in
``options.OPTIONS``.

Host logic only: the setting's validation and the plan ``WanDiT.denoise`` takes.  Nothing here imports torch.
"""

from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

MIN_FRAMES, MAX_FRAMES = 2, 32        # latent frames of a call: one 32-row tile of the score kernel


@dataclass(frozen=True)
class EnhancePlan:
    """What WanDiT.denoise(enhance=...) takes: the weight of the rule."""
    weight: float

    @property
    def key(self) -> Tuple[float]:
        """The scalar a captured forward holds by value: part of the graph cache's key."""
        return (float(self.weight),)

    def record(self, frames: int, scores: Optional[Sequence[Sequence[float]]] = None) -> dict:
        """``scores``: E per layer per branch of the last computed forward (None: no forward ran the blocks)."""
        return dict(weight=float(self.weight), frames=int(frames), scores=None if scores is None else [[float(e) for e in b] for b in scores])


def validate(enhance_weight) -> Optional[float]:
    """The weight of a call with the feature on, None when it is off (``enhance_weight`` None).  Raises ValueError for anything
    that is not a finite number >= 0."""
    if enhance_weight is None:
        return None
    if isinstance(enhance_weight, bool) or not isinstance(enhance_weight, (int, float)) or not math.isfinite(enhance_weight):
        raise ValueError(f"enhance_weight must be a finite number >= 0 or None, got {enhance_weight!r}")
    if enhance_weight < 0:
        raise ValueError(f"enhance_weight must be a finite number >= 0 or None, got {enhance_weight!r}")
    return float(enhance_weight)


def check_frames(frames: int, who: str = "enhance_weight") -> None:
    if not MIN_FRAMES <= frames <= MAX_FRAMES:
        raise ValueError(f"{who} cannot be combined with a clip of {frames} latent frames: the cross-frame measurement needs "
                         f"{MIN_FRAMES} to {MAX_FRAMES} (5 to 125 frames); longer clips are sliding-window calls, which are not supported yet")


def check_call(world: int, windows: bool, frames: int) -> None:
    """The first-version scope of a call with the feature on, in the pipeline's terms."""
    if world > 1:
        raise ValueError(f"enhance_weight cannot be combined with a process group of {world} ranks yet (the mean over positions would "
                         "need a cross-rank reduction)")
    if windows:
        raise ValueError("enhance_weight cannot be combined with sliding_window_size (more than one window) in the same call yet")
    check_frames(frames)
