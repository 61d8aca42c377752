"""Normalized Attention Guidance: the negative prompt in ONE forward per step.

Classifier-free guidance needs a second DiT forward per step for the negative prompt.  Normalized Attention Guidance (Chen et al.
2025, "Normalized Attention Guidance: Universal Negative Guidance for Diffusion Models") [EXT: restated from memory of the paper
and of its Wan2.1 code, ORACLE_RISKS.md R28] applies the negative prompt inside every block's text cross-attention instead, on the
attention output in front of ``cross_attn.o``.  With z+ / z- the outputs of the same queries against the positive / negative text:

    g    = scale * z+ - (scale - 1) * z-                      extrapolate
    c    = min(|g|_1 / |z+|_1, tau) / (|g|_1 / |z+|_1)        clip the per-token L1 norm (over all heads) against z+'s
    out  = alpha * c * g + (1 - alpha) * z+                   blend back into z+

The engine runs it as one more text cross-attention launch and one token-local launch per layer (icv_nag_combine_bf16), in place
in the attention-output buffer; an image-to-video DiT adds its CLIP-token softmax AFTER the combine (the order of the common Wan
wrappers; unverified, R28).  ``nag_scale`` of None or exactly 1 is off: today's launches, allocations and bits.

First-version scope, each refused with a ValueError in the pipeline before any GPU work and, where the engine can observe it, in
``WanDiT.denoise``; none falls back:

* ``cfg_scale != 1`` - the point is the single forward; NAG on the conditional branch of a CFG pair is a later change;
* more than one rank (sequence or CFG-branch parallelism);
* more than one sliding temporal window;
* ``cfg_zero_star`` raises on its own without CFG.

NAG composes with TeaCache (a skipped step runs no blocks), the multistep solvers, ``input_video`` / ``input_mask``, LoRA (the
negative context is encoded after the merges, like the others), the frame window, the e4m3 mode and an image-to-video DiT.

The settings are keywords of the call with pipeline attributes of the same names as their fallback (``pipe.nag_scale = 11.0;
pipe.cfg_scale = 1.0`` for the caller of the unchanged generator).  There is deliberately no environment route and no row in
``options.OPTIONS`` - an ``ICV_NAG_SCALE`` would be useless without an ``ICV_CFG_SCALE``, which does not exist either.

Host logic only: the settings' validation and the plan ``WanDiT.denoise`` takes.  Nothing here imports torch.
"""

from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Any, Optional, Tuple

DEFAULT_TAU, DEFAULT_ALPHA = 2.5, 0.25        # what the Wan wrappers ship next to nag_scale = 11


@dataclass(frozen=True, eq=False)
class NagPlan:
    """What WanDiT.denoise(nag=...) takes.  ``ctx_neg``: an ordinary ``encode_context`` result of the negative prompt (with the same
    CLIP features as the positive one on an image-to-video DiT); the three numbers of the rule."""
    ctx_neg: Any
    scale: float
    tau: float
    alpha: float

    @property
    def key(self) -> Tuple[float, float, float]:
        """The scalars a captured forward holds by value: part of the graph cache's key."""
        return (float(self.scale), float(self.tau), float(self.alpha))

    def record(self) -> dict:
        return dict(scale=float(self.scale), tau=float(self.tau), alpha=float(self.alpha))


def _number(name: str, value) -> float:
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(value):
        raise ValueError(f"{name} must be a finite number, got {value!r}")
    return float(value)


def validate(nag_scale, nag_tau=None, nag_alpha=None) -> Optional[Tuple[float, float, float]]:
    """(scale, tau, alpha) of a call with NAG on, None when it is off (``nag_scale`` None or exactly 1).  Raises ValueError for a
    non-numeric or non-finite value, nag_scale < 1, nag_tau < 1, nag_alpha outside (0, 1], and nag_tau / nag_alpha without
    nag_scale."""
    if nag_scale is None:
        given = [n for n, v in (("nag_tau", nag_tau), ("nag_alpha", nag_alpha)) if v is not None]
        if given:
            raise ValueError(f"{' / '.join(given)} given without nag_scale: they only shape Normalized Attention Guidance")
        return None
    scale = _number("nag_scale", nag_scale)
    if scale < 1.0:
        raise ValueError(f"nag_scale must be >= 1 (1 = off), got {nag_scale!r}")
    tau = DEFAULT_TAU if nag_tau is None else _number("nag_tau", nag_tau)
    if tau < 1.0:
        raise ValueError(f"nag_tau must be >= 1, got {nag_tau!r}")
    alpha = DEFAULT_ALPHA if nag_alpha is None else _number("nag_alpha", nag_alpha)
    if not 0.0 < alpha <= 1.0:
        raise ValueError(f"nag_alpha must be in (0, 1], got {nag_alpha!r}")
    return None if scale == 1.0 else (scale, tau, alpha)


def check_call(cfg_scale: float, world: int, windows: bool) -> None:
    """The first-version scope of a call with NAG on, in the pipeline's terms."""
    if float(cfg_scale) != 1.0:
        raise ValueError(f"nag_scale needs cfg_scale=1 (got {cfg_scale!r}): it replaces the unconditional forward; NAG on the "
                         "conditional branch of a CFG pair is not implemented yet")
    if world > 1:
        raise ValueError(f"nag_scale cannot be combined with a process group of {world} ranks yet")
    if windows:
        raise ValueError("nag_scale cannot be combined with sliding_window_size (more than one window) in the same call yet")
