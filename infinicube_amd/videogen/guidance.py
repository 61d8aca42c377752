"""CFG-Zero* guidance for the flow-matching loop: the optimised scale and zero-init.

Classifier-free guidance combines the two velocities of a step as ``v = v_u + w (v_c - v_u)``.  CFG-Zero* (Fan et al. 2025,
"CFG-Zero*: Improved Classifier-Free Guidance for Flow Matching Models") [EXT: restated from memory of the paper and of its Wan2.1
script, ORACLE_RISKS.md R24] changes two things, independent of each other:

* optimised scale (``cfg_zero_star``): ``v_u`` is replaced by ``s* v_u`` with ``s* = <v_c, v_u> / (|v_u|^2 + 1e-8)``, the
  projection of the conditional velocity onto the unconditional one over every latent element of the sample:
  ``v = s* v_u + w (v_c - s* v_u)``.  The engine forms s* on the device from the two head outputs (icv_cfg_zero_scale_f32: fp64
  sums, no host read), scales the unconditional head output in place and runs the step's usual update launch unchanged.
* zero-init (``cfg_zero_init_steps = K``): the velocity of the first K steps is zero.  Here those steps run no forward and no
  update launch at all - the latent's bits do not change - and the first executed step is step K for everything that keeps
  state (a multistep solver's history, a TeaCache plan).  That is NOT a zero prediction handed to the scheduler
  (ORACLE_RISKS.md R25).

This module is host logic only: the settings' validation, the two environment variables and the plan WanDiT.denoise takes.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

ENV_STAR, ENV_INIT_STEPS = "ICV_CFG_ZERO_STAR", "ICV_CFG_ZERO_INIT_STEPS"
EPS = 1e-8          # added to |v_u|^2; the kernel's constant (csrc/guidance.hip)


@dataclass(frozen=True)
class GuidancePlan:
    """What WanDiT.denoise(guidance=...) takes.  ``optimized_scale``: scale the unconditional head output by s* before the
    update of every executed step; ``zero_init_steps``: the steps ``i < K`` of the call run nothing."""
    optimized_scale: bool
    zero_init_steps: int

    def skips(self, step: int) -> bool:
        return step < self.zero_init_steps

    def record(self, scales: Optional[List[Optional[float]]] = None) -> dict:
        """``scales``: per step of the call, s* as the device computed it (None for a step that computed none)."""
        return dict(optimized_scale=self.optimized_scale, zero_init_steps=self.zero_init_steps, scales=list(scales or []))


def validate(cfg_zero_star, cfg_zero_init_steps, num_steps: int, cfg_scale: float) -> Optional[GuidancePlan]:
    """The plan of a call of ``num_steps`` steps, or None when both settings are off (None / False / 0): today's path."""
    if cfg_zero_star is None:
        cfg_zero_star = False
    if not isinstance(cfg_zero_star, bool):
        raise ValueError(f"cfg_zero_star must be a bool (or None), got {cfg_zero_star!r}")
    k = 0 if cfg_zero_init_steps is None else cfg_zero_init_steps
    if isinstance(k, bool) or not isinstance(k, int):
        raise ValueError(f"cfg_zero_init_steps must be an integer >= 0 (or None), got {cfg_zero_init_steps!r}")
    if k < 0:
        raise ValueError(f"cfg_zero_init_steps must be an integer >= 0 (or None), got {k}")
    if k >= num_steps and k > 0:
        raise ValueError(f"cfg_zero_init_steps={k} leaves no step to run: it must be less than the {num_steps} steps of the call")
    if cfg_zero_star and float(cfg_scale) == 1.0:
        raise ValueError("cfg_zero_star needs classifier-free guidance: cfg_scale is 1, so the call runs no unconditional forward")
    if not cfg_zero_star and k == 0:
        return None
    return GuidancePlan(bool(cfg_zero_star), int(k))
