"""TeaCache ("timestep embedding aware cache") step skipping for the denoising loop.

Upstream DiffSynth-Studio's ``WanVideoPipeline.__call__(tea_cache_l1_thresh=, tea_cache_model_id=)`` [EXT] keeps one
``TeaCache`` per CFG branch.  At step i it measures how far the time projection ``t_mod`` moved since the previous step
(``mean|t_i - t_{i-1}| / mean|t_{i-1}|``), maps that through a per-model polynomial and accumulates it; while the sum stays
under the threshold the step skips the transformer blocks and adds the residual the last computed step left
(``x_after_blocks - x_before_blocks``).  Steps 0 and N-1 are always computed and reset the sum; so is every step that
reaches the threshold.

``t_mod`` depends on the timestep and the weights only, never on the latent, so the whole schedule is decided ONCE per call,
before the loop (``plan``): the rows of every step go into one table, ``icv_rel_l1_steps_f32`` turns it into the distances
(deterministic, so every rank gets the same bits), N floats come back once, and the accumulate / reset rule runs here in
float64.  The same schedule holds for both CFG branches and for every sequence-parallel rank.
"""

from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

ENV_THRESH, ENV_MODEL_ID = "ICV_TEACACHE_L1_THRESH", "ICV_TEACACHE_MODEL_ID"

# Polynomial coefficients, highest degree first (np.poly1d), as published with TeaCache4Wan2.1 and copied into DiffSynth.
# Not checked against a copy of upstream (ORACLE_RISKS.md R16); tests/test_teacache_cpu.py pins them.
COEFFICIENTS: Dict[str, Tuple[float, ...]] = {
    "Wan2.1-T2V-1.3B": (-5.21862437e+04, 9.23041404e+03, -5.28275948e+02, 1.36987616e+01, -4.99875664e-02),
    "Wan2.1-T2V-14B": (-3.03318725e+05, 4.90537029e+04, -2.65530556e+03, 5.87365115e+01, -3.15583525e-01),
    "Wan2.1-I2V-14B-480P": (2.57151496e+05, -3.54229917e+04, 1.40286849e+03, -1.35890334e+01, 1.32517977e-01),
    "Wan2.1-I2V-14B-720P": (8.10705460e+03, 2.13393892e+03, -3.72934672e+02, 1.66203073e+01, -4.17769401e-02),
}

# t2v model id by DiT width, for a threshold given through the environment without an id (pipeline.py)
T2V_MODEL_ID_BY_DIM = {1536: "Wan2.1-T2V-1.3B", 5120: "Wan2.1-T2V-14B"}


def coefficients(model_id: str) -> Tuple[float, ...]:
    """The coefficients of ``model_id``; DiffSynth's error for an id it does not know (the default "" included)."""
    if model_id not in COEFFICIENTS:
        ids = list(COEFFICIENTS)
        raise ValueError(f"{model_id} is not a supported TeaCache model id. Please choose a valid model id in ({', '.join(ids)}).")
    return COEFFICIENTS[model_id]


def infer_t2v_model_id(cfg) -> str:
    """The t2v model id of a DiT config (by width); i2v DiTs have two ids per width, so they need an explicit one."""
    if cfg.has_image_input:
        raise ValueError("TeaCache on an image-to-video DiT needs an explicit model id (tea_cache_model_id / ICV_TEACACHE_MODEL_ID): "
                         "Wan2.1-I2V-14B-480P or Wan2.1-I2V-14B-720P")
    if cfg.dim not in T2V_MODEL_ID_BY_DIM:
        raise ValueError(f"TeaCache: no t2v model id for a DiT of width {cfg.dim}; pass tea_cache_model_id / ICV_TEACACHE_MODEL_ID")
    return T2V_MODEL_ID_BY_DIM[cfg.dim]


def settings(thresh: Optional[float], model_id: str, cfg, from_keyword: bool):
    """(threshold, model id) of one call, validated, from the values in effect (options.resolve); (None, "") = TeaCache off.
    A threshold without an id raises DiffSynth's unknown-id error, except when neither was a keyword and the threshold's variable
    is set: then a t2v DiT's id follows from its width."""
    if thresh is None:
        return None, ""
    if not model_id and not from_keyword and ENV_THRESH in os.environ:
        model_id = infer_t2v_model_id(cfg)
    coefficients(model_id)          # validate before any work is done
    return float(thresh), model_id


@dataclass
class TeaCachePlan:
    """The skip schedule of one call.  ``steps``: the loop's steps in order; ``distances[k]``: the relative L1 distance of
    step ``steps[k]``'s t_mod to the previous step's (entry 0 unused, 0.0); ``computed``: the steps that run the blocks."""
    model_id: str
    thresh: float
    steps: Tuple[int, ...]
    distances: Tuple[float, ...]
    computed: Tuple[int, ...]
    _computed: frozenset = field(default=frozenset(), repr=False, compare=False)

    def __post_init__(self):
        self._computed = frozenset(self.computed)

    def skip(self, step: int) -> bool:
        return step not in self._computed

    def record(self) -> dict:
        return dict(model_id=self.model_id, thresh=self.thresh, computed=list(self.computed), distances=list(self.distances))


def schedule(distances: Sequence[float], steps: Sequence[int], num_steps: int, thresh: float,
             coeffs: Sequence[float]) -> Tuple[int, ...]:
    """DiffSynth's ``TeaCache.check`` over a whole loop: the steps that are computed.  Step 0, step ``num_steps - 1`` and the
    first step of ``steps`` (a partial range must start with a residual) are forced and reset the accumulator; any other
    step adds ``poly(coeffs)(distance)`` and is skipped while the sum stays below ``thresh``, else computed (sum reset)."""
    rescale = np.poly1d(np.asarray(coeffs, dtype=np.float64))
    acc, computed = 0.0, []
    for k, i in enumerate(steps):
        if k == 0 or i == 0 or i == num_steps - 1:
            acc, calc = 0.0, True
        else:
            acc += float(rescale(float(distances[k])))
            calc = not acc < thresh
            if calc:
                acc = 0.0
        if calc:
            computed.append(int(i))
    return tuple(computed)


def plan(engine, scheduler, thresh: float, model_id: str, steps: Optional[Sequence[int]] = None,
         coeffs: Optional[Sequence[float]] = None) -> TeaCachePlan:
    """Build the schedule of one denoise call on a prepared ``engine`` (dit.WanDiT).  ``coeffs`` overrides the table
    (tests / tools force a known schedule with it); otherwise ``model_id`` must be one of ``COEFFICIENTS``."""
    if coeffs is None:
        coeffs = coefficients(model_id)
    thresh = float(thresh)
    n_all = len(scheduler.timesteps)
    steps = tuple(int(i) for i in (steps if steps is not None else range(n_all)))
    if not steps:
        return TeaCachePlan(model_id, thresh, (), (), ())
    ops, cols = engine.ops, engine.t_mod.shape[-1]
    table = ops.alloc((len(steps), cols), torch.float32)
    for k, i in enumerate(steps):
        engine._time_state(scheduler.timesteps[i])
        table[k].copy_(engine.t_mod.reshape(-1))
    dist = ops.alloc((len(steps),), torch.float32)
    ops.rel_l1_steps(table, dist)
    distances = tuple(float(v) for v in dist.cpu().tolist())      # the one read-back of the call
    return TeaCachePlan(model_id, thresh, steps, distances, schedule(distances, steps, n_all, thresh, coeffs))
