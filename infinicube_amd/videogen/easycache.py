"""EasyCache runtime-adaptive step skipping: ``easy_cache_thresh``.

EasyCache (Zhou et al. 2025, "Less is Enough: Training-Free Video Diffusion Acceleration via Runtime-Adaptive Caching") [EXT:
restated from memory of the paper and of its Wan2.1 code, simplified where that code is inconsistent across skipped steps,
ORACLE_RISKS.md R31] needs no per-checkpoint table: at run time it measures how fast the model's output moves per unit of input
change, accumulates the predicted relative output change and skips the DiT while that stays under ONE threshold.  A skipped step
runs no forward at all; it forms the head outputs as ``cached output + (input - cached input)`` (icv_easycache_predict_f32).

The rule, over the loop's executed steps e_0, e_1, ... (zero-init steps of CFG-Zero* are not executed and do not count).  Step i
has input latent x_i and, when computed, conditional head output v_i (slot 0; with NAG the only one).  Means over all elements.
State: acc = 0, k = None, n_out = None, j = None (the last computed step).  At the m-th executed step i:

1. for m > 0, d_in = mean|x_i - x_prev|, x_prev the previous executed step's input;
2. the step is FORCED when m < warmup_steps, when i is the scheduler's last step, or when k is None or n_out == 0: computed, acc = 0;
3. otherwise acc += k * d_in / n_out; the step is skipped iff acc < thresh, else computed and acc = 0;
4. computed: run the forwards; if j exists and d_x = mean|x_i - x_j| > 0, k = mean|v_i - v_j| / d_x (else k keeps its value);
   n_out = mean|v_i|; x_last <- x_i, h_last[b] <- head output of branch b; j = i;
5. skipped: head[b] <- h_last[b] + P(x_i - x_last) for every branch (both follow the one decision);
6. x_prev <- x_i; the step's usual tail (the CFG-Zero* scale, the Euler / multistep update, the pin) runs unchanged.

The sums come from the device (icv_l1_change_f64, fp64, deterministic); the rule itself runs here in float64.  Host logic only:
nothing here imports torch.
"""

from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

DEFAULT_WARMUP_STEPS = 10            # the paper's warm-up [EXT: from memory, R31]


def validate(thresh, warmup_steps=None) -> Optional[Tuple[float, int]]:
    """(thresh, warmup_steps) of a call with EasyCache on, None when it is off (``thresh`` None).  Raises ValueError for a threshold
    that is not a finite real number > 0 (a bool included), a warm-up that is not an integer >= 2 (k needs two computed steps), and
    a warm-up given without a threshold."""
    if thresh is None:
        if warmup_steps is not None:
            raise ValueError("easy_cache_warmup_steps given without easy_cache_thresh: it only shapes EasyCache step skipping")
        return None
    if isinstance(thresh, bool) or not isinstance(thresh, (int, float)) or not math.isfinite(thresh) or not thresh > 0:
        raise ValueError(f"easy_cache_thresh must be a finite number > 0, got {thresh!r}")
    if warmup_steps is None:
        warmup_steps = DEFAULT_WARMUP_STEPS
    if isinstance(warmup_steps, bool) or not isinstance(warmup_steps, int) or warmup_steps < 2:
        raise ValueError(f"easy_cache_warmup_steps must be an integer >= 2, got {warmup_steps!r}")
    return float(thresh), int(warmup_steps)


def check_call(world: int, windows: bool, tea_cache: bool) -> None:
    """The first-version scope of a call with EasyCache on, in the pipeline's terms."""
    if tea_cache:
        raise ValueError("easy_cache_thresh cannot be combined with TeaCache (tea_cache_l1_thresh / ICV_TEACACHE_L1_THRESH) in the same call yet")
    if world > 1:
        raise ValueError(f"easy_cache_thresh cannot be combined with a process group of {world} ranks yet")
    if windows:
        raise ValueError("easy_cache_thresh cannot be combined with sliding_window_size (more than one window) in the same call yet")


class Rule:
    """The rule above as a state machine in float64: one ``decide`` per executed step, then ``computed`` and ``output`` for a step
    that was not skipped - in the order the loop learns the numbers (a computed step's output sums arrive with the next step's
    input sums, before the next ``decide``)."""

    def __init__(self, thresh: float, warmup_steps: int = DEFAULT_WARMUP_STEPS, force_skip=frozenset()):
        self.thresh, self.warmup_steps, self.force_skip = float(thresh), int(warmup_steps), frozenset(force_skip)
        self.acc, self.k, self.n_out, self.j, self.m, self._d_x = 0.0, None, None, None, 0, None

    def decide(self, i: int, last_step: bool, d_in: Optional[float]):
        """Steps 1-3 for the next executed step ``i`` -> (skip, k in effect, the sum compared with thresh | None where forced).
        ``d_in``: mean|x_i - x_prev| (ignored at the first executed step)."""
        m, self.m = self.m, self.m + 1
        forced = m < self.warmup_steps or last_step or self.k is None or self.n_out == 0.0
        if forced:
            self.acc = 0.0
            # force_skip: wherever a skip is possible - not forced by warm-up / last step, and something is cached
            if i in self.force_skip and self.j is not None and not (m < self.warmup_steps or last_step):
                return True, self.k, None
            return False, self.k, None
        self.acc += self.k * float(d_in) / self.n_out
        compared = self.acc
        skip = compared < self.thresh or i in self.force_skip
        if not skip:
            self.acc = 0.0
        return skip, self.k, compared

    def computed(self, i: int, d_x: Optional[float]) -> None:
        """Step 4, the input's half, for computed step ``i``: d_x = mean|x_i - x_j| (ignored while j is None); j = i."""
        self._d_x = float(d_x) if self.j is not None and d_x is not None else None
        self.j = int(i)

    def output(self, d_v: float, n_out: float) -> None:
        """Step 4, the output's half, for the step ``computed`` was just told about: d_v = mean|v_i - v_j| (ignored where d_x was
        ignored or is 0: k keeps its value), n_out = mean|v_i|.  Must precede the next ``decide``."""
        if self._d_x is not None and self._d_x > 0.0:
            self.k = float(d_v) / self._d_x
        self.n_out = float(n_out)


def trace(thresh: float, warmup_steps: int, steps, last_step: int, measure, force_skip=frozenset()) -> dict:
    """The rule over a whole loop.  ``steps``: the executed steps in order; ``last_step``: the scheduler's last step;
    ``measure(i, j)`` -> (d_in, d_x, d_v, n_out) of step i given the last computed step j (None at first): d_in for every
    step, the other three only read when the step is computed.  Returns EasyCachePlan.record()'s lists."""
    rule, computed, skipped, ks, accs = Rule(thresh, warmup_steps, force_skip), [], [], [], []
    for i in steps:
        d_in, d_x, d_v, n_out = measure(i, rule.j)
        skip, k, acc = rule.decide(i, i == last_step, d_in)
        ks.append(k)
        accs.append(acc)
        if skip:
            skipped.append(int(i))
        else:
            rule.computed(i, d_x)
            rule.output(d_v, n_out)
            computed.append(int(i))
    return dict(computed=computed, skipped=skipped, k=ks, accumulated=accs)


@dataclass(eq=False)
class EasyCachePlan:
    """What WanDiT.denoise(easy_cache=...) takes.  ``force_skip``: steps that skip regardless of the rule wherever a skip is possible
    (not forced by the warm-up or the last step, and a computed step exists) - the handle tests and tools use.  The loop fills the
    four lists; ``k`` / ``accumulated`` hold, per executed step, the k in effect at its decision (None before two computed steps)
    and the sum that was compared with the threshold (None for a forced step)."""
    thresh: float
    warmup_steps: int = DEFAULT_WARMUP_STEPS
    force_skip: frozenset = frozenset()
    computed: List[int] = field(default_factory=list)
    skipped: List[int] = field(default_factory=list)
    k: List[Optional[float]] = field(default_factory=list)
    accumulated: List[Optional[float]] = field(default_factory=list)

    def __post_init__(self):
        self.thresh, self.warmup_steps = validate(self.thresh, self.warmup_steps)
        self.force_skip = frozenset(int(i) for i in self.force_skip)

    def begin(self) -> Rule:
        """A fresh rule state for one denoise call; the record's lists start empty."""
        self.computed, self.skipped, self.k, self.accumulated = [], [], [], []
        return Rule(self.thresh, self.warmup_steps, self.force_skip)

    def record(self) -> dict:
        return dict(thresh=self.thresh, warmup_steps=self.warmup_steps, computed=list(self.computed), skipped=list(self.skipped),
                    k=list(self.k), accumulated=list(self.accumulated))
