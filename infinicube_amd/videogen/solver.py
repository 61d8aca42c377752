"""Multistep samplers on the flow-match sigma list: UniPC (bh2, order 2, x0-prediction) as linear forms.

The pipeline's sigma list stays what scheduler.py builds: sigma_0 > sigma_1 > ... > sigma_{N-1}, and sigma_N = 0.  With
alpha = 1 - sigma and lambda(sigma) = ln((1 - sigma) / sigma) (lambda(0) = +inf, lambda(1) = -inf) a step i takes the CFG-combined
velocity v_i at the sample x_i, forms the x0-prediction m_i = x_i - sigma_i v_i, corrects x_i from the step before (UniC) and
predicts x_{i+1} (UniP).  [EXT]: restated from the UniPC paper and Wan2.1's scheduler, ORACLE_RISKS.md R23.

Everything here is float64 host arithmetic.  What leaves this module is, per step, two linear forms over the buffers the
kernel holds (icv_unpatchify_cfg_multistep knows nothing of UniPC):

    x_c     = a0 x_hat + a1 m_{i-1} + a2 m_{i-2} + a3 m_i        (``a`` is None: no corrector, x_c = x_i)
    x_{i+1} = c0 x_c   + c1 m_i     + c2 m_{i-1}

x_hat is the sample the previous predictor started from (the previous step's x_c).  State lives per denoise() call
(``MultistepPlan.begin()``): the first step a call executes is the "first step", whatever its index.
"""

from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

ENV_SOLVER, ENV_STEPS = "ICV_SAMPLE_SOLVER", "ICV_SAMPLE_STEPS"
SOLVERS = ("euler", "unipc")


def validate(name) -> Optional[str]:
    """The multistep solver a call runs: None for today's Euler path (``None`` or ``"euler"``), else the solver's name."""
    if name is None or name == "euler":
        return None
    if name not in SOLVERS:
        raise ValueError(f"sample_solver must be one of {', '.join(repr(s) for s in SOLVERS)} (or None), got {name!r}")
    return name


def lam(sigma: float) -> float:
    """Half log-SNR of the flow-match path: ln((1 - sigma) / sigma)."""
    if sigma <= 0.0:
        return math.inf
    if sigma >= 1.0:
        return -math.inf
    return math.log((1.0 - sigma) / sigma)


def bh2(h: float) -> Tuple[float, float, float, float]:
    """(phi1, B, b1, b2) of a step of size h > 0 in lambda; h = +inf: the limits."""
    if math.isinf(h):
        return -1.0, -1.0, 1.0, 1.0
    phi1 = math.expm1(-h)
    B = phi1
    g1 = phi1 / (-h) - 1.0
    g2 = g1 / (-h) - 0.5
    return phi1, B, g1 / B, 2.0 * g2 / B


@dataclass(frozen=True)
class Step:
    """One step's update.  ``a`` = (a0, a1, a2, a3) or None (no corrector), ``c`` = (c0, c1, c2); ``order`` is the predictor's,
    ``corrector_order`` 0 when there is no corrector."""
    index: int
    sigma: float
    a: Optional[Tuple[float, float, float, float]]
    c: Tuple[float, float, float]
    order: int
    corrector_order: int


class _Run:
    """The solver state of one denoise() call: which steps ran, and at which predictor order."""

    def __init__(self, sigmas: Sequence[float]):
        self.sigmas = [float(s) for s in sigmas] + [0.0]
        self.n = len(sigmas)
        self.done: List[Tuple[int, int]] = []          # (step index, predictor order) of the executed steps, oldest first

    def _usable(self, j: int) -> bool:
        """An x0-prediction taken at sigma = 1 (lambda = -inf) cannot serve as the second point."""
        return self.sigmas[j] < 1.0

    def step(self, i: int) -> Step:
        sig = self.sigmas
        if self.done and self.done[-1][0] != i - 1:
            raise ValueError(f"multistep solver: step {i} does not follow step {self.done[-1][0]} (the history belongs to consecutive steps)")
        a, q = None, 0
        if self.done:
            # UniC from s = sigma_{i-1} to t = sigma_i at the order the previous predictor ran
            q = self.done[-1][1]
            s, t = sig[i - 1], sig[i]
            h = lam(t) - lam(s)
            phi1, B, b1, b2 = bh2(h)
            K = (1.0 - t) * B
            a0, a1 = t / s, -(1.0 - t) * phi1
            if q == 1:
                a1, a2, a3 = a1 + 0.5 * K, 0.0, -0.5 * K
            else:
                r = (lam(sig[i - 2]) - lam(s)) / h
                rho1 = (b1 - b2) / (1.0 - r)
                rho2 = b1 - rho1
                a1, a2, a3 = a1 + K * rho1 / r + K * rho2, -K * rho1 / r, -K * rho2
            a = (a0, a1, a2, a3)
        # UniP from s = sigma_i to t = sigma_{i+1}
        order = min(2, len(self.done) + 1, self.n - i)
        if order == 2 and not self._usable(i - 1):
            order = 1
        s, t = sig[i], sig[i + 1]
        h = lam(t) - lam(s)
        phi1, B, _, _ = bh2(h)
        c0, c1, c2 = t / s, -(1.0 - t) * phi1, 0.0
        if order == 2:
            r = (lam(sig[i - 1]) - lam(s)) / h
            K = (1.0 - t) * B
            c1, c2 = c1 + 0.5 * K / r, -0.5 * K / r
        self.done.append((i, order))
        return Step(i, s, a, (c0, c1, c2), order, q)


class MultistepPlan:
    """What WanDiT.denoise(solver=...) takes: a named solver over one call's sigma list."""

    def __init__(self, name: str, sigmas: Sequence[float]):
        if validate(name) is None:
            raise ValueError(f"MultistepPlan: {name!r} is not a multistep solver")
        s = [float(x) for x in sigmas]
        if not s or not (0.0 < s[-1] and s[0] <= 1.0) or any(b >= a for a, b in zip(s, s[1:])):
            raise ValueError("MultistepPlan: sigmas must be a non-empty strictly decreasing list in (0, 1]")
        self.name, self.sigmas = name, s

    def begin(self) -> _Run:
        return _Run(self.sigmas)

    def steps(self, indices=None) -> List[Step]:
        """Every step of a call that runs ``indices`` (default: all) in order."""
        run = self.begin()
        return [run.step(i) for i in (range(len(self.sigmas)) if indices is None else indices)]

    def record(self, indices=None) -> dict:
        st = self.steps(indices)
        return dict(name=self.name, steps=len(st), orders=[s.order for s in st])
