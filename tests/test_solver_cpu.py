"""The UniPC multistep sampler (infinicube_amd/videogen/solver.py) on CPU: the per-step linear forms against a float64
restatement of the predictor / corrector in their D / rho form, the closed-form Gaussian problem (UniPC is the better solver, and of
second order), the host loop (dit.WanDiT.denoise(solver=)) on the TEST-ONLY oracle operator set against oracle.wan_ref forwards driven
by the restated solver, off = nothing new (bits, launches, allocations), the scope errors, the two environment variables through the
unchanged generator, and the C entry point's argument checks (they run on the host, before any launch)."""
import contextlib
import io
import math

import numpy as np
import pytest
import torch

from dit_launch_trace import Trace, TracedOps
from infinicube_amd.videogen import options
from infinicube_amd.videogen import solver as S
from infinicube_amd.videogen import synthetic as syn
from infinicube_amd.videogen.config import TokenGrid, preset
from infinicube_amd.videogen.dit import WanDiT
from infinicube_amd.videogen.pipeline import DiTHolder, WanVideoPipeline
from infinicube_amd.videogen.scheduler import FlowMatchScheduler, flow_match_sigmas
from oracle import wan_ref as R
from standins import HashTextEncoder, PoolVAE
from test_teacache_cpu import TeaOps

CFG, GRID = preset("tiny"), TokenGrid(17, 64, 96)        # 5 latent frames of 4 x 6 tokens
ENV = options.ENV_NAMES
F32 = torch.float32
# The step count of the loop tests, chosen in 4..8 on the CPU: on the stiff DiT below the host loop scores 60.6 dB against the restated
# UniPC loop and the restated Euler loop 37.1 dB - under the 40 dB bar itself (5 steps: 60.8 / 39.2 dB with the head scaled by 6)
LOOP_STEPS = 6


# ---- the restatement: UniPC bh2 in its D / rho form, float64, none of the module's code ---------------------------------------------
def _lam(sigma):
    return math.inf if sigma <= 0.0 else -math.inf if sigma >= 1.0 else math.log((1.0 - sigma) / sigma)


def _bh2(h):
    """phi1, B, b1, b2 of a step h in lambda (the limits at h = +inf)."""
    if h == math.inf:
        return -1.0, -1.0, 1.0, 1.0
    phi1 = math.expm1(-h)
    B = phi1
    g1 = phi1 / (-h) - 1.0
    g2 = g1 / (-h) - 0.5
    return phi1, B, g1 / B, 2.0 * g2 / B


def restated_predictor(sig, i, order, x, m_i, m_im1):
    """UniP from sigma_i to sigma_{i+1} (``sig`` ends with sigma_N = 0)."""
    s, t = sig[i], sig[i + 1]
    h = _lam(t) - _lam(s)
    phi1, B, _, _ = _bh2(h)
    xbar = (t / s) * x - (1.0 - t) * phi1 * m_i
    if order == 1:
        return xbar
    r = (_lam(sig[i - 1]) - _lam(s)) / h
    D = (m_im1 - m_i) / r
    return xbar - (1.0 - t) * B * 0.5 * D


def restated_corrector(sig, i, q, x_hat, m_im1, m_im2, m_i):
    """UniC from sigma_{i-1} to sigma_i at order q, from the sample x_hat the previous predictor started from."""
    s, t = sig[i - 1], sig[i]
    h = _lam(t) - _lam(s)
    phi1, B, b1, b2 = _bh2(h)
    m0 = m_im1
    xbar = (t / s) * x_hat - (1.0 - t) * phi1 * m0
    if q == 1:
        return xbar - (1.0 - t) * B * 0.5 * (m_i - m0)
    r = (_lam(sig[i - 2]) - _lam(s)) / h
    D = (m_im2 - m0) / r
    rho1 = (b1 - b2) / (1.0 - r)
    rho2 = b1 - rho1
    return xbar - (1.0 - t) * B * (rho1 * D + rho2 * (m_i - m0))


def restated_orders(sigmas, first=0):
    """Predictor order of every step a call executes from step ``first`` on: min(2, predictions held, steps left), and never 2 on a
    second point taken at sigma = 1."""
    n, out = len(sigmas), []
    for i in range(first, n):
        p = min(2, i - first + 1, n - i)
        if p == 2 and sigmas[i - 1] >= 1.0:
            p = 1
        out.append(p)
    return out


def restated_sample(velocity, x, sigmas, solver="unipc", first=0):
    """The whole loop in float64 on ``x`` (numpy or torch): velocity(x, i) is the model.  ``solver`` "euler": the first-order update."""
    sig = [float(s) for s in sigmas] + [0.0]
    if solver == "euler":
        for i in range(first, len(sigmas)):
            x = x + velocity(x, i) * (sig[i + 1] - sig[i])
        return x
    orders, ms, x_hat = restated_orders(sigmas, first), {}, None
    for k, i in enumerate(range(first, len(sigmas))):
        ms[i] = x - sig[i] * velocity(x, i)                  # from the predictor's output; never recomputed after the corrector
        if k > 0:
            x = restated_corrector(sig, i, orders[k - 1], x_hat, ms[i - 1], ms.get(i - 2), ms[i])
        x_hat = x
        x = restated_predictor(sig, i, orders[k], x, ms[i], ms.get(i - 1))
    return x


def module_sample(velocity, x, sigmas, first=0):
    """The same loop on the module's linear forms."""
    run = S.MultistepPlan("unipc", sigmas).begin()
    x_hat, ms = None, {}
    for i in range(first, len(sigmas)):
        st = run.step(i)
        ms[i] = x - st.sigma * velocity(x, i)
        xc = x
        if st.a is not None:
            xc = st.a[0] * x_hat + st.a[1] * ms[i - 1] + (st.a[2] * ms[i - 2] if st.a[2] != 0.0 else 0.0) + st.a[3] * ms[i]
        x = st.c[0] * xc + st.c[1] * ms[i] + (st.c[2] * ms[i - 1] if st.c[2] != 0.0 else 0.0)
        x_hat = xc
    return x


# ---- 1. coefficients ----------------------------------------------------------------------------------------------------------------
def _close(got, want, what):
    for g, w in zip(got, want):
        assert abs(g - w) <= 1e-12 * abs(w), f"{what}: {got} vs the restatement's {want}"


@pytest.mark.parametrize("n,shift,strength", [(1, 5.0, 1.0), (2, 5.0, 1.0), (3, 5.0, 1.0), (8, 5.0, 1.0), (25, 5.0, 1.0), (8, 1.0, 1.0), (8, 5.0, 0.6)])
def test_linear_forms_match_the_restatement(n, shift, strength):
    sigmas = flow_match_sigmas(n, shift, denoising_strength=strength)
    sig = sigmas + [0.0]
    plan = S.MultistepPlan("unipc", sigmas)
    steps, orders = plan.steps(), restated_orders(sigmas)
    assert [st.order for st in steps] == orders and plan.record() == dict(name="unipc", steps=n, orders=orders)
    e = np.eye(4)
    for i, st in enumerate(steps):
        assert st.index == i and st.sigma == sigmas[i]
        if i == 0:
            assert st.a is None and st.corrector_order == 0
        else:
            assert st.corrector_order == orders[i - 1]
            want = restated_corrector(sig, i, orders[i - 1], e[0], e[1], e[2], e[3])      # unit vectors: the form's four coefficients
            _close(st.a, want, f"N={n} step {i} corrector (order {orders[i - 1]})")
            assert (st.a[2] != 0.0) == (orders[i - 1] == 2)
        want = restated_predictor(sig, i, orders[i], e[0, :3], e[1, :3], e[2, :3])
        _close(st.c, want, f"N={n} step {i} predictor (order {orders[i]})")
        assert (st.c[2] != 0.0) == (orders[i] == 2)
    assert steps[-1].c == (0.0, 1.0, 0.0), "the last step has t = 0: x_N = m_{N-1}"


def test_orders():
    assert S.MultistepPlan("unipc", flow_match_sigmas(1)).record()["orders"] == [1]
    one = S.MultistepPlan("unipc", flow_match_sigmas(1)).steps()[0]
    assert one.a is None and one.c == (0.0, 1.0, 0.0)                                     # x_1 = m_0
    assert S.MultistepPlan("unipc", flow_match_sigmas(2)).record()["orders"] == [1, 1]
    for n in (4, 8, 25):
        assert flow_match_sigmas(n)[0] == 1.0
        assert S.MultistepPlan("unipc", flow_match_sigmas(n)).record()["orders"] == [1, 1] + [2] * (n - 3) + [1], "step 1's second point lies at sigma = 1"
        assert S.MultistepPlan("unipc", flow_match_sigmas(n, denoising_strength=0.6)).record()["orders"] == [1] + [2] * (n - 2) + [1]
    # at sigma = 1 the order-1 predictor is the Euler step: sigma_t x + (1 - sigma_t) m
    sig = flow_match_sigmas(8)
    st = S.MultistepPlan("unipc", sig).steps()[0]
    assert st.c == (sig[1], 1.0 - sig[1], 0.0)
    # state lives per call: the first step a call executes is the first step, whatever its index
    late = S.MultistepPlan("unipc", sig).steps(range(3, 8))
    assert late[0].a is None and [s.order for s in late] == [1, 2, 2, 2, 1] == restated_orders(sig, first=3)
    assert S.MultistepPlan("unipc", sig).record(range(3, 8)) == dict(name="unipc", steps=5, orders=[1, 2, 2, 2, 1])
    with pytest.raises(ValueError, match="does not follow"):
        S.MultistepPlan("unipc", sig).steps([0, 2])
    with pytest.raises(ValueError, match="strictly decreasing"):
        S.MultistepPlan("unipc", [0.5, 0.5])
    with pytest.raises(ValueError, match="not a multistep solver"):
        S.MultistepPlan("euler", sig)


# ---- 2. it is a better solver -------------------------------------------------------------------------------------------------------
def _gaussian():
    """Data N(0.7, 0.5^2), noise N(0, 1), x_sigma = (1 - sigma) x0 + sigma eps: the exact marginal velocity E[eps - x0 | x_sigma] and
    the exact end point 0.7 + 0.5 x(1) of its flow."""
    eps = np.random.default_rng(0).standard_normal(4096)

    def velocity(sigmas):
        def v(x, i):
            s = sigmas[i]
            mean, var = (1.0 - s) * 0.7, (1.0 - s) ** 2 * 0.25 + s * s
            return s / var * (x - mean) - (0.7 + (1.0 - s) * 0.25 / var * (x - mean))
        return v

    return eps, velocity, 0.7 + 0.5 * eps


def test_unipc_beats_euler_on_the_closed_form_problem():
    eps, velocity, exact = _gaussian()

    def err(solver, n, shift):
        sigmas = flow_match_sigmas(n, shift)
        x = restated_sample(velocity(sigmas), eps.copy(), sigmas, "euler") if solver == "euler" else module_sample(velocity(sigmas), eps.copy(), sigmas)
        return float(np.sqrt(np.mean((x - exact) ** 2)))

    e = {k: err(*k) for k in (("unipc", 25, 5.0), ("euler", 50, 5.0), ("unipc", 30, 5.0), ("euler", 30, 5.0), ("unipc", 80, 1.0), ("unipc", 160, 1.0))}
    print({f"{s} N={n} shift={sh:g}": f"{v:.3e}" for (s, n, sh), v in e.items()})
    # the float64 prototype of the rule: 0.0330 / 0.0428, 0.019 / 0.070, ratio 4.2 - a different figure is a different rule
    for key, proto in ((("unipc", 25, 5.0), 3.30e-2), (("euler", 50, 5.0), 4.28e-2), (("unipc", 30, 5.0), 1.91e-2), (("euler", 30, 5.0), 6.96e-2),
                       (("unipc", 80, 1.0), 2.72e-4), (("unipc", 160, 1.0), 6.41e-5)):
        assert abs(e[key] / proto - 1.0) <= 0.10, f"{key}: {e[key]:.3e}, the prototype gave {proto:.3e}"
    assert e[("unipc", 25, 5.0)] < e[("euler", 50, 5.0)]
    assert e[("unipc", 30, 5.0)] < 0.5 * e[("euler", 30, 5.0)]
    assert e[("unipc", 80, 1.0)] / e[("unipc", 160, 1.0)] >= 3.0, "second order: the error falls about 4x per doubling of N"
    # the module's forms and the D / rho restatement are one rule
    sigmas = flow_match_sigmas(25)
    a, b = module_sample(velocity(sigmas), eps.copy(), sigmas), restated_sample(velocity(sigmas), eps.copy(), sigmas)
    assert float(np.abs(a - b).max()) <= 1e-12


# ---- the CPU twin of icv_unpatchify_cfg_multistep -----------------------------------------------------------------------------------
def rb(t):
    return t.to(torch.bfloat16).to(F32)


def multistep_twin(latent, x_hat, m_new, m_prev, m_prev2, hc, hu, cfg_scale, sigma, a, c, tok0, n_tok, round_bf16=False):
    """Torch twin of the kernel, one f32 tensor op per rounding point, sums left to right (include/icvideo.h)."""
    C, T, H8, W8 = latent.shape
    grid = (T, H8 // 2, W8 // 2)
    hc = hc[:n_tok]
    hu = None if hu is None else hu[:n_tok]
    if round_bf16:
        v = rb(hc) if hu is None else rb(rb(hu) + rb(cfg_scale * rb(rb(hc) - rb(hu))))
    else:
        v = hc if hu is None else hu + cfg_scale * (hc - hu)
    full, mask = torch.zeros((T * grid[1] * grid[2], 4 * C), dtype=F32), torch.zeros((T * grid[1] * grid[2], 4 * C), dtype=F32)
    full[tok0: tok0 + n_tok] = v
    mask[tok0: tok0 + n_tok] = 1.0
    vel, own = R.unpatchify(full, grid, C), R.unpatchify(mask, grid, C) > 0
    f = lambda x: float(torch.tensor(float(x), dtype=F32))      # noqa: E731  (the scalars reach the kernel as f32)
    zero = torch.zeros_like(latent)
    x = latent.clone()
    m = x - f(sigma) * vel
    xc = x
    if a is not None:
        if (m_prev is None and a[1] != 0.0) or (m_prev2 is None and a[2] != 0.0):
            raise ValueError("multistep twin: a buffer that is None has a nonzero coefficient")
        xc = (f(a[0]) * (x_hat if a[0] != 0.0 else zero) + f(a[1]) * (m_prev if a[1] != 0.0 else zero)
              + f(a[2]) * (m_prev2 if a[2] != 0.0 else zero) + f(a[3]) * m)
    nxt = f(c[0]) * xc + f(c[1]) * m + f(c[2]) * (m_prev if c[2] != 0.0 else zero)
    m_new.copy_(torch.where(own, m, m_new))
    x_hat.copy_(torch.where(own, xc, x_hat))
    latent.copy_(torch.where(own, nxt, latent))


class SolverOps(TeaOps):
    """OracleOps + the TeaCache twins + the CPU twin of icv_unpatchify_cfg_multistep; keeps each call's (sigma, a, c)."""

    def __init__(self, device="cpu"):
        super().__init__(device)
        self.multistep_calls = []

    def unpatchify_cfg_multistep(self, latent, x_hat, m_new, m_prev, m_prev2, hc, hu, cfg_scale, sigma, a, c, tok0, n_tok, round_bf16=False):
        bufs = (latent, x_hat, m_new, m_prev, m_prev2)
        assert len({b.data_ptr() for b in bufs}) == 5 and all(b.dtype == F32 and b.shape == latent.shape for b in bufs)
        self.multistep_calls.append((sigma, a, c))
        multistep_twin(latent, x_hat, m_new, m_prev, m_prev2, hc, hu, cfg_scale, sigma, a, c, tok0, n_tok, round_bf16)


# ---- 3. the host loop ------------------------------------------------------------------------------------------------------------------
STIFF = {"head.head.weight": 8.0, "time_embedding.0.weight": 8.0}


def stiff_state_dict():
    """The synthetic tiny DiT with its output head and the first time-embedding matrix scaled by 8.  With the synthetic weights as
    they come, the CFG velocity changes by 2 % between sigma = 1 and sigma = 0.2 at a fixed sample and is a third of the sample's
    size: the ODE is almost x' = const, every solver integrates it exactly (restated Euler vs restated UniPC: 65-69 dB at 4-8
    steps) and no bar could tell the solvers apart.  Scaled, the velocity depends on time and sample, as a trained model's does."""
    sd = syn.make_dit_state_dict(CFG)
    for k, g in STIFF.items():
        sd[k] = sd[k] * g
    return sd


def inputs(grid=GRID):
    sd, bsd = stiff_state_dict(), syn.make_buffer_embedder_state_dict(CFG)
    return sd, bsd, syn.make_latent_noise(grid), syn.make_text_context(CFG, 1), syn.make_text_context(CFG, 2), syn.make_buffer_latents(CFG, grid)


def oracle_velocity(sigmas, cfg_scale=5.0, fp8=False, grid=GRID):
    """velocity(x, i) of restated_sample on oracle.wan_ref forwards (bf16-rounded weights, fp32 arithmetic), CFG combined."""
    sd, bsd, _, c1, c2, bl = inputs(grid)
    rsd, rbsd = R.round_state_dict_to_bf16(sd), R.round_state_dict_to_bf16(bsd)
    buf = R.buffer_embed(rbsd, bl)

    def v(x, i):
        ts = float(sigmas[i]) * 1000.0
        v_c = R.dit_forward(rsd, CFG, x.float(), c1, ts, buf, fp8=fp8)
        v_u = R.dit_forward(rsd, CFG, x.float(), c2, ts, buf, fp8=fp8)
        return (v_u + cfg_scale * (v_c - v_u)).double()
    return v


_REFS = {}


def reference(solver, steps=LOOP_STEPS, strength=1.0, fp8=False):
    """The restated loop's latent on the oracle's forwards, computed once per setting."""
    key = (solver, steps, strength, fp8)
    if key not in _REFS:
        sigmas = flow_match_sigmas(steps, denoising_strength=strength)
        _REFS[key] = restated_sample(oracle_velocity(sigmas, fp8=fp8), inputs()[2].double(), sigmas, solver).float()
    return _REFS[key]


def engine_loop(ops, solver="unipc", steps=LOOP_STEPS, strength=1.0, setup=None, prep=None, dev="cpu", kw=None, tea=None):
    """dit.WanDiT.denoise on ``ops`` -> (engine, latent).  ``tea``: a function of (engine, scheduler) that returns the TeaCache plan."""
    sd, bsd, noise, c1, c2, bl = inputs()
    m = WanDiT(CFG, sd, ops, bsd, **(kw or {})).prepare(GRID, **(prep or {}))
    if setup is not None:
        setup(m)
    sch = FlowMatchScheduler(steps, denoising_strength=strength)
    lat = noise.clone().to(dev)
    extra = dict(solver=S.MultistepPlan(solver, sch.sigmas)) if solver != "euler" else {}
    if tea is not None:
        extra["tea_cache"] = tea(m, sch)
    m.denoise(lat, m.encode_context(c1), m.encode_context(c2), m.embed_buffers(bl), sch, 5.0, **extra)
    return m, lat


@pytest.mark.parametrize("cfg_batch", [True, False])
def test_host_loop_matches_restated_solver(cfg_batch):
    """Tiny preset, 5 latent frames, CFG 5, LOOP_STEPS steps.  Bar: the project's loop bar (>= 40 dB) against the restated UniPC loop -
    and the restated EULER loop scores at least 10 dB lower against it than the engine does, so the bar tells the solvers apart."""
    ops = SolverOps()
    m, lat = engine_loop(ops, setup=lambda m: setattr(m, "cfg_batch", cfg_batch))
    assert (m._pair is not None) == cfg_batch
    assert 4 <= LOOP_STEPS <= 8 and len(ops.multistep_calls) == LOOP_STEPS
    plan = S.MultistepPlan("unipc", flow_match_sigmas(LOOP_STEPS))
    assert ops.multistep_calls == [(st.sigma, st.a, st.c) for st in plan.steps()]
    ref = reference("unipc")
    p, p_euler = R.psnr(lat, ref), R.psnr(reference("euler"), ref)
    print(f"UniPC host loop vs restated UniPC: {p:.1f} dB; restated Euler vs restated UniPC: {p_euler:.1f} dB")
    assert p >= 40.0, f"{p:.1f} dB"
    assert p_euler <= p - 10.0, f"the bar cannot tell the solvers apart at {LOOP_STEPS} steps: Euler {p_euler:.1f} dB, loop {p:.1f} dB"
    # the state buffers: four, the latent's shape, allocated once and reused by a second call
    x_hat, ring = m._solver_state
    assert len(ring) == 3 and all(t.shape == lat.shape and t.dtype == F32 for t in [x_hat] + ring)
    sch = FlowMatchScheduler(LOOP_STEPS)
    again = inputs()[2].clone()
    sd, bsd, noise, c1, c2, bl = inputs()
    m.denoise(again, m.encode_context(c1), m.encode_context(c2), m.embed_buffers(bl), sch, 5.0, solver=S.MultistepPlan("unipc", sch.sigmas))
    assert m._solver_state[0] is x_hat and torch.equal(again, lat), "a second call starts from a clean history"


def test_partial_range_starts_a_fresh_history():
    """denoise(steps=range(2, N)): the first step the call executes runs without a corrector, at order 1."""
    sd, bsd, noise, c1, c2, bl = inputs()
    ops = SolverOps()
    m = WanDiT(CFG, sd, ops, bsd).prepare(GRID)
    sch = FlowMatchScheduler(5)
    m.denoise(noise.clone(), m.encode_context(c1), None, m.embed_buffers(bl), sch, 1.0, steps=range(2, 5), solver=S.MultistepPlan("unipc", sch.sigmas))
    assert [a is None for _, a, _ in ops.multistep_calls] == [True, False, False]
    assert ops.multistep_calls == [(st.sigma, st.a, st.c) for st in S.MultistepPlan("unipc", sch.sigmas).steps(range(2, 5))]
    with pytest.raises(ValueError, match="not built on this scheduler's sigmas"):
        m.denoise(noise.clone(), m.encode_context(c1), None, m.embed_buffers(bl), sch, 1.0, solver=S.MultistepPlan("unipc", flow_match_sigmas(4)))


# ---- 4. off means nothing new ---------------------------------------------------------------------------------------------------------
def _pipe(ops=None, vae=None, dtype=torch.bfloat16):
    return WanVideoPipeline("cpu", dtype, DiTHolder(syn.make_dit_state_dict(CFG), CFG), HashTextEncoder(CFG), vae or PoolVAE(),
                            ops=ops or SolverOps())


def _call_kw(**extra):
    kw = dict(prompt="a street", negative_prompt="bad", height=GRID.height, width=GRID.width, num_frames=GRID.num_frames, seed=3,
              num_inference_steps=3, return_latents=True)
    kw.update(extra)
    return kw


def test_off_is_the_euler_path(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)

    def run(**kw):
        tr = Trace()
        ops = TracedOps(tr)                       # has no unpatchify_cfg_multistep: calling it would raise
        p = _pipe(ops)
        allocs, raw = [], ops.alloc
        monkeypatch.setattr(ops, "alloc", lambda shape, dtype: (allocs.append((tuple(shape), dtype)), raw(shape, dtype))[1])
        tr.on = True
        lat = p(**_call_kw(**kw))
        tr.on = False
        assert p.solver_record is None and p._engine._solver_state is None
        return tr.log, allocs, lat

    log0, allocs0, lat0 = run()
    assert sum(e[0] == "unpatchify_cfg_euler" for e in log0) == 3
    for name in (None, "euler"):
        log1, allocs1, lat1 = run(sample_solver=name)
        assert torch.equal(lat1, lat0) and log1 == log0 and allocs1 == allocs0, f"sample_solver={name!r} must be the path without the keyword"
    # ... and "unipc" replaces exactly the step's last launch and adds the four state buffers
    ops = SolverOps()
    p = _pipe(ops)
    allocs, raw = [], ops.alloc
    monkeypatch.setattr(ops, "alloc", lambda shape, dtype: (allocs.append((tuple(shape), dtype)), raw(shape, dtype))[1])
    lat = p(**_call_kw(sample_solver="unipc"))
    assert p.sample_solver is None and p.solver_record == dict(name="unipc", steps=3, orders=[1, 1, 1])
    assert len(ops.multistep_calls) == 3 and not torch.equal(lat, lat0)
    assert allocs == allocs0 + [(tuple(lat.shape), F32)] * 4, "allocated on first use, after everything the Euler path allocates"
    base = p(**_call_kw())                          # the setting does not outlive its call
    assert p.solver_record is None and len(ops.multistep_calls) == 3 and torch.equal(base, lat0)


# ---- 5. scope, names, the step-count variable -----------------------------------------------------------------------------------------
def test_scope_errors(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    p = _pipe()
    monkeypatch.setattr(p, "_get_engine", lambda: pytest.fail("the engine was built before the settings were validated"))
    with pytest.raises(ValueError, match=r"sample_solver must be one of 'euler', 'unipc' \(or None\), got 'dpm\+\+'"):
        p(**_call_kw(sample_solver="dpm++"))
    with pytest.raises(ValueError, match="sample_solver='unipc' cannot be combined with sliding_window_size.* yet"):
        p(**_call_kw(sample_solver="unipc", sliding_window_size=3, sliding_window_stride=2))
    import torch.distributed as dist
    with monkeypatch.context() as mp:
        mp.setattr(dist, "is_initialized", lambda: True)
        mp.setattr(dist, "get_world_size", lambda *a: 2)
        mp.setattr(dist, "get_rank", lambda *a: 0)
        with pytest.raises(ValueError, match="sample_solver='unipc' cannot be combined with a process group of 2 ranks yet"):
            p(**_call_kw(sample_solver="unipc"))
    # one sliding window is no combination: the plain loop with the solver
    p = _pipe()
    one = p(**_call_kw(sample_solver="unipc", sliding_window_size=GRID.T, sliding_window_stride=GRID.T))
    assert p.sliding_window_record is None and p.solver_record["name"] == "unipc" and torch.equal(one, p(**_call_kw(sample_solver="unipc")))
    # the engine says the same when it is driven directly, before any launch
    sd, bsd, noise, c1, c2, bl = inputs()
    sch = FlowMatchScheduler(2)
    plan = S.MultistepPlan("unipc", sch.sigmas)
    from infinicube_amd.videogen import sliding_window as SW
    ops = SolverOps()
    m = WanDiT(CFG, sd, ops, bsd).prepare(TokenGrid(9, 64, 96))
    with pytest.raises(ValueError, match="cannot be combined with more than one sliding temporal window yet"):
        m.denoise(noise.clone(), None, None, None, sch, 5.0, sliding_window=SW.plan(GRID.T, 3, 2), solver=plan)
    msp = WanDiT(CFG, sd, ops, bsd).prepare(GRID, force_sp=True)
    with pytest.raises(ValueError, match=r"cannot be combined with sequence / CFG-branch parallelism \(world > 1\) yet"):
        msp.denoise(noise.clone(), None, None, None, sch, 5.0, solver=plan)
    m = WanDiT(CFG, sd, ops, bsd).prepare(GRID)
    with pytest.raises(ValueError, match=r"cannot be combined with sequence / CFG-branch parallelism \(world > 1\) yet"):
        m.denoise(noise.clone(), m.encode_context(c1), None, None, sch, 5.0, branch_exchange=lambda own, both: None, solver=plan)
    assert not ops.multistep_calls and m._solver_state is None


def test_worker_pool_combination_raises(monkeypatch):
    """ICV_WORLD > 1 behind the unchanged generator: refused in the client before a request reaches the ranks."""
    from infinicube_amd.videogen.inference import WanVideoGenerator
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    g = WanVideoGenerator.__new__(WanVideoGenerator)
    g._pool, g.pipe = object(), _pipe()
    g.pipe.sample_solver = "unipc"
    sem, co = syn.make_dummy_buffers(TokenGrid(9, 64, 96))
    with pytest.raises(ValueError, match="ICV_SAMPLE_SOLVER.*ICV_WORLD > 1"):
        g.generate(sem, co, seed=0)


def test_environment_values(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    p = _pipe()
    assert (p.sample_solver, p.solver_record, p.num_inference_steps) == (None, None, 50) and len(p.scheduler.sigmas) == 50
    for bad in ("0", "-3", "2.5", "ten", " "):
        monkeypatch.setenv("ICV_SAMPLE_STEPS", bad)
        with pytest.raises(ValueError, match="ICV_SAMPLE_STEPS must be an integer >= 1"):
            _pipe()
    monkeypatch.setenv("ICV_SAMPLE_STEPS", "25")
    p = _pipe()
    assert p.num_inference_steps == 25 and p.sample_solver is None and len(p.scheduler.sigmas) == 25      # for any solver
    monkeypatch.setenv("ICV_SAMPLE_SOLVER", "unipc")
    assert _pipe().sample_solver == "unipc"
    monkeypatch.setenv("ICV_SAMPLE_SOLVER", "heun")
    with pytest.raises(ValueError, match="sample_solver must be one of 'euler', 'unipc'"):
        _pipe()
    monkeypatch.setenv("ICV_SAMPLE_SOLVER", "euler")
    assert _pipe().sample_solver == "euler"


# ---- 6. the unchanged generator, through the environment ------------------------------------------------------------------------------
class CountingVAE(PoolVAE):
    """PoolVAE that keeps the last latent it was asked to decode."""

    def __init__(self):
        super().__init__()
        self.last_decoded = None

    def decode(self, latent, **kw):
        self.last_decoded = latent.detach().clone().cpu()
        return super().decode(latent, **kw)


def generator_through_env(factory, tmp_path, monkeypatch, grid, device, **env):
    """WanVideoGenerator built and run with ``env`` set -> the generator."""
    from safetensors.torch import save_file
    from infinicube.videogen import WanVideoGenerator
    ck = str(tmp_path / "step-1.safetensors")
    save_file({"buffer_embedder." + k: v for k, v in syn.make_buffer_embedder_state_dict(CFG).items()}, ck)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sem, co = syn.make_dummy_buffers(grid)
    with contextlib.redirect_stdout(io.StringIO()):
        g = WanVideoGenerator(ck, device=device, use_wan_1pt3b=True, pipeline_factory=factory)
        video = g.generate(sem, co, prompt="a street", negative_prompt="bad", seed=3)
    assert len(video) == grid.num_frames
    for k in env:
        monkeypatch.delenv(k)
    return g, sem, co


def test_generator_through_the_environment(tmp_path, monkeypatch):
    from PIL import Image
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    grid = TokenGrid(9, 64, 96)
    vae = CountingVAE()
    g, sem, co = generator_through_env(lambda torch_dtype, device, model_configs: _pipe(vae=vae), tmp_path, monkeypatch, grid, "cpu",
                                       ICV_SAMPLE_SOLVER="unipc", ICV_SAMPLE_STEPS="4")
    assert (g.pipe.sample_solver, g.pipe.num_inference_steps) == ("unipc", 4)
    assert g.pipe.solver_record == dict(name="unipc", steps=4, orders=[1, 1, 2, 1])
    p = _pipe()                                                    # the keyword route on a pipeline built with nothing set
    p.initialize_buffer_embedder(16, zero_init=False)
    p.buffer_embedder.load_state_dict(syn.make_buffer_embedder_state_dict(CFG))
    kw = dict(prompt="a street", negative_prompt="bad", semantic_buffer_video=[Image.fromarray(f) for f in sem],
              coordinate_buffer_video=[Image.fromarray(f) for f in co], height=grid.height, width=grid.width, num_frames=grid.num_frames,
              seed=3, return_latents=True)
    want = p(**kw, sample_solver="unipc", num_inference_steps=4)
    assert p.solver_record == g.pipe.solver_record
    assert torch.equal(vae.last_decoded, want), "the environment must select what the keywords select"
    assert not torch.equal(want, p(**kw, num_inference_steps=4))
    # the step count alone: Euler steps, N of them
    g2, _, _ = generator_through_env(lambda torch_dtype, device, model_configs: _pipe(vae=vae), tmp_path, monkeypatch, grid, "cpu", ICV_SAMPLE_STEPS="4")
    assert g2.pipe.solver_record is None and torch.equal(vae.last_decoded, p(**kw, num_inference_steps=4))


# ---- 7. the C entry point's argument checks -------------------------------------------------------------------------------------------
def test_argument_errors_without_gpu():
    from infinicube_amd import native
    lib = native.lib()

    def call(**kw):
        a = dict(latent=0x1000, x_hat=0x2000, m_new=0x3000, m_prev=0x4000, m_prev2=0x5000, hc=0x6000, hu=0x7000, ldh=64, corrector=1,
                 a=(0.5, 0.25, 0.125, 0.125), c=(0.5, 0.25, 0.25), C=16, T=3, H8=6, W8=10, tok0=7, n_tok=23)
        a.update(kw)
        rc = lib.icv_unpatchify_cfg_multistep(a["latent"], a["x_hat"], a["m_new"], a["m_prev"], a["m_prev2"], a["hc"], a["hu"], a["ldh"], 5.0, 0.9,
                                              a["corrector"], *a["a"], *a["c"], a["C"], a["T"], a["H8"], a["W8"], a["tok0"], a["n_tok"], 0, None)
        return rc, lib.icv_last_error()

    for kw, msg in ((dict(latent=None), b"null argument"), (dict(x_hat=None), b"null argument"), (dict(m_new=None), b"null argument"),
                    (dict(hc=None), b"null argument"), (dict(H8=5), b"bad shape"), (dict(W8=9), b"bad shape"), (dict(n_tok=0), b"bad shape"),
                    (dict(C=0), b"bad shape"), (dict(ldh=63), b"ldh (63) is less than the 4 * C = 64 columns"),
                    (dict(tok0=23), b"token range"), (dict(tok0=-1), b"token range"),
                    (dict(m_prev=None), b"m_prev is NULL but its coefficient is not 0"),
                    (dict(m_prev=None, a=(0.5, 0.0, 0.0, 0.5)), b"m_prev is NULL but its coefficient is not 0"),       # c2 still reads it
                    (dict(m_prev2=None), b"m_prev2 is NULL but its coefficient is not 0"),
                    (dict(corrector=0), b"corrector coefficients given for a step without a corrector"),
                    (dict(m_new=0x4000), b"must differ"), (dict(x_hat=0x1000), b"must differ"), (dict(m_prev2=0x1000), b"must differ"),
                    (dict(x_hat=0x2004), b"8-byte aligned")):
        rc, err = call(**kw)
        assert rc != 0 and msg in err, (kw, rc, err)
