"""CFG-Zero* guidance (infinicube_amd/videogen/guidance.py) on CPU: the torch twin of icv_cfg_zero_scale_f32 against
closed forms, the host loop (dit.WanDiT.denoise(guidance=)) on the TEST-ONLY oracle operator set against a float64 restatement on
oracle.wan_ref forwards, the two exact cases (s = 1; zero-init = a later start), off = nothing new (bits, launches, allocations),
the scope and value errors, the two environment variables through the unchanged generator, and the C entry point's argument checks
(they run on the host, before any launch).

The loop test's inputs.  With the synthetic weights and contexts as they come the two CFG branches are almost parallel: s = 1.0000
at every step and plain CFG scores 102 dB against CFG-Zero*, so no bar could tell the rules apart.  GAINS below (the stiff state dict
of test_solver_cpu with every cross-attention output projection x 32, the cond context x 20, the uncond context a fresh draw at 20 x
the cond context's std) pull the branches apart.  Measured on the CPU oracle with these gains, Euler, 6 steps, CFG 5: restated
s = [0.9499, 0.9534, 0.9479, 0.9573, 0.9593, 0.9749]; restated plain CFG vs restated CFG-Zero* 32.5 dB; the engine loop vs restated
CFG-Zero* 54.9 dB with the CFG pair and 54.9 dB without (bar: 40 dB), its scales within 2e-4 of the restated ones."""
import contextlib
import io
import math
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from dit_launch_trace import Trace, TracedOps
from infinicube_amd.videogen import guidance as G
from infinicube_amd.videogen import solver as S
from infinicube_amd.videogen import synthetic as syn
from infinicube_amd.videogen import teacache
from infinicube_amd.videogen.config import TokenGrid
from infinicube_amd.videogen.dit import WanDiT
from infinicube_amd.videogen.pipeline import DiTHolder, WanVideoPipeline
from infinicube_amd.videogen.scheduler import FlowMatchScheduler, flow_match_sigmas
from infinicube_amd.videogen.seqpar import ShardPlan
from oracle import wan_ref as R
from standins import HashTextEncoder, PoolVAE
from test_solver_cpu import CFG, ENV, GRID, LOOP_STEPS, CountingVAE, SolverOps, generator_through_env, rb, restated_sample
from test_solver_cpu import inputs as solver_inputs

F32, F64 = torch.float32, torch.float64
WORKSPACE = 512                      # ICV_CFG_ZERO_WORKSPACE_DOUBLES
CFG_SCALE = 5.0
GAINS = dict(cross_attn_o=32.0, cond_context=20.0, uncond_context=20.0)


# ---- the CPU twin of icv_cfg_zero_scale_f32 -------------------------------------------------------------------------------------------
def cfg_zero_twin(hc, hu, n_tok, scale_out, round_bf16=False):
    """Torch twin of the kernel (include/icvideo.h): fp64 sums of exact products, one f32 quotient, one f32 multiply per element."""
    c, u = hc[:n_tok], hu[:n_tok]
    if round_bf16:
        c, u = rb(c), rb(u)
    num, den = (c.double() * u.double()).sum(), (u.double() * u.double()).sum()
    s = (num / (den + 1e-8)).to(F32)
    if round_bf16:
        s = rb(s)
    scale_out[0] = s
    hu[:n_tok] = rb(s * u) if round_bf16 else s * u


class ZeroOps(SolverOps):
    """SolverOps + the CPU twin of icv_cfg_zero_scale_f32; keeps each call's moments' denominator."""

    def __init__(self, device="cpu"):
        super().__init__(device)
        self.zero_calls = []

    def cfg_zero_scale(self, hc, hu, n_tok, workspace, scale_out, round_bf16=False):
        assert hc.dtype == F32 and hu.dtype == F32 and workspace.dtype == F64 and workspace.numel() >= WORKSPACE and scale_out.numel() == 1
        assert hc.stride(0) == hu.stride(0) and hc.data_ptr() != hu.data_ptr()
        self.zero_calls.append(float((hu[:n_tok].double() ** 2).sum()))
        cfg_zero_twin(hc, hu, n_tok, scale_out, round_bf16)


# ---- 1. the twin against closed forms -------------------------------------------------------------------------------------------------
def test_twin_against_closed_forms():
    g = torch.Generator().manual_seed(11)
    n, cols = 23, 64
    out = torch.zeros(1)
    u = torch.randn((n, cols), generator=g)
    # c = 2u: s = 2 |u|^2 / (|u|^2 + eps)
    hu = u.clone()
    cfg_zero_twin(2.0 * u, hu, n, out)
    uu = float((u.double() ** 2).sum())
    assert abs(float(out) - 2.0 * uu / (uu + 1e-8)) <= 2.0 ** -23 * 2.0 and abs(float(out) - 2.0) <= 1e-6
    assert torch.equal(hu, out * u)
    # <c, u> = 0: s = 0 and v = w c
    half = torch.randn((n, cols // 2), generator=g)
    u2, c2 = torch.cat([half, torch.zeros_like(half)], 1), torch.cat([torch.zeros_like(half), torch.randn((n, cols // 2), generator=g)], 1)
    hu = u2.clone()
    cfg_zero_twin(c2, hu, n, out)
    assert float(out) == 0.0 and torch.equal(hu, torch.zeros_like(hu))
    assert torch.equal(hu + CFG_SCALE * (c2 - hu), CFG_SCALE * c2)
    # random inputs: what is left of c after the projection is orthogonal to u
    c = 0.7 * u + 0.5 * torch.randn((n, cols), generator=g)
    hu = u.clone()
    cfg_zero_twin(c, hu, n, out)
    s = float(out)
    resid = float(((c.double() - s * u.double()) * u.double()).sum())
    assert abs(resid) <= 1e-6 * float(c.double().norm()) * float(u.double().norm()), resid
    assert abs(s - 0.7) < 0.1
    # rows beyond n_tok are neither summed nor scaled
    tall_c, tall_u = torch.cat([c, torch.full((3, cols), 9.0)]), torch.cat([u, torch.full((3, cols), 9.0)])
    cfg_zero_twin(tall_c, tall_u, n, out)
    assert float(out) == s and torch.equal(tall_u[n:], torch.full((3, cols), 9.0)) and torch.equal(tall_u[:n], hu)
    # u = 0: s = 0, finite
    hu = torch.zeros((n, cols))
    cfg_zero_twin(c, hu, n, out)
    assert float(out) == 0.0 and torch.equal(hu, torch.zeros((n, cols)))
    # reference rounding: s is a bf16 value, hu holds bf16 values
    hu = u.clone()
    cfg_zero_twin(c, hu, n, out, round_bf16=True)
    assert torch.equal(out, rb(out)) and torch.equal(hu, rb(hu)) and abs(float(out) - s) <= 2.0 ** -8 * abs(s) + 0.01


# ---- 2. the host loop against a float64 restatement -----------------------------------------------------------------------------------
_INPUTS = {}


def inputs():
    """test_solver_cpu.inputs() with GAINS applied -> (sd, bsd, noise, cond context, uncond context, buffer latents)."""
    if "v" not in _INPUTS:
        sd, bsd, noise, c1, _, bl = solver_inputs()
        sd = dict(sd)
        hit = [k for k in sd if k.endswith("cross_attn.o.weight")]
        assert len(hit) == CFG.num_layers
        for k in hit:
            sd[k] = sd[k] * GAINS["cross_attn_o"]
        cu = torch.randn(c1.shape, generator=torch.Generator().manual_seed(5)) * float(c1.std()) * GAINS["uncond_context"]
        _INPUTS["v"] = (sd, bsd, noise, c1 * GAINS["cond_context"], cu.to(c1.dtype), bl)
    return _INPUTS["v"]


def restated_scale(v_c, v_u):
    """s* of one step in float64 from the two f32 velocities."""
    c, u = v_c.double(), v_u.double()
    return float((c * u).sum() / ((u * u).sum() + 1e-8))


def oracle_velocity(sigmas, zero_star, scales=None, fp8=False, tea_skipped=()):
    """velocity(x, i) of restated_sample on oracle.wan_ref forwards, combined by plain CFG or by CFG-Zero* (float64); ``scales``
    collects s* per call.  ``tea_skipped``: DiffSynth's TeaCache bookkeeping on those steps (tests/test_solver_gpu.py)."""
    sd, bsd, noise, c1, c2, bl = inputs()
    rsd, rbsd = R.round_state_dict_to_bf16(sd), R.round_state_dict_to_bf16(bsd)
    buf = R.buffer_embed(rbsd, bl)
    ctxs = (R.text_embed(rsd, c1), R.text_embed(rsd, c2))
    grid = (noise.shape[1], noise.shape[2] // 2, noise.shape[3] // 2)
    freqs = R.rope_freqs_3d(CFG.head_dim, *grid)
    residual = [None, None]

    def branches(x, i):
        ts = float(sigmas[i]) * 1000.0
        if not tea_skipped:
            return [R.dit_forward(rsd, CFG, x.float(), c, ts, buf, fp8=fp8) for c in (c1, c2)]
        t, t_mod = R.time_embed(rsd, CFG, ts)
        vs = []
        for b in range(2):
            tok = R.patchify_tokens(x.float(), rsd["patch_embedding.weight"], rsd["patch_embedding.bias"]) + buf
            if i in tea_skipped:
                tok = tok + residual[b]
            else:
                before = tok.clone()
                for layer in range(CFG.num_layers):
                    tok = R.dit_block(rsd, CFG, layer, tok, ctxs[b], t_mod, freqs)
                residual[b] = tok - before
            vs.append(R.unpatchify(R.head(rsd, CFG, tok, t), grid, CFG.out_dim))
        return vs

    def v(x, i):
        v_c, v_u = branches(x, i)
        v_c, v_u = v_c.double(), v_u.double()
        if zero_star:
            s = restated_scale(v_c, v_u)
            if scales is not None:
                scales.append(s)
            v_u = s * v_u
        return v_u + CFG_SCALE * (v_c - v_u)
    return v


_REFS = {}


def reference(zero_star, solver="euler", steps=LOOP_STEPS, first=0, fp8=False, tea_skipped=()):
    """(latent, scales) of the restated loop on the oracle's forwards, computed once per setting."""
    key = (zero_star, solver, steps, first, fp8, tuple(tea_skipped))
    if key not in _REFS:
        sigmas, scales = flow_match_sigmas(steps), []
        lat = restated_sample(oracle_velocity(sigmas, zero_star, scales, fp8, tea_skipped), inputs()[2].double(), sigmas, solver, first=first)
        _REFS[key] = (lat.float(), scales)
    return _REFS[key]


def engine_loop(ops, zero_star=True, k=0, solver="euler", steps=LOOP_STEPS, setup=None, prep=None, dev="cpu", kw=None, tea=None,
                same_context=False, data=None, loop_steps=None, on_step=None):
    """dit.WanDiT.denoise on ``ops`` with the CFG-Zero* plan -> (engine, latent)."""
    sd, bsd, noise, c1, c2, bl = data or inputs()
    m = WanDiT(CFG, sd, ops, bsd, **(kw or {})).prepare(GRID, **(prep or {}))
    if setup is not None:
        setup(m)
    sch = FlowMatchScheduler(steps)
    lat = noise.clone().to(dev)
    extra = dict(solver=S.MultistepPlan(solver, sch.sigmas)) if solver != "euler" else {}
    if tea is not None:
        extra["tea_cache"] = tea(m, sch)
    plan = G.validate(zero_star, k, steps, CFG_SCALE)
    if plan is not None:
        extra["guidance"] = plan
    if loop_steps is not None:
        extra["steps"] = loop_steps
    m.denoise(lat, m.encode_context(c1), m.encode_context(c1 if same_context else c2), m.embed_buffers(bl), sch, CFG_SCALE,
              on_step=on_step, **extra)
    return m, lat


def check_loop(lat, scales, what, ref=None, plain=None, bar=40.0):
    """The three conditions of the loop test: >= ``bar`` dB against the restated CFG-Zero* loop; the restated plain-CFG loop at
    least 10 dB lower against it than the engine; every scale within a quarter of the restated scale's distance from 1."""
    ref_lat, ref_scales = ref or reference(True)
    plain_lat = (plain or reference(False))[0]
    p, p_plain = R.psnr(lat.cpu(), ref_lat), R.psnr(plain_lat, ref_lat)
    print(f"{what}: engine vs restated CFG-Zero* {p:.1f} dB; restated plain CFG vs restated CFG-Zero* {p_plain:.1f} dB")
    print(f"{what}: scales {[round(s, 4) for s in scales]}, restated {[round(s, 4) for s in ref_scales]}")
    assert p >= bar, f"{what}: {p:.1f} dB"
    assert p_plain <= p - 10.0, f"{what}: the bar cannot tell the rules apart: plain CFG {p_plain:.1f} dB, engine {p:.1f} dB"
    assert len(scales) == len(ref_scales)
    for i, (s, r) in enumerate(zip(scales, ref_scales)):
        assert abs(s - r) <= 0.25 * abs(1.0 - r), f"{what}: step {i}: s = {s:.5f}, restated {r:.5f} - not told apart from 'no scaling'"


@pytest.mark.parametrize("cfg_batch", [True, False])
def test_host_loop_matches_restated_cfg_zero_star(cfg_batch):
    """Tiny preset, 5 latent frames, CFG 5, Euler, 6 steps, the inputs of this file's header."""
    ops = ZeroOps()
    m, lat = engine_loop(ops, setup=lambda m: setattr(m, "cfg_batch", cfg_batch))
    assert (m._pair is not None) == cfg_batch and LOOP_STEPS == 6
    assert len(ops.zero_calls) == LOOP_STEPS and not ops.multistep_calls
    assert len(m.guidance_scales) == LOOP_STEPS
    check_loop(lat, m.guidance_scales, f"cfg_batch={cfg_batch}")
    work, out = m._guidance_state
    assert work.dtype == F64 and work.numel() == WORKSPACE and out.dtype == F32 and out.numel() == LOOP_STEPS
    # a second call reuses the buffers and gives the same bits; a longer one grows the scale array
    c1, c2, bl = inputs()[3:]
    again, sch = inputs()[2].clone(), FlowMatchScheduler(LOOP_STEPS)
    m.denoise(again, m.encode_context(c1), m.encode_context(c2), m.embed_buffers(bl), sch, CFG_SCALE, guidance=G.GuidancePlan(True, 0))
    assert m._guidance_state[1] is out and torch.equal(again, lat)
    m.denoise(again, m.encode_context(c1), m.encode_context(c2), m.embed_buffers(bl), FlowMatchScheduler(LOOP_STEPS + 1), CFG_SCALE,
              guidance=G.GuidancePlan(True, 0))
    assert m._guidance_state[1].numel() == LOOP_STEPS + 1 and len(m.guidance_scales) == LOOP_STEPS + 1


# ---- 3. exact: identical branches give s = 1 ------------------------------------------------------------------------------------------
def test_identical_branches_are_the_plain_path_bit_for_bit():
    """Both branches on one context, sequential forwards: c == u bit for bit, so s = sum u^2 / (sum u^2 + 1e-8), which rounds to
    exactly 1.0f once 1e-8 / sum u^2 < 2^-25 - guaranteed by sum u^2 > 1, checked on every step."""
    seq = lambda m: setattr(m, "cfg_batch", False)                                # noqa: E731
    ops = ZeroOps()
    m, lat = engine_loop(ops, setup=seq, same_context=True, data=solver_inputs())
    assert m._pair is None and len(ops.zero_calls) == LOOP_STEPS and all(d > 1.0 for d in ops.zero_calls), ops.zero_calls
    assert m.guidance_scales == [1.0] * LOOP_STEPS
    m0, lat0 = engine_loop(ZeroOps(), zero_star=False, setup=seq, same_context=True, data=solver_inputs())
    assert m0.guidance_scales is None and m0._guidance_state is None
    assert torch.equal(lat, lat0)


# ---- 4. exact: zero-init is a later start ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["euler", "unipc"])
@pytest.mark.parametrize("k", [1, 2])
def test_zero_init_is_a_later_start(solver, k):
    seen = []
    ops = ZeroOps()
    m, lat = engine_loop(ops, zero_star=False, k=k, solver=solver, data=solver_inputs(), on_step=lambda i, x: seen.append((i, x.clone())))
    m0, lat0 = engine_loop(ZeroOps(), zero_star=False, solver=solver, data=solver_inputs(), loop_steps=range(k, LOOP_STEPS))
    assert torch.equal(lat, lat0) and not ops.zero_calls
    noise = solver_inputs()[2]
    assert [i for i, _ in seen] == list(range(LOOP_STEPS))
    assert all(torch.equal(x, noise) for _, x in seen[:k]) and not torch.equal(seen[k][1], noise)
    assert m.guidance_scales == [None] * LOOP_STEPS and m._guidance_state is None
    if solver == "unipc":
        want = S.MultistepPlan("unipc", flow_match_sigmas(LOOP_STEPS)).steps(range(k, LOOP_STEPS))
        assert ops.multistep_calls == [(st.sigma, st.a, st.c) for st in want] and ops.multistep_calls[0][1] is None


def test_zero_init_records_through_the_pipeline(monkeypatch):
    """solver_record and the TeaCache plan are built over range(K, N): orders as for a call that starts at K, step K computed."""
    for key in ENV:
        monkeypatch.delenv(key, raising=False)
    p = _pipe()
    n, k = 6, 2
    lat = p(**_call_kw(num_inference_steps=n, sample_solver="unipc", cfg_zero_init_steps=k, tea_cache_l1_thresh=1e9,
                       tea_cache_model_id="Wan2.1-T2V-1.3B"))
    assert p.solver_record == S.MultistepPlan("unipc", flow_match_sigmas(n)).record(range(k, n)) and p.solver_record["steps"] == n - k
    assert p.tea_cache_record["computed"] == [k, n - 1], "step K is the first step of the plan: computed"
    assert p.guidance_record == dict(optimized_scale=False, zero_init_steps=k, scales=[None] * n)
    assert torch.isfinite(lat).all()
    both = p(**_call_kw(num_inference_steps=n, cfg_zero_star=True, cfg_zero_init_steps=k))
    rec = p.guidance_record
    assert rec["optimized_scale"] and rec["scales"][:k] == [None] * k and all(math.isfinite(s) for s in rec["scales"][k:]) and len(rec["scales"]) == n
    assert not torch.equal(both, p(**_call_kw(num_inference_steps=n))) and p.guidance_record is None


# ---- 5. off means nothing new ---------------------------------------------------------------------------------------------------------
def _pipe(ops=None, vae=None, dtype=torch.bfloat16):
    return WanVideoPipeline("cpu", dtype, DiTHolder(syn.make_dit_state_dict(CFG), CFG), HashTextEncoder(CFG), vae or PoolVAE(),
                            ops=ops or ZeroOps())


def _call_kw(**extra):
    kw = dict(prompt="a street", negative_prompt="bad", height=GRID.height, width=GRID.width, num_frames=GRID.num_frames, seed=3,
              num_inference_steps=3, return_latents=True)
    kw.update(extra)
    return kw


class TracedZeroOps(TracedOps):
    """TracedOps + the twin: the new op shows in the log."""

    def cfg_zero_scale(self, hc, hu, n_tok, workspace, scale_out, round_bf16=False):
        cfg_zero_twin(hc, hu, n_tok, scale_out, round_bf16)


def test_off_is_the_plain_path(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)

    def run(ops_cls, **kw):
        tr = Trace()
        ops = ops_cls(tr)                         # TracedOps has no cfg_zero_scale: calling it would raise
        p = _pipe(ops)
        allocs, raw = [], ops.alloc
        monkeypatch.setattr(ops, "alloc", lambda shape, dtype: (allocs.append((tuple(shape), dtype)), raw(shape, dtype))[1])
        tr.on = True
        lat = p(**_call_kw(**kw))
        tr.on = False
        return tr.log, allocs, lat, p

    log0, allocs0, lat0, _ = run(TracedOps)
    assert sum(e[0] == "unpatchify_cfg_euler" for e in log0) == 3
    for kw in (dict(cfg_zero_star=None, cfg_zero_init_steps=None), dict(cfg_zero_star=False), dict(cfg_zero_init_steps=0),
               dict(cfg_zero_star=False, cfg_zero_init_steps=0)):
        log1, allocs1, lat1, p = run(TracedOps, **kw)
        assert p.guidance_record is None and p._engine._guidance_state is None and p._engine.guidance_scales is None
        assert torch.equal(lat1, lat0) and log1 == log0 and allocs1 == allocs0, f"{kw} must be the path without the keywords"
    # on: exactly one more op per executed CFG step, right in front of the update, and the two buffers after everything else
    log2, allocs2, lat2, p = run(TracedZeroOps, cfg_zero_star=True)
    names0, names2 = [e[0] for e in log0], [e[0] for e in log2]
    assert [n for n in names2 if n != "cfg_zero_scale"] == names0 and names2.count("cfg_zero_scale") == 3
    assert all(names2[j + 1] == "unpatchify_cfg_euler" for j, n in enumerate(names2) if n == "cfg_zero_scale")
    assert allocs2 == allocs0 + [((WORKSPACE,), F64), ((3,), F32)]
    assert p.cfg_zero_star is None and p.guidance_record["optimized_scale"] and len(p.guidance_record["scales"]) == 3
    assert p.guidance_record["scales"] == p._engine.guidance_scales and all(math.isfinite(s) for s in p.guidance_record["scales"])
    # zero-init alone: the skipped step's launches are gone, nothing else changes, nothing is allocated for it
    log3, allocs3, _, p = run(TracedOps, cfg_zero_init_steps=1)
    assert sum(e[0] == "unpatchify_cfg_euler" for e in log3) == 2 and len(log3) < len(log0) and p._engine._guidance_state is None
    assert p.guidance_record == dict(optimized_scale=False, zero_init_steps=1, scales=[None, None, None])
    # a keyword does not outlive its call
    p = _pipe()
    p(**_call_kw(cfg_zero_star=True, cfg_zero_init_steps=1))
    assert p.guidance_record["zero_init_steps"] == 1
    base = p(**_call_kw())
    assert p.guidance_record is None and (p.cfg_zero_star, p.cfg_zero_init_steps) == (None, None) and torch.equal(base, lat0)


# ---- 6. scope and value errors --------------------------------------------------------------------------------------------------------
def test_value_errors(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    assert G.validate(None, None, 6, 5.0) is None and G.validate(False, 0, 6, 5.0) is None
    assert G.validate(True, None, 6, 5.0) == G.GuidancePlan(True, 0) and G.validate(None, 5, 6, 1.0) == G.GuidancePlan(False, 5)
    p = _pipe()
    monkeypatch.setattr(p, "_get_engine", lambda: pytest.fail("the engine was built before the settings were validated"))
    with pytest.raises(ValueError, match="cfg_zero_star needs classifier-free guidance"):
        p(**_call_kw(cfg_zero_star=True, cfg_scale=1.0))
    for bad in (3, 4):
        with pytest.raises(ValueError, match=f"cfg_zero_init_steps={bad} leaves no step to run"):
            p(**_call_kw(cfg_zero_init_steps=bad))
    for bad in (-1, 1.0, "1", True):
        with pytest.raises(ValueError, match=r"cfg_zero_init_steps must be an integer >= 0"):
            p(**_call_kw(cfg_zero_init_steps=bad))
    for bad in (1, "yes"):
        with pytest.raises(ValueError, match="cfg_zero_star must be a bool"):
            p(**_call_kw(cfg_zero_star=bad))
    for bad in ("2", "true", "yes", " "):
        monkeypatch.setenv(G.ENV_STAR, bad)
        with pytest.raises(ValueError, match="ICV_CFG_ZERO_STAR must be 0 or 1"):
            _pipe()
    monkeypatch.setenv(G.ENV_STAR, "0")
    assert _pipe().cfg_zero_star is False
    monkeypatch.setenv(G.ENV_STAR, "1")
    assert _pipe().cfg_zero_star is True
    for bad in ("-1", "1.5", "two", " "):
        monkeypatch.setenv(G.ENV_INIT_STEPS, bad)
        with pytest.raises(ValueError, match="ICV_CFG_ZERO_INIT_STEPS must be an integer >= 0"):
            _pipe()
    monkeypatch.setenv(G.ENV_INIT_STEPS, "2")
    assert _pipe().cfg_zero_init_steps == 2


def test_scope_errors(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    p = _pipe()
    monkeypatch.setattr(p, "_get_engine", lambda: pytest.fail("the engine was built before the settings were validated"))
    for on in (dict(cfg_zero_star=True), dict(cfg_zero_init_steps=1)):
        with pytest.raises(ValueError, match="cfg_zero_star / cfg_zero_init_steps cannot be combined with sliding_window_size.* yet"):
            p(**_call_kw(sliding_window_size=3, sliding_window_stride=2, **on))
    # one sliding window is no combination
    p = _pipe()
    one = p(**_call_kw(cfg_zero_star=True, sliding_window_size=GRID.T, sliding_window_stride=GRID.T))
    assert p.sliding_window_record is None and torch.equal(one, p(**_call_kw(cfg_zero_star=True)))
    # the engine says the same when it is driven directly, before any launch
    sd, bsd, noise, c1, c2, bl = solver_inputs()
    sch = FlowMatchScheduler(2)
    plan = G.GuidancePlan(True, 0)
    from infinicube_amd.videogen import sliding_window as SW
    ops = ZeroOps()
    m = WanDiT(CFG, sd, ops, bsd).prepare(TokenGrid(9, 64, 96))
    with pytest.raises(ValueError, match="cannot be combined with more than one sliding temporal window yet"):
        m.denoise(noise.clone(), None, None, None, sch, 5.0, sliding_window=SW.plan(GRID.T, 3, 2), guidance=plan)
    msp = WanDiT(CFG, sd, ops, bsd).prepare(GRID, force_sp=True)
    with pytest.raises(ValueError, match=r"cannot be combined with sequence / CFG-branch parallelism \(world > 1\).* yet"):
        msp.denoise(noise.clone(), None, None, None, sch, 5.0, guidance=plan)
    m = WanDiT(CFG, sd, ops, bsd).prepare(GRID)
    with pytest.raises(ValueError, match=r"cannot be combined with sequence / CFG-branch parallelism \(world > 1\).* yet"):
        m.denoise(noise.clone(), m.encode_context(c1), None, None, sch, 5.0, branch_exchange=lambda own, both: None, guidance=plan)
    with pytest.raises(ValueError, match="cfg_zero_star needs classifier-free guidance"):
        m.denoise(noise.clone(), m.encode_context(c1), None, None, sch, 5.0, guidance=plan)
    with pytest.raises(ValueError, match="cfg_zero_star needs classifier-free guidance"):
        m.denoise(noise.clone(), m.encode_context(c1), m.encode_context(c2), None, sch, 1.0, guidance=plan)
    assert not ops.zero_calls and m._guidance_state is None


def _two_rank_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.set_num_threads(2)
        got = []
        p = _pipe()
        p._get_engine = lambda: got.append("the engine was built before the settings were validated")
        for on in (dict(cfg_zero_star=True), dict(cfg_zero_init_steps=1)):
            try:
                p(**_call_kw(**on))
                got.append("no error")
            except ValueError as e:
                got.append(str(e))
        sd, bsd, noise, c1, c2, bl = solver_inputs()
        m = WanDiT(CFG, sd, ZeroOps(), bsd).prepare(GRID, ShardPlan.make(GRID.S, world, rank), kv_exchange="allgather")
        try:
            m.denoise(noise.clone(), None, None, None, FlowMatchScheduler(2), 5.0, guidance=G.GuidancePlan(True, 0))
            got.append("no error")
        except ValueError as e:
            got.append(str(e))
        q.put((rank, got))
    finally:
        dist.destroy_process_group()


def test_two_ranks_raise():
    """A real gloo group of two ranks: the pipeline and the engine both refuse, on every rank, before any work."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() + 1381) % 2000
    procs = [ctx.Process(target=_two_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    got = dict(q.get(timeout=300) for _ in range(2))
    for pr in procs:
        pr.join(timeout=60)
        assert pr.exitcode == 0
    for rank in (0, 1):
        a, b, c = got[rank]
        for msg in (a, b):
            assert "cfg_zero_star / cfg_zero_init_steps cannot be combined with a process group of 2 ranks yet" in msg, got
        assert "cannot be combined with sequence / CFG-branch parallelism (world > 1)" in c and c.endswith(" yet"), got


def test_worker_pool_combination_raises(monkeypatch):
    """ICV_WORLD > 1 behind the unchanged generator: refused in the client before a request reaches the ranks."""
    from infinicube_amd.videogen.inference import WanVideoGenerator
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    sem, co = syn.make_dummy_buffers(TokenGrid(9, 64, 96))
    for attr, value in (("cfg_zero_star", True), ("cfg_zero_init_steps", 2)):
        g = WanVideoGenerator.__new__(WanVideoGenerator)
        g._pool, g.pipe = object(), _pipe()
        setattr(g.pipe, attr, value)
        with pytest.raises(ValueError, match="ICV_CFG_ZERO_STAR / ICV_CFG_ZERO_INIT_STEPS.*ICV_WORLD > 1"):
            g.generate(sem, co, seed=0)


def test_generator_through_the_environment(tmp_path, monkeypatch):
    from PIL import Image
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    grid = TokenGrid(9, 64, 96)
    vae = CountingVAE()
    g, sem, co = generator_through_env(lambda torch_dtype, device, model_configs: _pipe(vae=vae), tmp_path, monkeypatch, grid, "cpu",
                                       ICV_CFG_ZERO_STAR="1", ICV_CFG_ZERO_INIT_STEPS="1", ICV_SAMPLE_STEPS="4")
    assert (g.pipe.cfg_zero_star, g.pipe.cfg_zero_init_steps, g.pipe.num_inference_steps) == (True, 1, 4)
    rec = g.pipe.guidance_record
    assert rec["optimized_scale"] is True and rec["zero_init_steps"] == 1 and rec["scales"][0] is None and len(rec["scales"]) == 4
    assert all(math.isfinite(s) for s in rec["scales"][1:])
    p = _pipe()                                                    # the keyword route on a pipeline built with nothing set
    p.initialize_buffer_embedder(16, zero_init=False)
    p.buffer_embedder.load_state_dict(syn.make_buffer_embedder_state_dict(CFG))
    kw = dict(prompt="a street", negative_prompt="bad", semantic_buffer_video=[Image.fromarray(f) for f in sem],
              coordinate_buffer_video=[Image.fromarray(f) for f in co], height=grid.height, width=grid.width, num_frames=grid.num_frames,
              seed=3, return_latents=True, num_inference_steps=4)
    want = p(**kw, cfg_zero_star=True, cfg_zero_init_steps=1)
    assert p.guidance_record == rec
    assert torch.equal(vae.last_decoded, want), "the environment must select what the keywords select"
    assert not torch.equal(want, p(**kw))


# ---- 7. the C entry point's argument checks -------------------------------------------------------------------------------------------
def test_argument_errors_without_gpu():
    from infinicube_amd import native
    lib = native.lib()
    assert native.CFG_ZERO_WORKSPACE_DOUBLES == WORKSPACE

    def call(**kw):
        a = dict(hc=0x1000, hu=0x2000, ldh=64, rows=23, cols=64, workspace=0x3000, scale_out=0x4000)
        a.update(kw)
        rc = lib.icv_cfg_zero_scale_f32(a["hc"], a["hu"], a["ldh"], a["rows"], a["cols"], a["workspace"], a["scale_out"], 0, None)
        return rc, lib.icv_last_error()

    for kw, msg in ((dict(hc=None), b"null argument"), (dict(hu=None), b"null argument"), (dict(workspace=None), b"null argument"),
                    (dict(scale_out=None), b"null argument"), (dict(rows=0), b"bad shape"), (dict(cols=0), b"bad shape"),
                    (dict(rows=-1), b"bad shape"), (dict(ldh=63), b"ldh (63) is less than the 64 columns of a row"),
                    (dict(hu=0x1000), b"hc and hu must differ"), (dict(workspace=0x3004), b"workspace must be 8-byte aligned"),
                    (dict(hu=0x2002), b"4-byte aligned")):
        rc, err = call(**kw)
        assert rc != 0 and msg in err, (kw, rc, err)
