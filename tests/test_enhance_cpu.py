"""Enhance-A-Video (infinicube_amd/videogen/enhance.py) on CPU: the torch twins of icv_enhance_scores_bf16 and
icv_enhance_apply_bf16 against closed forms, the host loop (dit.WanDiT.denoise(enhance=)) on the TEST-ONLY oracle operator set
against the restated loop (tests/enhance_ref.py), off = nothing new (bits, launches, allocations), every ValueError before any
operator runs, the attribute route through the unchanged generator, the record, the graph cache's key, the compositions that need no
GPU (CFG-Zero*, input_video / input_mask, NAG, UniPC, TeaCache), and the C entry points' argument checks (they run on the host,
before any launch).

The loop test's inputs.  With the synthetic weights as they come, self-attention moves the residual stream so little that a loop
which ignored ``enhance_weight`` would still pass the 40 dB bar (restated plain vs restated enhanced loop: 58.6 dB at weight 4).
GAINS below (the stiff state dict of test_solver_cpu with every self-attention and cross-attention output projection x 32 and the
positive context x 20, so that the CFG branches part behind layer 0) make it matter.  Measured on the CPU oracle with these gains,
Euler, 6 steps, cfg_scale 5, enhance_weight 4: restated plain loop vs restated enhanced loop 21.5 dB (asserted < 30 dB); the engine loop
vs the restated enhanced loop 54.4 dB (bar: 40 dB).  The query norm keeps the model's own weight (gain 1): the bf16 planes of the engine
and the f32 q, k of the restatement give E values 1e-4 apart there, and a sharper softmax (x 4) moves them 7e-4 apart - the
distance between two trajectories, not an error of the kernels, which check_scores bounds on the engine's own q, k."""
import math

import numpy as np
import pytest
import torch

from dit_launch_trace import Trace, TracedOps
from enhance_ref import (BF16, LN2, EnhanceForward, EnhanceMixin, EnhanceOps, ScoreRecorder, enhance_apply_twin, enhance_bound, enhance_factor_twin,
                         enhance_rule, enhance_scores_twin, enhance_velocity)
from infinicube_amd.videogen import enhance as E
from infinicube_amd.videogen import nag as N
from infinicube_amd.videogen import solver as S
from infinicube_amd.videogen import synthetic as syn
from infinicube_amd.videogen.config import TokenGrid
from infinicube_amd.videogen.dit import WanDiT
from infinicube_amd.videogen.pipeline import DiTHolder, WanVideoPipeline
from infinicube_amd.videogen.scheduler import FlowMatchScheduler, flow_match_sigmas
from oracle import wan_ref as R
from standins import HashTextEncoder, PoolVAE
from test_solver_cpu import CFG, ENV, GRID, LOOP_STEPS, CountingVAE, generator_through_env, restated_sample
from test_solver_cpu import inputs as solver_inputs

F32, F64 = torch.float32, torch.float64
WEIGHT = 4.0
CFG_SCALE = 5.0
GAINS = dict(self_attn_o=32.0, cross_attn_o=32.0, self_attn_norm_q=1.0, cond_context=20.0)
NAG = (11.0, 2.5, 0.25)
LOG2E_RSQRT_HD = math.log2(math.e) / math.sqrt(128.0)      # what the engine folds into k


# ---- 1. the twins against closed forms ------------------------------------------------------------------------------------------------
def twin_E(q, k, T, P, H, weight, scale=LN2):
    ws = torch.zeros(P, dtype=F32)
    enhance_scores_twin(q, k, T, P, H, scale, ws)
    return enhance_factor_twin(ws, T, P, H, weight), ws


def one_hot_logits(T, P, H, shift, peak=30.0):
    """q, k bf16 [T * P, H * 128] with <q[(t, s), h], k[(t', s), h]> = peak where t' == (t + shift) % T and 0 elsewhere: frame t's
    query is peak * e_t, frame t's key is e_(t - shift)."""
    q, k = torch.zeros((T, P, H, 128)), torch.zeros((T, P, H, 128))
    for t in range(T):
        q[t, :, :, t] = peak
        k[t, :, :, (t - shift) % T] = 1.0
    return q.reshape(T * P, H * 128).to(BF16), k.reshape(T * P, H * 128).to(BF16)


@pytest.mark.parametrize("T,P,H", [(2, 1, 1), (5, 3, 2), (21, 4, 3), (32, 2, 1)])
def test_twin_against_closed_forms(T, P, H):
    for w in (0.0, WEIGHT, 10.5):
        # q = k = const: uniform attention, m = 1 / T, E = 1 + w / T
        q = torch.full((T * P, H * 128), 0.25, dtype=BF16)
        got, ws = twin_E(q, q.clone(), T, P, H, w)
        assert abs(got - max(1.0, 1.0 + w / T)) <= 4 * 2.0 ** -24 * (1.0 + w / T)
        assert torch.allclose(ws, torch.full((P,), H * T * (T - 1) / T), rtol=2.0 ** -22)
        assert abs(enhance_rule(q, q, T, P, H, LN2, w)[0] - (1.0 + w / T)) <= 1e-12
        # one-hot diagonal logits: nothing looks across frames, E = 1 and att keeps its bits
        q, k = one_hot_logits(T, P, H, 0, peak=200.0)
        got, ws = twin_E(q, k, T, P, H, w)
        assert got == 1.0 and enhance_rule(q, k, T, P, H, LN2, w)[0] == 1.0
        att = torch.randn((T * P, H * 128), generator=torch.Generator().manual_seed(T)).to(BF16)
        att[0, 0], att[0, 1] = float("inf"), -0.0
        want, out = att.clone(), torch.zeros(1, dtype=F32)
        enhance_apply_twin(att, ws, T, P, H, w, out)
        assert float(out) == 1.0 and torch.equal(att.view(torch.int16), want.view(torch.int16))
        # one-hot off-diagonal logits: everything looks at ONE other frame, the ceiling E = (T + w) / (T - 1)
        q, k = one_hot_logits(T, P, H, 1, peak=200.0)
        got, _ = twin_E(q, k, T, P, H, w)
        top = (T + w) / (T - 1)
        assert abs(got - top) <= 4 * 2.0 ** -24 * top and abs(enhance_rule(q, k, T, P, H, LN2, w)[0] - top) <= 1e-12


def test_twin_matches_the_rule_and_applies_one_rounding():
    T, P, H = 5, 7, 2
    g = torch.Generator().manual_seed(3)
    q = torch.randn((T * P, H * 128), generator=g).to(BF16)
    k = (torch.randn((T * P, H * 128), generator=g) * LOG2E_RSQRT_HD * 3.0).to(BF16)
    want, m, absdot = enhance_rule(q, k, T, P, H, LN2, WEIGHT)
    got, ws = twin_E(q, k, T, P, H, WEIGHT)
    assert 1.0 < want < (T + WEIGHT) / (T - 1) and tuple(m.shape) == (P, H)
    assert abs(got - want) <= enhance_bound(absdot) * want
    att = torch.randn((T * P, H * 128), generator=g).to(BF16)
    before, out = att.clone(), torch.zeros(1, dtype=F32)
    enhance_apply_twin(att, ws, T, P, H, WEIGHT, out)
    assert float(out) == got and torch.equal(att, (before.float() * float(out)).to(BF16)) and not torch.equal(att, before)


# ---- 2. the host loop against the restated loop ---------------------------------------------------------------------------------------
_INPUTS = {}


def inputs(gains=None):
    """test_solver_cpu.inputs() with ``gains`` (GAINS) applied -> (sd, bsd, noise, cond context, uncond context, buffer latents)."""
    gains = dict(GAINS, **(gains or {}))
    key = tuple(sorted(gains.items()))
    if key not in _INPUTS:
        sd, bsd, noise, c1, c2, bl = solver_inputs()
        sd = dict(sd)
        for suffix, gain in (("self_attn.o.weight", "self_attn_o"), ("cross_attn.o.weight", "cross_attn_o"),
                             ("self_attn.norm_q.weight", "self_attn_norm_q")):
            hit = [k for k in sd if k.endswith(suffix)]
            assert len(hit) == CFG.num_layers
            for k in hit:
                sd[k] = sd[k] * gains[gain]
        _INPUTS[key] = (sd, bsd, noise, c1 * gains["cond_context"], c2, bl)
    return _INPUTS[key]


_REFS = {}


def reference(weight=WEIGHT, solver="euler", steps=LOOP_STEPS, fp8=False, tea_skipped=(), window=None, nag=None, cfg_scale=CFG_SCALE, gains=None):
    """(the restated loop's latent, [E per layer] per branch and [max sum |q k|] per branch of its last computed forward), once per
    setting.  ``weight`` None: the plain loop.  ``nag``: cfg_scale 1, one forward per step with the uncond context as the negative."""
    key = (weight, solver, steps, fp8, tuple(tea_skipped), window, nag, cfg_scale, tuple(sorted((gains or {}).items())))
    if key not in _REFS:
        sd, bsd, noise, cc, cu, bl = inputs(gains)
        rsd, rbsd = R.round_state_dict_to_bf16(sd), R.round_state_dict_to_bf16(bsd)
        sigmas = flow_match_sigmas(steps)
        kw = dict(fp8=fp8, window=window, tea_skipped=tea_skipped)
        buf = R.buffer_embed(rbsd, bl)
        if nag is not None:
            fwd = [EnhanceForward(rsd, CFG, cc, weight, buf, neg_context=cu, nag=nag, **kw)]
        else:
            fwd = [EnhanceForward(rsd, CFG, c, weight, buf, **kw) for c in ((cc, cu) if cfg_scale != 1.0 else (cc,))]
        lat = restated_sample(enhance_velocity(fwd, sigmas, cfg_scale), noise.double(), sigmas, solver).float()
        _REFS[key] = (lat, [f.scores for f in fwd], [f.absdots for f in fwd])
    return _REFS[key]


def engine_loop(ops, weight=WEIGHT, solver="euler", steps=LOOP_STEPS, setup=None, prep=None, dev="cpu", kw=None, tea=None, nag=None,
                cfg_scale=CFG_SCALE, engine=None, gains=None):
    """dit.WanDiT.denoise on ``ops`` with the plan (``weight`` None: the plain call) -> (engine, latent).  An ``engine`` from an earlier
    call runs again on the SAME context objects, buffer tokens and latent tensor (what a graph is keyed on)."""
    sd, bsd, noise, cc, cu, bl = inputs(gains)
    m = engine or WanDiT(CFG, sd, ops, bsd, **(kw or {})).prepare(GRID, **(prep or {}))
    if setup is not None:
        setup(m)
    if engine is None:
        m.test_recorder = ScoreRecorder(ops) if not m._graphs_on else None      # its host copies cannot run inside a graph capture
        m.test_operands = (m.encode_context(cc), m.encode_context(cu), m.embed_buffers(bl), noise.clone().to(dev))
    ctx_c, ctx_u, buf, lat = m.test_operands
    lat.copy_(noise)
    sch = FlowMatchScheduler(steps)
    extra = dict(solver=S.MultistepPlan(solver, sch.sigmas)) if solver != "euler" else {}
    if tea is not None:
        extra["tea_cache"] = tea(m, sch)
    if weight is not None:
        extra["enhance"] = E.EnhancePlan(weight)
    if nag is not None:
        extra["nag"] = N.NagPlan(ctx_u, *nag)
        m.denoise(lat, ctx_c, None, buf, sch, 1.0, **extra)
    else:
        m.denoise(lat, ctx_c, ctx_u if cfg_scale != 1.0 else None, buf, sch, cfg_scale, **extra)
    return m, lat.clone()


def check_loop(lat, what, ref=None, bar=40.0):
    """>= ``bar`` dB against the restated enhanced loop."""
    ref = reference()[0] if ref is None else ref
    p = R.psnr(lat.cpu(), ref)
    print(f"{what}: engine vs restated enhanced loop {p:.1f} dB")
    assert p >= bar, f"{what}: {p:.1f} dB"
    return p


def check_scores(m, ref, what):
    """The record of the call.  Asserted: every E against the float64 rule on the engine's own q, k of that launch, within the kernel
    bound (enhance_ref.ScoreRecorder).  Printed: E against the restated loop's, whose q, k are f32 values of another trajectory - the
    engine's bf16 planes differ from them by more than the kernels' own error (tests/test_enhance_gpu.py asserts that one)."""
    got, (_, scores, absdots) = m.enhance_scores, ref
    assert got is not None and len(got) == len(scores) and all(len(g) == CFG.num_layers for g in got)
    m.test_recorder.check(m, what)
    worst = 0.0
    for b, (gb, sb, ab) in enumerate(zip(got, scores, absdots)):
        for i, (g, s, a) in enumerate(zip(gb, sb, ab)):
            err, bound = abs(g - s) / s, enhance_bound(a)
            worst = max(worst, err / bound)
            print(f"{what}: branch {b} layer {i}: E {g:.7f}, restated loop {s:.7f}, relative error {err:.2e}, kernel bound {bound:.2e}")
            assert err <= 2.0 ** -8, "E is a mean of softmax weights of logits taken from bf16 planes: one bf16 ulp at the very most"
    return worst


def test_restated_loops_are_told_apart():
    p_plain = R.psnr(reference(None)[0], reference()[0])
    print(f"restated plain loop vs restated enhanced loop: {p_plain:.1f} dB")
    assert p_plain < 30.0, f"the 40 dB bar could pass with the feature ignored: plain vs enhanced {p_plain:.1f} dB"
    sc = reference()[1]
    assert sc[0][0] == sc[1][0] and sc[0][1] != sc[1][1], "layer 0 sees no context; behind it every CFG branch has its own E"
    assert all(1.0 < e < (GRID.T + WEIGHT) / (GRID.T - 1) for b in sc for e in b)


@pytest.mark.parametrize("cfg_batch", [True, False])
def test_host_loop_matches_restated_loop(cfg_batch):
    """Tiny preset, 5 latent frames, CFG 5 (a pair: each branch its own E), Euler, LOOP_STEPS steps."""
    ops = EnhanceOps()
    m, lat = engine_loop(ops, setup=lambda m: setattr(m, "cfg_batch", cfg_batch))
    assert (m._pair is not None) == cfg_batch
    check_loop(lat, f"CPU operator set, cfg_batch={cfg_batch}")
    T, P, H, L = GRID.T, GRID.tokens_per_frame, CFG.num_heads, CFG.num_layers
    per_forward = 2 * (2 * L - 1)          # both branches in every layer but the shared layer 0: scores, then apply
    assert m.share_stem and len(ops.enhance_calls) == LOOP_STEPS * per_forward
    assert all(c[1:] == (T, P, H, WEIGHT) for c in ops.enhance_calls)
    assert [c[0] for c in ops.enhance_calls[:4]] == ["scores", "apply", "scores", "apply"]
    assert m._enhance is None and m._enhance_slot == 0
    buf = m._enhance_E
    assert buf.dtype == F32 and tuple(buf.shape) == (2, L)
    ws = (m._pair if cfg_batch else m)._enhance_ws
    assert ws.dtype == F32 and ws.numel() == P
    check_scores(m, reference(), f"cfg_batch={cfg_batch}")
    assert m.enhance_scores[0][0] == m.enhance_scores[1][0] and m.enhance_scores[0][1] != m.enhance_scores[1][1]
    _, again = engine_loop(ops, engine=m)
    assert m._enhance_E is buf and torch.equal(again, lat), "the buffers are allocated once"
    _, plain = engine_loop(ops, weight=None, engine=m)
    assert m.enhance_scores is None and R.psnr(plain, reference(None)[0]) >= 40.0


def test_single_forward_and_unshared_stem():
    ops = EnhanceOps()
    m, lat = engine_loop(ops, cfg_scale=1.0)
    check_loop(lat, "cfg_scale 1", ref=reference(cfg_scale=1.0)[0])
    assert len(m.enhance_scores) == 1 and len(ops.enhance_calls) == LOOP_STEPS * 2 * CFG.num_layers
    check_scores(m, reference(cfg_scale=1.0), "cfg_scale 1")
    for batch in (True, False):
        def setup(m, batch=batch):
            m.cfg_batch, m.share_stem = batch, False
        ops = EnhanceOps()
        m, lat = engine_loop(ops, setup=setup)
        check_loop(lat, f"cfg_batch={batch}, no shared stem")
        assert len(ops.enhance_calls) == LOOP_STEPS * 4 * CFG.num_layers
        check_scores(m, reference(), f"cfg_batch={batch}, no shared stem")


# ---- 3. compositions that need no GPU -------------------------------------------------------------------------------------------------
def test_with_unipc():
    m, lat = engine_loop(EnhanceOps(), solver="unipc")
    check_loop(lat, "UniPC", ref=reference(solver="unipc")[0])


def test_with_teacache_one_forced_skip():
    """Step 3 of 6 runs no blocks, so no measurement and no scaling: the residual of step 2 (computed with the feature) is added."""
    from infinicube_amd.videogen import teacache
    computed = (0, 1, 2, 4, 5)
    plan = lambda m, sch: teacache.TeaCachePlan("test-linear", 0.0, tuple(range(LOOP_STEPS)), (0.0,) * LOOP_STEPS, computed)      # noqa: E731
    ops = EnhanceOps()
    m, lat = engine_loop(ops, tea=plan)
    ref = reference(tea_skipped=(3,))
    check_loop(lat, "TeaCache (step 3 skipped)", ref=ref[0])
    assert len(ops.enhance_calls) == len(computed) * 2 * (2 * CFG.num_layers - 1)
    assert not torch.equal(ref[0], reference()[0]), "the skip must change the restated result"
    check_scores(m, ref, "TeaCache")


def test_with_nag():
    """Normalized Attention Guidance in the same forward (cfg_scale 1): the self-attention output is scaled, the text cross-attention
    output is combined, both restated in one block."""
    m, lat = engine_loop(EnhanceOps(), nag=NAG)
    ref = reference(nag=NAG, cfg_scale=1.0)
    check_loop(lat, "NAG", ref=ref[0])
    p_plain = R.psnr(reference(None, nag=NAG, cfg_scale=1.0)[0], ref[0])
    assert p_plain < 30.0, f"NAG alone vs NAG + enhance {p_plain:.1f} dB"
    check_scores(m, ref, "NAG")


def test_with_the_frame_window():
    """Window 1 + 1 anchor frame: the attention is masked, E is still taken over all T frames."""
    m, lat = engine_loop(EnhanceOps(), setup=lambda m: m.set_attention_window(1, 1))
    assert m._framewin() == (1, 1)
    ref = reference(window=(1, 1))
    check_loop(lat, "frame window", ref=ref[0])
    check_scores(m, ref, "frame window")
    assert not torch.equal(ref[0], reference()[0])


# ---- 4. the pipeline: off, errors, attributes, record ---------------------------------------------------------------------------------
def _pipe(ops=None, vae=None, dtype=torch.bfloat16):
    return WanVideoPipeline("cpu", dtype, DiTHolder(syn.make_dit_state_dict(CFG), CFG), HashTextEncoder(CFG), vae or PoolVAE(),
                            ops=ops or EnhanceOps())


def _call_kw(**extra):
    kw = dict(prompt="a street", negative_prompt="bad", height=GRID.height, width=GRID.width, num_frames=GRID.num_frames, seed=3,
              num_inference_steps=3, return_latents=True)
    kw.update(extra)
    return kw


class TracedEnhanceOps(EnhanceMixin, TracedOps):
    """TracedOps + the twins: the new ops show in the log."""


def test_off_is_the_plain_path(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)

    def run(ops_cls, **kw):
        tr = Trace()
        ops = ops_cls(tr)                         # TracedOps has no enhance_scores: calling it would raise
        p = _pipe(ops)
        allocs, raw = [], ops.alloc
        monkeypatch.setattr(ops, "alloc", lambda shape, dtype: (allocs.append((tuple(shape), dtype)), raw(shape, dtype))[1])
        tr.on = True
        lat = p(**_call_kw(**kw))
        tr.on = False
        return tr.log, allocs, lat, p

    log0, allocs0, lat0, _ = run(TracedOps)
    names0 = [e[0] for e in log0]
    L = CFG.num_layers
    assert names0.count("unpatchify_cfg_euler") == 3
    log1, allocs1, lat1, p = run(TracedOps, enhance_weight=None)
    assert p.enhance_record is None and p._engine._enhance_E is None and p._engine.enhance_scores is None
    assert torch.equal(lat1, lat0) and log1 == log0 and allocs1 == allocs0, "enhance_weight=None must be the path without the keyword"
    # on: per computed forward, branch and layer (the shared layer 0 once) scores + apply right behind the self-attention launch;
    # two small f32 buffers more
    for w in (0, WEIGHT):                         # 0 is not off: the launches run
        log2, allocs2, lat2, p = run(TracedEnhanceOps, enhance_weight=w)
        names2 = [e[0] for e in log2]
        n = 3 * (2 * L - 1)
        assert names2.count("enhance_scores") == n and names2.count("enhance_apply") == n
        assert [x for x in names2 if not x.startswith("enhance_")] == names0, "nothing else moves"
        assert all(names2[j - 1] == "attention" and names2[j + 1] == "enhance_apply" for j, x in enumerate(names2) if x == "enhance_scores")
        assert sorted(allocs2, key=str) == sorted(allocs0 + [((GRID.tokens_per_frame,), F32), ((2, L), F32)], key=str)
        rec = p.enhance_record
        assert rec["weight"] == float(w) and rec["frames"] == GRID.T and len(rec["scores"]) == 2 and all(len(b) == L for b in rec["scores"])
        assert all(isinstance(e, float) and e >= 1.0 for b in rec["scores"] for e in b)
        assert w == 0 or not torch.equal(lat2, lat0)      # weight 0 on near-uniform attention: E = max(1, T * mean) can be 1
        assert p.enhance_weight is None, "a keyword does not become an attribute"
    base = p(**_call_kw())                          # ... and does not outlive its call
    assert p.enhance_record is None and torch.equal(base, lat0)


def test_value_and_scope_errors(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    assert E.validate(None) is None and E.validate(0) == 0.0 and E.validate(4) == 4.0 and E.validate(2.5) == 2.5
    tr = Trace()
    ops = TracedEnhanceOps(tr)
    tr.on = True
    p = _pipe(ops)
    monkeypatch.setattr(p, "_get_engine", lambda: pytest.fail("the engine was built before the settings were validated"))
    for bad in (-0.5, -1, float("nan"), float("inf"), -float("inf"), "4", True, False, [4.0]):
        with pytest.raises(ValueError, match="enhance_weight must be a finite number >= 0"):
            p(**_call_kw(enhance_weight=bad))
    p.enhance_weight = -2.0                         # ... and so is the attribute
    with pytest.raises(ValueError, match="enhance_weight must be a finite number >= 0"):
        p(**_call_kw())
    p.enhance_weight = None
    # first-version scope: both sides named
    with pytest.raises(ValueError, match="enhance_weight cannot be combined with sliding_window_size.* yet"):
        p(**_call_kw(enhance_weight=WEIGHT, sliding_window_size=3, sliding_window_stride=2))
    with pytest.raises(ValueError, match="enhance_weight cannot be combined with a clip of 1 latent frames"):
        p(**_call_kw(enhance_weight=WEIGHT, num_frames=1))
    with pytest.raises(ValueError, match="enhance_weight cannot be combined with a clip of 33 latent frames"):
        p(**_call_kw(enhance_weight=WEIGHT, num_frames=129))
    import torch.distributed as dist
    with monkeypatch.context() as mp:
        mp.setattr(dist, "is_initialized", lambda: True)
        mp.setattr(dist, "get_world_size", lambda *a: 2)
        mp.setattr(dist, "get_rank", lambda *a: 0)
        with pytest.raises(ValueError, match="enhance_weight cannot be combined with a process group of 2 ranks yet"):
            p(**_call_kw(enhance_weight=WEIGHT))
    assert tr.log == [], "a refused call must not reach an operator"
    # the engine says the same when it is driven directly, before any launch
    sd, bsd, noise, c1, c2, bl = solver_inputs()
    sch = FlowMatchScheduler(2)
    from infinicube_amd.videogen import sliding_window as SW
    ops = EnhanceOps()
    m = WanDiT(CFG, sd, ops, bsd).prepare(GRID)
    ck, cu, plan = m.encode_context(c1), m.encode_context(c2), E.EnhancePlan(WEIGHT)
    calls = []
    monkeypatch.setattr(ops, "gemm", lambda *a, **k: calls.append("gemm"))
    with pytest.raises(ValueError, match=r"enhance=\) cannot be combined with sequence / CFG-branch parallelism \(world > 1\) yet"):
        m.denoise(noise.clone(), ck, None, None, sch, 1.0, branch_exchange=lambda own, both: None, enhance=plan)
    msp = WanDiT(CFG, sd, ops, bsd).prepare(GRID, force_sp=True)
    with pytest.raises(ValueError, match=r"enhance=\) cannot be combined with sequence / CFG-branch parallelism \(world > 1\) yet"):
        msp.denoise(noise.clone(), ck, cu, None, sch, 5.0, enhance=plan)
    mw = WanDiT(CFG, sd, ops, bsd).prepare(TokenGrid(9, 64, 96))
    with pytest.raises(ValueError, match=r"enhance=\) cannot be combined with more than one sliding temporal window yet"):
        mw.denoise(noise.clone(), ck, cu, None, sch, 5.0, sliding_window=SW.plan(GRID.T, 3, 2), enhance=plan)
    m1 = WanDiT(CFG, sd, ops, bsd).prepare(TokenGrid(1, 64, 96))
    with pytest.raises(ValueError, match=r"enhance=\) cannot be combined with a clip of 1 latent frames"):
        m1.denoise(syn.make_latent_noise(TokenGrid(1, 64, 96)), ck, cu, None, sch, 5.0, enhance=plan)
    with pytest.raises(ValueError, match="enhance_weight must be a finite number >= 0"):
        m.denoise(noise.clone(), ck, cu, None, sch, 5.0, enhance=E.EnhancePlan(-1.0))
    assert not calls and not getattr(ops, "enhance_calls", []) and m._enhance_E is None and m._enhance is None
    # one sliding window is no combination
    p = _pipe()
    one = p(**_call_kw(enhance_weight=WEIGHT, sliding_window_size=GRID.T, sliding_window_stride=GRID.T))
    assert p.sliding_window_record is None and torch.equal(one, p(**_call_kw(enhance_weight=WEIGHT)))


def test_attribute_precedence_and_record(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    p = _pipe()
    assert (p.enhance_weight, p.enhance_record) == (None, None)
    want = p(**_call_kw(enhance_weight=7.0))
    rec = p.enhance_record
    assert rec["weight"] == 7.0 and rec["frames"] == GRID.T and rec["scores"] == p._engine.enhance_scores
    p.enhance_weight = 7.0
    assert torch.equal(p(**_call_kw()), want) and p.enhance_record == rec
    other = p(**_call_kw(enhance_weight=2.0))          # the keyword wins over the attribute
    assert p.enhance_record["weight"] == 2.0 and not torch.equal(other, want)
    assert all(a < b for ra, rb in zip(p.enhance_record["scores"], rec["scores"]) for a, b in zip(ra, rb)), "E grows with the weight"
    single = p(**_call_kw(cfg_scale=1.0))
    assert len(p.enhance_record["scores"]) == 1 and not torch.equal(single, want)
    p.enhance_weight = None
    assert torch.equal(p(**_call_kw()), _pipe()(**_call_kw())) and p.enhance_record is None
    assert E.EnhancePlan(3).key == (3.0,) and E.EnhancePlan(3).record(5) == dict(weight=3.0, frames=5, scores=None)


def test_attribute_route_through_the_generator(tmp_path, monkeypatch):
    """The caller of the unchanged WanVideoGenerator: gen.pipe.enhance_weight = 4."""
    from PIL import Image
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    grid = TokenGrid(9, 64, 96)
    vae = CountingVAE()
    g, sem, co = generator_through_env(lambda torch_dtype, device, model_configs: _pipe(vae=vae), tmp_path, monkeypatch, grid, "cpu",
                                       ICV_SAMPLE_STEPS="3")
    assert g.pipe.enhance_record is None
    plain = vae.last_decoded
    g.pipe.enhance_weight = WEIGHT
    video = g.generate(sem, co, prompt="a street", negative_prompt="bad", seed=3)
    assert len(video) == grid.num_frames and g.pipe.enhance_record["weight"] == WEIGHT and g.pipe.enhance_record["frames"] == grid.T
    p = _pipe()                                                    # the keyword route on a pipeline built with nothing set
    p.initialize_buffer_embedder(16, zero_init=False)
    p.buffer_embedder.load_state_dict(syn.make_buffer_embedder_state_dict(CFG))
    kw = dict(prompt="a street", negative_prompt="bad", semantic_buffer_video=[Image.fromarray(f) for f in sem],
              coordinate_buffer_video=[Image.fromarray(f) for f in co], height=grid.height, width=grid.width, num_frames=grid.num_frames,
              seed=3, return_latents=True, num_inference_steps=3)
    want = p(**kw, enhance_weight=WEIGHT)
    assert torch.equal(vae.last_decoded, want), "the attribute must select what the keyword selects"
    assert not torch.equal(want, plain) and not torch.equal(want, p(**kw))


def test_worker_pool_combination_raises(monkeypatch):
    """ICV_WORLD > 1 behind the unchanged generator: refused in the client before a request reaches the ranks."""
    from infinicube_amd.videogen.inference import WanVideoGenerator
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    g = WanVideoGenerator.__new__(WanVideoGenerator)
    g._pool, g.pipe = object(), _pipe()
    g.pipe.enhance_weight = WEIGHT
    sem, co = syn.make_dummy_buffers(TokenGrid(9, 64, 96))
    with pytest.raises(ValueError, match="enhance_weight cannot be combined with ICV_WORLD > 1"):
        g.generate(sem, co, seed=0)


def test_pipeline_compositions(monkeypatch):
    """CFG-Zero* and input_video / input_mask through the pipeline on the CPU operator set: each call runs the measurement in every
    computed forward, fills the record and differs from the same call without the keyword."""
    from test_v2v_cpu import SHORT, make_clip, pil
    from test_v2v_cpu import _call_kw as v2v_kw
    from test_v2v_cpu import _pipe as v2v_pipe
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    L = CFG.num_layers
    clip = pil(make_clip(SHORT, 1))
    mask = np.ones((SHORT.num_frames, SHORT.height, SHORT.width), dtype=np.uint8)
    mask[:, :32] = 0
    for extra, forwards in ((dict(cfg_zero_star=True), 2), (dict(cfg_zero_star=True, cfg_zero_init_steps=1), 1),
                            (dict(input_video=clip, denoising_strength=0.6), 2),
                            (dict(input_video=clip, denoising_strength=0.6, input_mask=mask), 2)):
        ops = EnhanceOps()
        p = v2v_pipe(ops)
        got = p(**v2v_kw(**extra), enhance_weight=WEIGHT)
        rec = p.enhance_record
        assert rec["frames"] == SHORT.T and len(rec["scores"]) == 2 and len(ops.enhance_calls) == forwards * 2 * (2 * L - 1), extra
        assert not torch.equal(got, v2v_pipe(EnhanceOps())(**v2v_kw(**extra))), extra


# ---- 5. the graph cache's key -----------------------------------------------------------------------------------------------------------
def test_graph_keys(monkeypatch):
    """Under hipGraph mode the key of a captured forward holds the weight and the branch's row of the factor buffer, None when the
    feature is off.  The capture itself is stubbed out (no GPU here): every forward of the first step is a miss and runs eagerly."""
    import contextlib

    class FakeGraph:
        def replay(self):
            pass

    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    monkeypatch.setattr(torch.cuda, "CUDAGraph", FakeGraph)
    monkeypatch.setattr(torch.cuda, "graph", lambda g: contextlib.nullcontext())

    def setup(m):
        m._graphs_on = True

    m, _ = engine_loop(EnhanceOps(), weight=None, steps=1, setup=setup)
    assert sorted(k[-1] is None for k in m._graphs) == [True, True]
    _, _ = engine_loop(m.ops, steps=1, engine=m)
    tails = sorted((k[-1] for k in m._graphs if k[-1] is not None))
    assert len(m._graphs) == 4 and tails == [(WEIGHT, 0), (WEIGHT, 1)]
    _, _ = engine_loop(m.ops, weight=2.0, steps=1, engine=m)
    assert len(m._graphs) == 6 and sorted(k[-1] for k in m._graphs if k[-1] is not None)[:2] == [(2.0, 0), (2.0, 1)]


# ---- 6. the C entry points' argument checks ---------------------------------------------------------------------------------------------
def test_argument_errors_without_gpu():
    from infinicube_amd import native
    lib = native.lib()
    assert native.ENHANCE_WORKSPACE_FLOATS == 16384

    def scores(**kw):
        a = dict(q=0x1000, ldq=256, k=0x2000, ldk=256, T=5, P=24, heads=2, scale=LN2, weight=4.0, ws=0x3000, out=0x4000)
        a.update(kw)
        rc = lib.icv_enhance_scores_bf16(a["q"], a["ldq"], a["k"], a["ldk"], a["T"], a["P"], a["heads"], a["scale"], a["weight"], a["ws"],
                                         a["out"], None)
        return rc, lib.icv_last_error()

    def apply(**kw):
        a = dict(att=0x1000, ld=256, rows=120, d=256, ws=0x3000, T=5, P=24, heads=2, weight=4.0, out=0x4000)
        a.update(kw)
        rc = lib.icv_enhance_apply_bf16(a["att"], a["ld"], a["rows"], a["d"], a["ws"], a["T"], a["P"], a["heads"], a["weight"], a["out"], None)
        return rc, lib.icv_last_error()

    for kw, msg in ((dict(q=None), b"null argument"), (dict(k=None), b"null argument"), (dict(ws=None), b"null argument"),
                    (dict(T=1), b"T=1 latent frames must be in [2, 32]"), (dict(T=33), b"T=33 latent frames must be in [2, 32]"),
                    (dict(T=0), b"T=0"), (dict(heads=0), b"heads=0"), (dict(P=0), b"P=0"),
                    (dict(P=16385), b"P=16385 positions per frame must be in [1, 16384]"),
                    (dict(ldq=128), b"head width 128 only"), (dict(ldk=192), b"head width 128 only"),
                    (dict(ldq=260), b"must be multiples of 8"), (dict(ldk=257), b"must be multiples of 8"),
                    (dict(q=0x1008), b"16-byte aligned"), (dict(k=0x2002), b"16-byte aligned"), (dict(ws=0x3002), b"4-byte aligned"),
                    (dict(out=0x4001), b"4-byte aligned"), (dict(weight=-1.0), b"weight=-1"), (dict(weight=float("nan")), b"weight="),
                    (dict(weight=float("inf")), b"weight="), (dict(scale=0.0), b"scale=0"), (dict(scale=float("nan")), b"scale=")):
        rc, err = scores(**kw)
        assert rc != 0 and msg in err, (kw, rc, err)
    for kw, msg in ((dict(att=None), b"null argument"), (dict(ws=None), b"null argument"), (dict(out=None), b"null argument"),
                    (dict(T=1), b"T=1 latent frames must be in [2, 32]"), (dict(T=33), b"T=33"), (dict(P=16385), b"P=16385"),
                    (dict(heads=-1), b"heads=-1"), (dict(rows=0), b"rows=0"), (dict(d=260, ld=264), b"d=260 must be a positive multiple of 8"),
                    (dict(d=0), b"d=0"), (dict(ld=260), b"ld=260 must be a multiple of 8"), (dict(ld=248), b"ld=248 must be a multiple of 8 and >= d=256"),
                    (dict(att=0x1008), b"16-byte aligned"), (dict(ws=0x3001), b"4-byte aligned"), (dict(weight=-0.5), b"weight=-0.5")):
        rc, err = apply(**kw)
        assert rc != 0 and msg in err, (kw, rc, err)
