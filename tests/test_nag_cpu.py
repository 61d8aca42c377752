"""Normalized Attention Guidance (infinicube_amd/videogen/nag.py) on CPU: the torch twin of icv_nag_combine_bf16
against closed forms, the restated NAG block (tests/nag_ref.py) against oracle.wan_ref.dit_block where NAG has no effect, the host
loop (dit.WanDiT.denoise(nag=)) on the TEST-ONLY oracle operator set against the restated loop, the exact case (negative prompt ==
prompt), off = nothing new (bits, launches, allocations), every ValueError before any operator runs, the attribute route through the
unchanged generator, the record, and the C entry point's argument checks (they run on the host, before any launch).

The loop test's inputs.  With the synthetic weights and contexts as they come, cross-attention moves the residual stream so little
that a loop which ignored the negative prompt would still pass the 40 dB bar.  GAINS below (the stiff state dict of test_solver_cpu
with every cross-attention output projection x 32, the positive context x 20, the negative context a fresh draw at 20 x the positive
context's std - the gains of test_cfg_zero_cpu) make the text matter.  Measured on the CPU oracle with these gains, Euler, 6 steps,
cfg_scale 1, nag (11, 2.5, 0.25): restated plain loop vs restated NAG loop 23.9 dB (asserted < 30 dB); the engine loop vs the restated
NAG loop 62.0 dB (bar: 40 dB)."""
import pytest
import torch

from dit_launch_trace import Trace, TracedOps
from infinicube_amd.videogen import nag as N
from infinicube_amd.videogen import solver as S
from infinicube_amd.videogen import synthetic as syn
from infinicube_amd.videogen.config import TokenGrid
from infinicube_amd.videogen.dit import WanDiT
from infinicube_amd.videogen.pipeline import DiTHolder, WanVideoPipeline
from infinicube_amd.videogen.scheduler import FlowMatchScheduler, flow_match_sigmas
from nag_ref import BF16, NagForward, NagOps, nag_block, nag_rule, nag_twin, nag_velocity
from oracle import wan_ref as R
from standins import HashTextEncoder, PoolVAE
from test_solver_cpu import CFG, ENV, GRID, LOOP_STEPS, CountingVAE, generator_through_env, restated_sample
from test_solver_cpu import inputs as solver_inputs

F32, F64 = torch.float32, torch.float64
NAG = (11.0, 2.5, 0.25)              # nag_scale and the defaults of nag_tau / nag_alpha
GAINS = dict(cross_attn_o=32.0, cond_context=20.0, neg_context=20.0)


# ---- 1. the twin against closed forms -------------------------------------------------------------------------------------------------
def _rows(rows=9, d=256, seed=21):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn((rows, d), generator=g).to(BF16)
    return p, (p.float() + 0.5 * torch.randn((rows, d), generator=g)).to(BF16)


def test_twin_against_closed_forms():
    p, n = _rows()
    out = torch.empty_like(p)
    # n == p: g == p, Ng == Np, c == 1 -> p bit for bit (also in place)
    nag_twin(p, p.clone(), out, *NAG)
    assert torch.equal(out, p)
    # tau = 1e30: never clipped -> the plain blend alpha g + (1 - alpha) p
    scale, _, alpha = NAG
    nag_twin(p, n, out, scale, 1e30, alpha)
    g = scale * p.double() - (scale - 1.0) * n.double()
    want = alpha * g + (1.0 - alpha) * p.double()
    assert float((out.double() - want).abs().max()) <= 2.0 ** -8 * float(want.abs().max())
    ref, c, _ = nag_rule(p, n, scale, 1e30, alpha)
    assert torch.equal(c, torch.ones_like(c)) and torch.equal(ref, want)
    # clipped rows: with alpha = 1 the output IS c g, so its L1 norm is tau Np (to bf16 rounding) - c checked directly
    tau = 2.5
    ref, c, g = nag_rule(p, n, scale, tau, 1.0)
    Np, Ng = p.double().abs().sum(-1), g.abs().sum(-1)
    assert bool((Ng > tau * Np).all()), "every row of this draw is clipped at scale 11"
    assert torch.allclose(c[:, 0], tau * Np / Ng, rtol=1e-15) and torch.allclose(ref.abs().sum(-1), tau * Np, rtol=1e-12)
    nag_twin(p, n, out, scale, tau, 1.0)
    got = out.double().abs().sum(-1)
    assert float(((got - tau * Np).abs() / (tau * Np)).max()) <= 2.0 ** -8
    # ... and the twin is the rule at the defaults
    ref = nag_rule(p, n, *NAG)[0]
    nag_twin(p, n, out, *NAG)
    assert float((out.double() - ref).abs().max()) <= 2.0 ** -8 * float(ref.abs().max())
    # a zero positive row: zeros, nothing non-finite
    pz = p.clone()
    pz[3] = 0
    nag_twin(pz, n, out, *NAG)
    assert torch.equal(out[3], torch.zeros_like(out[3])) and torch.isfinite(out.float()).all()
    ref, c, _ = nag_rule(pz, n, *NAG)
    assert float(c[3]) == 0.0 and torch.equal(ref[3], torch.zeros_like(ref[3]))
    # in place
    inplace = p.clone()
    nag_twin(inplace, n, inplace, *NAG)
    nag_twin(p, n, out, *NAG)
    assert torch.equal(inplace, out)


# ---- 2. the restated block with no effect is the oracle's block -----------------------------------------------------------------------
def test_restated_block_without_effect_is_the_oracle():
    sd, bsd, noise, c1, _, bl = solver_inputs()
    rsd = R.round_state_dict_to_bf16(sd)
    x = R.patchify_tokens(noise, rsd["patch_embedding.weight"], rsd["patch_embedding.bias"]) + R.buffer_embed(R.round_state_dict_to_bf16(bsd), bl)
    _, t_mod = R.time_embed(rsd, CFG, 731.0)
    freqs = R.rope_freqs_3d(CFG.head_dim, GRID.T, GRID.Hp, GRID.Wp)
    ctx = R.text_embed(rsd, c1)
    for i in range(CFG.num_layers):
        want = R.dit_block(rsd, CFG, i, x, ctx, t_mod, freqs)
        assert torch.equal(nag_block(rsd, CFG, i, x, ctx, t_mod, freqs), want), "no NAG: the oracle's block"
        assert torch.equal(nag_block(rsd, CFG, i, x, ctx, t_mod, freqs, ctx_neg=ctx.clone(), nag=NAG), want), "negative == positive: the oracle's block"
        x = want
    fwd = NagForward(rsd, CFG, c1, c1, NAG, R.buffer_embed(R.round_state_dict_to_bf16(bsd), bl))
    assert torch.equal(fwd.step_velocity(noise, 0, 731.0), R.dit_forward(rsd, CFG, noise, c1, 731.0, fwd.buf))


# ---- 3. the host loop against the restated loop ---------------------------------------------------------------------------------------
_INPUTS = {}


def inputs():
    """test_solver_cpu.inputs() with GAINS applied -> (sd, bsd, noise, positive context, negative context, buffer latents)."""
    if "v" not in _INPUTS:
        sd, bsd, noise, c1, _, bl = solver_inputs()
        sd = dict(sd)
        hit = [k for k in sd if k.endswith("cross_attn.o.weight")]
        assert len(hit) == CFG.num_layers
        for k in hit:
            sd[k] = sd[k] * GAINS["cross_attn_o"]
        cn = torch.randn(c1.shape, generator=torch.Generator().manual_seed(5)) * float(c1.std()) * GAINS["neg_context"]
        _INPUTS["v"] = (sd, bsd, noise, c1 * GAINS["cond_context"], cn.to(c1.dtype), bl)
    return _INPUTS["v"]


_REFS = {}


def reference(nag=NAG, solver="euler", steps=LOOP_STEPS, fp8=False, tea_skipped=(), window=None):
    """The restated loop's latent (cfg_scale = 1, one forward per step; ``nag`` None: the plain loop), once per setting."""
    key = (nag, solver, steps, fp8, tuple(tea_skipped), window)
    if key not in _REFS:
        sd, bsd, noise, cp, cn, bl = inputs()
        rsd, rbsd = R.round_state_dict_to_bf16(sd), R.round_state_dict_to_bf16(bsd)
        sigmas = flow_match_sigmas(steps)
        fwd = NagForward(rsd, CFG, cp, cn, nag, R.buffer_embed(rbsd, bl), fp8=fp8, window=window, tea_skipped=tea_skipped)
        _REFS[key] = restated_sample(nag_velocity(fwd, sigmas), noise.double(), sigmas, solver).float()
    return _REFS[key]


def engine_loop(ops, nag=NAG, solver="euler", steps=LOOP_STEPS, setup=None, prep=None, dev="cpu", kw=None, tea=None, same_context=False,
                engine=None):
    """dit.WanDiT.denoise at cfg_scale = 1 on ``ops`` with the NAG plan (``nag`` None: the plain call) -> (engine, latent).  An
    ``engine`` from an earlier call runs again on the SAME context objects, buffer tokens and latent tensor (what a graph is keyed on)."""
    sd, bsd, noise, cp, cn, bl = inputs()
    m = engine or WanDiT(CFG, sd, ops, bsd, **(kw or {})).prepare(GRID, **(prep or {}))
    if setup is not None:
        setup(m)
    if engine is None:
        m.test_operands = (m.encode_context(cp), m.encode_context(cp if same_context else cn), m.embed_buffers(bl), noise.clone().to(dev))
    ctx_pos, ctx_neg, buf, lat = m.test_operands
    lat.copy_(noise)
    sch = FlowMatchScheduler(steps)
    extra = dict(solver=S.MultistepPlan(solver, sch.sigmas)) if solver != "euler" else {}
    if tea is not None:
        extra["tea_cache"] = tea(m, sch)
    if nag is not None:
        extra["nag"] = N.NagPlan(ctx_neg, *nag)
    m.denoise(lat, ctx_pos, None, buf, sch, 1.0, **extra)
    return m, lat.clone()


def check_loop(lat, what, ref=None, bar=40.0):
    """>= ``bar`` dB against the restated NAG loop - and the restated PLAIN loop is below 30 dB against it, so a loop that ignored the
    negative prompt could not pass."""
    ref = reference() if ref is None else ref
    p = R.psnr(lat.cpu(), ref)
    print(f"{what}: engine vs restated NAG loop {p:.1f} dB")
    assert p >= bar, f"{what}: {p:.1f} dB"
    return p


def test_restated_loops_are_told_apart():
    p_plain = R.psnr(reference(None), reference())
    print(f"restated plain cfg_scale=1 loop vs restated NAG loop: {p_plain:.1f} dB")
    assert p_plain < 30.0, f"the 40 dB bar could pass with the feature ignored: plain vs NAG {p_plain:.1f} dB"


def test_host_loop_matches_restated_nag_loop():
    ops = NagOps()
    m, lat = engine_loop(ops)
    check_loop(lat, "CPU operator set")
    assert len(ops.nag_calls) == LOOP_STEPS * CFG.num_layers and all(c == NAG + (True,) for c in ops.nag_calls), "one in-place combine per layer"
    assert m._nag is None and m._pair is None
    buf = m._nag_buf
    assert buf.dtype == BF16 and tuple(buf.shape) == tuple(m.att.shape)
    _, again = engine_loop(ops, engine=m)
    assert m._nag_buf is buf and torch.equal(again, lat), "the second buffer is allocated once"


def test_same_prompts_give_the_plain_call():
    _, lat = engine_loop(NagOps(), same_context=True)
    m0, lat0 = engine_loop(NagOps(), nag=None)
    assert torch.equal(lat, lat0) and m0._nag_buf is None


# ---- 4. the pipeline: off, errors, attributes, record ---------------------------------------------------------------------------------
def _pipe(ops=None, vae=None, dtype=torch.bfloat16):
    return WanVideoPipeline("cpu", dtype, DiTHolder(syn.make_dit_state_dict(CFG), CFG), HashTextEncoder(CFG), vae or PoolVAE(),
                            ops=ops or NagOps())


def _call_kw(**extra):
    kw = dict(prompt="a street", negative_prompt="bad", height=GRID.height, width=GRID.width, num_frames=GRID.num_frames, seed=3,
              num_inference_steps=3, return_latents=True, cfg_scale=1.0)
    kw.update(extra)
    return kw


class TracedNagOps(TracedOps):
    """TracedOps + the twin: the new op shows in the log."""

    def nag_combine(self, zp, zn, out, scale, tau, alpha):
        nag_twin(zp, zn, out, scale, tau, alpha)


def test_off_is_the_plain_path(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)

    def run(ops_cls, **kw):
        tr = Trace()
        ops = ops_cls(tr)                         # TracedOps has no nag_combine: calling it would raise
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
    for kw in (dict(nag_scale=None), dict(nag_scale=1.0), dict(nag_scale=1, nag_tau=3.0, nag_alpha=0.5)):
        log1, allocs1, lat1, p = run(TracedOps, **kw)
        assert p.nag_record is None and p._engine._nag_buf is None
        assert torch.equal(lat1, lat0) and log1 == log0 and allocs1 == allocs0, f"{kw} must be the path without the keywords"
    # on: one more context, then per layer and step one more attention and one combine, right behind the text softmax; one more buffer
    log2, allocs2, lat2, p = run(TracedNagOps, nag_scale=11.0)
    names2 = [e[0] for e in log2]
    assert names2.count("nag_combine") == 3 * L and names2.count("attention") == names0.count("attention") + 3 * L
    assert all(names2[j - 2: j] == ["attention", "attention"] for j, n in enumerate(names2) if n == "nag_combine")
    at = p._engine.att
    assert allocs2.count((tuple(at.shape), BF16)) == allocs0.count((tuple(at.shape), BF16)) + 1 and len(allocs2) > len(allocs0)
    assert p.nag_record == dict(scale=11.0, tau=2.5, alpha=0.25) and not torch.equal(lat2, lat0)
    assert (p.nag_scale, p.nag_tau, p.nag_alpha) == (None, None, None), "a keyword does not become an attribute"
    base = p(**_call_kw())                          # ... and does not outlive its call
    assert p.nag_record is None and torch.equal(base, lat0)


def test_same_prompts_through_the_pipeline_give_the_plain_call(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    p = _pipe()
    same = p(**_call_kw(negative_prompt="a street", nag_scale=11.0))
    assert p.nag_record is not None and torch.equal(same, _pipe()(**_call_kw()))


def test_value_and_scope_errors(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    assert N.validate(None) is None and N.validate(1.0) is None and N.validate(1, 3.0, 0.5) is None
    assert N.validate(11.0) == (11.0, 2.5, 0.25) and N.validate(4, 1.0, 1) == (4.0, 1.0, 1.0)
    tr = Trace()
    ops = TracedNagOps(tr)
    tr.on = True
    p = _pipe(ops)
    monkeypatch.setattr(p, "_get_engine", lambda: pytest.fail("the engine was built before the settings were validated"))
    for bad in (0.5, 0.0, -1.0, float("nan"), float("inf"), "11", True, [11.0]):
        with pytest.raises(ValueError, match="nag_scale must be"):
            p(**_call_kw(nag_scale=bad))
    for bad in (0.99, 0.0, float("nan"), "2.5"):
        with pytest.raises(ValueError, match="nag_tau must be"):
            p(**_call_kw(nag_scale=11.0, nag_tau=bad))
    for bad in (0.0, -0.25, 1.01, float("nan"), "0.25"):
        with pytest.raises(ValueError, match="nag_alpha must be"):
            p(**_call_kw(nag_scale=11.0, nag_alpha=bad))
    with pytest.raises(ValueError, match="nag_tau given without nag_scale"):
        p(**_call_kw(nag_tau=2.5))
    with pytest.raises(ValueError, match="nag_alpha given without nag_scale"):
        p(**_call_kw(nag_alpha=0.25))
    with pytest.raises(ValueError, match="nag_tau / nag_alpha given without nag_scale"):
        p(**_call_kw(nag_tau=2.5, nag_alpha=0.25))
    # first-version scope
    for cfg_scale in (5.0, None):                   # None: the pipeline's attribute, 5
        with pytest.raises(ValueError, match="nag_scale needs cfg_scale=1"):
            p(**_call_kw(nag_scale=11.0, cfg_scale=cfg_scale))
    with pytest.raises(ValueError, match="nag_scale cannot be combined with sliding_window_size.* yet"):
        p(**_call_kw(nag_scale=11.0, sliding_window_size=3, sliding_window_stride=2))
    with pytest.raises(ValueError, match="cfg_zero_star needs classifier-free guidance"):
        p(**_call_kw(nag_scale=11.0, cfg_zero_star=True))
    import torch.distributed as dist
    with monkeypatch.context() as mp:
        mp.setattr(dist, "is_initialized", lambda: True)
        mp.setattr(dist, "get_world_size", lambda *a: 2)
        mp.setattr(dist, "get_rank", lambda *a: 0)
        with pytest.raises(ValueError, match="nag_scale cannot be combined with a process group of 2 ranks yet"):
            p(**_call_kw(nag_scale=11.0))
    assert tr.log == [], "a refused call must not reach an operator"
    # the engine says the same when it is driven directly, before any launch
    sd, bsd, noise, c1, c2, bl = solver_inputs()
    sch = FlowMatchScheduler(2)
    from infinicube_amd.videogen import sliding_window as SW
    ops = NagOps()
    m = WanDiT(CFG, sd, ops, bsd).prepare(GRID)
    ck, plan = m.encode_context(c1), N.NagPlan(m.encode_context(c2), *NAG)
    calls = []
    monkeypatch.setattr(ops, "gemm", lambda *a, **k: calls.append("gemm"))
    with pytest.raises(ValueError, match="pass ctx_cond and cfg_scale=1"):
        m.denoise(noise.clone(), ck, plan.ctx_neg, None, sch, 5.0, nag=plan)
    with pytest.raises(ValueError, match="pass ctx_cond and cfg_scale=1"):
        m.denoise(noise.clone(), None, None, None, sch, 1.0, nag=plan)
    with pytest.raises(ValueError, match=r"nag=\) cannot be combined with sequence / CFG-branch parallelism \(world > 1\) yet"):
        m.denoise(noise.clone(), ck, None, None, sch, 1.0, branch_exchange=lambda own, both: None, nag=plan)
    msp = WanDiT(CFG, sd, ops, bsd).prepare(GRID, force_sp=True)
    with pytest.raises(ValueError, match=r"nag=\) cannot be combined with sequence / CFG-branch parallelism \(world > 1\) yet"):
        msp.denoise(noise.clone(), ck, None, None, sch, 1.0, nag=plan)
    mw = WanDiT(CFG, sd, ops, bsd).prepare(TokenGrid(9, 64, 96))
    with pytest.raises(ValueError, match=r"nag=\) cannot be combined with more than one sliding temporal window yet"):
        mw.denoise(noise.clone(), ck, None, None, sch, 1.0, sliding_window=SW.plan(GRID.T, 3, 2), nag=plan)
    assert not calls and not ops.nag_calls and m._nag_buf is None and m._nag is None
    # one sliding window is no combination
    p = _pipe()
    one = p(**_call_kw(nag_scale=11.0, sliding_window_size=GRID.T, sliding_window_stride=GRID.T))
    assert p.sliding_window_record is None and torch.equal(one, p(**_call_kw(nag_scale=11.0)))


def test_attributes_precedence_and_record(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    p = _pipe()
    assert (p.nag_scale, p.nag_tau, p.nag_alpha, p.nag_record) == (None, None, None, None)
    want = p(**_call_kw(nag_scale=7.0, nag_tau=2.0, nag_alpha=0.5))
    assert p.nag_record == dict(scale=7.0, tau=2.0, alpha=0.5)
    p.cfg_scale, p.nag_scale, p.nag_tau, p.nag_alpha = 1.0, 7.0, 2.0, 0.5
    kw = _call_kw()
    del kw["cfg_scale"]
    assert torch.equal(p(**kw), want) and p.nag_record == dict(scale=7.0, tau=2.0, alpha=0.5)
    other = p(**kw, nag_scale=11.0)                 # a keyword wins over its attribute, each setting on its own
    assert p.nag_record == dict(scale=11.0, tau=2.0, alpha=0.5) and not torch.equal(other, want)
    off = p(**kw, nag_scale=1.0)
    assert p.nag_record is None and torch.equal(off, _pipe()(**_call_kw()))


def test_attribute_route_through_the_generator(tmp_path, monkeypatch):
    """The caller of the unchanged WanVideoGenerator: gen.pipe.cfg_scale = 1; gen.pipe.nag_scale = 11."""
    from PIL import Image
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    grid = TokenGrid(9, 64, 96)
    vae = CountingVAE()
    g, sem, co = generator_through_env(lambda torch_dtype, device, model_configs: _pipe(vae=vae), tmp_path, monkeypatch, grid, "cpu",
                                       ICV_SAMPLE_STEPS="3")
    assert g.pipe.nag_record is None
    plain = vae.last_decoded
    g.pipe.cfg_scale, g.pipe.nag_scale = 1.0, 11.0
    video = g.generate(sem, co, prompt="a street", negative_prompt="bad", seed=3)
    assert len(video) == grid.num_frames and g.pipe.nag_record == dict(scale=11.0, tau=2.5, alpha=0.25)
    p = _pipe()                                                    # the keyword route on a pipeline built with nothing set
    p.initialize_buffer_embedder(16, zero_init=False)
    p.buffer_embedder.load_state_dict(syn.make_buffer_embedder_state_dict(CFG))
    kw = dict(prompt="a street", negative_prompt="bad", semantic_buffer_video=[Image.fromarray(f) for f in sem],
              coordinate_buffer_video=[Image.fromarray(f) for f in co], height=grid.height, width=grid.width, num_frames=grid.num_frames,
              seed=3, return_latents=True, num_inference_steps=3, cfg_scale=1.0)
    want = p(**kw, nag_scale=11.0)
    assert torch.equal(vae.last_decoded, want), "the attributes must select what the keywords select"
    assert not torch.equal(want, plain) and not torch.equal(want, p(**kw))


def test_worker_pool_combination_raises(monkeypatch):
    """ICV_WORLD > 1 behind the unchanged generator: refused in the client before a request reaches the ranks."""
    from infinicube_amd.videogen.inference import WanVideoGenerator
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    g = WanVideoGenerator.__new__(WanVideoGenerator)
    g._pool, g.pipe = object(), _pipe()
    g.pipe.cfg_scale, g.pipe.nag_scale = 1.0, 11.0
    sem, co = syn.make_dummy_buffers(TokenGrid(9, 64, 96))
    with pytest.raises(ValueError, match="nag_scale cannot be combined with ICV_WORLD > 1"):
        g.generate(sem, co, seed=0)


# ---- 5. the C entry point's argument checks -------------------------------------------------------------------------------------------
def test_argument_errors_without_gpu():
    from infinicube_amd import native
    lib = native.lib()

    def call(**kw):
        a = dict(zp=0x1000, ldp=256, zn=0x2000, ldn=256, out=0x3000, ldo=256, rows=5, d=256)
        a.update(kw)
        rc = lib.icv_nag_combine_bf16(a["zp"], a["ldp"], a["zn"], a["ldn"], a["out"], a["ldo"], a["rows"], a["d"], 11.0, 2.5, 0.25, None)
        return rc, lib.icv_last_error()

    for kw, msg in ((dict(zp=None), b"null argument"), (dict(zn=None), b"null argument"), (dict(out=None), b"null argument"),
                    (dict(rows=0), b"rows=0"), (dict(rows=-3), b"rows=-3"), (dict(d=264, ldp=264, ldn=264, ldo=264), b"d=264 must be a multiple of 256"),
                    (dict(d=0), b"d=0 must be"), (dict(d=8448, ldp=8448, ldn=8448, ldo=8448), b"d=8448 must be"),
                    (dict(ldp=260), b"must be multiples of 8"), (dict(ldo=248), b"must be multiples of 8 and >= d"),
                    (dict(ldn=128), b"must be multiples of 8 and >= d"), (dict(zn=0x2008), b"16-byte aligned"),
                    (dict(out=0x1000, ldo=264), b"out may be an input only with that input's leading dimension")):
        rc, err = call(**kw)
        assert rc != 0 and msg in err, (kw, rc, err)
