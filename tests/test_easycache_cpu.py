"""EasyCache step skipping (infinicube_amd/videogen/easycache.py) on CPU: the rule against a hand-written trace, the
settings' errors, the scope errors (pipeline, engine, worker-pool client) before any operator runs, off = nothing new (bits, launches,
allocations), and the host loop (dit.WanDiT.denoise(easy_cache=)) on the TEST-ONLY operator twins against a float64 restatement that
drives oracle.wan_ref.dit_forward with ITS OWN copy of the rule - alone and with UniPC, CFG-Zero* + a zero-init step, input_mask, NAG,
an image-to-video DiT and a ``steps=`` subrange.

The loop tests.  Tiny preset, TokenGrid(9, 64, 96) (3 latent frames of 4 x 6 tokens), 8 steps, warmup_steps = 2, the stiff state dict
of test_solver_cpu (a velocity that depends on time and sample).  The threshold of every case is a constant chosen from the
RESTATEMENT's own trace on the CPU (tools are not needed: ``restated(case)["compared"]`` is the trace).  check_trace() asserts, on the
restatement alone, that at least one step after the warm-up is skipped and one is computed, and that every sum that was compared
with the threshold lies at least 25 % away from it - so the engine (f32 state, other summation orders) decides the same steps without
the test being vacuous.  The restated traces at these thresholds, measured here, stand above CASES, one line per case."""
from collections import Counter

import pytest
import torch

from dit_launch_trace import Trace, TracedOps
from infinicube_amd.videogen import easycache as E
from infinicube_amd.videogen import guidance as G
from infinicube_amd.videogen import inpaint
from infinicube_amd.videogen import nag as N
from infinicube_amd.videogen import sliding_window as SW
from infinicube_amd.videogen import solver as S
from infinicube_amd.videogen import synthetic as syn
from infinicube_amd.videogen import teacache
from infinicube_amd.videogen.config import TokenGrid, preset
from infinicube_amd.videogen.dit import WanDiT
from infinicube_amd.videogen.pipeline import DiTHolder, WanVideoPipeline
from infinicube_amd.videogen.scheduler import FlowMatchScheduler, flow_match_sigmas
from nag_ref import NagForward, NagOps
from oracle import wan_ref as R
from standins import HashTextEncoder, PoolVAE
from test_inpaint_cpu import InpaintOps
from test_solver_cpu import CFG, ENV, STIFF, CountingVAE, generator_through_env, restated_sample
from test_solver_cpu import inputs as solver_inputs

F32, F64 = torch.float32, torch.float64
I2V_CFG = preset("tiny-i2v")
GRID = TokenGrid(9, 64, 96)
STEPS, WARMUP, CFG_SCALE = 8, 2, 5.0
WORKSPACE = 512                      # ICV_L1_CHANGE_WORKSPACE_DOUBLES
NAG = (11.0, 2.5, 0.25)
MARGIN = 0.25

# case -> what runs and the threshold chosen from the restatement's trace: the sums compared with it at steps 2..6 (s = skipped, C =
# computed; steps 0, 1 and 7 are forced):
#   plain     0.2773 s   0.6214 s   1.0598 C   0.1857 s   0.4411 s      (k: 7.99 after the warm-up, 2.23 after step 4)
#   unipc     0.2828 s   0.6180 s   1.0446 C   0.2097 s   0.4404 s
#   zero                 0.2771 s   0.6300 s   1.0947 C   0.2358 s      (one zero-init step: the warm-up is steps 1 and 2)
#   mask      0.2729 s   0.6157 s   1.0597 C   0.1648 s   0.3985 s
#   nag       0.2772 s   0.6213 s   1.0596 C   0.1858 s   0.4412 s      (cfg_scale 1, ONE branch)
#   i2v       0.2696 s   0.6043 s   1.0306 C   0.1742 s   0.4137 s
#   subrange                        0.2902 s   0.6723 C   0.2770 s      (steps=range(2, 8): the warm-up is steps 2 and 3)
# The sums grow by a third to a half per skipped step here, so a threshold 25 % above one sum and 25 % below the next has a window of
# a few per cent; each constant below sits in the middle of its case's window (margins 25.5 .. 26.5 %; subrange: 35 %).
CASES = {
    "plain": dict(thresh=0.84),
    "unipc": dict(thresh=0.83, solver="unipc"),
    "zero": dict(thresh=0.86, zero_star=True, first=1),
    "mask": dict(thresh=0.835, mask=True),
    "nag": dict(thresh=0.84, nag=True),
    "i2v": dict(thresh=0.815, i2v=True),
    "subrange": dict(thresh=0.45, first=2),
}


# ---- the CPU twins of the two kernels and of the read -----------------------------------------------------------------------------------
def head_layout(x):
    """P: a latent [C, T, H8, W8] in the head-output layout [(f hp wp), (y z c)] - R.unpatchify read in the other direction."""
    C, T, H8, W8 = x.shape
    return x.reshape(C, T, H8 // 2, 2, W8 // 2, 2).permute(1, 2, 4, 3, 5, 0).reshape(T * (H8 // 2) * (W8 // 2), 4 * C)


def l1_change_twin(a, b, out2, update_b=False):
    """Torch twin of icv_l1_change_f64: both sums in float64 from the f32 values, then b <- a."""
    out2[0] = (a.double() - b.double()).abs().sum()
    out2[1] = a.double().abs().sum()
    if update_b:
        b.copy_(a)


def predict_twin(x, x_last, hc_last, hu_last, hc, hu, tok0, n_tok):
    """Torch twin of icv_easycache_predict_f32: h = h_last + P(x - x_last) in f32, the subtraction first, columns < 4C of the local rows."""
    c4 = 4 * x.shape[0]
    d = head_layout(x - x_last)[tok0: tok0 + n_tok]
    hc[:n_tok, :c4] = hc_last[:n_tok, :c4] + d
    if hu is not None:
        hu[:n_tok, :c4] = hu_last[:n_tok, :c4] + d


class EasyTwins:
    """Mixin: the twins of icv_l1_change_f64 / icv_easycache_predict_f32 and the per-step read; logs what the engine promises."""

    def l1_change(self, a, b, workspace, out2, update_b=False):
        assert a.dtype == F32 and b.dtype == F32 and workspace.dtype == F64 and out2.dtype == F64 and a.shape == b.shape and a.dim() == 2
        assert workspace.numel() >= WORKSPACE and out2.numel() == 2 and a.data_ptr() != b.data_ptr()
        self.__dict__.setdefault("easy_calls", []).append(("l1_change", tuple(a.shape), bool(update_b)))
        l1_change_twin(a, b, out2, update_b)

    def easycache_predict(self, x, x_last, hc_last, hu_last, hc, hu, tok0, n_tok):
        assert all(t.dtype == F32 for t in (x, x_last, hc_last, hc)) and x.shape == x_last.shape and (hu is None) == (hu_last is None)
        assert len({t.data_ptr() for t in (hc_last, hu_last, hc, hu) if t is not None}) == (2 if hu is None else 4)
        self.__dict__.setdefault("easy_calls", []).append(("predict", hu is not None))
        predict_twin(x, x_last, hc_last, hu_last, hc, hu, tok0, n_tok)

    def read_doubles(self, t):
        assert t.dtype == F64
        self.__dict__.setdefault("easy_reads", []).append(t.numel() * 8)
        return t.tolist()


class EasyOps(EasyTwins, InpaintOps):
    """Every twin the compositions need (TeaCache, multistep, CFG-Zero*, the pin) + this feature's."""


class EasyNagOps(EasyTwins, NagOps):
    pass


# ---- 1. the rule against a hand-written trace -------------------------------------------------------------------------------------------
def test_rule_against_a_hand_written_trace():
    """thresh 1, warm-up 2, ten steps, the last forced.  Per step (d_in, d_x, d_v, n_out), the last three read only when computed."""
    table = {0: (None, None, None, 2.0),          # forced (warm-up); no j: k stays None
             1: (9.0, 0.5, 1.0, 2.0),             # forced (warm-up); k = 1 / 0.5 = 2
             2: (0.3, 7.0, 7.0, 7.0),             # acc = 2 * 0.3 / 2 = 0.3 < 1: skipped
             3: (0.5, 7.0, 7.0, 7.0),             # acc = 0.8: skipped
             4: (0.4, 0.0, 5.0, 4.0),             # acc = 1.2: computed, acc reset; d_x == 0: k keeps 2; n_out = 4
             5: (1.0, 7.0, 7.0, 7.0),             # acc = 2 * 1 / 4 = 0.5: skipped
             6: (2.0, 7.0, 7.0, 7.0),             # acc = 1.5 >= 1, but force_skip: skipped, the sum stays
             7: (0.2, 1.0, 3.0, 0.0),             # acc = 1.6: computed; k = 3; n_out = 0
             8: (5.0, 0.5, 1.0, 1.0),             # n_out == 0: forced, computed; k = 2; n_out = 1
             9: (0.1, 1.0, 1.0, 1.0)}             # the scheduler's last step: forced although acc would be 0.2
    seen = []

    def measure(i, j):
        seen.append((i, j))
        return table[i]

    got = E.trace(1.0, 2, range(10), 9, measure, force_skip={1, 6, 9})       # 1 (warm-up) and 9 (last) cannot skip
    assert got["computed"] == [0, 1, 4, 7, 8, 9] and got["skipped"] == [2, 3, 5, 6]
    assert got["k"] == [None, None, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 3.0, 2.0]
    assert got["accumulated"] == pytest.approx([None, None, 0.3, 0.8, 1.2, 0.5, 1.5, 1.6, None, None], abs=1e-15)
    assert seen == [(0, None), (1, 0), (2, 1), (3, 1), (4, 1), (5, 4), (6, 4), (7, 4), (8, 7), (9, 8)]
    # the threshold is exclusive: a sum equal to it is computed
    eq = E.trace(0.5, 2, range(4), 9, lambda i, j: (0.5, 1.0, 2.0, 2.0))
    assert eq["accumulated"] == [None, None, 0.5, 0.5] and eq["computed"] == [0, 1, 2, 3] and eq["skipped"] == []
    # two identical inputs in the warm-up leave k None: every later step is forced, and only force_skip can skip (j exists)
    none = E.trace(1e9, 2, range(5), 9, lambda i, j: (0.0, 0.0, 0.0, 1.0), force_skip={3})
    assert none["computed"] == [0, 1, 2, 4] and none["skipped"] == [3] and none["k"] == [None] * 5 and none["accumulated"] == [None] * 5
    # a longer warm-up counts executed steps, wherever the range starts
    late = E.trace(1e9, 3, range(4, 10), 9, lambda i, j: (1.0, 1.0, 1.0, 1.0))
    assert late["computed"] == [4, 5, 6, 9] and late["skipped"] == [7, 8]


def test_validate_errors():
    assert E.validate(None) is None and E.validate(None, None) is None
    assert E.validate(0.05) == (0.05, 10) and E.validate(1, 2) == (1.0, 2) and E.DEFAULT_WARMUP_STEPS == 10
    for bad in (0, 0.0, -0.1, float("nan"), float("inf"), "0.05", True, False, [0.05]):
        with pytest.raises(ValueError, match="easy_cache_thresh must be a finite number > 0"):
            E.validate(bad)
    for bad in (1, 0, -2, 2.0, "2", True):
        with pytest.raises(ValueError, match="easy_cache_warmup_steps must be an integer >= 2"):
            E.validate(0.05, bad)
    with pytest.raises(ValueError, match="easy_cache_warmup_steps given without easy_cache_thresh"):
        E.validate(None, 4)
    plan = E.EasyCachePlan(0.05)
    assert plan.record() == dict(thresh=0.05, warmup_steps=10, computed=[], skipped=[], k=[], accumulated=[])
    with pytest.raises(ValueError, match="easy_cache_thresh must be"):
        E.EasyCachePlan(-1.0)


# ---- 2. the restatement -----------------------------------------------------------------------------------------------------------------
_INPUTS = {}


def inputs(i2v=False):
    """(cfg, sd, bsd, noise, cond context, other context, buffer latents, clip features | None, y | None) on GRID, the stiff weights."""
    if i2v not in _INPUTS:
        if i2v:
            sd = syn.make_dit_state_dict(I2V_CFG)
            for k, g in STIFF.items():
                sd[k] = sd[k] * g
            _INPUTS[i2v] = (I2V_CFG, sd, syn.make_buffer_embedder_state_dict(I2V_CFG), syn.make_latent_noise(GRID), syn.make_text_context(I2V_CFG, 1),
                            syn.make_text_context(I2V_CFG, 2), syn.make_buffer_latents(I2V_CFG, GRID), syn.make_clip_features(I2V_CFG),
                            syn.make_cond_latents(I2V_CFG, GRID))
        else:
            _INPUTS[i2v] = (CFG,) + tuple(solver_inputs(GRID)) + (None, None)
    return _INPUTS[i2v]


def known_plan(dev="cpu"):
    """input_mask's plan: a known clip x0, the start noise, the left half of every frame kept."""
    noise = inputs()[3]
    x0 = torch.randn(noise.shape, generator=torch.Generator().manual_seed(17))
    keep = torch.zeros(noise.shape[1:], dtype=torch.uint8)
    keep[:, :, : noise.shape[3] // 2] = 1
    return inpaint.KnownPlan(x0.to(dev), noise.clone().to(dev), keep.to(dev))


def restated(case, force_skip=(), fp8=False, thresh=None):
    """The float64 restatement of the loop with its own copy of the rule -> dict(lat, computed, skipped, compared, k).  Forwards:
    oracle.wan_ref.dit_forward on bf16-rounded weights (NAG: tests/nag_ref.py's forward)."""
    spec = CASES[case]
    thresh = spec["thresh"] if thresh is None else thresh
    cfg, sd, bsd, noise, c1, c2, bl, clip, y = inputs(spec.get("i2v", False))
    rsd, rbsd = R.round_state_dict_to_bf16(sd), R.round_state_dict_to_bf16(bsd)
    buf = R.buffer_embed(rbsd, bl)
    sigmas, last = flow_match_sigmas(STEPS), STEPS - 1
    if spec.get("nag"):
        fwd = NagForward(rsd, cfg, c1, c2, NAG, buf, fp8=fp8)
        forwards = lambda x, i: [fwd.step_velocity(x, i, float(sigmas[i]) * 1000.0)]                       # noqa: E731
    else:
        forwards = lambda x, i: [R.dit_forward(rsd, cfg, x, c, float(sigmas[i]) * 1000.0, buf, clip_fea=clip, y=y, fp8=fp8)      # noqa: E731
                                 for c in (c1, c2)]
    st = dict(acc=0.0, k=None, n_out=None, j=None, m=0, x_prev=None, x_last=None, v_last=None)
    log = dict(computed=[], skipped=[], compared=[], k=[])

    def velocity(x, i):
        x = x.double()
        m, st["m"] = st["m"], st["m"] + 1
        forced = m < WARMUP or i == last or st["k"] is None or st["n_out"] == 0.0
        compared = None
        if forced:
            st["acc"] = 0.0
            skip = i in force_skip and st["j"] is not None and m >= WARMUP and i != last
        else:
            st["acc"] += st["k"] * float((x - st["x_prev"]).abs().mean()) / st["n_out"]
            compared = st["acc"]
            skip = compared < thresh or i in force_skip
            if not skip:
                st["acc"] = 0.0
        log["compared"].append(compared)
        log["k"].append(st["k"])
        log["skipped" if skip else "computed"].append(i)
        if skip:
            vs = [v + (x - st["x_last"]) for v in st["v_last"]]
        else:
            vs = [v.double() for v in forwards(x.float(), i)]
            if st["j"] is not None:
                d_x = float((x - st["x_last"]).abs().mean())
                if d_x > 0.0:
                    st["k"] = float((vs[0] - st["v_last"][0]).abs().mean()) / d_x
            st["n_out"] = float(vs[0].abs().mean())
            st["x_last"], st["v_last"], st["j"] = x, vs, i
        st["x_prev"] = x
        if len(vs) == 1:
            return vs[0]
        v_c, v_u = vs
        if spec.get("zero_star"):
            v_u = float((v_c * v_u).sum() / ((v_u * v_u).sum() + 1e-8)) * v_u
        return v_u + CFG_SCALE * (v_c - v_u)

    first = spec.get("first", 0)
    if spec.get("mask"):
        kp = known_plan()
        keep, x0, nz = (kp.keep != 0).expand_as(noise), kp.x0.double(), kp.noise.double()
        sig = list(sigmas) + [0.0]
        x = noise.double()
        for i in range(STEPS):
            x = x + velocity(x, i) * (sig[i + 1] - sig[i])
            x = torch.where(keep, (1.0 - sig[i + 1]) * x0 + sig[i + 1] * nz, x)
    else:
        x = restated_sample(velocity, noise.double(), sigmas, spec.get("solver", "euler"), first=first)
    return dict(log, lat=x.float())


_REFS = {}


def reference(case, force_skip=(), fp8=False):
    key = (case, tuple(force_skip), fp8)
    if key not in _REFS:
        _REFS[key] = restated(case, force_skip, fp8)
    return _REFS[key]


def forced_reference():
    """The restatement with a threshold nothing stays under and steps 3 and 5 forced to skip (test_force_skip, here and on the GPU)."""
    if "forced" not in _REFS:
        _REFS["forced"] = restated("plain", force_skip=(3, 5), thresh=1e-12)
    return _REFS["forced"]


def check_trace(ref, thresh, what):
    """The two conditions on the restatement alone."""
    compared = [c for c in ref["compared"] if c is not None]
    print(f"{what}: restated computed {ref['computed']}, skipped {ref['skipped']}, compared {[None if c is None else round(c, 4) for c in ref['compared']]}")
    assert ref["skipped"] and any(c >= thresh for c in compared), f"{what}: needs a skipped and a rule-computed step after the warm-up"
    for c in compared:
        assert abs(c - thresh) >= MARGIN * thresh, f"{what}: compared sum {c:.4f} is within 25 % of the threshold {thresh}"


# ---- 3. the host loop ---------------------------------------------------------------------------------------------------------------------
def engine_loop(ops, case="plain", dev="cpu", setup=None, prep=None, kw=None, force_skip=(), engine=None, on_step=None, thresh=None):
    """dit.WanDiT.denoise(easy_cache=) on ``ops`` with the case's settings -> (engine, latent, plan)."""
    spec = CASES[case]
    cfg, sd, bsd, noise, c1, c2, bl, clip, y = inputs(spec.get("i2v", False))
    m = engine or WanDiT(cfg, sd, ops, bsd, **(kw or {})).prepare(GRID, **(prep or {}))
    if setup is not None:
        setup(m)
    sch = FlowMatchScheduler(STEPS)
    lat = noise.clone().to(dev)
    extra = {}
    if spec.get("solver"):
        extra["solver"] = S.MultistepPlan(spec["solver"], sch.sigmas)
    if spec.get("zero_star"):
        extra["guidance"] = G.GuidancePlan(True, spec["first"])
    elif spec.get("first"):
        extra["steps"] = range(spec["first"], STEPS)
    if spec.get("mask"):
        extra["known"] = known_plan(dev)
    buf = m.embed_buffers(bl)
    if y is not None:
        buf = m.embed_cond_latents(y, add_to=buf)
    plan = E.EasyCachePlan(spec["thresh"] if thresh is None else thresh, WARMUP, frozenset(force_skip))
    if spec.get("nag"):
        m.denoise(lat, m.encode_context(c1), None, buf, sch, 1.0, nag=N.NagPlan(m.encode_context(c2), *NAG), easy_cache=plan, on_step=on_step, **extra)
    else:
        m.denoise(lat, m.encode_context(c1, clip), m.encode_context(c2, clip), buf, sch, CFG_SCALE, easy_cache=plan, on_step=on_step, **extra)
    return m, lat, plan


def check_loop(lat, plan, ref, what, bar=40.0):
    """The same computed / skipped steps as the restatement, the latent bit-equal or at the loop bar of the project (>= 40 dB)."""
    rec = plan.record()
    print(f"{what}: engine computed {rec['computed']}, skipped {rec['skipped']}")
    print(f"{what}: engine   compared {[None if c is None else round(c, 5) for c in rec['accumulated']]}")
    print(f"{what}: restated compared {[None if c is None else round(c, 5) for c in ref['compared']]}")
    assert rec["computed"] == ref["computed"] and rec["skipped"] == ref["skipped"], f"{what}: the decisions differ from the restatement's"
    p = R.psnr(lat.cpu(), ref["lat"])
    print(f"{what}: engine vs restated EasyCache loop {p:.1f} dB")
    assert p >= bar, f"{what}: {p:.1f} dB"
    return p


@pytest.mark.parametrize("cfg_batch", [True, False])
def test_host_loop_matches_restatement(cfg_batch):
    ref = reference("plain")
    check_trace(ref, CASES["plain"]["thresh"], "plain")
    ops = EasyOps()
    m, lat, plan = engine_loop(ops, setup=lambda m: setattr(m, "cfg_batch", cfg_batch))
    assert (m._pair is not None) == cfg_batch
    check_loop(lat, plan, ref, f"cfg_batch={cfg_batch}")
    # a skipped step must matter: the plain loop is another latent, and so is the restatement that skips nothing
    _, plain, p0 = engine_loop(EasyOps(), thresh=1e-12)
    assert p0.skipped == [] and p0.computed == list(range(STEPS)) and not torch.equal(plain, lat)
    # one blocking read of at most 64 bytes per executed step; one predict per skipped step, for both branches
    assert ops.easy_reads == [64] * STEPS
    assert [c for c in ops.easy_calls if c[0] == "predict"] == [("predict", True)] * len(ref["skipped"])
    rec = plan.record()
    assert rec["thresh"] == CASES["plain"]["thresh"] and rec["warmup_steps"] == WARMUP and len(rec["k"]) == len(rec["accumulated"]) == STEPS
    assert rec["k"][:2] == [None, None] and all(k is not None and k > 0 for k in rec["k"][2:])
    for got, want in zip(rec["accumulated"], ref["compared"]):
        assert (got is None) == (want is None) and (got is None or abs(got - want) <= 0.02 * want)
    # the state: two latents, the head outputs, the workspace, 8 doubles - once per engine; a second call gives the same bits
    x_prev, x_last, h_last, work, sums = state = m._easy_state
    assert x_prev.shape == x_last.shape == lat.shape and h_last.shape == m.head_out.shape and work.numel() == WORKSPACE and sums.numel() == 8
    _, again, plan2 = engine_loop(ops, engine=m)
    assert m._easy_state is state and torch.equal(again, lat) and plan2.record() == rec


def test_off_runs_nothing_new_in_the_engine():
    """easy_cache=None: no twin is called (the plain operator set has none), the engine allocates no state."""
    cfg, sd, bsd, noise, c1, c2, bl, _, _ = inputs()
    m = WanDiT(cfg, sd, InpaintOps(), bsd).prepare(GRID)
    lat = noise.clone()
    m.denoise(lat, m.encode_context(c1), m.encode_context(c2), m.embed_buffers(bl), FlowMatchScheduler(STEPS), CFG_SCALE, easy_cache=None)
    _, plain, _ = engine_loop(EasyOps(), thresh=1e-12)
    assert m._easy_state is None and torch.equal(lat, plain), "a loop that computes every step is the plain loop, bit for bit"


@pytest.mark.parametrize("case", ["unipc", "zero", "mask", "nag", "i2v", "subrange"])
def test_combinations(case):
    ref = reference(case)
    check_trace(ref, CASES[case]["thresh"], case)
    ops = EasyNagOps() if case == "nag" else EasyOps()
    seen = []
    m, lat, plan = engine_loop(ops, case, on_step=lambda i, x: seen.append(i))
    check_loop(lat, plan, ref, case)
    first = CASES[case].get("first", 0)
    executed = STEPS - first
    assert ops.easy_reads == [64] * executed and len(plan.k) == executed
    assert plan.computed[:WARMUP] == [first, first + 1] and plan.computed[-1] == STEPS - 1, "the warm-up counts EXECUTED steps; the last step is forced"
    assert seen == (list(range(STEPS)) if case != "subrange" else list(range(first, STEPS)))
    predicts = [c for c in ops.easy_calls if c[0] == "predict"]
    assert predicts == [("predict", case != "nag")] * len(ref["skipped"])
    if case == "unipc":
        assert len(ops.multistep_calls) == STEPS
    if case == "zero":
        assert len(ops.zero_calls) == executed and m.guidance_scales[0] is None, "the scale runs on skipped steps' head outputs as well"
    if case == "mask":
        kp = known_plan()
        k = (kp.keep != 0).expand_as(lat)
        assert len(ops.pins) == STEPS and torch.equal(lat[k], kp.x0[k])
    if case == "nag":
        assert len(ops.nag_calls) == len(ref["computed"]) * CFG.num_layers, "a skipped step runs no forward"


def test_force_skip():
    """Steps 3 and 5 skip whatever the sums say; the restatement does the same."""
    m, lat, plan = engine_loop(EasyOps(), force_skip=(3, 5), thresh=1e-12)
    want = forced_reference()
    assert plan.skipped == [3, 5] == want["skipped"] and plan.computed == [0, 1, 2, 4, 6, 7]
    p = R.psnr(lat, want["lat"])
    assert p >= 40.0, f"{p:.1f} dB"


# ---- 4. scope ---------------------------------------------------------------------------------------------------------------------------
def _pipe(ops=None, vae=None, dtype=torch.bfloat16):
    return WanVideoPipeline("cpu", dtype, DiTHolder(syn.make_dit_state_dict(CFG), CFG), HashTextEncoder(CFG), vae or PoolVAE(),
                            ops=ops or EasyOps())


def _call_kw(**extra):
    kw = dict(prompt="a street", negative_prompt="bad", height=GRID.height, width=GRID.width, num_frames=GRID.num_frames, seed=3,
              num_inference_steps=6, return_latents=True)
    kw.update(extra)
    return kw


class TracedEasyOps(EasyTwins, TracedOps):
    """TracedOps + the twins: the new ops show in the log."""


def test_scope_errors(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    tr = Trace()
    ops = TracedEasyOps(tr)
    tr.on = True
    p = _pipe(ops)
    monkeypatch.setattr(p, "_get_engine", lambda: pytest.fail("the engine was built before the settings were validated"))
    for bad in (0.0, -1.0, float("nan"), "0.05", True):
        with pytest.raises(ValueError, match="easy_cache_thresh must be"):
            p(**_call_kw(easy_cache_thresh=bad))
    for bad in (1, 2.0, "2", True):
        with pytest.raises(ValueError, match="easy_cache_warmup_steps must be"):
            p(**_call_kw(easy_cache_thresh=0.05, easy_cache_warmup_steps=bad))
    with pytest.raises(ValueError, match="easy_cache_warmup_steps given without easy_cache_thresh"):
        p(**_call_kw(easy_cache_warmup_steps=4))
    with pytest.raises(ValueError, match="easy_cache_thresh cannot be combined with TeaCache .* yet"):
        p(**_call_kw(easy_cache_thresh=0.05, tea_cache_l1_thresh=0.1, tea_cache_model_id="Wan2.1-T2V-1.3B"))
    with pytest.raises(ValueError, match="easy_cache_thresh cannot be combined with sliding_window_size.* yet"):
        p(**_call_kw(easy_cache_thresh=0.05, sliding_window_size=2, sliding_window_stride=1))
    import torch.distributed as dist
    with monkeypatch.context() as mp:
        mp.setattr(dist, "is_initialized", lambda: True)
        mp.setattr(dist, "get_world_size", lambda *a: 2)
        mp.setattr(dist, "get_rank", lambda *a: 0)
        with pytest.raises(ValueError, match="easy_cache_thresh cannot be combined with a process group of 2 ranks yet"):
            p(**_call_kw(easy_cache_thresh=0.05))
    assert tr.log == [], "a refused call must not reach an operator"
    # the engine says the same when it is driven directly, before any launch
    cfg, sd, bsd, noise, c1, c2, bl, _, _ = inputs()
    sch = FlowMatchScheduler(3)
    ops = EasyOps()
    m = WanDiT(cfg, sd, ops, bsd).prepare(GRID)
    cc, cu, plan = m.encode_context(c1), m.encode_context(c2), E.EasyCachePlan(0.05, 2)
    calls = []
    monkeypatch.setattr(ops, "gemm", lambda *a, **k: calls.append("gemm"))
    tea = teacache.TeaCachePlan("test-linear", 0.0, (0, 1, 2), (0.0,) * 3, (0, 1, 2))
    with pytest.raises(ValueError, match=r"easy_cache=\) cannot be combined with TeaCache \(tea_cache=\) in the same call yet"):
        m.denoise(noise.clone(), cc, cu, None, sch, 5.0, tea_cache=tea, easy_cache=plan)
    with pytest.raises(ValueError, match=r"easy_cache=\) cannot be combined with sequence / CFG-branch parallelism \(world > 1\) yet"):
        m.denoise(noise.clone(), cc, None, None, sch, 5.0, branch_exchange=lambda own, both: None, easy_cache=plan)
    msp = WanDiT(cfg, sd, ops, bsd).prepare(GRID, force_sp=True)
    with pytest.raises(ValueError, match=r"easy_cache=\) cannot be combined with sequence / CFG-branch parallelism \(world > 1\) yet"):
        msp.denoise(noise.clone(), cc, cu, None, sch, 5.0, easy_cache=plan)
    mw = WanDiT(cfg, sd, ops, bsd).prepare(TokenGrid(5, 64, 96))
    with pytest.raises(ValueError, match=r"easy_cache=\) cannot be combined with more than one sliding temporal window yet"):
        mw.denoise(noise.clone(), cc, cu, None, sch, 5.0, sliding_window=SW.plan(GRID.T, 2, 1), easy_cache=plan)
    with pytest.raises(ValueError, match=r"easy_cache=\) measures the conditional head output"):
        m.denoise(noise.clone(), None, cu, None, sch, 5.0, easy_cache=plan)
    assert not calls and not getattr(ops, "easy_calls", []) and m._easy_state is None and plan.record()["computed"] == []
    # one sliding window is no combination
    p = _pipe()
    one = p(**_call_kw(easy_cache_thresh=1e9, easy_cache_warmup_steps=2, sliding_window_size=GRID.T, sliding_window_stride=GRID.T))
    assert p.sliding_window_record is None and torch.equal(one, p(**_call_kw(easy_cache_thresh=1e9, easy_cache_warmup_steps=2)))


def test_worker_pool_combination_raises(monkeypatch):
    """ICV_WORLD > 1 behind the unchanged generator: refused in the client before a request reaches the ranks."""
    from infinicube_amd.videogen.inference import WanVideoGenerator
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    g = WanVideoGenerator.__new__(WanVideoGenerator)
    g._pool, g.pipe = object(), _pipe()
    g.pipe.easy_cache_thresh = 0.05
    sem, co = syn.make_dummy_buffers(GRID)
    with pytest.raises(ValueError, match="easy_cache_thresh cannot be combined with ICV_WORLD > 1"):
        g.generate(sem, co, seed=0)


# ---- 5. the pipeline: off, keyword, attribute, record -----------------------------------------------------------------------------------
def test_off_is_the_plain_path(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)

    def run(ops_cls, **kw):
        tr = Trace()
        ops = ops_cls(tr)                         # TracedOps has none of the three new ops: calling one would raise
        p = _pipe(ops)
        allocs, raw = [], ops.alloc
        monkeypatch.setattr(ops, "alloc", lambda shape, dtype: (allocs.append((tuple(shape), dtype)), raw(shape, dtype))[1])
        tr.on = True
        lat = p(**_call_kw(**kw))
        tr.on = False
        return tr.log, allocs, lat, p

    log0, allocs0, lat0, _ = run(TracedOps)
    names0 = [e[0] for e in log0]
    assert names0.count("unpatchify_cfg_euler") == 6
    log1, allocs1, lat1, p = run(TracedOps, easy_cache_thresh=None, easy_cache_warmup_steps=None)
    assert p.easy_cache_record is None and p._engine._easy_state is None
    assert torch.equal(lat1, lat0) and log1 == log0 and allocs1 == allocs0, "None must be the path without the keywords"
    # on, every rule step skipped (steps 2, 3, 4 of 6): three forwards' launches are gone, one predict each, one read per step, five buffers
    log2, allocs2, lat2, p = run(TracedEasyOps, easy_cache_thresh=1e9, easy_cache_warmup_steps=2)
    names2 = [e[0] for e in log2]
    rec = p.easy_cache_record
    assert rec["computed"] == [0, 1, 5] and rec["skipped"] == [2, 3, 4] and rec["thresh"] == 1e9 and rec["warmup_steps"] == 2
    assert names2.count("easycache_predict") == 3 and names2.count("read_doubles") == 6 and names2.count("unpatchify_cfg_euler") == 6
    assert names0.count("attention") % 6 == 0 and names2.count("attention") == names0.count("attention") // 2, "attention runs in the blocks only"
    assert all(names2[j + 1] == "unpatchify_cfg_euler" for j, n in enumerate(names2) if n == "easycache_predict")
    # 6 x (x vs x_prev) + 5 x (x vs x_last, once a computed step exists) + 3 x (the computed steps' head outputs)
    assert names2.count("l1_change") == 6 + 5 + 3
    eng = p._engine
    new = [(tuple(lat0.shape), F32)] * 2 + [(tuple(eng.head_out.shape), F32), ((WORKSPACE,), F64), ((8,), F64)]
    assert Counter(allocs2) == Counter(allocs0) + Counter(new), "the four state buffers, the workspace and the sums, nothing else"
    assert not torch.equal(lat2, lat0) and torch.isfinite(lat2).all()
    assert (p.easy_cache_thresh, p.easy_cache_warmup_steps) == (None, None), "a keyword does not become an attribute"
    base = p(**_call_kw())                          # ... and does not outlive its call
    assert p.easy_cache_record is None and torch.equal(base, lat0)


def test_attributes_precedence_and_record(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    p = _pipe()
    assert (p.easy_cache_thresh, p.easy_cache_warmup_steps, p.easy_cache_record) == (None, None, None)
    plain = p(**_call_kw())
    want = p(**_call_kw(easy_cache_thresh=1e9, easy_cache_warmup_steps=3))
    assert p.easy_cache_record["computed"] == [0, 1, 2, 5] and not torch.equal(want, plain)
    p.easy_cache_thresh, p.easy_cache_warmup_steps = 1e9, 3
    assert torch.equal(p(**_call_kw()), want) and p.easy_cache_record["skipped"] == [3, 4]
    other = p(**_call_kw(easy_cache_warmup_steps=2))              # a keyword wins over its attribute, each setting on its own
    assert p.easy_cache_record["computed"] == [0, 1, 5] and p.easy_cache_record["thresh"] == 1e9 and not torch.equal(other, want)
    never = p(**_call_kw(easy_cache_thresh=1e-12))
    assert p.easy_cache_record["skipped"] == [] and p.easy_cache_record["warmup_steps"] == 3 and torch.equal(never, plain)
    rec = p.easy_cache_record
    assert set(rec) == {"thresh", "warmup_steps", "computed", "skipped", "k", "accumulated"} and len(rec["k"]) == len(rec["accumulated"]) == 6
    # the default warm-up is 10 executed steps: a 6-step call computes every step
    p.easy_cache_warmup_steps = None
    assert torch.equal(p(**_call_kw()), plain) and p.easy_cache_record["warmup_steps"] == 10 and p.easy_cache_record["skipped"] == []


def test_attribute_route_through_the_generator(tmp_path, monkeypatch):
    """The caller of the unchanged WanVideoGenerator: gen.pipe.easy_cache_thresh = ...; gen.pipe.easy_cache_warmup_steps = ..."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    vae = CountingVAE()
    g, sem, co = generator_through_env(lambda torch_dtype, device, model_configs: _pipe(vae=vae), tmp_path, monkeypatch, GRID, "cpu",
                                       ICV_SAMPLE_STEPS="6")
    assert g.pipe.easy_cache_record is None
    plain = vae.last_decoded
    g.pipe.easy_cache_thresh, g.pipe.easy_cache_warmup_steps = 1e9, 2
    video = g.generate(sem, co, prompt="a street", negative_prompt="bad", seed=3)
    assert len(video) == GRID.num_frames and g.pipe.easy_cache_record["skipped"] == [2, 3, 4]
    assert not torch.equal(vae.last_decoded, plain)


# ---- 6. the C entry points' argument checks (they run on the host, before any launch) -----------------------------------------------------
def test_argument_errors_without_gpu():
    from infinicube_amd import native
    lib = native.lib()
    assert native.L1_CHANGE_WORKSPACE_DOUBLES == WORKSPACE

    def l1(**kw):
        a = dict(a=0x10000, lda=64, b=0x20000, ldb=64, rows=23, cols=64, work=0x30000, out=0x40000)
        a.update(kw)
        rc = lib.icv_l1_change_f64(a["a"], a["lda"], a["b"], a["ldb"], a["rows"], a["cols"], 1, a["work"], a["out"], None)
        return rc, lib.icv_last_error()

    for kw, msg in ((dict(a=None), b"null argument"), (dict(b=None), b"null argument"), (dict(work=None), b"null argument"),
                    (dict(out=None), b"null argument"), (dict(rows=0), b"bad shape"), (dict(cols=-1), b"bad shape"),
                    (dict(lda=63), b"is less than the 64 columns of a row"), (dict(ldb=10), b"is less than the 64 columns of a row"),
                    (dict(a=0x10002), b"4-byte aligned"), (dict(work=0x30004), b"8-byte aligned"), (dict(out=0x40004), b"8-byte aligned"),
                    (dict(b=0x10000), b"must not overlap"), (dict(b=0x10000 + 22 * 64 * 4), b"must not overlap"),
                    (dict(out=0x30000 + 8 * 100), b"out2 lies inside the workspace")):
        rc, err = l1(**kw)
        assert rc != 0 and msg in err, (kw, rc, err)

    def predict(**kw):
        a = dict(x=0x10000, xl=0x20000, hcl=0x30000, hul=0x40000, hc=0x50000, hu=0x60000, ldh=64, C=16, T=3, H8=8, W8=12, tok0=0, n_tok=72)
        a.update(kw)
        rc = lib.icv_easycache_predict_f32(a["x"], a["xl"], a["hcl"], a["hul"], a["hc"], a["hu"], a["ldh"], a["C"], a["T"], a["H8"], a["W8"],
                                           a["tok0"], a["n_tok"], None)
        return rc, lib.icv_last_error()

    for kw, msg in ((dict(x=None), b"null argument"), (dict(xl=None), b"null argument"), (dict(hcl=None), b"null argument"),
                    (dict(hc=None), b"null argument"), (dict(hu=None), b"given together"), (dict(hul=None), b"given together"),
                    (dict(hc=0x30000), b"buffers of their own"), (dict(hu=0x50000), b"buffers of their own"),
                    (dict(H8=7), b"bad latent shape"), (dict(W8=11), b"bad latent shape"), (dict(C=0), b"bad latent shape"),
                    (dict(ldh=63), b"is less than the 64 columns of a row"), (dict(n_tok=0), b"token range"),
                    (dict(tok0=1), b"token range [1, 73)"), (dict(tok0=-1), b"token range"), (dict(x=0x10004), b"8-byte aligned"),
                    (dict(hc=0x50002), b"4-byte aligned")):
        rc, err = predict(**kw)
        assert rc != 0 and msg in err, (kw, rc, err)
