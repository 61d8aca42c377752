"""Enhance-A-Video on the HIP path (csrc/enhance.hip): icv_enhance_scores_bf16 against the float64 rule (tests/enhance_ref.py) on the
same bf16 inputs - the smallest grid, ragged tiles, a full 32-frame tile, ld != d, NaN around the slice, peaked logits, two runs and
two pointer alignments - icv_enhance_apply_bf16 bit for bit against one rounding of f32(att) * E with its guard columns, the refused
calls; the loop of tests/test_enhance_cpu.py on the per-op, graph and one-call drivers, a second graph key, the record, the
compositions (UniPC, a forced TeaCache skip, NAG, the frame window, the e4m3 mode, an image-to-video DiT, LoRA), and the pipeline.

Score shapes are (T, P, H): T frames on the lanes of one 32 x 32 MFMA tile (T = 2: two live rows; 21, 24, 31: a ragged tile; 32: a
full one), one work-group of four waves per position (P = 1, 3, 7, 64, 130), the heads dealt to the waves (H = 1: three idle waves;
2, 5: some idle / an uneven deal; 12, 40: several heads per wave).

The bound on E, per case: relative error <= 2 ln 2 * 128 * 2^-24 * max_(t, t', s, h) sum_c |q k| + 8 * 2^-24 (the f32 accumulation of
128 bf16 products pushed through the softmax's derivative; the exp and the divisions)."""
import math

import pytest
import torch

from enhance_ref import BF16, LN2, EnhanceForward, ScoreRecorder, enhance_bound, enhance_rule, enhance_velocity
from infinicube_amd.videogen import enhance as E
from infinicube_amd.videogen import synthetic as syn
from infinicube_amd.videogen import teacache
from infinicube_amd.videogen.config import TokenGrid, preset
from infinicube_amd.videogen.dit import WanDiT
from infinicube_amd.videogen.scheduler import FlowMatchScheduler, flow_match_sigmas
from oracle import wan_ref as R
from test_enhance_cpu import (CFG, CFG_SCALE, ENV, GAINS, GRID, LOG2E_RSQRT_HD, LOOP_STEPS, NAG, WEIGHT, check_loop, check_scores, engine_loop,
                              one_hot_logits, reference)
from test_solver_cpu import STIFF, restated_sample

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
SENTINEL = -7.0
SHAPES = [(2, 1, 1), (21, 7, 12), (24, 130, 5), (32, 3, 40), (31, 64, 2)]
APPLY_SHAPES = [(1, 1536, 1536), (63, 2304, 2312), (4099, 5120, 5120), (63, 5120, 5184), (4099, 1536, 1544)]      # (rows, d, ld)

_DATA = {}


def data(T, P, H, kind="normal"):
    """q, k bf16 [T * P, H * 128] and the float64 rule on them, once per case.  "normal": q ~ N(0, 1), k ~ N(0, 1) * 3 (1 / sqrt(hd))
    log2 e - logits of std 3, a softmax that is neither uniform nor one-hot.  "peaked": the same with one channel of every q row
    at +-40 and of every k row at +-8, logits of +-320 in units of log2: the max subtraction."""
    key = (T, P, H, kind)
    if key not in _DATA:
        g = torch.Generator().manual_seed(1000 * T + 10 * P + H)
        q = torch.randn((T * P, H * 128), generator=g)
        k = torch.randn((T * P, H * 128), generator=g) * 3.0 * LOG2E_RSQRT_HD
        if kind == "peaked":
            sq = torch.randint(0, 2, (T * P, H), generator=g).float() * 2 - 1
            sk = torch.randint(0, 2, (T * P, H), generator=g).float() * 2 - 1
            q.view(T * P, H, 128)[:, :, 5] = 40.0 * sq
            k.view(T * P, H, 128)[:, :, 5] = 8.0 * sk
        q, k = q.to(BF16), k.to(BF16)
        _DATA[key] = (q, k) + enhance_rule(q, k, T, P, H, LN2, WEIGHT)
    return _DATA[key]


def run_scores(hip_ops, q, k, T, P, H, weight=WEIGHT, ld=None, offset=0, nan_around=False):
    """E from icv_enhance_scores_bf16 (+ its one-group second launch) and, separately, from icv_enhance_apply_bf16's own sum; the
    partial sums.  q, k live at element ``offset`` of a larger allocation with row stride ``ld``; ``nan_around``: everything in that
    allocation outside the [T * P, H * 128] slice - the columns beyond d and 40 more rows behind the last - holds NaN."""
    d = H * 128
    ld = ld or d
    rows = T * P
    fill = float("nan") if nan_around else SENTINEL

    def place(x):
        flat = torch.full((offset + (rows + 40) * ld + 8,), fill, dtype=BF16, device=DEV)
        view = flat[offset: offset + rows * ld].view(rows, ld)[:, :d]
        view.copy_(x.to(DEV))
        assert view.data_ptr() % 16 == 0
        return view

    qv, kv = place(q), place(k)
    ws = torch.full((P + 3,), SENTINEL, dtype=F32, device=DEV)
    out = torch.full((3,), SENTINEL, dtype=F32, device=DEV)
    hip_ops.enhance_scores(qv, kv, T, P, H, LN2, weight, ws, out[1:2])
    att = torch.ones((8, 8), dtype=BF16, device=DEV)
    out2 = torch.full((3,), SENTINEL, dtype=F32, device=DEV)
    hip_ops.enhance_apply(att, ws, T, P, H, weight, out2[1:2])
    torch.cuda.synchronize()
    assert float(out[0]) == SENTINEL == float(out[2]) and float(out2[0]) == SENTINEL == float(out2[2])
    assert bool((ws[P:] == SENTINEL).all()), "partial sums written beyond P"
    assert torch.equal(qv.cpu(), q) and torch.equal(kv.cpu(), k)
    assert float(out[1]) == float(out2[1]), "both launches must form the same E from the same partial sums"
    assert torch.equal(att.cpu(), (torch.ones((8, 8)) * float(out2[1])).to(BF16))
    return float(out[1]), ws[:P].cpu()


# ---- 1. the score kernel against float64 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,P,H", SHAPES)
@pytest.mark.parametrize("kind", ["normal", "peaked"])
def test_scores_match_float64(hip_ops, T, P, H, kind):
    q, k, want, m, absdot = data(T, P, H, kind)
    got, ws = run_scores(hip_ops, q, k, T, P, H)
    bound = enhance_bound(absdot)
    err = abs(got - want) / want
    part = float(((ws.double() / (T * (T - 1)) - m.sum(-1)).abs() / m.sum(-1).clamp_min(1e-300)).max())
    print(f"{(T, P, H)} {kind}: E {got:.7f}, float64 {want:.7f}, relative error {err:.2e}, bound {bound:.2e} (max sum |q k| {absdot:.1f}); "
          f"worst per-position partial sum {part:.2e}")
    assert kind == "peaked" or 1.0 < want < (T + WEIGHT) / (T - 1), "the case must not sit on either end of E's range"
    assert err <= bound
    assert part <= bound or kind == "peaked", "every position's own sum, not only their mean"


def test_scores_with_ld_and_nan_around_the_slice(hip_ops):
    """ld != d; a slice of a larger tensor whose columns >= d and whose rows after T * P hold NaN: the padding frames of the 32-row tile
    are neither read nor leaked.  Two runs and two pointer alignments (16 and 48 bytes into the allocation) give identical bits."""
    for T, P, H in ((21, 7, 12), (31, 64, 2), (2, 1, 1)):
        q, k, want, _, absdot = data(T, P, H)
        base, ws0 = run_scores(hip_ops, q, k, T, P, H)
        for ld, offset, nan in ((H * 128 + 8, 8, False), (H * 128 + 72, 24, True), (H * 128, 24, True), (H * 128 + 8, 8, False)):
            got, ws = run_scores(hip_ops, q, k, T, P, H, ld=ld, offset=offset, nan_around=nan)
            assert math.isfinite(got) and got == base and torch.equal(ws, ws0), (T, P, H, ld, offset, nan)
        assert abs(base - want) / want <= enhance_bound(absdot)


@pytest.mark.parametrize("T,P,H", [(2, 1, 1), (21, 7, 12), (32, 3, 40)])
def test_scores_closed_forms(hip_ops, T, P, H):
    for w in (0.0, WEIGHT):
        const = torch.full((T * P, H * 128), 0.25, dtype=BF16)
        got, _ = run_scores(hip_ops, const, const.clone(), T, P, H, weight=w)
        assert abs(got - (1.0 + w / T)) <= 8 * 2.0 ** -24 * (1.0 + w / T) or (w == 0.0 and got == 1.0), "uniform attention"
        q, k = one_hot_logits(T, P, H, 0, peak=200.0)
        got, ws = run_scores(hip_ops, q, k, T, P, H, weight=w)
        assert got == 1.0 and bool((ws == 0).all()), "one-hot diagonal logits: E = 1"
        q, k = one_hot_logits(T, P, H, 1, peak=200.0)
        got, _ = run_scores(hip_ops, q, k, T, P, H, weight=w)
        top = (T + w) / (T - 1)
        assert abs(got - top) <= 8 * 2.0 ** -24 * top, "one-hot off-diagonal logits: the ceiling"


# ---- 2. apply ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,d,ld", APPLY_SHAPES)
def test_apply_is_one_rounding_of_the_product(hip_ops, rows, d, ld):
    T, P, H = 21, 7, 12
    q, k, want, _, absdot = data(T, P, H)
    ws = torch.zeros((P,), dtype=F32, device=DEV)
    hip_ops.enhance_scores(q.to(DEV), k.to(DEV), T, P, H, LN2, WEIGHT, ws)
    g = torch.Generator().manual_seed(rows + d)
    att = (torch.randn((rows, d), generator=g) * 3.0).to(BF16)
    att[0, :4] = torch.tensor([0.0, -0.0, float("inf"), 1e-30]).to(BF16)
    pad = 64
    flat = torch.full((pad + rows * ld + pad,), SENTINEL, dtype=BF16, device=DEV)
    view = flat[pad: pad + rows * ld].view(rows, ld)[:, :d]
    view.copy_(att.to(DEV))
    out = torch.zeros((1,), dtype=F32, device=DEV)
    hip_ops.enhance_apply(view, ws, T, P, H, WEIGHT, out)
    torch.cuda.synchronize()
    e = float(out)
    assert abs(e - want) / want <= enhance_bound(absdot) and e > 1.0
    assert torch.equal(view.cpu().view(torch.int16), (att.float() * out.cpu()).to(BF16).view(torch.int16)), "bf16(f32(att) * E), bit for bit"
    body = flat[pad: pad + rows * ld].view(rows, ld)
    assert bool((body[:, d:] == SENTINEL).all() and (flat[:pad] == SENTINEL).all() and (flat[-pad:] == SENTINEL).all()), "guard columns"
    # E == 1 (nothing looks across frames): the plain bits, NaN payloads and all
    qd, kd = one_hot_logits(T, P, H, 0, peak=200.0)
    hip_ops.enhance_scores(qd.to(DEV), kd.to(DEV), T, P, H, LN2, WEIGHT, ws)
    raw = torch.randint(-32768, 32767, (rows, d), generator=g, dtype=torch.int16)
    view.copy_(raw.view(BF16).to(DEV))
    hip_ops.enhance_apply(view, ws, T, P, H, WEIGHT, out)
    torch.cuda.synchronize()
    assert float(out) == 1.0 and torch.equal(view.cpu().view(torch.int16), raw)


def test_refused_calls_launch_nothing(hip_ops):
    from infinicube_amd import native
    lib = native.lib()
    T, P, H = 5, 3, 2
    q = torch.zeros((T * P, H * 128), dtype=BF16, device=DEV)
    ws = torch.full((P,), SENTINEL, dtype=F32, device=DEV)
    out = torch.full((1,), SENTINEL, dtype=F32, device=DEV)
    att = torch.full((T * P, H * 128), SENTINEL, dtype=BF16, device=DEV)
    st = hip_ops._stream()
    for frames in (1, 33):
        with pytest.raises(ValueError, match="2 <= frames <= 32"):
            hip_ops.enhance_scores(torch.zeros((frames * P, H * 128), dtype=BF16, device=DEV), torch.zeros((frames * P, H * 128), dtype=BF16, device=DEV),
                                   frames, P, H, LN2, WEIGHT, ws, out)
        assert lib.icv_enhance_scores_bf16(q.data_ptr(), 256, q.data_ptr(), 256, frames, P, H, LN2, WEIGHT, ws.data_ptr(), out.data_ptr(), st) != 0
        assert b"must be in [2, 32]" in lib.icv_last_error()
        with pytest.raises(ValueError, match="2 <= frames <= 32"):
            hip_ops.enhance_apply(att, ws, frames, P, H, WEIGHT, out)
    with pytest.raises(ValueError, match="heads \\* 128"):                           # a head width other than 128
        hip_ops.enhance_scores(q[:, :192], q[:, :192], T, P, H, LN2, WEIGHT, ws, out)
    with pytest.raises(ValueError, match="multiples of 8"):                          # a bad ld
        odd = torch.zeros((T * P, H * 128 + 4), dtype=BF16, device=DEV)
        hip_ops.enhance_scores(odd[:, :H * 128], q, T, P, H, LN2, WEIGHT, ws, out)
    with pytest.raises(ValueError, match="16-byte-aligned"):
        flat = torch.zeros((T * P * H * 128 + 8,), dtype=BF16, device=DEV)
        hip_ops.enhance_scores(flat[4: 4 + T * P * H * 128].view(T * P, H * 128), q, T, P, H, LN2, WEIGHT, ws, out)
    with pytest.raises(ValueError, match="one contiguous float per position"):
        hip_ops.enhance_scores(q, q, T, P, H, LN2, WEIGHT, ws[:2], out)
    with pytest.raises(ValueError, match="one contiguous float per position"):
        hip_ops.enhance_apply(att, ws, T, native.ENHANCE_WORKSPACE_FLOATS + 1, H, WEIGHT, out)
    with pytest.raises(ValueError, match="d % 8 == 0"):
        hip_ops.enhance_apply(att[:, :100], ws, T, P, H, WEIGHT, out)
    for bad in (dict(q=q.float()), dict(k=q.to(torch.float16)), dict(ws=ws.double())):
        a = dict(q=q, k=q, ws=ws)
        a.update(bad)
        with pytest.raises(TypeError, match="enhance_scores"):
            hip_ops.enhance_scores(a["q"], a["k"], T, P, H, LN2, WEIGHT, a["ws"], out)
    with pytest.raises(TypeError, match="enhance_apply"):
        hip_ops.enhance_apply(att.float(), ws, T, P, H, WEIGHT, out)
    torch.cuda.synchronize()
    assert bool((ws == SENTINEL).all() and (out == SENTINEL).all() and (att == SENTINEL).all()), "a refused call must not launch"


# ---- 3. the loop, per driver ----------------------------------------------------------------------------------------------------------
_PER_OP = {}


def per_op(hip_ops):
    if "v" not in _PER_OP:
        m, lat = engine_loop(hip_ops, prep=dict(graphs=False), dev=DEV)
        torch.cuda.synchronize()
        assert not m._graphs_on and m._enhance_E is not None and m._enhance is None
        _PER_OP["v"] = (m, lat.cpu())
    return _PER_OP["v"]


@pytest.fixture(autouse=True)
def _unwrap(hip_ops):
    """ScoreRecorder wraps the two operators on the shared operator set: take the wrappers off behind every test."""
    yield
    for name in ("enhance_scores", "enhance_apply"):
        hip_ops.__dict__.pop(name, None)


@pytest.mark.parametrize("mode", ["per-op", "graphs", "native"])
def test_loop_matches_restated_loop(hip_ops, mode, monkeypatch):
    """The loop of test_enhance_cpu on HipOps (tiny preset, 5 latent frames, a CFG pair at cfg_scale 5, Euler, 6 steps, that file's
    gains)."""
    if mode == "per-op":
        m, lat = per_op(hip_ops)
        check_scores(m, reference(), mode)
        got = m.enhance_scores
        assert got[0][0] == got[1][0] and got[0][1] != got[1][1], "a CFG pair: layer 0 is shared, behind it each branch has its own E"
    elif mode == "graphs":
        m, lat = engine_loop(hip_ops, prep=dict(graphs=True), dev=DEV)
        torch.cuda.synchronize()
        assert m._graphs_on and len(m._graphs) == 2 and sorted(k[-1] for k in m._graphs) == [(WEIGHT, 0), (WEIGHT, 1)]
        assert m.enhance_scores == per_op(hip_ops)[0].enhance_scores, "replayed launches write the same factors"
    else:
        monkeypatch.setenv("ICV_NATIVE_FORWARD", "1")
        m, lat = engine_loop(hip_ops, prep=dict(graphs=False), dev=DEV)
        torch.cuda.synchronize()
        assert m.native_forward and m._native is None, "the one-call driver does not know the launches: the per-op driver runs"
        assert torch.equal(lat.cpu(), per_op(hip_ops)[1]), "... with the per-op driver's bits"
    assert torch.isfinite(lat).all()
    check_loop(lat, mode)
    p_plain = R.psnr(reference(None)[0], reference()[0])
    assert p_plain < 30.0, f"plain vs enhanced {p_plain:.1f} dB: the bar could pass with the feature ignored"


def test_dual_stream_and_sequential_drivers(hip_ops):
    """The uncond forward on a second stream in a twin engine (its own partial sums, row 1 of the SAME factor buffer), and the two
    forwards one after the other without the 2n-row batch: the batched pair's bits and factors."""
    want_m, want = per_op(hip_ops)
    assert want_m._pair is not None

    def dual(m):
        m.dual_stream = True

    def sequential(m):
        m.cfg_batch = False

    for name, setup in (("dual stream", dual), ("sequential", sequential)):
        m, lat = engine_loop(hip_ops, prep=dict(graphs=False), dev=DEV, setup=setup)
        torch.cuda.synchronize()
        assert m._pair is None and (m._twin is not None) == (name == "dual stream")
        check_loop(lat, name)
        m.test_recorder.check(m, name)
        assert torch.equal(lat.cpu(), want) and m.enhance_scores == want_m.enhance_scores, name


def test_record_against_the_restated_loop(hip_ops):
    """Per-layer E of the record against the RESTATED LOOP's E of its last forward, within the kernel bound 2 ln 2 * 128 * 2^-24 *
    max sum |q k| + 8 * 2^-24, on the per-op loop (CFG pair, Euler, 6 steps).  The two sides' q, k are not the same numbers here: the
    restatement's are f32 values of its own trajectory rounded to bf16 once, the engine's come out of bf16 activations, a bf16 GEMM
    output and a bf16 store.  Measured on one MI355X: relative errors 9.1e-05 to 1.19e-04 against bounds of 1.42e-04 to 1.46e-04 (the
    worst at 0.82 of its bound); against float64 on the engine's OWN q, k (check_scores, every loop test here) the same factors are
    within 1e-07."""
    m, _ = per_op(hip_ops)
    _, scores, absdots = reference()
    worst = 0.0
    for b, (gb, sb, ab) in enumerate(zip(m.enhance_scores, scores, absdots)):
        for i, (g, s, a) in enumerate(zip(gb, sb, ab)):
            err, bound = abs(g - s) / s, enhance_bound(a)
            worst = max(worst, err / bound)
            print(f"branch {b} layer {i}: E {g:.7f}, restated loop {s:.7f}, relative error {err:.2e}, bound {bound:.2e}")
    assert worst <= 1.0, f"worst relative error / bound = {worst:.2f}"


def test_two_graph_keys(hip_ops):
    """One engine under graphs, the same contexts, buffer tokens and latent tensor in every call: a plain call, an enhanced call and one
    with another weight each match their own restatement - a graph captured for one is never replayed for another."""
    m, plain = engine_loop(hip_ops, weight=None, prep=dict(graphs=True), dev=DEV)
    torch.cuda.synchronize()
    assert m._graphs_on and len(m._graphs) == 2 and m._enhance_E is None
    check_loop(plain, "graphs, plain", ref=reference(None)[0])
    _, first = engine_loop(hip_ops, engine=m)
    torch.cuda.synchronize()
    assert len(m._graphs) == 4
    check_loop(first, "graphs, weight 4")
    _, second = engine_loop(hip_ops, weight=1.0, engine=m)
    torch.cuda.synchronize()
    assert len(m._graphs) == 6
    check_loop(second, "graphs, weight 1", ref=reference(1.0)[0])
    assert max(R.psnr(reference(1.0)[0], reference()[0]), R.psnr(reference(1.0)[0], reference(None)[0])) < 35.0, "a stale graph must miss the bar"
    _, again = engine_loop(hip_ops, engine=m)                                    # replayed
    torch.cuda.synchronize()
    assert len(m._graphs) == 6 and torch.equal(again, first)


# ---- 4. compositions ------------------------------------------------------------------------------------------------------------------
def test_with_unipc(hip_ops):
    m, lat = engine_loop(hip_ops, solver="unipc", dev=DEV)
    torch.cuda.synchronize()
    check_loop(lat, "UniPC", ref=reference(solver="unipc")[0])
    check_scores(m, reference(solver="unipc"), "UniPC")
    assert m._solver_state is not None


def test_with_teacache_one_forced_skip(hip_ops):
    """Step 3 of 6 runs no blocks, so no measurement and no scaling: the residual of step 2 (computed with the feature) is added."""
    computed = (0, 1, 2, 4, 5)
    plan = lambda m, sch: teacache.TeaCachePlan("test-linear", 0.0, tuple(range(LOOP_STEPS)), (0.0,) * LOOP_STEPS, computed)      # noqa: E731
    m, lat = engine_loop(hip_ops, dev=DEV, tea=plan)
    torch.cuda.synchronize()
    ref = reference(tea_skipped=(3,))
    check_loop(lat, "TeaCache (step 3 skipped)", ref=ref[0])
    check_scores(m, ref, "TeaCache")
    assert m._tc_res is not None and not torch.equal(ref[0], reference()[0]), "the skip must change the restated result"


def test_with_nag(hip_ops):
    m, lat = engine_loop(hip_ops, dev=DEV, nag=NAG)
    torch.cuda.synchronize()
    ref = reference(nag=NAG, cfg_scale=1.0)
    check_loop(lat, "NAG", ref=ref[0])
    check_scores(m, ref, "NAG")
    assert R.psnr(reference(None, nag=NAG, cfg_scale=1.0)[0], ref[0]) < 30.0 and m._nag_buf is not None


def test_with_the_frame_window(hip_ops):
    """Window 1 + 1 anchor frame (tests/test_attn_window_gpu.py's setting and bar): the attention is masked, E is over all T frames."""
    m, lat = engine_loop(hip_ops, dev=DEV, prep=dict(graphs=False), setup=lambda m: m.set_attention_window(1, 1))
    torch.cuda.synchronize()
    assert m._framewin() == (1, 1)
    ref = reference(window=(1, 1))
    check_loop(lat, "frame window", ref=ref[0])
    check_scores(m, ref, "frame window")
    assert not torch.equal(lat.cpu(), per_op(hip_ops)[1])


E4M3 = dict(weight=16.0, gains=dict(self_attn_o=4.0))


def test_with_the_e4m3_mode(hip_ops):
    """The six projections on the fp8 MFMA, then the e4m3 self-attention too: the bf16 q / k exist in front of attention_fp8, the scaled
    output is what the O projection quantises.  Bar: the e4m3 mode's loop bar, >= 40 dB against the restatement with the same e4m3 row
    quantisation (tests/test_dit_gpu.py test_fp8_gemm_mode_forward_and_loop).
    Inputs.  The e4m3 operand of the O projection carries a rounding of 2^-4 per element against 2^-9 in bf16, and E multiplies that
    noise with the signal: with the self-attention O projection x g, the feature's effect on the latent grows like g (E - 1) and the
    e4m3 noise of that path like g E.  At g = 32 (the bf16 tests' gain) the PLAIN e4m3 loop sits at its own bar (40.9 dB on the CPU
    operator set), so no boost of that path can stay above it.  g = 4 with weight 16 (E = 4.1) keeps the effect (restated plain vs
    restated enhanced loop 27.7 dB, asserted < 30) at 1/8 of that noise; measured on the CPU operator set: 43.0 dB, the plain e4m3 loop
    at the same gains 43.1 dB."""
    ref = reference(E4M3["weight"], fp8=True, gains=E4M3["gains"])
    p_plain = R.psnr(reference(None, fp8=True, gains=E4M3["gains"])[0], ref[0])
    assert p_plain < 30.0, f"plain vs enhanced {p_plain:.1f} dB"
    m, lat = engine_loop(hip_ops, dev=DEV, kw=dict(gemm_dtype="fp8", fp8_weights=WanDiT.FP8_WEIGHTS), **E4M3)
    torch.cuda.synchronize()
    check_loop(lat, "e4m3 GEMMs", ref=ref[0])
    m.test_recorder.check(m, "e4m3 GEMMs")
    m, lat = engine_loop(hip_ops, dev=DEV, kw=dict(gemm_dtype="fp8", attn_dtype="fp8", fp8_weights=WanDiT.FP8_WEIGHTS), **E4M3)
    torch.cuda.synchronize()
    assert m.attn8_ws is not None
    p = R.psnr(lat.cpu(), ref[0])
    print(f"e4m3 GEMMs + e4m3 self-attention vs the fake-quant restatement (bf16 attention): {p:.1f} dB")
    m.test_recorder.check(m, "e4m3 attention")
    assert torch.isfinite(lat).all() and all(e > 1.0 for b in m.enhance_scores for e in b)


def test_with_an_image_to_video_dit(hip_ops):
    """tiny-i2v (tests/test_dit_gpu.py test_i2v_forward_and_loop_parity's config, steps and bar)."""
    cfg, grid = preset("tiny-i2v"), TokenGrid(9, 64, 96)
    sd, bsd = syn.make_dit_state_dict(cfg), syn.make_buffer_embedder_state_dict(cfg)
    for k, g in STIFF.items():             # test_solver_cpu's stiff DiT: a velocity that depends on time and sample
        sd[k] = sd[k] * g
    for suffix, gain in (("self_attn.o.weight", "self_attn_o"), ("cross_attn.o.weight", "cross_attn_o")):
        for k in [k for k in sd if k.endswith(suffix)]:
            sd[k] = sd[k] * GAINS[gain]
    noise, c1, c2 = syn.make_latent_noise(grid), syn.make_text_context(cfg, 1) * GAINS["cond_context"], syn.make_text_context(cfg, 2)
    bl, clip, y = syn.make_buffer_latents(cfg, grid), syn.make_clip_features(cfg), syn.make_cond_latents(cfg, grid)
    m = WanDiT(cfg, sd, hip_ops, bsd).prepare(grid, graphs=False)
    rec = ScoreRecorder(hip_ops)
    ck, cu = m.encode_context(c1, clip), m.encode_context(c2, clip)
    add = m.embed_cond_latents(y, add_to=m.embed_buffers(bl))
    steps = 6
    lat = noise.to(DEV)
    m.denoise(lat, ck, cu, add, FlowMatchScheduler(steps), CFG_SCALE, enhance=E.EnhancePlan(WEIGHT))
    torch.cuda.synchronize()
    sdr, bsdr = R.round_state_dict_to_bf16(sd), R.round_state_dict_to_bf16(bsd)
    sigmas = flow_match_sigmas(steps)
    refs = []
    for w in (WEIGHT, None):
        fwd = [EnhanceForward(sdr, cfg, c, w, R.buffer_embed(bsdr, bl), clip_fea=clip, y=y) for c in (c1, c2)]
        refs.append(restated_sample(enhance_velocity(fwd, sigmas, CFG_SCALE), noise.double(), sigmas, "euler").float())
    p, p_plain = R.psnr(lat.cpu(), refs[0]), R.psnr(refs[1], refs[0])
    print(f"i2v loop vs its restatement: {p:.1f} dB; restated plain i2v loop vs restated enhanced i2v loop: {p_plain:.1f} dB")
    assert p >= 40.0, f"{p:.1f} dB"
    assert p_plain < 40.0 and p_plain <= p - 10.0, f"the bar cannot tell the feature from the plain loop here: plain {p_plain:.1f} dB, engine {p:.1f} dB"
    assert len(m.enhance_scores) == 2 and len(m.enhance_scores[0]) == cfg.num_layers
    rec.check(m, "i2v")


# ---- 5. the pipeline ------------------------------------------------------------------------------------------------------------------
def _pipe():
    from infinicube_amd.videogen.ops import HipOps
    from infinicube_amd.videogen.pipeline import DiTHolder, WanVideoPipeline
    from standins import HashTextEncoder, PoolVAE
    return WanVideoPipeline(DEV, torch.bfloat16, DiTHolder(syn.make_dit_state_dict(CFG), CFG), HashTextEncoder(CFG), PoolVAE(), ops=HipOps(DEV))


def test_pipeline_and_lora(monkeypatch):
    from test_lora_cpu import gridded_adapter
    for key in ENV:
        monkeypatch.delenv(key, raising=False)
    monkeypatch.delenv("ICV_LORA", raising=False)
    kw = dict(prompt="a street", negative_prompt="bad", height=GRID.height, width=GRID.width, num_frames=GRID.num_frames, seed=3,
              num_inference_steps=4, return_latents=True)
    p = _pipe()
    lat = p(**kw, enhance_weight=WEIGHT).cpu()
    rec = p.enhance_record
    assert rec["weight"] == WEIGHT and rec["frames"] == GRID.T and len(rec["scores"]) == 2 and all(len(b) == CFG.num_layers for b in rec["scores"])
    assert all(1.0 < e < (GRID.T + WEIGHT) / (GRID.T - 1) for b in rec["scores"] for e in b)
    plain = p(**kw).cpu()                                                        # the keyword does not outlive its call
    assert p.enhance_record is None
    fresh = _pipe()(**kw).cpu()
    assert torch.equal(plain, fresh), "a call without the keyword must give a fresh pipeline's bits"
    assert torch.isfinite(lat).all() and not torch.equal(lat, fresh), "enhance_weight must not be swallowed"
    # LoRA: the adapter is merged into the weights the measurement's q, k come from
    p.load_lora(p.dit, gridded_adapter(CFG), alpha=0.5)
    both = p(**kw, enhance_weight=WEIGHT).cpu()
    assert p.lora_record is not None and p.enhance_record["scores"] != rec["scores"]
    assert torch.isfinite(both).all() and not torch.equal(both, lat) and not torch.equal(both, p(**kw).cpu())
