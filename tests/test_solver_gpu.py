"""The UniPC multistep sampler on the HIP path (csrc/multistep.hip, icv_unpatchify_cfg_multistep): the kernel against a float64
restatement on the same f32-rounded coefficients at every step kind (bound derived from the arithmetic), its write guard, five steps
in a row through the operator layer against the restated D / rho sequence, the first step at sigma = 1 against icv_unpatchify_cfg_euler,
the loop in every driver mode, its compositions (TeaCache, a shortened sigma range, the e4m3 mode) and the pipeline."""
import pytest
import torch

from infinicube_amd.videogen import solver as S
from infinicube_amd.videogen import synthetic as syn
from infinicube_amd.videogen import teacache
from infinicube_amd.videogen.dit import WanDiT
from infinicube_amd.videogen.scheduler import flow_match_sigmas
from oracle import wan_ref as R
from test_solver_cpu import CFG, ENV, GRID, LOOP_STEPS, engine_loop, inputs, reference, restated_sample

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24               # unit roundoff of f32
SENTINEL = -7.0
PAD = 64                     # floats behind every allocation's last row


def f32(x):
    return float(torch.tensor(float(x), dtype=F32))


def step_kinds():
    """The four kinds of step, from a real plan (8 steps over the range that starts at 0.6: no history entry at sigma = 1)."""
    st = S.MultistepPlan("unipc", flow_match_sigmas(8, denoising_strength=0.6)).steps()
    kinds = {"first": st[0], "corrector 1 + predictor 2": st[1], "both order 2": st[2], "last, t = 0": st[7]}
    assert (kinds["first"].a, kinds["first"].order) == (None, 1)
    assert (kinds["corrector 1 + predictor 2"].corrector_order, kinds["corrector 1 + predictor 2"].order) == (1, 2)
    assert (kinds["both order 2"].corrector_order, kinds["both order 2"].order) == (2, 2)
    assert kinds["last, t = 0"].c == (0.0, 1.0, 0.0) and kinds["last, t = 0"].corrector_order == 2
    return kinds


def scatter(rows, shape, tok0, n_tok):
    """[n_tok, 4C] head rows of the local tokens -> the latent's layout (zeros elsewhere), and the mask of the tokens' elements."""
    C, T, H8, W8 = shape
    grid = (T, H8 // 2, W8 // 2)
    full = torch.zeros((T * grid[1] * grid[2], 4 * C), dtype=rows.dtype)
    mask = torch.zeros((T * grid[1] * grid[2], 4 * C), dtype=F32)
    full[tok0: tok0 + n_tok] = rows[:n_tok]
    mask[tok0: tok0 + n_tok] = 1.0
    return R.unpatchify(full, grid, C), R.unpatchify(mask, grid, C) > 0


def restated_step(x, x_hat, m_prev, m_prev2, hc, hu, cfg_scale, sigma, a, c, tok0, n_tok):
    """One launch in float64 on the f32-rounded scalars -> (m, x_c, x_next, their error bounds), all in the latent's layout.

    The bound.  With u = 2^-24, an f32 sum of products  sum_j coef_j buf_j  evaluated left to right, no fused multiply-adds, has an
    error of at most (roundings on the longest path) u sum_j |coef_j buf_j| to first order in u.  m = x - sigma v: 2 roundings.  x_c:
    the product and three additions for x_hat's term (4), the product and one addition for m's, which is added last (2 + 2).  x_next:
    one product and two additions on top (3).  The longest path has 7 roundings; 8 u sum |coef_j buf_j|, with m expanded into its two
    terms, covers the second-order terms as well.  On top comes the CFG combine's own error e_v = 4 u (|hu| + |cfg| |hc - hu|)
    (three f32 operations, one spare; fused or not), carried to
    each output by the coefficients it passes through."""
    shape = x.shape
    s, cf = f32(sigma), f32(cfg_scale)
    hc64 = hc.double()
    if hu is None:
        v, e_v = hc64, torch.zeros_like(hc64)
    else:
        hu64 = hu.double()
        v = hu64 + cf * (hc64 - hu64)
        e_v = 4.0 * U * (hu64.abs() + abs(cf) * (hc64 - hu64).abs())
    (v, own), (e_v, _) = scatter(v, shape, tok0, n_tok), scatter(e_v, shape, tok0, n_tok)
    x = x.double()
    m, s_m = x - s * v, x.abs() + (s * v).abs()
    b_m = 8.0 * U * s_m + s * e_v
    if a is None:
        xc, s_c, b_c, a3 = x, x.abs(), torch.zeros_like(x), 0.0
    else:
        a0, a1, a2, a3 = (f32(t) for t in a)
        terms = [(a0, x_hat), (a1, m_prev), (a2, m_prev2)]
        xc = sum(k * b.double() for k, b in terms if k != 0.0) + a3 * m
        s_c = sum((k * b.double()).abs() for k, b in terms if k != 0.0) + abs(a3) * s_m
        b_c = 8.0 * U * s_c + abs(a3) * s * e_v
    c0, c1, c2 = (f32(t) for t in c)
    nxt = c0 * xc + c1 * m + (c2 * m_prev.double() if c2 != 0.0 else 0.0)
    s_n = abs(c0) * s_c + abs(c1) * s_m + ((c2 * m_prev.double()).abs() if c2 != 0.0 else 0.0)
    b_n = 8.0 * U * s_n + (abs(c0 * a3) + abs(c1)) * s * e_v
    return own, (m, xc, nxt), (b_m, b_c, b_n)


def padded(shape, values):
    """A latent-shaped view of an allocation with PAD sentinel floats behind its last row -> (view, whole allocation)."""
    n = values.numel()
    flat = torch.full((n + PAD,), SENTINEL, dtype=F32, device=DEV)
    flat[:n] = values.reshape(-1).to(DEV)
    return flat[:n].view(shape), flat


# ---- 1. the kernel against the float64 restatement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("C,T,H8,W8,tok0,n_tok,with_u", [(16, 3, 6, 10, 7, 23, True), (16, 1, 2, 2, 0, 1, True), (16, 2, 4, 6, 0, 12, False)])
def test_kernel_matches_float64_restatement(hip_ops, C, T, H8, W8, tok0, n_tok, with_u):
    """Every step kind at every shape: the three outputs within the derived bound (restated_step), nothing written outside the
    tokens' elements or behind an allocation, a buffer whose coefficient is 0 not read (it holds NaN), the same bits twice."""
    shape = (C, T, H8, W8)
    g = torch.Generator().manual_seed(100 + T)
    ldh = 4 * C + 8                                              # head rows wider than 4 C
    for name, st in step_kinds().items():
        x, x_hat, m_prev, m_prev2 = (torch.randn(shape, generator=g) * sc for sc in (1.0, 1.0, 1.5, 1.5))
        heads = torch.randn((2, n_tok, ldh), generator=g)
        hc, hu = heads[0, :, :4 * C], (heads[1, :, :4 * C] if with_u else None)
        own, want, bound = restated_step(x, x_hat, m_prev, m_prev2, hc, hu, 5.0, st.sigma, st.a, st.c, tok0, n_tok)
        # outside the tokens' elements every buffer holds the sentinel; inside, what the step does not read is NaN
        nan = torch.full(shape, float("nan"))
        reads_hat, reads_p1 = st.a is not None, (st.a is not None and st.a[1] != 0.0) or st.c[2] != 0.0
        reads_p2 = st.a is not None and st.a[2] != 0.0
        fill = lambda t, read: torch.where(own, t if read else nan, torch.full(shape, SENTINEL))      # noqa: E731
        runs = []
        for _ in range(2):
            bufs = [padded(shape, fill(t, read)) for t, read in ((x, True), (x_hat, reads_hat), (nan, False), (m_prev, reads_p1), (m_prev2, reads_p2))]
            (lat, xh, mn, p1, p2) = (b[0] for b in bufs)
            hd = heads.to(DEV)
            hip_ops.unpatchify_cfg_multistep(lat, xh, mn, p1, p2, hd[0, :, :4 * C], hd[1, :, :4 * C] if with_u else None, 5.0,
                                             st.sigma, st.a, st.c, tok0, n_tok)
            torch.cuda.synchronize()
            assert torch.equal(hd.cpu(), heads), "the head outputs were written"
            got = [b[0].cpu() for b in bufs]
            for what, t, (_, flat) in zip(("latent", "x_hat", "m_new", "m_prev", "m_prev2"), got, bufs):
                assert (t[~own] == SENTINEL).all(), f"{name}: {what} was written outside the token range"
                assert (flat[-PAD:] == SENTINEL).all(), f"{name}: {what} was written behind its last row"
            for t, src, read in ((got[3], m_prev, reads_p1), (got[4], m_prev2, reads_p2)):
                assert torch.equal(t[own].nan_to_num(nan=123.0), (src if read else nan)[own].nan_to_num(nan=123.0)), f"{name}: a read-only buffer changed"
            runs.append(got)
        assert all(torch.equal(a_, b_) for a_, b_ in zip(runs[0][:3], runs[1][:3])), f"{name}: two runs differ"
        lat, xh, mn = runs[0][:3]
        for what, t, w, b in zip(("m", "x_c", "x_next"), (mn, xh, lat), want, bound):
            assert torch.isfinite(t[own]).all(), f"{name}: {what} read a buffer whose coefficient is 0"
            err = (t.double() - w).abs()[own]
            worst = float((err / b[own].clamp_min(1e-300)).max()) if float(b[own].max()) > 0 else 0.0
            print(f"{shape} {name}: {what} max |err| {float(err.max()):.2e}, worst err / bound {worst:.3f}")
            assert (err <= b[own]).all(), f"{name}: {what} misses the derived bound, worst err / bound {worst:.2f}"
        if st.a is None:
            assert torch.equal(xh[own], x[own]), "without a corrector x_c is x, bit for bit"


# ---- 2. five steps in a row ---------------------------------------------------------------------------------------------------------
def test_five_consecutive_steps_match_the_restated_sequence(hip_ops):
    """Fresh random head outputs every step, the three x0-prediction slots rotated through new / previous / one before as the engine
    does, x_hat handed over, the latent in place.  Two checks per step:
    - the launch's three outputs against restated_step on host copies of the buffers the launch must have read if the rotation and
      the hand-over are right (kept by the test in a list, newest first), within that function's bound;
    - the latent against the D / rho restatement of the whole sequence (float64, exact coefficients).  Bound: a scalar recurrence in
      max norms.  E bounds the error of every state buffer before the step; the launch adds 10 u sum |coef_j buf_j| (the kernel's
      8 u plus 2 u for the f32 rounding of sigma and of each coefficient) with every buffer bounded by B, the largest magnitude held
      so far, and the CFG combine adds sigma e_v; E then passes through the step's coefficients."""
    C, T, H8, W8, n = 16, 2, 4, 6, 5
    shape, n_tok = (C, T, H8, W8), 12
    g = torch.Generator().manual_seed(7)
    sigmas = flow_match_sigmas(n)
    steps = S.MultistepPlan("unipc", sigmas).steps()
    assert [s.order for s in steps] == [1, 1, 2, 2, 1]
    x0 = torch.randn(shape, generator=g)
    heads = torch.randn((n, 2, n_tok, 4 * C), generator=g)
    want = []

    def velocity(x, i):
        want.append(x)                                        # the sample each step starts from = the latent after the step before
        v = heads[i, 1].double() + f32(5.0) * (heads[i, 0].double() - heads[i, 1].double())
        return scatter(v, shape, 0, n_tok)[0]

    want.append(restated_sample(velocity, x0.double(), sigmas))
    lat = x0.clone().to(DEV)
    x_hat, ring = torch.zeros_like(lat), [torch.zeros_like(lat) for _ in range(3)]
    held = [None, None]                                       # host copies: [m of the step before, m of the one before that]
    hat, E, B = None, 0.0, float(x0.abs().max())
    for k, st in enumerate(steps):
        hd = heads[k].to(DEV)
        before = lat.cpu()
        hip_ops.unpatchify_cfg_multistep(lat, x_hat, ring[k % 3], ring[(k - 1) % 3], ring[(k - 2) % 3], hd[0], hd[1], 5.0, st.sigma, st.a, st.c, 0, n_tok)
        torch.cuda.synchronize()
        got = (ring[k % 3].cpu(), x_hat.cpu(), lat.cpu())
        own, exp, bound = restated_step(before, hat, held[0], held[1], heads[k, 0], heads[k, 1], 5.0, st.sigma, st.a, st.c, 0, n_tok)
        assert own.all()
        for what, t, w, b in zip(("m", "x_c", "x_next"), got, exp, bound):
            assert ((t.double() - w).abs() <= b).all(), f"step {k}: {what} is not what the rotated buffers give"
        held, hat = [got[0], held[0]], got[1]
        v_max = float((heads[k, 1].abs() + 5.0 * (heads[k, 0] - heads[k, 1]).abs()).max())
        a = st.a or (0.0, 0.0, 0.0, 0.0)
        a_read = abs(a[0]) + abs(a[1]) + abs(a[2])
        s_m = B + st.sigma * v_max
        e_m = E + 10.0 * U * s_m + st.sigma * 4.0 * U * v_max
        s_c, e_c = (a_read * B + abs(a[3]) * s_m, a_read * E + abs(a[3]) * e_m) if st.a else (B, E)
        e_c += 10.0 * U * s_c if st.a else 0.0
        s_n = abs(st.c[0]) * s_c + abs(st.c[1]) * s_m + abs(st.c[2]) * B
        e_n = abs(st.c[0]) * e_c + abs(st.c[1]) * e_m + abs(st.c[2]) * E + 10.0 * U * s_n
        E = max(E, e_m, e_c, e_n)
        B = 1.001 * max([B] + [float(t.abs().max()) for t in got])
        err = float((got[2].double() - want[k + 1]).abs().max())
        print(f"step {k}: max |latent - restated sequence| {err:.2e}, bound {E:.2e}")
        assert err <= E, f"step {k}: {err:.3e} > {E:.3e}"
    assert E <= 1e-3 * B, "the recurrence must stay a rounding bound"
    assert torch.equal(lat.cpu(), ring[(n - 1) % 3].cpu()), "the last step has t = 0: the latent is the last x0-prediction"


# ---- 3. the first step at sigma = 1 is the Euler step -----------------------------------------------------------------------------
@pytest.mark.parametrize("round_bf16", [False, True])
def test_first_step_at_sigma_one_is_the_euler_kernel(hip_ops, round_bf16):
    """At sigma_0 = 1 the order-1 predictor is sigma_1 x + (1 - sigma_1)(x - v) = x + (sigma_1 - 1) v.  Bound: the multistep kernel's
    (restated_step) plus the Euler kernel's own two roundings, 2 u (|x| + |v dsigma|), plus the CFG combine's error on both sides.
    round_bf16 rounds the velocity's intermediates in both kernels and, in the Euler kernel alone, x, v dsigma and their sum (the
    solver arithmetic stays f32).  So with round_bf16 on: on random inputs the velocity must agree - (x - m) / sigma against the Euler
    kernel's vel_out, which is bf16-rounded - and the latents are compared on inputs on a dyadic grid, where those three extra
    roundings are exact (x, hc, hu multiples of 1/8 with |hc - hu| <= 3, dsigma = -1/2: every value has at most 8 significant bits)."""
    C, T, H8, W8, tok0, n_tok = 16, 3, 6, 10, 7, 23
    shape = (C, T, H8, W8)
    g = torch.Generator().manual_seed(31)
    for dyadic in ((False, True) if round_bf16 else (False,)):
        if dyadic:
            sigmas = [1.0, 0.5]
            x = torch.randint(-16, 17, shape, generator=g).float() / 8.0
            hu = torch.randint(-16, 17, (n_tok, 4 * C), generator=g).float() / 8.0
            hc = hu + torch.randint(-24, 25, (n_tok, 4 * C), generator=g).float() / 8.0
        else:
            sigmas = flow_match_sigmas(8)
            x, hc, hu = torch.randn(shape, generator=g), torch.randn((n_tok, 4 * C), generator=g), torch.randn((n_tok, 4 * C), generator=g)
        st = S.MultistepPlan("unipc", sigmas).steps()[0]
        assert st.sigma == 1.0 and st.a is None and st.c == (sigmas[1], 1.0 - sigmas[1], 0.0)
        dsigma = sigmas[1] - 1.0
        euler, vel = x.clone().to(DEV), torch.zeros(shape, device=DEV)
        hip_ops.unpatchify_cfg_euler(euler, hc.to(DEV), hu.to(DEV), 5.0, dsigma, tok0, n_tok, vel_out=vel, round_bf16=round_bf16)
        lat, x_hat, m_new = x.clone().to(DEV), torch.zeros(shape, device=DEV), torch.zeros(shape, device=DEV)
        hip_ops.unpatchify_cfg_multistep(lat, x_hat, m_new, None, None, hc.to(DEV), hu.to(DEV), 5.0, st.sigma, st.a, st.c, tok0, n_tok,
                                         round_bf16=round_bf16)
        torch.cuda.synchronize()
        euler, vel, lat, m_new = euler.cpu(), vel.cpu(), lat.cpu(), m_new.cpu()
        own, _, (b_m, _, b_n) = restated_step(x, None, None, None, hc, hu, 5.0, st.sigma, st.a, st.c, tok0, n_tok)
        assert torch.equal(lat[~own], x[~own]) and torch.equal(euler[~own], x[~own])
        if round_bf16:
            # the velocity both kernels formed: bf16 values, so x - m reproduces them to the rounding of one subtraction each way
            assert torch.equal(vel, vel.to(torch.bfloat16).float())
            err = ((x.double() - m_new.double()) - vel.double()).abs()[own]
            assert (err <= 2.0 * U * (x.double().abs() + vel.double().abs())[own]).all(), "round_bf16: the two kernels formed different velocities"
        if round_bf16 and not dyadic:
            continue
        b = b_n + 2.0 * U * (x.double().abs() + (vel.double() * dsigma).abs()) + scatter(
            4.0 * U * (hu.double().abs() + 5.0 * (hc.double() - hu.double()).abs()), shape, tok0, n_tok)[0] * abs(dsigma)
        err = (lat.double() - euler.double()).abs()
        print(f"round_bf16={round_bf16} dyadic={dyadic}: max |multistep - euler| {float(err.max()):.2e}")
        assert (err[own] <= b[own]).all(), f"worst err / bound {float((err[own] / b[own]).max()):.2f}"
        assert not torch.equal(lat, x)


# ---- 4. the loop, and every driver mode ---------------------------------------------------------------------------------------------
def _sequential(m):
    m.cfg_batch = False


def test_sequential_loop_matches_restated_solver_and_differs_from_euler(hip_ops):
    """The stiff tiny DiT, 5 latent frames, LOOP_STEPS steps with CFG through the sequential per-op driver: >= 40 dB against the CPU
    restatement of the UniPC loop (the project's loop bar; the restated Euler loop stays under it, test_solver_cpu), and not the
    Euler loop's latent."""
    m, lat = engine_loop(hip_ops, setup=_sequential, prep=dict(graphs=False), dev=DEV)
    torch.cuda.synchronize()
    assert m._pair is None and m._solver_state is not None
    ref = reference("unipc")
    p, p_euler = R.psnr(lat.cpu(), ref), R.psnr(reference("euler"), ref)
    print(f"HIP UniPC loop vs restated UniPC: {p:.1f} dB (restated Euler: {p_euler:.1f} dB)")
    assert p >= 40.0, f"{p:.1f} dB"
    assert p_euler <= p - 10.0
    m2, euler = engine_loop(hip_ops, solver="euler", setup=_sequential, prep=dict(graphs=False), dev=DEV)
    torch.cuda.synchronize()
    assert m2._solver_state is None and not torch.equal(lat, euler)
    pe = R.psnr(euler.cpu(), reference("euler"))
    assert pe >= 40.0, f"Euler loop on the same DiT vs restated Euler: {pe:.1f} dB"


@pytest.mark.parametrize("mode", ["pair", "pair-no-stem", "native", "graphs", "dual-stream"])
def test_driver_modes_match_sequential_loop(hip_ops, mode, monkeypatch):
    """The update is the step's last launch in every driver mode, issued outside captured graphs: bit-identical to the sequential loop."""
    _, ref = engine_loop(hip_ops, setup=_sequential, prep=dict(graphs=False), dev=DEV)
    prep, setup = dict(graphs=False), None
    if mode == "pair-no-stem":
        setup = lambda m: setattr(m, "share_stem", False)                        # noqa: E731
    elif mode == "native":
        setup = lambda m: setattr(m, "native_forward", True)                     # noqa: E731
    elif mode == "graphs":
        prep = dict(graphs=True)
    elif mode == "dual-stream":
        monkeypatch.setenv("ICV_DUAL_STREAM", "1")
    m, got = engine_loop(hip_ops, setup=setup, prep=prep, dev=DEV)
    torch.cuda.synchronize()
    assert torch.isfinite(got).all()
    if mode in ("pair", "pair-no-stem"):
        assert m._pair is not None
    if mode == "native":
        assert m.native_forward and m._native_eligible()
    if mode == "graphs":
        assert m._graphs_on and m._graphs
    if mode == "dual-stream":
        assert m.dual_stream and m._twin is not None
    assert torch.equal(got, ref), f"{mode}: max |d| {float((got - ref).abs().max())}"


# ---- 5. compositions ----------------------------------------------------------------------------------------------------------------
def _teacache_velocity(sigmas, skipped, cfg_scale=5.0):
    """velocity(x, i) of restated_sample with DiffSynth's TeaCache bookkeeping on oracle.wan_ref pieces (tests/test_teacache_cpu.py):
    a computed step stores x_after_blocks - x_before_blocks per CFG branch, a skipped one adds it to the patch embedding and runs the
    head only."""
    sd, bsd, noise, c1, c2, bl = inputs()
    sd, bsd = R.round_state_dict_to_bf16(sd), R.round_state_dict_to_bf16(bsd)
    buf = R.buffer_embed(bsd, bl)
    ctxs = (R.text_embed(sd, c1), R.text_embed(sd, c2))
    grid = (noise.shape[1], noise.shape[2] // 2, noise.shape[3] // 2)
    freqs = R.rope_freqs_3d(CFG.head_dim, *grid)
    residual = [None, None]

    def v(x, i):
        t, t_mod = R.time_embed(sd, CFG, float(sigmas[i]) * 1000.0)
        vs = []
        for b in range(2):
            tok = R.patchify_tokens(x.float(), sd["patch_embedding.weight"], sd["patch_embedding.bias"]) + buf
            if i in skipped:
                tok = tok + residual[b]
            else:
                before = tok.clone()
                for layer in range(CFG.num_layers):
                    tok = R.dit_block(sd, CFG, layer, tok, ctxs[b], t_mod, freqs)
                residual[b] = tok - before
            vs.append(R.unpatchify(R.head(sd, CFG, tok, t), grid, CFG.out_dim))
        return (vs[1] + cfg_scale * (vs[0] - vs[1])).double()
    return v


def test_with_teacache_one_forced_skip(hip_ops):
    """Step 3 of 6 runs no blocks: the solver takes the skipped step's velocity like any other."""
    computed = (0, 1, 2, 4, 5)
    plan = lambda m, sch: teacache.TeaCachePlan("test-linear", 0.0, tuple(range(LOOP_STEPS)), (0.0,) * LOOP_STEPS, computed)      # noqa: E731
    m, lat = engine_loop(hip_ops, dev=DEV, tea=plan)
    torch.cuda.synchronize()
    sigmas = flow_match_sigmas(LOOP_STEPS)
    ref = restated_sample(_teacache_velocity(sigmas, {3}), inputs()[2].double(), sigmas).float()
    p = R.psnr(lat.cpu(), ref)
    print(f"UniPC + TeaCache (step 3 skipped) vs its restatement: {p:.1f} dB")
    assert p >= 40.0, f"{p:.1f} dB"
    assert m._tc_res is not None and not torch.equal(ref, reference("unipc")), "the skip must change the restated result"


def test_with_a_shortened_sigma_range(hip_ops):
    """denoising_strength = 0.6: the list starts at shift-warped 0.6, no history entry at sigma = 1, orders [1, 2, ..., 2, 1]."""
    m, lat = engine_loop(hip_ops, strength=0.6, dev=DEV)
    torch.cuda.synchronize()
    ref = reference("unipc", strength=0.6)
    p, p_euler = R.psnr(lat.cpu(), ref), R.psnr(reference("euler", strength=0.6), ref)
    print(f"UniPC over the 0.6 range vs its restatement: {p:.1f} dB (restated Euler: {p_euler:.1f} dB)")
    assert p >= 40.0, f"{p:.1f} dB"


def test_with_the_e4m3_mode(hip_ops):
    """The six per-layer projections on the fp8 MFMA: the e4m3 mode's loop bar, >= 40 dB against the oracle run with the same e4m3 row
    quantisation (tests/test_dit_gpu.py test_fp8_gemm_mode_forward_and_loop), here with both driven by UniPC."""
    m, lat = engine_loop(hip_ops, dev=DEV, kw=dict(gemm_dtype="fp8", fp8_weights=WanDiT.FP8_WEIGHTS))
    torch.cuda.synchronize()
    p8, p = R.psnr(lat.cpu(), reference("unipc", fp8=True)), R.psnr(lat.cpu(), reference("unipc"))
    print(f"UniPC e4m3 loop: vs fake-quant restatement {p8:.1f} dB, vs unquantised restatement {p:.1f} dB")
    assert p8 >= 40.0, f"{p8:.1f} dB"


# ---- 6. the pipeline ------------------------------------------------------------------------------------------------------------------
def _pipe():
    from infinicube_amd.videogen.ops import HipOps
    from infinicube_amd.videogen.pipeline import DiTHolder, WanVideoPipeline
    from standins import HashTextEncoder, PoolVAE
    return WanVideoPipeline(DEV, torch.bfloat16, DiTHolder(syn.make_dit_state_dict(CFG), CFG), HashTextEncoder(CFG), PoolVAE(), ops=HipOps(DEV))


def test_pipeline(monkeypatch):
    for key in ENV:
        monkeypatch.delenv(key, raising=False)
    kw = dict(prompt="a street", negative_prompt="bad", height=GRID.height, width=GRID.width, num_frames=GRID.num_frames, seed=3)
    p = _pipe()
    frames = p(**kw, sample_solver="unipc", num_inference_steps=6)
    assert len(frames) == GRID.num_frames and frames[0].size == (GRID.width, GRID.height)
    assert p.solver_record == dict(name="unipc", steps=6, orders=[1, 1, 2, 2, 2, 1]) and p._engine._solver_state is not None
    uni = p(**kw, sample_solver="unipc", num_inference_steps=6, return_latents=True).cpu()
    after = p(**kw, num_inference_steps=6, return_latents=True).cpu()            # the setting does not outlive its call
    assert p.solver_record is None
    fresh = _pipe()(**kw, num_inference_steps=6, return_latents=True).cpu()
    assert torch.equal(after, fresh), "a call without the keyword must give a fresh pipeline's Euler bits"
    assert torch.isfinite(uni).all() and not torch.equal(uni, fresh)
