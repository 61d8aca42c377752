"""The premise of tests/test_gemm_exact_gpu.py, checked without a GPU, so that an edit of a range, a seed or a shape there is screened
before it reaches one:
  * every case the GPU file hands to a kernel is exact: accumulator, scaled accumulator, acc + bias and the gated residual are all
    below 2^24 and survive f64 -> f32 -> f64 (the asserts live in gemm_exact.py and run when a case is built);
  * the BF16-epilogue cases really round: with K >= 192 at least 1 % of the outputs are not representable in bf16 and at least 100
    are exact ties - a condition, not a measurement: it is what lets the test tell round-to-nearest-even from truncation (every
    inexact value differs) and from round-half-away (half of the ties differ);
  * the expectations themselves are checked by a second implementation: OracleOps.gemm / gemm_fp8 / gemv (tests/oracle_ops.py, f32
    arithmetic) give the same bits on the same inputs."""
import pytest
import torch

import gemm_exact as G
from oracle_ops import OracleOps

BF16_SHAPES = G.G128_SHAPES + G.G256_SHAPES + [G.G256P_BIG]
ALL = [("bf16", s) for s in BF16_SHAPES] + [("fp8", s) for s in G.FP8_SHAPES]
IDS = [f"{fmt}-{M}x{N}x{K}" for fmt, (M, N, K) in ALL]


def cases_of(fmt, shape):
    # the GPU file runs the big persistent-kernel shape with the BF16 and GELU epilogues only
    return [c for c in G.epi_cases(shape[1]) if shape != G.G256P_BIG or c[0] in ("bf16+bias", "gelu+bias")]


def oracle_out(inp, epi, use_bias, use_gate, nsplit):
    M, N = inp.M, inp.N
    out = torch.empty((M, N) if nsplit is None else (N // nsplit, M, nsplit), dtype=G.BF16 if epi in (G.EPI_BF16, G.EPI_GELU_BF16) else G.F32)
    kw = dict(resid=inp.resid if epi == G.EPI_RESID_F32 else None, gate=inp.gate if use_gate else None, nsplit=nsplit)
    bias = inp.bias if use_bias else None
    if inp.fmt == "bf16":
        OracleOps().gemm(inp.a, inp.w, bias, out, epi, **kw)
    else:
        OracleOps().gemm_fp8(inp.a, inp.a_scale, inp.w, inp.w_scale, bias, out, epi, **kw)
    return out


@pytest.mark.parametrize("fmt,shape", ALL, ids=IDS)
def test_cases_are_exact_and_the_oracle_agrees(fmt, shape):
    for name, epi, kind, use_bias, use_gate, _, split in cases_of(fmt, shape):
        inp = G.make(fmt, *shape, kind)
        exp = G.expected(inp, epi, use_bias, use_gate)          # raises if the premise does not hold
        nsplit = shape[1] // 3 if split else None
        got = oracle_out(inp, epi, use_bias, use_gate, nsplit)
        if epi == G.EPI_GELU_BF16:
            # the oracle evaluates 0.5 x (1 + tanh u) in f32: 1 + tanh u carries an absolute error of up to 2^-24 (it cancels for
            # x < 0), i.e. |x| 2^-25 in the product, doubled here for tanh's own rounding.  Outside x in about [-5.2, -4] that is far
            # below a bf16 spacing and the faithful-rounding criterion of the GPU test decides alone.
            x = G.pre_activation(inp, use_bias)
            tol = torch.clamp(G.spacing_bf16(exp), min=2.0 ** -24) + x.abs() * 2.0 ** -24
            bad = ~((got.float().double() - exp).abs() < tol)
            assert not bool(bad.any()), f"{fmt} {shape} {name}: the f32 oracle is off at {int(bad.sum())} elements"
            assert float(G.gelu_bad(got, exp).double().mean()) < 0.02, f"{fmt} {shape} {name}: oracle outside the faithful bound too often"
        else:
            assert torch.equal(got, exp if nsplit is None else G.split_planes(exp, nsplit)), f"{fmt} {shape} {name}: oracle and expectation differ"


def gelu_tanh_f32(x):
    """gelu_tanh of csrc/icv_common.h restated in f32: x / (1 + 2^(-w)), w = x (C3 x^2 + C1)."""
    c1 = torch.tensor(2.0 * 0.7978845608028654 * 1.4426950408889634, dtype=G.F32)
    c3 = c1 * torch.tensor(0.044715, dtype=G.F32)
    return x * (1.0 / (1.0 + torch.exp2(-(x * (x * x * c3 + c1)))))


@pytest.mark.parametrize("fmt,shape", ALL, ids=IDS)
def test_gelu_criterion_is_met_by_an_f32_restatement_of_the_kernels_formula(fmt, shape):
    """The criterion is derived, not tuned: this shows it can be met in f32 at every pre-activation the GPU file produces."""
    inp = G.make(fmt, *shape, "gelu")
    for use_bias in (True, False):
        x = G.pre_activation(inp, use_bias)
        got = gelu_tanh_f32(x.to(G.F32)).to(G.BF16)
        assert not bool(G.gelu_bad(got, G.gelu64(x)).any()), f"{fmt} {shape} bias={use_bias}"


@pytest.mark.parametrize("fmt,shape", [c for c in ALL if c[1][2] >= 192], ids=[i for i, c in zip(IDS, ALL) if c[1][2] >= 192])
def test_bf16_epilogue_cases_round(fmt, shape):
    inp = G.make(fmt, *shape, "int")
    for use_bias in (True, False):
        share, ties = G.rounding_census(G.pre_activation(inp, use_bias))
        assert share >= 0.01 and ties >= 100, f"{fmt} {shape} bias={use_bias}: {share:.2%} not representable in bf16, {ties} exact ties"


def test_rounding_census_counts_what_it_says():
    v = torch.tensor([256.0, 257.0, 258.0, 259.0, 513.0, 514.0, -257.0, 1.5, 0.0], dtype=G.F64)
    # 257, 259, -257 are ties of spacing 2; 513 is inexact at spacing 4 but no tie; 514 is a tie
    share, ties = G.rounding_census(v)
    assert ties == 4 and abs(share - 5 / 9) < 1e-12


def test_gelu_criterion_accepts_both_neighbours_and_nothing_else():
    ref = torch.tensor([1.00001, 3.999, -0.1700001, 1e-31, -1e-40], dtype=G.F64)
    rne = ref.to(G.F32).to(G.BF16)
    assert not bool(G.gelu_bad(rne, ref).any())
    step = G.spacing_bf16(ref)
    other = (rne.double() + torch.where(rne.double() > ref, -step, step)).to(G.F32).to(G.BF16)       # the neighbour on the other side
    assert not bool(G.gelu_bad(other, ref)[:3].any())
    two_off = (rne.double() + 2 * torch.where(rne.double() > ref, step, -step)).to(G.F32).to(G.BF16)
    assert bool(G.gelu_bad(two_off, ref)[:3].all())
    assert float(G.spacing_bf16(torch.tensor([1.0, 1.99, 2.0, 300.0], dtype=G.F64))[3]) == 2.0
    # the f64 reference keeps its precision where 0.5 x (1 + tanh u) would cancel to zero
    assert -1e-6 < float(G.gelu64(torch.tensor([-5.0], dtype=G.F64))) < -1e-7


@pytest.mark.parametrize("M", G.GEMV_M)
def test_gemv_cases_are_exact_and_the_oracle_agrees(M):
    for N in G.GEMV_N:
        for K in G.GEMV_K:
            inp = G.make_gemv(M, N, K)
            for use_bias in (True, False):
                exp = G.expected_gemv(inp, use_bias)
                got = torch.empty((M, N))
                OracleOps().gemv(inp.x, inp.w, inp.bias if use_bias else None, got)
                assert torch.equal(got, exp), f"gemv {M}x{N}x{K} bias={use_bias}"
