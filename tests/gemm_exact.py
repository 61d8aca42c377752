"""TEST-ONLY constructions for the bit-exact GEMM tests (tests/test_gemm_exact_cpu.py, tests/test_gemm_exact_gpu.py).  No GPU here.

Premise: operands that are small integers (bf16 or e4m3), an integer (or dyadic) bias, scales and gates that are powers of two.  Every
product and every partial sum is then an integer (or a multiple of one fixed power of two) far below 2^24, so every summation order,
MFMA shape and FMA contraction gives the same f32 bits, and the expected output is known exactly: float64 matmul on the CPU, the
epilogue in float64, one cast.  The helpers assert that premise for every case they hand out; a deviation of a kernel from these
values is a defect, never rounding.

The GELU epilogue's INPUT is exact in the same way (multiples of 1/8 over roughly +-12); the activation is not, and is judged by
``gelu_bad``: the stored bf16 must be one of the two bf16 neighbours of the float64 tanh-GELU of the exact pre-activation.
"""
import functools
import zlib
from types import SimpleNamespace

import torch

BF16, F32, F64, FP8 = torch.bfloat16, torch.float32, torch.float64, torch.float8_e4m3fn
EPI_BF16, EPI_GELU_BF16, EPI_RESID_F32, EPI_F32 = 0, 1, 2, 3
LIMIT = float(2 ** 24)

# ---- the shapes (M, N, K) of the GPU file; the CPU file checks the premise on every one of them ----
G128_SHAPES = [(1, 4, 64), (127, 132, 192), (129, 124, 64), (257, 260, 128), (130, 516, 320), (1030, 264, 64)]
G256_SHAPES = [(256, 256, 64), (257, 256, 128), (511, 768, 192), (513, 256, 320), (2305, 512, 64)]
G256P_BIG = (33025, 1024, 64)      # 130 x 4 = 520 tiles of 256 x 256: at least two per CU, ragged M
FP8_SHAPES = [(1, 4, 128), (255, 252, 128), (257, 260, 256), (513, 516, 384), (1030, 264, 128)]
GEMV_M, GEMV_N, GEMV_K = tuple(range(1, 9)), (4, 6, 1536), (8, 264, 1536)

# ---- epilogue cases: (name, epilogue, generator kind, bias?, gate?, resid layout, split planes?) ----
# resid layout: "inplace" = resid is out, "ldr" = a separate view with ldr = N + 16 != ldo
EPI_CASES = [
    ("f32+bias", EPI_F32, "int", True, False, None, False),
    ("f32", EPI_F32, "int", False, False, None, False),
    ("bf16+bias", EPI_BF16, "int", True, False, None, False),
    ("bf16", EPI_BF16, "int", False, False, None, False),
    ("gelu+bias", EPI_GELU_BF16, "gelu", True, False, None, False),
    ("gelu", EPI_GELU_BF16, "gelu", False, False, None, False),
    ("resid inplace+gate+bias", EPI_RESID_F32, "int", True, True, "inplace", False),
    ("resid inplace", EPI_RESID_F32, "int", False, False, "inplace", False),
    ("resid ldr+gate", EPI_RESID_F32, "int", False, True, "ldr", False),
    ("resid ldr+bias", EPI_RESID_F32, "int", True, False, "ldr", False),
    ("split bf16+bias", EPI_BF16, "int", True, False, None, True),
    ("split f32", EPI_F32, "int", False, False, None, True),
]


def epi_cases(N):
    """The epilogue cases that exist at width N (split planes: nsplit = N / 3 where 12 | N)."""
    return [c for c in EPI_CASES if not c[6] or N % 12 == 0]


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


def _pick(g, shape, values):
    v = torch.tensor(values, dtype=F64)
    return v[torch.randint(0, len(values), shape, generator=g)]


class Inputs(SimpleNamespace):
    """One GEMM's operands.  ``resid`` (integers in [-1000, 1000], f32 [M, N]) is made on first use: most epilogues never read it."""

    @functools.cached_property
    def resid(self):
        return exact_f32(_ints(_gen("resid", self.fmt, self.M, self.N, self.K, self.kind), (self.M, self.N), -1000, 1000), "resid")


def exact_f32(x64, what):
    """The premise: |x| < 2^24 and x is an f32.  Returns that f32."""
    assert x64.dtype == F64
    assert float(x64.abs().max()) < LIMIT, f"{what}: max |value| {float(x64.abs().max())} >= 2^24"
    x32 = x64.to(F32)
    assert torch.equal(x32.double(), x64), f"{what}: not exactly representable in f32"
    return x32


def _narrow(x64, dtype, what):
    y = x64.to(F32).to(dtype)
    assert torch.equal(y.to(F32).double(), x64), f"{what}: not exact in {dtype}"
    return y


@functools.lru_cache(maxsize=4)
def make_bf16(M, N, K, kind="int"):
    """Inputs of icv_gemm_bf16.  kind "int": a, w integers in [-2, 5] (non-zero mean: sums pass 256, so a bf16 store really rounds);
    kind "gelu": a integers in [-3, 3], w integers in [-3, 3] / 8, bias multiples of 1/8."""
    g = _gen("bf16", M, N, K, kind)
    if kind == "int":
        a, w, bias = _ints(g, (M, K), -2, 5), _ints(g, (N, K), -2, 5), _ints(g, (N,), -64, 64)
    else:
        a, w, bias = _ints(g, (M, K), -3, 3), _ints(g, (N, K), -3, 3) / 8, _ints(g, (N,), -16, 16) / 8
    return Inputs(fmt="bf16", kind=kind, M=M, N=N, K=K, a=_narrow(a, BF16, "a"), w=_narrow(w, BF16, "w"), bias=exact_f32(bias, "bias"),
                  gate=exact_f32(_pick(g, (N,), [1, -1, 2, -2, 0.5, -0.5]), "gate"))


@functools.lru_cache(maxsize=4)
def make_fp8(M, N, K, kind="int"):
    """Inputs of icv_gemm_fp8: e4m3 codes of small integers, one power-of-two scale per row of A and per row of W.
    kind "int": integers in [-2, 5], scales 2^-2 ... 2^1, bias multiples of 1/16; kind "gelu": integers in [-3, 3], the 1/8 of the
    weights in w_scale (1/8 or 1/16), a_scale 1 or 1/2, bias multiples of 1/8."""
    g = _gen("fp8", M, N, K, kind)
    if kind == "int":
        a, w = _ints(g, (M, K), -2, 5), _ints(g, (N, K), -2, 5)
        sa, sw = _pick(g, (M,), [0.25, 0.5, 1, 2]), _pick(g, (N,), [0.25, 0.5, 1, 2])
        bias = _ints(g, (N,), -1024, 1024) / 16
    else:
        a, w = _ints(g, (M, K), -3, 3), _ints(g, (N, K), -3, 3)
        sa, sw = _pick(g, (M,), [1, 0.5]), _pick(g, (N,), [0.125, 0.0625])
        bias = _ints(g, (N,), -16, 16) / 8
    return Inputs(fmt="fp8", kind=kind, M=M, N=N, K=K, a=_narrow(a, FP8, "a"), w=_narrow(w, FP8, "w"), a_scale=exact_f32(sa, "a_scale"),
                  w_scale=exact_f32(sw, "w_scale"), bias=exact_f32(bias, "bias"), gate=exact_f32(_pick(g, (N,), [1, -1, 2, -2, 0.5, -0.5]), "gate"))


def make(fmt, M, N, K, kind="int"):
    return (make_bf16 if fmt == "bf16" else make_fp8)(M, N, K, kind)


@functools.lru_cache(maxsize=4)
def _scaled_acc(fmt, M, N, K, kind):
    inp = make(fmt, M, N, K, kind)
    acc = inp.a.to(F32).double() @ inp.w.to(F32).double().t()
    exact_f32(acc, "accumulator")
    if fmt == "fp8":
        acc = acc * inp.a_scale.double()[:, None] * inp.w_scale.double()[None, :]
        exact_f32(acc, "scaled accumulator")
    return acc


def pre_activation(inp, use_bias):
    """float64 [M, N]: (A . W^T) (* a_scale[m] * w_scale[n]) (+ bias[n]), exact in f32 (asserted)."""
    v = _scaled_acc(inp.fmt, inp.M, inp.N, inp.K, inp.kind)
    if use_bias:
        v = v + inp.bias.double()[None, :]
    exact_f32(v, "acc + bias")
    return v


def gelu64(x):
    """tanh-GELU in float64, in the form x * sigmoid(2u), u = sqrt(2/pi) (x + 0.044715 x^3): it keeps its relative precision in the
    negative tail, where 0.5 x (1 + tanh u) cancels."""
    u = 0.7978845608028654 * (x + 0.044715 * x * x * x)
    return x / (1.0 + torch.exp(-2.0 * u))


def expected(inp, epi, use_bias, use_gate):
    """The exact output [M, N]: f32 for F32 / RESID, bf16 (round to nearest even of the exact f32) for BF16; for GELU the float64
    reference value of the activation (judged by gelu_bad, not by equality)."""
    v = pre_activation(inp, use_bias)
    if epi == EPI_GELU_BF16:
        return gelu64(v)
    if epi == EPI_RESID_F32:
        v = inp.resid.double() + (inp.gate.double()[None, :] * v if use_gate else v)
        return exact_f32(v, "resid + gate * (acc + bias)")
    v32 = exact_f32(v, "acc + bias")
    return v32.to(BF16) if epi == EPI_BF16 else v32


def split_planes(t, nsplit):
    """[M, N] -> [N / nsplit, M, nsplit], the split-plane output layout."""
    M, N = t.shape
    return t.reshape(M, N // nsplit, nsplit).permute(1, 0, 2).contiguous()


def spacing_bf16(ref):
    """Distance between neighbouring bf16 values around |ref| (8 significand bits: 2^(floor(log2 |ref|) - 7)); 0 for ref == 0."""
    _, e = torch.frexp(ref.double().abs())            # |ref| = m * 2^e, m in [0.5, 1)
    return torch.where(ref == 0, torch.zeros_like(ref, dtype=F64), torch.ldexp(torch.ones_like(ref, dtype=F64), e - 8))


def gelu_tol(ref64):
    """max(spacing_bf16(ref), 2^-24): the bound of gelu_bad."""
    return torch.clamp(spacing_bf16(ref64), min=2.0 ** -24)


def gelu_bad(got_bf16, ref64, tol=None):
    """Mask of stored values that are NOT a faithful rounding: |got - ref| >= max(spacing_bf16(ref), 2^-24).  gelu_tanh is seven f32
    operations on an exact input: its error is orders of magnitude below one bf16 spacing, so the stored value must be one of the two
    bf16 neighbours of the true value.  Where the device's exp2 saturates (x <~ -10) the true value is below 1e-30: the floor.
    (``tol`` = gelu_tol(ref64) made earlier, for a caller that compares on another device.)"""
    tol = gelu_tol(ref64) if tol is None else tol
    return ~((got_bf16.to(F32).double() - ref64).abs() < tol)


def rounding_census(v64):
    """(share of values not representable in bf16, number of exact ties) of an exact f32-representable tensor."""
    down = v64.to(F32).view(torch.int32).bitwise_and(-65536).view(F32).double()      # truncation toward zero
    inexact = down != v64
    up = down + torch.copysign(spacing_bf16(down), v64)
    # (truncating the low 16 bits of an f32 stays inside v's binade, so spacing_bf16(down) is the spacing around v)
    ties = inexact & ((v64 - down).abs() == (up - v64).abs())
    return float(inexact.double().mean()), int(ties.sum())


# ---- GEMV: out[m, n] = sum_k x[m, k] W[n, k] + bias[n], in_act = out_act = 0 ----
@functools.lru_cache(maxsize=4)
def make_gemv(M, N, K):
    g = _gen("gemv", M, N, K)
    x, w, bias = _ints(g, (M, K), -3, 3), _ints(g, (N, K), -2, 5), _ints(g, (N,), -64, 64)
    return SimpleNamespace(M=M, N=N, K=K, x=exact_f32(x, "x"), w=_narrow(w, BF16, "W"), bias=exact_f32(bias, "bias"))


def expected_gemv(inp, use_bias):
    acc = inp.x.double() @ inp.w.to(F32).double().t()
    exact_f32(acc, "gemv accumulator")
    return exact_f32(acc + inp.bias.double()[None, :] if use_bias else acc, "gemv acc + bias")
