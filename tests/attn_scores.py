"""Score-distribution constructions, a float64 restatement and derived error bounds for the attention kernels.

Every shipped attention kernel (csrc/attn7.hip, attn7p.hip, attn8.hip) runs a LAZY running max: a 32- (bf16) or 64-key
(e4m3) block re-bases O, l and m only when a lane's partial sum of P exceeds 2^thr (thr = option attn_defer_max_log2,
default 8) or there is no reference yet.  Random N(0, 1) inputs give near-uniform softmax rows that take that branch on the
first tile and then almost never; the constructions here make it run where they say.

Constructions realise per-row integer score profiles EXACTLY: row group g owns channels (2g, 2g+1) of every head, its
queries hold (1, 1) there and key j holds (16 a_j, b_j) with s_j = 16 a_j + b_j, |a_j| <= 16, |b_j| <= 8.  Those values
have <= 4 significant bits, so they are exact in bf16 AND in e4m3 after the head's power-of-two scale, and every score is
an f32-exact integer.  V entries are +-(1 + k/8) 2^e, e in [-2, 2]: exact in both formats and never 0.

Units: a score s is in log2 units.  The unit-scale launches (scale * log2 e == 1) and attn8 compute exactly q.k; the
sc != 1 path of attn7 / attn7p keeps m in RAW score units and multiplies by sc = fl32(fl32(scale) * fl32(log2 e)), so the
carried m of that path compares as m * sc.

The bounds (derived, not fitted; u = 2^-24, e_x = 2^-22 for v_exp_f32):
  m (carried, non-last chunk):  m <= max_j s_j + ds  and  max_j s_j - m <= thr + ds      (ds: the row's score error bound)
  l (carried):  |l - sum_j 2^(s_j - m)| <= r_l * sum_j 2^(s_j - m)                         (the kernels sum UNROUNDED P)
                r_l = (n_tiles + 40) u + (2 n_tiles + 2) e_x + ln2 ds
  acc (carried), per element:  |acc_i - sum_j P_j v_ji| <= eps_P * sum_j P_j |v_ji| (+ abs_P * sum_j |v_ji| for e4m3)
                eps_P = 2^-8 + ln2 ds + 6 n_tiles u (bf16: the unit roundoff of P (8 significant bits), the alpha
                multiplies, the MFMA sums)
                eps_P = 2^-4 + ...,  abs_P = 2^-10 (e4m3: half an ulp of a normal, half the smallest subnormal)
  output:  |o - ref| <= (1 + 2^-8) (E_acc / L + r_l |ref|) / (1 - r_l) + 2^-8 (1 + 2^-8) |ref|
           (the acc and l bounds, the f32 division and the final bf16 rounding, unit roundoff 2^-8; holds for any score
           distribution)

A numpy-free torch emulator of the loop (64-key tiles, per-lane partial sums, thr, bf16 or e4m3 P, alpha re-bases,
carried state, masked ragged tail, attn8's pipelined S(t+1) correction) exists only to show that these bounds hold for a
correct loop and REJECT the mutants in MUTATIONS (tests/test_attn_scores_cpu.py).
"""
import math
from typing import Dict, List, Optional, Sequence

import torch

D = 128
KVB = 64
NEG_BIG = -1.0e30
U32 = 2.0 ** -24
EXP2_ERR = 2.0 ** -22
LN2 = math.log(2.0)
LOG2E_F32 = float(torch.tensor(1.4426950408889634, dtype=torch.float32))
FP8_MAX = 448.0
A_MAX, B_MAX = 16, 8
S_MAX = 16 * A_MAX + B_MAX                  # largest |score| a profile may hold


def kernel_sc(scale: float) -> float:
    """attc::fill_params: sc = fl32(scale * fl32(log2 e)), snapped to 1 when within 1e-6 (the unit-scale convention)."""
    sc = float(torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E_F32, dtype=torch.float32))
    return 1.0 if abs(sc - 1.0) < 1e-6 else sc


def scale_for_sc(sc: float) -> float:
    """The launch scale whose kernel sc is (close to) ``sc`` log2 units per unit of q.k."""
    return sc * LN2


# ---------------------------------------------------------------------------------------------------------------------
# constructions
# ---------------------------------------------------------------------------------------------------------------------
def v_values(rows: int, heads: int, seed: int) -> torch.Tensor:
    """bf16 [rows, heads*128] of +-(1 + k/8) 2^e, e in [-2, 2]: exact in bf16 and in e4m3 after any power-of-two scale."""
    g = torch.Generator().manual_seed(seed)
    mant = 1.0 + torch.randint(0, 8, (rows, heads * D), generator=g).float() / 8.0
    ex = torch.randint(-2, 3, (rows, heads * D), generator=g).float()
    sgn = torch.randint(0, 2, (rows, heads * D), generator=g).float() * 2 - 1
    return (sgn * mant * torch.exp2(ex)).to(torch.bfloat16)


def realise(profiles: torch.Tensor, group: torch.Tensor, heads: int, v_seed: int) -> Dict:
    """profiles int [G, Skv] (|s| <= S_MAX), group int [Sq] (row -> profile) -> bf16 q [Sq, H*128], k, v [Skv, H*128].
    Every head gets the same scores (its own V)."""
    G, Skv = profiles.shape
    assert G <= D // 2 and int(profiles.abs().max()) <= S_MAX
    a = torch.round(profiles.double() / 16.0)
    a = a.clamp(-A_MAX, A_MAX)
    b = profiles.double() - 16.0 * a
    assert bool((b.abs() <= B_MAX).all())
    Sq = group.shape[0]
    qh = torch.zeros((Sq, D), dtype=torch.float64)
    qh[torch.arange(Sq), 2 * group] = 1.0
    qh[torch.arange(Sq), 2 * group + 1] = 1.0
    kh = torch.zeros((Skv, D), dtype=torch.float64)
    kh[:, 0:2 * G:2] = (16.0 * a).t()
    kh[:, 1:2 * G:2] = b.t()
    q = qh.repeat(1, heads).to(torch.bfloat16)
    k = kh.repeat(1, heads).to(torch.bfloat16)
    assert torch.equal(q.double(), qh.repeat(1, heads)) and torch.equal(k.double(), kh.repeat(1, heads))
    return dict(q=q, k=k, v=v_values(Skv, heads, v_seed), profiles=profiles, group=group)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def one_hot(Sq: int, Skv: int, heads: int, positions: Sequence[int], seed: int = 0, margin: int = 80) -> Dict:
    """Row group g has ONE dominant key, at positions[g], ``margin`` log2 units above every other key of the row
    (background: integers in [-64, 0]).  The dominant key always forces a re-base, so P_dom = 2^0 exactly and every other
    P <= 2^-margin: the output row must be that key's V row bit for bit."""
    pos = [p % Skv for p in positions]
    G = len(pos)
    assert margin + 64 <= 2 * S_MAX
    prof = -torch.randint(0, 65, (G, Skv), generator=_gen(seed)) + (S_MAX - margin)
    prof[torch.arange(G), torch.tensor(pos)] = S_MAX
    group = torch.arange(Sq) % G
    c = realise(prof, group, heads, seed + 1)
    c["dom"] = torch.tensor(pos)[group]
    c["name"] = "one_hot"
    return c


def staircase(Sq: int, Skv: int, heads: int, rise_tiles: Sequence[int], step: int = 9, seed: int = 0) -> Dict:
    """The row max rises by ``step`` (> thr = 8) at the first key of tile t for every t in rise_tiles (64-key tiles
    counted over the whole key axis); inside a level every other key sits 1 or 2 units below it, so the earlier keys'
    mass (2^-step of their old weight) stays visible after the re-base.  A correct loop raises m exactly at tile 0 and
    the rise tiles."""
    nt = (Skv + KVB - 1) // KVB
    rises = sorted(set(int(t) for t in rise_tiles if 0 < t < nt))
    level = torch.empty((nt,), dtype=torch.long)
    cur = -S_MAX + 2
    for t in range(nt):
        if t in rises:
            cur += step
        level[t] = cur
    assert cur <= S_MAX
    key_level = level.repeat_interleave(KVB)[:Skv]
    g = _gen(seed)
    prof = key_level[None, :] - torch.randint(1, 3, (1, Skv), generator=g)
    for t in [0] + rises:      # the level's top key: the tile's first key (the re-base must see it in that tile)
        prof[0, t * KVB] = level[t]
    group = torch.zeros(Sq, dtype=torch.long)
    c = realise(prof, group, heads, seed + 1)
    c["rises"] = [0] + rises
    c["name"] = "staircase"
    return c


def falling(Sq: int, Skv: int, heads: int, seed: int = 0) -> Dict:
    """The max is in the first tile; every later tile sits 20-100 log2 units below it (its P underflows or nearly so)."""
    g = _gen(seed)
    prof = -torch.randint(20, 101, (1, Skv), generator=g)
    prof[0, :min(KVB, Skv)] = -torch.randint(0, 8, (min(KVB, Skv),), generator=g)
    prof[0, min(5, Skv - 1)] = 0
    prof = prof + 150
    c = realise(prof, torch.zeros(Sq, dtype=torch.long), heads, seed + 1)
    c["name"] = "falling"
    return c


def mixed_rows(Sq: int, Skv: int, heads: int, seed: int = 0) -> Dict:
    """Inside every 32-row sub-block the even rows climb a staircase (a jump every 3rd tile) and the odd rows are flat:
    the wave-wide re-base runs with alpha = 1 on the rows that did not need it."""
    st = staircase(1, Skv, heads, range(3, (Skv + KVB - 1) // KVB, 3), seed=seed)["profiles"]
    flat = -torch.randint(0, 4, (1, Skv), generator=_gen(seed + 7))
    prof = torch.cat([st, flat], 0)
    c = realise(prof, torch.arange(Sq) % 2, heads, seed + 1)
    c["name"] = "mixed"
    return c


def ties(Sq: int, Skv: int, heads: int, seed: int = 0, value: int = 37) -> Dict:
    """All scores equal: P = 1 exactly (unit scale), the output is the column mean of V up to the f32 summation order."""
    prof = torch.full((1, Skv), value, dtype=torch.long)
    c = realise(prof, torch.zeros(Sq, dtype=torch.long), heads, seed + 1)
    c["name"] = "ties"
    return c


def temperature(Sq: int, Skv: int, heads: int, std_nat: float, seed: int = 0, offset: float = 192.0) -> Dict:
    """Random q.k with a score std of ``std_nat`` natural units (in log2 units: std_nat * log2 e), plus a per-row offset
    of +-offset log2 units (or 0) carried by channel 127 that every key holds as 1: softmax does not change, the kernel
    works far from 0 (and so does the ragged tail's NEG_BIG mask)."""
    g = _gen(seed)
    q = torch.zeros((Sq, heads * D))
    k = torch.zeros((Skv, heads * D))
    for h in range(heads):
        o = h * D
        q[:, o:o + D - 1] = torch.randn((Sq, D - 1), generator=g)
        k[:, o:o + D - 1] = torch.randn((Skv, D - 1), generator=g) * (std_nat * math.log2(math.e) / math.sqrt(D - 1))
        q[:, o + D - 1] = offset * (torch.randint(0, 3, (Sq,), generator=g).float() - 1.0)
        k[:, o + D - 1] = 1.0
    return dict(q=q.to(torch.bfloat16), k=k.to(torch.bfloat16), v=v_values(Skv, heads, seed + 1), name=f"temp{std_nat:g}")


# ---------------------------------------------------------------------------------------------------------------------
# e4m3 view of the inputs (R.attention_fp8's quantisation: per-head power-of-two scale from the abs-max)
# ---------------------------------------------------------------------------------------------------------------------
def fp8_dequant(x: torch.Tensor, heads: int) -> torch.Tensor:
    """[S, H*128] -> the dequantised e4m3 values (f64), per head scaled by 2^e, e = ceil(log2(amax / 448))."""
    x = x.double()
    out = torch.empty_like(x)
    for h in range(heads):
        sl = slice(h * D, (h + 1) * D)
        amax = float(x[:, sl].abs().max())
        e = math.ceil(math.log2(amax / FP8_MAX)) if amax > 0 else 0
        out[:, sl] = (x[:, sl] * 2.0 ** -e).float().to(torch.float8_e4m3fn).double() * 2.0 ** e
    return out


def is_fp8_exact(x: torch.Tensor, heads: int) -> bool:
    return bool(torch.equal(fp8_dequant(x, heads), x.double()))


# ---------------------------------------------------------------------------------------------------------------------
# float64 restatement
# ---------------------------------------------------------------------------------------------------------------------
def fp8_dequant_cuts(x: torch.Tensor, heads: int, cuts: Optional[Sequence[int]] = None) -> torch.Tensor:
    """fp8_dequant of every row range [cuts[i], cuts[i+1]) on its own (a chunk prepared with its own abs-max)."""
    if cuts is None:
        return fp8_dequant(x, heads)
    return torch.cat([fp8_dequant(x[a:b], heads) for a, b in zip(cuts[:-1], cuts[1:]) if b > a], 0)


def scores(q: torch.Tensor, k: torch.Tensor, heads: int, sc: float = 1.0, fp8: bool = False, cuts=None):
    """(s [H, Sq, Skv] in log2 units, ds [H, Sq] the row's bound on the kernel's score error) in float64 on q's device.
    ``cuts``: key rows quantised per range (fp8 chunks prepared one by one)."""
    if fp8:
        q, k = fp8_dequant(q, heads).to(q.device), fp8_dequant_cuts(k, heads, cuts).to(k.device)
    qh = q.double().reshape(q.shape[0], heads, D).transpose(0, 1)
    kh = k.double().reshape(k.shape[0], heads, D).transpose(0, 1)
    s = torch.matmul(qh, kh.transpose(1, 2)) * sc
    mag = torch.matmul(qh.abs(), kh.abs().transpose(1, 2)).amax(-1)
    # integer operands whose partial sums stay below 2^24: the MFMA's f32 sums are exact, only the scale / reference
    # subtraction rounds
    exact = bool(torch.equal(qh, torch.round(qh)) and torch.equal(kh, torch.round(kh))) and float(mag.max()) < 2.0 ** 23
    ds = U32 * ((0.0 if exact else 130.0) * mag * sc + 8.0 * s.abs().amax(-1))
    return s, ds


def heads_v(v: torch.Tensor, heads: int, fp8: bool = False, cuts=None) -> torch.Tensor:
    """V [Skv, H*128] -> [H, Skv, 128] float64 (dequantised e4m3 for the fp8 kernels)."""
    vv = fp8_dequant_cuts(v, heads, cuts).to(v.device) if fp8 else v.double()
    return vv.reshape(v.shape[0], heads, D).transpose(0, 1)


def ref_sums(s: torch.Tensor, vh: torch.Tensor, m: torch.Tensor):
    """At the reference m [H, Sq] (log2 units): L = sum_j 2^(s_j - m), A = sum_j 2^(s_j - m) v_j, B = sum_j 2^(s_j - m) |v_j|."""
    p = torch.exp2(s - m[..., None])
    return p.sum(-1), torch.matmul(p, vh), torch.matmul(p, vh.abs())


def ref_output(s, vh):
    """softmax output [H, Sq, 128] in float64 and the sums at the true row max."""
    m = s.amax(-1)
    L, A, B = ref_sums(s, vh, m)
    return A / L[..., None], L, A, B


def to_rows(x_h: torch.Tensor) -> torch.Tensor:
    """[H, Sq, 128] -> [Sq, H*128]."""
    return x_h.transpose(0, 1).reshape(x_h.shape[1], -1)


def from_rows(x: torch.Tensor, heads: int) -> torch.Tensor:
    """[Sq, H*128] -> [H, Sq, 128]."""
    return x.reshape(x.shape[0], heads, D).transpose(0, 1)


# ---------------------------------------------------------------------------------------------------------------------
# bounds (each check returns a list of failure strings: [] = pass)
# ---------------------------------------------------------------------------------------------------------------------
def n_tiles(keys: int, chunks: int = 1) -> int:
    return (keys + KVB - 1) // KVB + chunks


def eps_p(fp8: bool, ds: torch.Tensor, nt: int):
    rel = (2.0 ** -4 if fp8 else 2.0 ** -8) + 2 * EXP2_ERR + LN2 * ds + 6 * nt * U32
    return rel, (2.0 ** -10 if fp8 else 2.0 ** -126)


def r_l(ds: torch.Tensor, nt: int):
    return (nt + 40) * U32 + (2 * nt + 2) * EXP2_ERR + LN2 * ds


def check_state(s, ds, vh, acc, ml, thr: float, sc: float = 1.0, fp8: bool = False, chunks: int = 1, what: str = "") -> List[str]:
    """The carried (acc f32 [Sq, H*128], ml f32 [Sq, H, 2]) after the keys of s [H, Sq, n] / vh [H, n, 128] (everything
    attended so far).  m is compared in log2 units (m * sc)."""
    H = s.shape[0]
    dev = s.device
    m = ml[..., 0].double().to(dev).t() * sc              # [H, Sq] log2 units
    l = ml[..., 1].double().to(dev).t()
    a = from_rows(acc.double().to(dev), H)
    fails = []
    smax = s.amax(-1)
    if not bool(torch.isfinite(m).all() and torch.isfinite(l).all() and torch.isfinite(a).all()):
        return [f"{what}: non-finite carried state"]
    over = m - smax - ds
    if bool((over > 0).any()):
        fails.append(f"{what}: m above the row max by {float(over.max()):.4g}")
    lag = smax - m - thr - ds
    if bool((lag > 0).any()):
        fails.append(f"{what}: m lags the row max by {float((smax - m).max()):.4g} > thr {thr}")
    nt = n_tiles(s.shape[-1], chunks)
    L, A, B = ref_sums(s, vh, m)
    rl = r_l(ds, nt)
    el = (l - L).abs() / L
    if bool((el > rl).any()):
        fails.append(f"{what}: l off by {float(el.max()):.4g} relative (bound {float(rl.max()):.3g})")
    eps, absp = eps_p(fp8, ds, nt)
    sum_abs_v = vh.abs().sum(1)[:, None, :]
    bound = eps[..., None] * B + absp * sum_abs_v + 1e-30
    ea = (a - A).abs()
    if bool((ea > bound).any()):
        i = torch.argmax((ea / bound).flatten())
        fails.append(f"{what}: acc off by {float(ea.flatten()[i]):.4g} > bound {float(bound.flatten()[i]):.4g} "
                     f"({int((ea > bound).sum())} elements)")
    return fails


def output_bound(s, ds, vh, fp8: bool = False, chunks: int = 1):
    """(ref [H, Sq, 128] float64, per-element bound) for the normalised bf16 output of attention over s / vh."""
    ref, L, A, B = ref_output(s, vh)
    nt = n_tiles(s.shape[-1], chunks)
    rl = r_l(ds, nt)[..., None]
    eps, absp = eps_p(fp8, ds, nt)
    e_acc = eps[..., None] * B + absp * vh.abs().sum(1)[:, None, :]
    e1 = (e_acc / L[..., None] + rl * ref.abs()) / (1 - rl)
    return ref, (1 + 2.0 ** -8) * (e1 + 2.0 ** -8 * ref.abs()) + 1e-30


def check_output(o, s, ds, vh, fp8: bool = False, chunks: int = 1, prev=None, what: str = "") -> List[str]:
    """o bf16 [Sq, H*128]; ``prev`` (attention_add): the bf16 o before the launch, expected bf16(prev + attention)."""
    H = s.shape[0]
    ref, bnd = output_bound(s, ds, vh, fp8, chunks)
    got = from_rows(o.double().to(s.device), H)
    if prev is not None:
        pv = from_rows(prev.double().to(s.device), H)
        bnd = bnd + 2.0 ** -8 * (pv + ref).abs() * (1 + 2.0 ** -8)
        ref = ref + pv
    if not bool(torch.isfinite(got).all()):
        return [f"{what}: non-finite output"]
    err = (got - ref).abs()
    if bool((err > bnd).any()):
        i = torch.argmax((err / bnd).flatten())
        return [f"{what}: output off by {float(err.flatten()[i]):.4g} > bound {float(bnd.flatten()[i]):.4g} "
                f"({int((err > bnd).sum())}/{err.numel()} elements)"]
    return []


def check_suite_bar(o, s, vh, prev=None, what: str = "") -> List[str]:
    """The suite's attention bar (tests/test_kernels_gpu.py): |d| <= 2^-7 |ref| + 2^-5 rms(ref), rms err <= 2^-7 rms(ref)."""
    H = s.shape[0]
    ref = ref_output(s, vh)[0]
    if prev is not None:
        ref = ref + from_rows(prev.double().to(s.device), H)
    got = from_rows(o.double().to(s.device), H)
    rms = ref.pow(2).mean().sqrt()
    fails = []
    if float((got - ref).pow(2).mean().sqrt()) > 2.0 ** -7 * float(rms):
        fails.append(f"{what}: rms err above 2^-7 rms")
    if bool(((got - ref).abs() > 2.0 ** -7 * ref.abs() + 2.0 ** -5 * rms).any()):
        fails.append(f"{what}: element outside 2^-7 |ref| + 2^-5 rms")
    return fails


def expected_one_hot(c: Dict, heads: int, fp8: bool = False) -> torch.Tensor:
    """bf16 [Sq, H*128]: the dominant key's V row (e4m3: its dequantised code times the head's scale, exact in bf16)."""
    v = fp8_dequant(c["v"], heads) if fp8 else c["v"].double()
    e = v[c["dom"]]
    out = e.to(torch.bfloat16)
    assert torch.equal(out.double(), e)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# CPU emulator of the lazy-max loop (for the bounds only)
# ---------------------------------------------------------------------------------------------------------------------
MUTATIONS = ("alpha_not_on_l", "alpha_not_on_o", "alpha_twice", "no_rebase_last_tile", "no_dm_correction",
             "mask_off_by_one", "ignore_incoming_m", "permute_v_rows")

# key slot of the accumulator layout: lane (row, hi) holds keys (r & 3) + 8 (r >> 2) + 4 hi, r = 0..15, of a 32-key block
_HALF = torch.tensor([[(r & 3) + 8 * (r >> 2) + 4 * hi for r in range(16)] for hi in range(2)])


def _round_p(p: torch.Tensor, fp8: bool) -> torch.Tensor:
    return p.to(torch.float8_e4m3fn).float() if fp8 else p.to(torch.bfloat16).float()


def emulate(s: torch.Tensor, vh: torch.Tensor, chunks: Sequence[int], thr: float, fp8: bool = False,
            mutation: Optional[str] = None):
    """Run the loop over s [H, Sq, Skv] (f32-exact log2 scores, unit scale) / vh [H, Skv, 128] with the key axis cut into
    launches of ``chunks`` keys (carried state between them).  bf16 = attn7p's loop (a re-base decision per 32-key half,
    16-key lane partials, the not-yet-used half re-based by dm); fp8 = attn8's pipelined loop (one decision per 64-key
    tile, 32-key lane partials, S(t+1) computed against the old reference and corrected by dm).
    Returns (o bf16 [Sq, H*128], states [(acc, ml, keys_so_far) after every non-last chunk], rebase_tiles[H][Sq]: the
    64-key tiles of the whole key axis whose key raised the row's m)."""
    assert mutation is None or mutation in MUTATIONS
    H, Sq, Skv = s.shape
    assert sum(chunks) == Skv
    nb = (Sq + 31) // 32
    pad = nb * 32 - Sq
    sf = torch.cat([s.float(), s[:, -1:].float().expand(H, pad, Skv)], 1) if pad else s.float()
    vf = vh.float()
    R = nb * 32
    o_all, states = [], []
    rebases = [[set() for _ in range(Sq)] for _ in range(H)]
    ot = torch.zeros((H, R, D))
    m_run = torch.full((H, R), NEG_BIG)
    l_run = torch.zeros((H, R))
    p_lim = 2.0 ** thr
    k0 = 0
    for ci, n in enumerate(chunks):
        last_chunk = ci == len(chunks) - 1
        if ci > 0 and mutation == "ignore_incoming_m":
            m_run = torch.full((H, R), NEG_BIG)
        m_base = torch.where(m_run < -1e29, torch.zeros_like(m_run), m_run)
        nt = (n + KVB - 1) // KVB
        ss = sf[:, :, k0:k0 + n]
        vv = vf[:, k0:k0 + n]
        # one padding key past the end: the clamped re-read of the last row (what an off-by-one mask would let in)
        ss = torch.cat([ss, ss[:, :, -1:].expand(H, R, nt * KVB - n)], -1)
        vv = torch.cat([vv, vv[:, -1:].expand(H, nt * KVB - n, D)], 1)
        lim = n + (1 if mutation == "mask_off_by_one" else 0)
        valid = torch.arange(nt * KVB) < lim

        def tile_scores(t, ref):
            st = ss[:, :, t * KVB:(t + 1) * KVB] - ref[..., None]
            return torch.where(valid[t * KVB:(t + 1) * KVB], st, torch.full_like(st, NEG_BIG))

        sn = tile_scores(0, m_base)
        for t in range(nt):
            st = sn
            m_base_top = m_base          # the reference S(t+1) is started against (attn8 issues it before tile t's re-base)
            vt = vv[:, t * KVB:(t + 1) * KVB]
            if mutation == "permute_v_rows" and t == nt - 1:
                vt = vt.flip(1)
            blocks = [(0, 32), (32, 64)] if not fp8 else [(0, 64)]
            psum = torch.zeros((H, R))
            for (b0, b1) in blocks:
                pv = torch.exp2(st[..., b0:b1])
                lane_ps = torch.stack([sum(pv[..., _HALF[hi] + off].sum(-1) for off in range(0, b1 - b0, 32)) for hi in range(2)], -1)
                no_ref = m_run < -1e29
                need = ((lane_ps > p_lim).any(-1) | no_ref).reshape(H, nb, 32).any(-1)      # __any over the wave's 32 rows
                need = need[..., None].expand(H, nb, 32).reshape(H, R)
                if mutation == "no_rebase_last_tile" and t == nt - 1:
                    need = torch.zeros_like(need)
                if bool(need.any()):
                    mloc = st[..., b0:b1].amax(-1) + m_base
                    m_new = torch.where(need, torch.maximum(m_run, mloc), m_run)
                    alpha = torch.exp2(m_run - m_new)
                    arg = st[..., b0:b1].argmax(-1)
                    for hh in range(H):
                        for r in torch.nonzero(m_new[hh, :Sq] > m_run[hh, :Sq]).flatten().tolist():
                            rebases[hh][r].add((k0 + t * KVB + b0 + int(arg[hh, r])) // KVB)
                    a_l = torch.ones_like(alpha) if mutation == "alpha_not_on_l" else alpha
                    a_o = torch.ones_like(alpha) if mutation == "alpha_not_on_o" else alpha
                    if mutation == "alpha_twice":
                        a_l, a_o = alpha * alpha, alpha * alpha
                    m_run = m_new
                    l_run = (l_run + psum) * a_l
                    psum = torch.zeros_like(psum)
                    ot = ot * a_o[..., None]
                    dm = (m_new - m_base)[..., None]
                    m_base = m_new
                    keep = b0 if (fp8 or mutation != "no_dm_correction") else 32
                    st = torch.cat([st[..., :b0], st[..., b0:b1] - dm, st[..., b1:] - (dm if keep < b1 else 0)], -1)
                    pv = torch.exp2(st[..., b0:b1])
                psum = psum + pv.sum(-1)
                ot = ot + torch.matmul(_round_p(pv, fp8), vt[:, b0:b1])     # this block's PV, issued before the next block's re-base
            l_run = l_run + psum
            if t + 1 < nt:
                ref = m_base_top if (fp8 and mutation == "no_dm_correction") else m_base
                sn = tile_scores(t + 1, ref)
        k0 += n
        if not last_chunk:
            acc = to_rows(ot[:, :Sq])
            ml = torch.stack([m_run[:, :Sq].t(), l_run[:, :Sq].t()], -1)
            states.append((acc.clone(), ml.clone(), k0))
    o = to_rows(ot[:, :Sq] / l_run[:, :Sq, None]).to(torch.bfloat16)
    return o, states, rebases
