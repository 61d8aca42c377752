"""Call-by-call checking of the padded-volume VAE executor (infinicube_amd/videogen/vae_hip.py) - a helper, no tests in it.

  * ``HostVaeHip``: VaeHip with the two libicvideo kernels restated in torch (the C ABI's contract), so the host logic runs without a GPU.
  * ``recording(base)``: a class over ``VH.VaeHip`` or ``HostVaeHip`` that keeps one ``Record`` per ``conv`` / ``norm_act`` call.
  * ``check_record(rec)``: an fp64 reference of that ONE call, computed on the CPU from the INTERIOR of its input with zero padding -
    never from the buffer's halo, margins or padding frames: a halo that should have been zero shows up as a mismatch instead of being
    reproduced - plus the layout the next call relies on (zero padding frames / margins, nothing written before ``first_frame``).
  * the cases of tests/test_vae_widths_gpu.py (every convolution geometry, block and tile network of the shipped ``dim=96`` VAE at the
    smallest shapes that still span two 256-row tiles with a ragged tail) and their runners, shared with tests/test_vae_trace_cpu.py,
    which runs them on ``HostVaeHip`` and shows that every mutant of ``MUTANTS`` is rejected: that is what makes the checks trustworthy.

A failed check raises ``CheckError`` whose ``check`` names it (``conv.value``, ``norm.layout``, ``block.d``, ...)."""
import contextlib
import copy
import functools
import inspect
import textwrap
import zlib
from unittest import mock

import torch
import torch.nn as nn
import torch.nn.functional as F

from infinicube_amd.videogen import vae as V
from infinicube_amd.videogen import vae_hip as VH

BF16 = torch.bfloat16
PT = VH.PT


class HostVaeHip(VH.VaeHip):
    """VaeHip with the two kernels restated in torch (the C ABI's contract, fp32 accumulate, one rounding)."""

    def __init__(self, net, device="cpu"):
        self.net, self.device, self.lib = net, torch.device(device), None
        self._w, self._g = {}, {}

    def conv(self, x, mod, taps, resid=None, first_frame=0):
        rec = self._conv_w(mod, taps)
        assert x.C == rec.cin
        out = VH.Vol(x.T, x.H, x.W, rec.cout, self.device)
        m0, m1 = (VH.PT + first_frame) * x.frame_rows, x.rows
        offs = list(rec.offsets(x.Hp, x.Wp))
        assert m0 + min(offs) >= -x.margin and (m1 - 1) + max(offs) < m1 + x.margin, "a tap leaves the buffer"
        W = rec.w.float()[:, : len(taps) * rec.cin].view(rec.cout, len(taps), rec.cin)
        assert float(rec.w.float()[:, len(taps) * rec.cin:].abs().sum()) == 0.0
        acc = rec.bias[None].repeat(m1 - m0, 1)
        for i, off in enumerate(offs):
            acc = acc + x.buf[x.margin + m0 + off: x.margin + m1 + off].float() @ W[:, i].T
        if resid is not None:
            acc = acc + resid.mat[m0:m1].float()
        out.mat[m0:m1] = acc.to(torch.bfloat16)
        return out

    def norm_act(self, x, norm, act):
        out = VH.Vol(x.T, x.H, x.W, x.C, self.device, zero_pads=False)
        out.buf.zero_()
        xi = x.interior().float()
        y = xi / xi.norm(dim=-1, keepdim=True).clamp_min(1e-12) * norm.scale * self._gamma(norm)
        out.interior().copy_((F.silu(y) if act else y).to(torch.bfloat16))
        return out


# ---- recording ---------------------------------------------------------------------------------------------------------------

class Record:
    """One ``conv`` / ``norm_act`` call.  ``x`` / ``resid``: clones of the operands' interiors [T, H, W, C] taken BEFORE the call;
    ``out``: the output volume as the call left it - a copy, because later steps write into volumes they were handed (``upsample``
    zeroes frame 0 of its input, ``downsample`` its halo)."""

    def __init__(self, op, mod, x, out, taps=None, first_frame=0, resid=None, act=0):
        self.op, self.mod, self.taps, self.first_frame, self.act = op, mod, taps, first_frame, act
        self.x, self.resid, self.out, self.poison = x, resid, out, VH.Vol.POISON

    def __repr__(self):
        w = "" if self.op == "norm" else f" {tuple(self.mod.weight.shape)} taps={len(self.taps)} first_frame={self.first_frame} resid={self.resid is not None}"
        return f"<{self.op}{w} on {tuple(self.x.shape)}>"


def _snapshot(v):
    s = copy.copy(v)
    s.buf = v.buf.clone()
    return s


@functools.lru_cache(maxsize=None)
def recording(base):
    """``base`` (VH.VaeHip or HostVaeHip) with every kernel call appended to ``self.records``."""

    class Recording(base):
        def __init__(self, *args, **kwargs):
            super().__init__(*args, **kwargs)
            self.records = []

        def conv(self, x, mod, taps, resid=None, first_frame=0):
            xi = x.interior().clone()
            ri = resid.interior().clone() if resid is not None else None
            out = super().conv(x, mod, taps, resid=resid, first_frame=first_frame)
            self.records.append(Record("conv", mod, xi, _snapshot(out), taps=taps, first_frame=first_frame, resid=ri))
            return out

        def norm_act(self, x, norm, act):
            xi = x.interior().clone()
            out = super().norm_act(x, norm, act)
            self.records.append(Record("norm", norm, xi, _snapshot(out), act=act))
            return out

    Recording.__name__ = f"Recording{base.__name__}"
    return Recording


# ---- the checks --------------------------------------------------------------------------------------------------------------

class CheckError(AssertionError):
    def __init__(self, check, msg):
        super().__init__(f"[{check}] {msg}")
        self.check = check


def _require(ok, check, msg):
    if not ok:
        raise CheckError(check, msg() if callable(msg) else msg)


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def _all_zero(t):
    return bool((t == 0).all())          # a NaN is not == 0


def conv_reference(rec):
    """fp64: ref[t, h, w] = bias + sum_taps xpad[t + dt, h + dh, w + dw] . W_tap^T (+ resid), the interior zero-padded by 2 on every side
    of H and W and by 2 frames in front; weights = the module's own, bf16-rounded, taps in the order of reshape(cout, cin, -1)."""
    w = rec.mod.weight.detach().to(BF16).double().cpu()
    cout, cin = w.shape[:2]
    w = w.reshape(cout, cin, -1)
    assert w.shape[2] == len(rec.taps)
    x = rec.x.double().cpu()[..., :cin]
    T, H, W_, _ = x.shape
    xp = F.pad(x, (0, 0, 2, 2, 2, 2, 2, 0))
    ref = torch.zeros((T, H, W_, cout), dtype=torch.float64)
    if rec.mod.bias is not None:
        ref += rec.mod.bias.detach().double().cpu()
    for i, (dt, dh, dw) in enumerate(rec.taps):
        assert -2 <= dt <= 0 and abs(dh) <= 2 and abs(dw) <= 2
        ref += xp[2 + dt: 2 + dt + T, 2 + dh: 2 + dh + H, 2 + dw: 2 + dw + W_] @ w[:, :, i].T
    if rec.resid is not None:
        ref += rec.resid.double().cpu()[..., :cout]
    return ref


def _check_conv(rec):
    out, ff = rec.out, rec.first_frame
    cout = rec.mod.weight.shape[0]
    ref = conv_reference(rec)[ff:]
    got = out.interior()[ff:].float().cpu()
    _require(bool(torch.isfinite(got).all()), "conv.finite",
             lambda: f"{rec}: {int((~torch.isfinite(got)).sum())} non-finite values on the real positions: a halo / margin / padding value reached them")
    # the project's per-op bar (test_vae_hip_gpu._per_op_ok): the one bf16 rounding is off by at most 2^-8 |ref| (half an ulp just
    # above a power of two), fp32 accumulation over K <= 10368 adds about 2^-16 rms: a correct call stays below half of the bar
    d = (got[..., :cout].double() - ref).abs()
    tol = ref.abs() * 2 ** -7 + ref.pow(2).mean().sqrt() * 2 ** -8
    bad = d > tol
    _require(not bad.any(), "conv.value", lambda: f"{rec}: {int(bad.sum())} of {bad.numel()} outside the per-op bar, max |d| {float(d.max()):.4g}, rms(ref) {float(ref.pow(2).mean().sqrt()):.4g}")
    _require(_all_zero(got[..., cout:]), "conv.pad_channels", f"{rec}: padded output channels must be exactly 0")
    _require(_all_zero(out.vol()[:PT]) and _all_zero(out.buf[: out.margin]) and _all_zero(out.buf[out.margin + out.rows:]), "conv.padding",
             f"{rec}: the output's padding frames and margins must be exactly 0")
    if rec.poison and ff:
        _require(bool(torch.isnan(out.vol()[PT: PT + ff].float()).all()), "conv.untouched", f"{rec}: something was written before first_frame = {ff}")
    return float((d / tol).max())


def _check_norm(rec):
    out = rec.out
    x = rec.x.double().cpu()
    ref = x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12) * rec.mod.scale * rec.mod.gamma.detach().double().cpu().reshape(-1)
    if rec.act:
        ref = ref * torch.sigmoid(ref)
    got = out.interior().double().cpu()
    d = (got - ref).abs()          # NaN compares false below
    tol = 2.0 ** -8 * ref.abs() + 1e-6
    _require(bool((d <= tol).all()), "norm.value", lambda: f"{rec}: max err {float(d.max())}, non-finite {int((~torch.isfinite(got)).sum())}")
    full = out.vol().clone()
    full[PT:, 1:-1, 1:-1] = 0
    _require(_all_zero(full) and _all_zero(out.buf[: out.margin]) and _all_zero(out.buf[out.margin + out.rows:]), "norm.layout",
             f"{rec}: padding frames, halo and margins must be written as zeros")
    return float((d / tol).max())


def check_record(rec):
    """Raises CheckError; returns the call's largest error as a fraction of its bar."""
    return _check_conv(rec) if rec.op == "conv" else _check_norm(rec)


def check_records(records):
    """check_record on every call; returns the largest fraction per op.  (A norm reaches 0.99 of its bar as a matter of course: the
    bar IS one bf16 rounding, relative 2^-8 at its worst just above a power of two; a convolution stays below half of its bar.)"""
    assert records, "nothing was recorded"
    worst = {}
    for r in records:
        worst[r.op] = max(worst.get(r.op, 0.0), check_record(r))
    return worst


# ---- modules and inputs ------------------------------------------------------------------------------------------------------

def _seed(name):
    torch.manual_seed(zlib.crc32(name.encode()) & 0x7FFFFFFF)


def _randomise(mod):
    """bf16-exact parameters: weights as initialised, gammas in [0.5, 1.5], biases random."""
    with torch.no_grad():
        for name, p in mod.named_parameters():
            if name.endswith("gamma"):
                p.copy_(torch.rand_like(p) + 0.5)
            elif name.endswith("bias"):
                p.copy_(torch.randn_like(p) * 0.1)
            p.copy_(p.to(BF16).float())
    return mod.eval()


CONV_KINDS = {
    "111": (lambda ci, co: V.CausalConv3d(ci, co, 1), VH.TAPS_111),
    "311": (lambda ci, co: V.CausalConv3d(ci, co, (3, 1, 1), padding=(1, 0, 0)), VH.TAPS_311),
    "333": (lambda ci, co: V.CausalConv3d(ci, co, 3, padding=1), VH.TAPS_333),
}

# (kind, cin, cout, with_resid, first_frame) on T, H, W = 3, 5, 9: 5 x 7 x 11 = 385 padded rows = one full row tile + a ragged one
CONV_THW = (3, 5, 9)
CONV_CASES = [
    ("111", 32, 96, False, 0),           # one K-tile
    ("111", 64, 128, False, 0),          # one K-tile
    ("311", 96, 96, False, 0),           # 9 halves: the last K-tile's upper half is padding
    ("311", 384, 768, False, 0),         # the decoder's time_conv: 4 N-tiles of 192
    ("111", 384, 1152, False, 0),        # to_qkv: 6 N-tiles of 192
    ("111", 96, 288, False, 0),          # 3 N-tiles of 96: the cout % 96 == 0 && cout % 192 != 0 branch
    ("333", 384, 384, False, 0),         # 162 K-tiles
    ("333", 384, 384, True, 0),
    ("333", 3, 96, False, 0),            # input channels padded to 32
    ("333", 16, 384, False, 0),          # input channels padded to 32
    ("333", 96, 3, False, 0),            # filters padded to 4
    ("333", 384, 32, False, 0),
    ("311", 192, 192, False, 1),         # the temporal resamplers' row ranges
    ("311", 192, 192, False, 2),
]


def conv_case_id(case):
    kind, ci, co, resid, ff = case
    return f"{kind}-{ci}to{co}" + ("-resid" if resid else "") + (f"-from{ff}" if ff else "")


def run_conv_case(make_exec, device, case):
    """One convolution through the recording executor; every check of check_record."""
    kind, ci, co, with_resid, ff = case
    _seed("conv" + conv_case_id(case))
    make, taps = CONV_KINDS[kind]
    mod = _randomise(make(ci, co))
    T, H, W = CONV_THW
    x = (torch.randn(1, ci, T, H, W) * 0.5).to(BF16)
    r = torch.randn(1, co, T, H, W).to(BF16)
    hip = make_exec(nn.Identity(), device)
    xv = hip._to_vol(x.to(device), VH._ceil(ci, 32))
    rv = hip._to_vol(r.to(device), VH._ceil(co, 4)) if with_resid else None
    hip.conv(xv, mod, taps, resid=rv, first_frame=ff)
    (rec,) = hip.records
    assert rec.x.shape == (T, H, W, VH._ceil(ci, 32)) and rec.out.rows == 385
    return check_record(rec)


# (block, cin, cout, (T, H, W)): the shipped widths
BLOCK_CASES = [("res_block", ci, co, (3, 6, 10)) for ci, co in ((96, 96), (96, 192), (192, 384), (384, 384))]
BLOCK_CASES += [("attn_block", 384, 384, (2, 5, 7))]
BLOCK_CASES += [("upsample3d", 384, 192, (T, 4, 6)) for T in (1, 2, 3)]
BLOCK_CASES += [("upsample2d", 192, 96, (2, 4, 6)), ("downsample2d", 96, 96, (2, 8, 12))]
BLOCK_CASES += [("downsample3d", 192, 192, (T, 8, 12)) for T in (1, 3, 5)]
BLOCK_CASES += [("downsample3d", 384, 384, (5, 4, 6))]


def block_case_id(case):
    kind, ci, co, thw = case
    return f"{kind}-{ci}" + (f"to{co}" if kind == "res_block" else "") + "-" + "x".join(map(str, thw))


def _run_block(hip, kind, mod, x):
    """The VaeHip method of the stock module ``mod`` on _to_vol(x) -> [1, C, T, H, W] on the CPU, fp32."""
    xv = hip._to_vol(x.to(hip.device), x.shape[1])
    method = {"res_block": hip.res_block, "attn_block": hip.attn_block}.get(kind, hip.upsample if kind.startswith("up") else hip.downsample)
    out = method(mod, xv)
    return out.interior().permute(3, 0, 1, 2)[None].float().cpu()


_ACTIVE_MUTANTS = []


@functools.lru_cache(maxsize=None)
def block_setup(case):
    """(stock module, input, the module's fp32 output, HostVaeHip's output, e_host) - computed once per case and left unchanged."""
    assert not _ACTIVE_MUTANTS, "the references must come from the unpatched executor"
    kind, ci, co, (T, H, W) = case
    _seed("block" + block_case_id(case))
    if kind == "res_block":
        mod = V.ResidualBlock(ci, co)
    elif kind == "attn_block":
        mod = V.AttentionBlock(ci)
        with torch.no_grad():
            mod.to_qkv.weight.mul_(3)          # scores with some contrast
    else:
        mod = V.Resample(ci, kind)
    mod = _randomise(mod)
    x = torch.randn(1, ci, T, H, W).to(BF16)
    with torch.no_grad():
        ref = mod(x.float())
        host = _run_block(HostVaeHip(nn.Identity()), kind, mod, x)
    assert host.shape == ref.shape and ref.shape[1] == co
    return mod, x, ref, host, _rel(host, ref)


def run_block_case(make_exec, device, case):
    """Every recorded call passes check_record; the output is finite and has the stock module's shape; against HostVaeHip (d) and the
    fp32 module (e) the result is no farther than the restatement's own rounding allows.  Returns the figures."""
    kind = case[0]
    mod, x, ref, host, e_host = block_setup(case)
    hip = make_exec(nn.Identity(), device)
    with torch.no_grad():
        got = _run_block(hip, kind, mod, x)
    worst = check_records(hip.records)
    _require(got.shape == ref.shape, "block.shape", f"{got.shape} != {ref.shape}")
    _require(bool(torch.isfinite(got).all()), "block.finite", "non-finite output")
    figs = dict(calls=len(hip.records), worst_call=worst, e_host=e_host, d=_rel(got, host), e=_rel(got, ref))
    if kind == "attn_block":          # the executor's stock SDPA may round differently from the CPU's: the factor 2 is for that alone
        _require(figs["e"] <= 2 * e_host, "block.attn", f"rel-L2 vs fp32 {figs['e']:.3g} > 2 x e_host = 2 x {e_host:.3g}")
    else:                             # same rounding points: the two can differ only where summation order / __expf flips a bf16 rounding
        _require(figs["d"] <= e_host, "block.d", f"rel-L2 vs HostVaeHip {figs['d']:.3g} > e_host {e_host:.3g}")
    return figs


# ---- the whole tile networks at the shipped width ------------------------------------------------------------------------------

NET_CASES = [("decode", (1, 16, 2, 3, 4)), ("decode", (1, 16, 1, 2, 2)), ("encode", (1, 3, 5, 16, 24)), ("encode", (1, 3, 1, 8, 8))]


def net_case_id(case):
    return case[0] + "-" + "x".join(map(str, case[1][2:]))


@functools.lru_cache(maxsize=None)
def net96():
    torch.manual_seed(4)
    ref = V.WanVAENet(dim=96, z_dim=16).eval()
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(p.to(BF16).float())
    return ref


@functools.lru_cache(maxsize=None)
def net_setup(case):
    """(input, the fp32 network's output) of one tile-network case."""
    what, shape = case
    net = net96()
    _seed("net" + net_case_id(case))
    x = (torch.randn(shape) if what == "decode" else torch.rand(shape) * 2 - 1).to(BF16)
    with torch.no_grad():
        ref = net.decode(x.float()) if what == "decode" else net.encode(x.float())
    return x, ref


def run_net_case(make_exec, device, case):
    """decode_tile / encode_tile of WanVAENet(dim=96, z_dim=16): EVERY kernel call passes check_record (each layer of the shipped
    configuration on the activations the network really produces); outer cap: the network bar against fp32."""
    x, ref = net_setup(case)
    hip = make_exec(copy.deepcopy(net96()).to(device=device, dtype=BF16), device)
    with torch.no_grad():
        got = (hip.decode_tile if case[0] == "decode" else hip.encode_tile)(x.to(device)).float().cpu()
    worst = check_records(hip.records)
    _require(got.shape == ref.shape, "net.shape", f"{got.shape} != {ref.shape}")
    _require(bool(torch.isfinite(got).all()), "net.finite", "non-finite output")
    figs = dict(calls=len(hip.records), worst_call=worst, rel=_rel(got, ref), cos=float(F.cosine_similarity(got.flatten().double(), ref.flatten().double(), dim=0)))
    _require(figs["rel"] <= 2e-2 and figs["cos"] >= 0.999, "net.bar", f"rel-L2 {figs['rel']:.3g}, cosine {figs['cos']:.6f}")
    return figs


# ---- mutants: named wrong executors ------------------------------------------------------------------------------------------------

def _edited(fn, old, new):
    """``fn`` recompiled with one piece of its source replaced (in its own module's namespace)."""
    src = textwrap.dedent(inspect.getsource(fn))
    assert src.count(old) == 1, f"{fn.__qualname__}: the mutation site {old!r} is gone - update MUTANTS"
    ns = {}
    exec(compile(src.replace(old, new), inspect.getsourcefile(fn), "exec"), fn.__globals__, ns)
    return ns[fn.__name__]


def _conv_w_with(edit):
    def make(orig):
        def _conv_w(self, mod, taps):
            rec = copy.copy(orig(self, mod, taps))
            rec.w = rec.w.clone()
            edit(rec, len(taps))
            return rec
        return _conv_w
    return make


def _drop_last_tap(rec, ntaps):
    rec.w[:, (ntaps - 1) * rec.cin: ntaps * rec.cin] = 0


def _swap_halves(rec, ntaps):
    if rec.cin >= 64:
        w = rec.w[:, : ntaps * rec.cin].view(rec.cout, ntaps, rec.cin)
        w[:, :, :64] = torch.cat((w[:, :, 32:64], w[:, :, :32]), dim=2)


def _conv_no_resid(orig):
    return lambda self, x, mod, taps, resid=None, first_frame=0: orig(self, x, mod, taps, None, first_frame)


def _conv_frame_before(orig):
    def conv(self, x, mod, taps, resid=None, first_frame=0):
        out = orig(self, x, mod, taps, resid, first_frame)
        out.vol()[PT + first_frame - 1] = out.vol()[PT + first_frame]
        return out
    return conv


def _norm_halo_copied(orig):
    def norm_act(self, x, norm, act):
        out = orig(self, x, norm, act)
        keep = out.interior().clone()
        out.vol()[PT:] = x.vol()[PT:]
        out.interior().copy_(keep)
        return out
    return norm_act


def _norm_no_silu(orig):
    return lambda self, x, norm, act: orig(self, x, norm, 0)


# name -> (owner, attribute, replacement(original))
MUTANTS = {
    "zero_halo does nothing": (VH.Vol, "zero_halo", lambda orig: lambda self: self),
    "upsample swaps the two interleaved frames": (HostVaeHip, "upsample", lambda orig: _edited(orig, "ui[1 + s::2, a::2, b::2]", "ui[2 - s::2, a::2, b::2]")),
    "downsample takes the odd positions": (HostVaeHip, "downsample", lambda orig: _edited(orig, "full.interior()[:, 0::2, 0::2]", "full.interior()[:, 1::2, 1::2]")),
    "conv drops the last tap": (HostVaeHip, "_conv_w", _conv_w_with(_drop_last_tap)),
    "conv ignores resid": (HostVaeHip, "conv", _conv_no_resid),
    "conv swaps the first two 32-channel halves of every tap": (HostVaeHip, "_conv_w", _conv_w_with(_swap_halves)),
    "conv writes frame first_frame - 1": (HostVaeHip, "conv", _conv_frame_before),
    "norm_act copies the input onto the halo": (HostVaeHip, "norm_act", _norm_halo_copied),
    "norm_act skips SiLU": (HostVaeHip, "norm_act", _norm_no_silu),
}


@contextlib.contextmanager
def mutant(name):
    owner, attr, make = MUTANTS[name]
    with mock.patch.object(owner, attr, make(getattr(owner, attr))):
        _ACTIVE_MUTANTS.append(name)
        try:
            yield
        finally:
            _ACTIVE_MUTANTS.pop()
