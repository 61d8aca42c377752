"""Launch trace of dit.WanDiT.denoise on the TEST-ONLY CPU operator set: which op is called, in which order, on which
rows of which buffer.  Shared by tests/test_dit_launch_trace.py (compares against the golden) and
tests/golden/make_dit_launch_trace.py (writes the golden).

Every public op of the operator set and every call into the K|V exchange appends ``[name, args, kwargs]`` to ONE list, so the
interleaving of exchange and compute is part of the trace.  A tensor is described as (buffer id, storage offset, shape,
stride, dtype); buffer id = order of first appearance of its storage in the log.  The tracer keeps every tensor it has seen
alive: a freed temporary would otherwise hand its address to a later buffer and the ids would differ from run to run."""
import hashlib
import json
from collections import Counter

import torch

from infinicube_amd.videogen import synthetic as syn
from infinicube_amd.videogen import teacache
from infinicube_amd.videogen.config import TokenGrid, preset
from infinicube_amd.videogen.dit import WanDiT
from infinicube_amd.videogen.scheduler import FlowMatchScheduler
from infinicube_amd.videogen.seqpar import KVGather, ShardPlan
from oracle_ops import OracleOps

GRID = TokenGrid(9, 64, 96)
FP8_KW = dict(gemm_dtype="fp8", attn_dtype="fp8", fp8_weights=WanDiT.FP8_WEIGHTS)
MODELS = {                       # name -> (preset, WanDiT keywords, force_sp)
    "tiny-bf16": ("tiny", {}, False),
    "tiny-i2v-bf16": ("tiny-i2v", {}, False),
    "tiny-fp8-sp3": ("tiny", FP8_KW, True),
    "tiny-bf16-sp3": ("tiny", {}, True),
}
NOT_LAUNCHES = ("alloc", "to_device")


class Trace:
    def __init__(self):
        self.log, self.on, self.depth = [], False, 0
        self._ids, self._keep = {}, []

    def describe(self, v):
        if isinstance(v, torch.Tensor):
            key = v.untyped_storage().data_ptr()
            if key not in self._ids:
                self._ids[key] = len(self._ids)
            self._keep.append(v)
            return ["T", self._ids[key], v.storage_offset(), list(v.shape), list(v.stride()), str(v.dtype)]
        if isinstance(v, (list, tuple)):
            return [self.describe(x) for x in v]
        if isinstance(v, dict):
            return {str(k): self.describe(x) for k, x in sorted(v.items())}
        if isinstance(v, float):
            return repr(v)
        if v is None or isinstance(v, (bool, int, str)):
            return v
        if isinstance(v, (torch.dtype, slice, range)):
            return str(v)
        if hasattr(v, "__dataclass_fields__"):       # ops.RopeTable
            return {k: self.describe(getattr(v, k)) for k in v.__dataclass_fields__}
        raise TypeError(f"launch trace: cannot describe an argument of type {type(v).__name__}")

    def wrap(self, name, fn):
        def call(*args, **kwargs):
            if self.on and self.depth == 0:         # ops an op calls internally are its business, not the driver's
                self.log.append([name, self.describe(args), self.describe(kwargs)])
            self.depth += 1
            try:
                return fn(*args, **kwargs)
            finally:
                self.depth -= 1
        return call

    def wrap_public(self, obj, prefix, names=None):
        for name in (names or [n for n in dir(obj) if not n.startswith("_") and n not in NOT_LAUNCHES]):
            fn = getattr(obj, name)
            if callable(fn):
                setattr(obj, name, self.wrap(prefix + name, fn))


class TracedOps(OracleOps):
    """OracleOps + CPU twins of the two TeaCache kernels, every public op logged."""

    def __init__(self, trace):
        super().__init__()
        trace.wrap_public(self, "")

    def sub_rows(self, x, r):
        r.copy_(x - r)

    def rel_l1_steps(self, table, out):
        t = table.double()
        out[0] = 0.0
        out[1:] = ((t[1:] - t[:-1]).abs().mean(1) / t[:-1].abs().mean(1)).float()


def cases():
    """name -> (model, cfg_batch, share_stem, tea_cache, branch): 4 models x {plain, TeaCache} x ({cfg_batch} x {share_stem}
    + the cfg+sp loop with only the cond / only the uncond context)."""
    out = {}
    for model in MODELS:
        for tea in (False, True):
            suffix = "/teacache" if tea else ""
            for batch in (False, True):
                for share in (False, True):
                    out[f"{model}/batch{int(batch)}-share{int(share)}{suffix}"] = (model, batch, share, tea, None)
            for branch in ("cond", "uncond"):
                out[f"{model}/branch-exchange-{branch}{suffix}"] = (model, True, True, tea, branch)
    return out


def run_case(model, batch, share, tea, branch):
    """-> (log of the two encode_context calls and the loop, final latent).  2 steps, CFG 5.0; TeaCache: 3 steps, the middle
    one skipped (teacache.plan forces the first and the last step of a loop to be computed)."""
    name, kw, force_sp = MODELS[model]
    cfg = preset(name)
    sd, bsd = syn.make_dit_state_dict(cfg), syn.make_buffer_embedder_state_dict(cfg)
    noise, c1, c2, bl = syn.make_latent_noise(GRID), syn.make_text_context(cfg, 1), syn.make_text_context(cfg, 2), syn.make_buffer_latents(cfg, GRID)
    clip = syn.make_clip_features(cfg) if cfg.has_image_input else None
    y = syn.make_cond_latents(cfg, GRID) if cfg.has_image_input else None
    tr = Trace()
    gather = None
    if force_sp:
        gather = KVGather(ShardPlan.make(GRID.S))
        tr.wrap_public(gather, "kv_gather.", ("start", "wait", "acquire", "allreduce_max"))
    m = WanDiT(cfg, sd, TracedOps(tr), bsd, **kw).prepare(GRID, force_sp=force_sp, sp_chunks=3, kv_gather=gather)
    assert m.sp_on == force_sp
    m.cfg_batch, m.share_stem = batch, share
    add = m.embed_buffers(bl)
    if y is not None:
        add = m.embed_cond_latents(y, add_to=add)
    tr.on = True
    cc, cu = m.encode_context(c1, clip), m.encode_context(c2, clip)
    lat = noise.clone()
    sch = FlowMatchScheduler(3 if tea else 2)
    plan = None
    if tea:
        plan = teacache.plan(m, sch, 1e9, "test-linear", coeffs=(1.0, 0.0))
        assert plan.computed == (0, 2)
    if branch is None:
        m.denoise(lat, cc, cu, add, sch, 5.0, tea_cache=plan)
        assert (m._pair is not None) == batch, "forward_pair must be the path taken exactly when cfg_batch is on"
    else:
        def exchange(own, both):               # stand-in for seqpar.BranchExchange: the peer's branch = a copy of this one
            both[0].copy_(own)
            both[1].copy_(own)
        m.denoise(lat, cc if branch == "cond" else None, cu if branch == "uncond" else None, add, sch, 5.0,
                  branch_exchange=exchange, tea_cache=plan)
    tr.on = False
    return tr.log, lat


def summarize(log, lat):
    blob = json.dumps(log, sort_keys=True, separators=(",", ":")).encode()
    return dict(ops=len(log), histogram=dict(sorted(Counter(e[0] for e in log).items())),
                log_sha256=hashlib.sha256(blob).hexdigest(),
                latent_sha256=hashlib.sha256(lat.contiguous().numpy().tobytes()).hexdigest())
