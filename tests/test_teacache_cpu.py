"""TeaCache step skipping (infinicube_amd/videogen/teacache.py) on CPU: the schedule against a line-by-line restatement of
upstream DiffSynth's ``TeaCache.check``, the pinned coefficient table and its error, where the settings come from, the host
loop (dit.WanDiT.denoise(tea_cache=)) on the TEST-ONLY oracle operator set against an independent torch restatement built
from oracle.wan_ref pieces, and a gloo world-2 sequence-parallel run against world 1."""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from infinicube_amd.videogen import multigpu, options, teacache
from infinicube_amd.videogen import synthetic as syn
from infinicube_amd.videogen.config import TokenGrid, preset
from infinicube_amd.videogen.dit import WanDiT
from infinicube_amd.videogen.pipeline import DiTHolder, WanVideoPipeline
from infinicube_amd.videogen.scheduler import FlowMatchScheduler
from infinicube_amd.videogen.seqpar import ShardPlan, gather_latent
from oracle import wan_ref as R
from oracle_ops import OracleOps

CFG, GRID = preset("tiny"), TokenGrid(9, 64, 96)
LINEAR = (1.0, 0.0)          # test-only coefficients: poly(r) = r, so a threshold picks known steps
# tiny preset, 10 steps: the t_mod distances are 0.25-0.32 per step, so a threshold of 0.6 computes steps 0, 3, 6 and 9
FORCED_THRESH, FORCED_COMPUTED = 0.6, (0, 3, 6, 9)


class TeaOps(OracleOps):
    """OracleOps + CPU twins of the two TeaCache kernels."""

    def sub_rows(self, x, r):
        r.copy_(x - r)

    def rel_l1_steps(self, table, out):
        t = table.double()
        out[0] = 0.0
        out[1:] = ((t[1:] - t[:-1]).abs().mean(1) / t[:-1].abs().mean(1)).float()


class DiffSynthTeaCache:
    """Upstream's TeaCache.check, restated line by line (the residual bookkeeping lives in the loop restatement below)."""

    def __init__(self, num_inference_steps, rel_l1_thresh, coefficients):
        self.num_inference_steps = num_inference_steps
        self.step = 0
        self.accumulated_rel_l1_distance = 0
        self.previous_modulated_input = None
        self.rel_l1_thresh = rel_l1_thresh
        self.coefficients = coefficients

    def check(self, t_mod):
        modulated_inp = t_mod.clone()
        if self.step == 0 or self.step == self.num_inference_steps - 1:
            should_calc = True
            self.accumulated_rel_l1_distance = 0
        else:
            rescale_func = np.poly1d(self.coefficients)
            self.accumulated_rel_l1_distance += rescale_func(((modulated_inp - self.previous_modulated_input).abs().mean()
                                                              / self.previous_modulated_input.abs().mean()).cpu().item())
            if self.accumulated_rel_l1_distance < self.rel_l1_thresh:
                should_calc = False
            else:
                should_calc = True
                self.accumulated_rel_l1_distance = 0
        self.previous_modulated_input = modulated_inp
        self.step += 1
        if self.step == self.num_inference_steps:
            self.step = 0
        return not should_calc


def _diffsynth_computed(t_mods, thresh, coeffs):
    tc = DiffSynthTeaCache(len(t_mods), thresh, coeffs)
    return tuple(i for i, t in enumerate(t_mods) if not tc.check(t))


def _distances(t_mods):
    out = torch.zeros(len(t_mods))
    TeaOps().rel_l1_steps(torch.stack([t.reshape(-1) for t in t_mods]).float(), out)
    return [float(v) for v in out]


def _hand_built(n, seed=0):
    """t_mod sequences with step-to-step changes of very different sizes."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(6, 32, generator=g, dtype=torch.float64)
    rows = [base]
    for i in range(1, n):
        rows.append(rows[-1] + torch.randn(6, 32, generator=g, dtype=torch.float64) * (0.01 + 0.2 * (i % 3)))
    return rows


@pytest.mark.parametrize("thresh", [0.0, 0.05, 0.3, 0.8, 1e9])
@pytest.mark.parametrize("coeffs", [LINEAR, teacache.COEFFICIENTS["Wan2.1-T2V-1.3B"], (2.0, -0.5, 0.1)])
def test_schedule_matches_diffsynth_check(thresh, coeffs):
    t_mods = _hand_built(12)
    got = teacache.schedule(_distances(t_mods), range(12), 12, thresh, coeffs)
    assert got == _diffsynth_computed(t_mods, thresh, coeffs)
    assert got[0] == 0 and got[-1] == 11                     # first and last step forced


def test_schedule_edges():
    d = [0.0] + [0.1] * 9
    assert teacache.schedule(d, range(10), 10, 0.0, LINEAR) == tuple(range(10))     # threshold 0: every step computed
    assert teacache.schedule(d, range(10), 10, 1e9, LINEAR) == (0, 9)                # huge threshold: only the ends
    # reset after a compute: 0.1 + 0.1 + 0.1 reaches 0.25 at step 3, then the sum starts again from step 4
    assert teacache.schedule(d, range(10), 10, 0.25, LINEAR) == (0, 3, 6, 9)
    # a partial range starts with a computed step (a residual must exist); the last step of the loop stays forced
    assert teacache.schedule(d[4:], range(4, 10), 10, 0.25, LINEAR) == (4, 7, 9)
    assert teacache.schedule(d[2:6], range(2, 6), 10, 1e9, LINEAR) == (2,)
    # restated on a full hand-built sequence, the range form equals upstream from the range's first step on
    t_mods = _hand_built(12, seed=3)
    full = _distances(t_mods)
    assert teacache.schedule(full[5:], range(5, 12), 12, 0.3, LINEAR) == tuple(i + 5 for i in _diffsynth_computed(t_mods[5:], 0.3, LINEAR))


def test_coefficient_table_pinned_and_unknown_id():
    assert teacache.COEFFICIENTS == {
        "Wan2.1-T2V-1.3B": (-5.21862437e+04, 9.23041404e+03, -5.28275948e+02, 1.36987616e+01, -4.99875664e-02),
        "Wan2.1-T2V-14B": (-3.03318725e+05, 4.90537029e+04, -2.65530556e+03, 5.87365115e+01, -3.15583525e-01),
        "Wan2.1-I2V-14B-480P": (2.57151496e+05, -3.54229917e+04, 1.40286849e+03, -1.35890334e+01, 1.32517977e-01),
        "Wan2.1-I2V-14B-720P": (8.10705460e+03, 2.13393892e+03, -3.72934672e+02, 1.66203073e+01, -4.17769401e-02),
    }
    ids = "Wan2.1-T2V-1.3B, Wan2.1-T2V-14B, Wan2.1-I2V-14B-480P, Wan2.1-I2V-14B-720P"
    for bad in ("", "Wan2.2-T2V-5B"):
        with pytest.raises(ValueError) as e:
            teacache.coefficients(bad)
        assert str(e.value) == f"{bad} is not a supported TeaCache model id. Please choose a valid model id in ({ids})."


def _pipe(ops=None):
    from standins import HashTextEncoder, PoolVAE
    return WanVideoPipeline("cpu", torch.bfloat16, DiTHolder(syn.make_dit_state_dict(CFG), CFG), HashTextEncoder(CFG), PoolVAE(),
                            ops=ops or TeaOps())


def _settings(p, thresh, model_id, cfg):
    """What WanVideoPipeline.__call__ does with its two keywords: keyword or attribute, then the feature's own rule."""
    opt = options.resolve(p, dict(tea_cache_l1_thresh=thresh, tea_cache_model_id=model_id or None))
    return teacache.settings(opt.tea_cache_l1_thresh, opt.tea_cache_model_id, cfg, from_keyword=thresh is not None)


def test_settings_precedence(monkeypatch):
    for k in options.ENV_NAMES:
        monkeypatch.delenv(k, raising=False)
    p = _pipe()
    assert (p.tea_cache_l1_thresh, p.tea_cache_model_id, p.tea_cache_record) == (None, "", None)
    assert _settings(p, None, "", CFG) == (None, "")                                   # off by default
    assert _settings(p, 0.2, "Wan2.1-T2V-14B", CFG) == (0.2, "Wan2.1-T2V-14B")
    with pytest.raises(ValueError, match=" is not a supported TeaCache model id"):             # a threshold with the default id
        _settings(p, 0.2, "", CFG)
    monkeypatch.setenv("ICV_TEACACHE_L1_THRESH", "0.3")
    monkeypatch.setenv("ICV_TEACACHE_MODEL_ID", "Wan2.1-I2V-14B-480P")
    p = _pipe()
    assert (p.tea_cache_l1_thresh, p.tea_cache_model_id) == (0.3, "Wan2.1-I2V-14B-480P")        # environment -> attributes
    assert _settings(p, None, "", CFG) == (0.3, "Wan2.1-I2V-14B-480P")
    assert _settings(p, 0.1, "Wan2.1-T2V-14B", CFG) == (0.1, "Wan2.1-T2V-14B")         # keywords win
    p.tea_cache_l1_thresh, p.tea_cache_model_id = 0.05, "Wan2.1-T2V-1.3B"                       # attributes set after construction
    assert _settings(p, None, "", CFG) == (0.05, "Wan2.1-T2V-1.3B")
    # a threshold from the environment without an id: a t2v DiT's id follows from its width; i2v needs one
    monkeypatch.delenv("ICV_TEACACHE_MODEL_ID")
    p = _pipe()
    assert _settings(p, None, "", dataclasses.replace(CFG, dim=1536)) == (0.3, "Wan2.1-T2V-1.3B")
    assert _settings(p, None, "", dataclasses.replace(CFG, dim=5120)) == (0.3, "Wan2.1-T2V-14B")
    with pytest.raises(ValueError, match="explicit model id"):
        _settings(p, None, "", preset("tiny-i2v"))
    with pytest.raises(ValueError, match="is not a supported TeaCache model id"):             # a keyword threshold never infers
        _settings(p, 0.3, "", dataclasses.replace(CFG, dim=1536))
    # the worker ranks behind ICV_WORLD=N get both attributes with every request
    assert {"tea_cache_l1_thresh", "tea_cache_model_id"} <= set(multigpu._PIPE_SETTINGS)


def test_pipeline_call_records_schedule(monkeypatch):
    """WanVideoPipeline.__call__(tea_cache_l1_thresh=, tea_cache_model_id=) plans, records and honours the schedule; a threshold
    of 0 computes every step and equals the loop without TeaCache bit for bit."""
    for k in ("ICV_TEACACHE_L1_THRESH", "ICV_TEACACHE_MODEL_ID"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setitem(teacache.COEFFICIENTS, "test-linear", LINEAR)
    p = _pipe()
    kw = dict(prompt="a street", negative_prompt="bad", height=GRID.height, width=GRID.width, num_frames=GRID.num_frames, seed=3,
              num_inference_steps=10, return_latents=True)
    base = p(**kw)
    assert p.tea_cache_record is None
    same = p(**kw, tea_cache_l1_thresh=0.0, tea_cache_model_id="test-linear")
    assert p.tea_cache_record["computed"] == list(range(10)) and torch.equal(same, base)
    cached = p(**kw, tea_cache_l1_thresh=FORCED_THRESH, tea_cache_model_id="test-linear")
    rec = p.tea_cache_record
    assert rec["model_id"] == "test-linear" and rec["thresh"] == FORCED_THRESH and len(rec["distances"]) == 10
    assert tuple(rec["computed"]) == FORCED_COMPUTED
    assert not torch.equal(cached, base) and R.psnr(cached, base) > 15.0
    with pytest.raises(ValueError, match="is not a supported TeaCache model id"):
        p(**kw, tea_cache_l1_thresh=0.1)


def _tea_cache_reference(sd, bsd, cfg, noise, c1, c2, bl, num_steps, thresh, coeffs, cfg_scale=5.0):
    """DiffSynth's TeaCache loop restated on oracle.wan_ref pieces: one cache per CFG branch; a computed step stores
    x_after_blocks - x_before_blocks, a skipped one adds it to the patch embedding and runs the head only."""
    sig = R.flow_match_sigmas(num_steps)
    buf = R.buffer_embed(bsd, bl)
    ctxs = (R.text_embed(sd, c1), R.text_embed(sd, c2))
    grid = (noise.shape[1], noise.shape[2] // 2, noise.shape[3] // 2)
    freqs = R.rope_freqs_3d(cfg.head_dim, *grid)
    caches = [DiffSynthTeaCache(num_steps, thresh, coeffs) for _ in range(2)]
    residual = [None, None]
    x, computed = noise.clone().float(), []
    for i in range(num_steps):
        t, t_mod = R.time_embed(sd, cfg, float(sig[i]) * 1000.0)
        vs, skips = [], []
        for b in range(2):
            skip = caches[b].check(t_mod)
            skips.append(skip)
            tok = R.patchify_tokens(x, sd["patch_embedding.weight"], sd["patch_embedding.bias"]) + buf
            if skip:
                tok = tok + residual[b]
            else:
                before = tok.clone()
                for layer in range(cfg.num_layers):
                    tok = R.dit_block(sd, cfg, layer, tok, ctxs[b], t_mod, freqs)
                residual[b] = tok - before
            vs.append(R.unpatchify(R.head(sd, cfg, tok, t), grid, cfg.out_dim))
        assert skips[0] == skips[1]                  # the branches see the same t_mod: one schedule
        if not skip:
            computed.append(i)
        v = vs[1] + cfg_scale * (vs[0] - vs[1])
        nxt = float(sig[i + 1]) if i + 1 < num_steps else 0.0
        x = x + v * (nxt - float(sig[i]))
    return x, tuple(computed)


def _inputs():
    sd, bsd = syn.make_dit_state_dict(CFG), syn.make_buffer_embedder_state_dict(CFG)
    return sd, bsd, syn.make_latent_noise(GRID), syn.make_text_context(CFG, 1), syn.make_text_context(CFG, 2), syn.make_buffer_latents(CFG, GRID)


class CountingOps(TeaOps):
    def __init__(self):
        super().__init__()
        self.ffn_gemms = 0

    def gemm(self, a, w, bias, out, epilogue, resid=None, gate=None, nsplit=None):
        self.ffn_gemms += int(epilogue == 1 and w.shape[0] == CFG.ffn_dim)      # FFN1 (GELU epilogue): once per block
        super().gemm(a, w, bias, out, epilogue, resid, gate, nsplit)


@pytest.mark.parametrize("cfg_batch", [True, False])
def test_host_loop_matches_restatement(cfg_batch):
    sd, bsd, noise, c1, c2, bl = _inputs()
    ops = CountingOps()
    m = WanDiT(CFG, sd, ops, bsd).prepare(GRID)
    m.cfg_batch = cfg_batch
    ck, cu, bt = m.encode_context(c1), m.encode_context(c2), m.embed_buffers(bl)
    sch = FlowMatchScheduler(10)
    plan = teacache.plan(m, sch, FORCED_THRESH, "test-linear", coeffs=LINEAR)
    assert plan.computed == FORCED_COMPUTED
    lat = noise.clone()
    ops.ffn_gemms = 0
    m.denoise(lat, ck, cu, bt, sch, 5.0, tea_cache=plan)
    # blocks ran on the computed steps only: one FFN1 GEMM per layer per forward (the pair runs both branches in one)
    assert ops.ffn_gemms == len(FORCED_COMPUTED) * CFG.num_layers * (1 if cfg_batch else 2)
    ref, ref_computed = _tea_cache_reference(R.round_state_dict_to_bf16(sd), R.round_state_dict_to_bf16(bsd), CFG, noise, c1, c2, bl,
                                             10, FORCED_THRESH, LINEAR)
    assert ref_computed == plan.computed
    p = R.psnr(lat, ref)
    assert p >= 40.0, f"TeaCache loop vs restatement: {p:.1f} dB"
    full = noise.clone()
    m.denoise(full, ck, cu, bt, sch, 5.0)
    assert R.psnr(lat, full) < p, "the skipped steps must actually change the result"


def _sp_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.set_num_threads(2)
        sd, bsd, noise, c1, c2, bl = _inputs()
        plan = ShardPlan.make(GRID.S, world, rank)
        m = WanDiT(CFG, sd, TeaOps(), bsd).prepare(GRID, plan, kv_exchange="allgather")
        sch = FlowMatchScheduler(6)
        tc = teacache.plan(m, sch, 0.45, "test-linear", coeffs=LINEAR)
        lat = noise.clone()
        m.denoise(lat, m.encode_context(c1), m.encode_context(c2), m.embed_buffers(bl), sch, 5.0, tea_cache=tc)
        q.put((rank, gather_latent(lat, plan, GRID), tc.computed))
    finally:
        dist.destroy_process_group()


def test_gloo_world2_sequence_parallel_equals_single():
    sd, bsd, noise, c1, c2, bl = _inputs()
    single = WanDiT(CFG, sd, TeaOps(), bsd).prepare(GRID)
    sch = FlowMatchScheduler(6)
    tc = teacache.plan(single, sch, 0.45, "test-linear", coeffs=LINEAR)
    assert 0 < len(tc.computed) < 6
    ref = noise.clone()
    single.denoise(ref, single.encode_context(c1), single.encode_context(c2), single.embed_buffers(bl), sch, 5.0, tea_cache=tc)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() + 977) % 2000
    procs = [ctx.Process(target=_sp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = {r: (lat, comp) for r, lat, comp in (q.get(timeout=300) for _ in range(2))}
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert got[0][1] == got[1][1] == tc.computed
    assert torch.equal(got[0][0], got[1][0])
    assert float((got[0][0] - ref).norm() / ref.norm()) < 2e-3 and R.psnr(got[0][0], ref) > 55.0


def _cfg_sp_worker(rank, world, port, q):
    from infinicube_amd.videogen.seqpar import BranchExchange, ParallelLayout
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.set_num_threads(2)
        sd, bsd, noise, c1, c2, bl = _inputs()
        lay = ParallelLayout.make(world, rank, "cfg+sp")
        m = WanDiT(CFG, sd, TeaOps(), bsd).prepare(GRID, lay.shard_plan(GRID.S), group=lay.sp_group, kv_exchange="allgather")
        sch = FlowMatchScheduler(6)
        tc = teacache.plan(m, sch, 0.45, "test-linear", coeffs=LINEAR)
        lat = noise.clone()
        m.denoise(lat, m.encode_context(c1) if lay.branch == 0 else None, m.encode_context(c2) if lay.branch == 1 else None,
                  m.embed_buffers(bl), sch, 5.0, branch_exchange=BranchExchange(lay), tea_cache=tc)
        q.put((rank, gather_latent(lat, lay.shard_plan(GRID.S), GRID, group=lay.sp_group), tc.computed))
    finally:
        dist.destroy_process_group()


def test_gloo_cfg_branch_parallel_equals_single():
    """cfg+sp, world 2 (one rank per CFG branch): each rank skips the same steps, and the velocity swap of a skipped step carries
    the head outputs of the residual-only forwards."""
    sd, bsd, noise, c1, c2, bl = _inputs()
    single = WanDiT(CFG, sd, TeaOps(), bsd).prepare(GRID)
    sch = FlowMatchScheduler(6)
    tc = teacache.plan(single, sch, 0.45, "test-linear", coeffs=LINEAR)
    ref = noise.clone()
    single.denoise(ref, single.encode_context(c1), single.encode_context(c2), single.embed_buffers(bl), sch, 5.0, tea_cache=tc)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() + 1311) % 2000
    procs = [ctx.Process(target=_cfg_sp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = {r: (lat, comp) for r, lat, comp in (q.get(timeout=300) for _ in range(2))}
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert got[0][1] == got[1][1] == tc.computed
    assert torch.equal(got[0][0], got[1][0])
    assert float((got[0][0] - ref).norm() / ref.norm()) < 1e-5       # no sharding: the per-token math of the single process
