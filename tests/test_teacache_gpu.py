"""TeaCache step skipping on the HIP path: the two kernels (icv_sub_rows_f32, icv_rel_l1_steps_f32), a forced-schedule CFG loop
against the torch restatement of upstream's loop, tea_cache=None unchanged, every driver mode against the sequential TeaCache
loop, and the pipeline end to end (one process, and two ranks sharing the GPU behind a worker pool)."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

from infinicube_amd.videogen import synthetic as syn
from infinicube_amd.videogen import teacache
from infinicube_amd.videogen.dit import WanDiT
from infinicube_amd.videogen.scheduler import FlowMatchScheduler
from oracle import wan_ref as R
from test_teacache_cpu import CFG, FORCED_COMPUTED, FORCED_THRESH, GRID, LINEAR, _tea_cache_reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))


def test_sub_rows_bit_exact_on_strided_views(hip_ops):
    torch.manual_seed(0)
    for rows, d, ldx, ldr in ((301, 512, 773, 600), (4096, 5120, 5120, 5120 + 64)):      # the second one takes the grid-stride loop
        xb = torch.randn(rows, ldx, device=DEV)
        rb = torch.randn(rows, ldr, device=DEV)
        x, r = xb[:, ldx - d:], rb[:, 16:16 + d] if ldr >= d + 16 else rb[:, :d]
        want, before = x - r, rb.clone()
        hip_ops.sub_rows(x, r)
        torch.cuda.synchronize()
        assert torch.equal(r, want)
        mask = torch.ones_like(rb, dtype=torch.bool)
        mask[:, r.storage_offset() - rb.storage_offset(): r.storage_offset() - rb.storage_offset() + d] = False
        assert torch.equal(rb[mask], before[mask]), "columns outside the view were written"
    with pytest.raises(ValueError):
        hip_ops.sub_rows(x, r[:, :-1])


def test_rel_l1_steps_against_float64_and_deterministic(hip_ops):
    torch.manual_seed(1)
    n, cols = 50, 6 * 5120
    steps = torch.randn(n, cols, device=DEV) * torch.linspace(0.01, 0.5, n, device=DEV)[:, None]
    big = torch.zeros(n, cols + 256, device=DEV)
    big[:, :cols] = torch.randn(1, cols, device=DEV) + steps.cumsum(0)
    table = big[:, :cols]                                                  # row stride != cols
    t = table.double()
    want = torch.cat([torch.zeros(1, dtype=torch.float64, device=DEV),
                      (t[1:] - t[:-1]).abs().mean(1) / t[:-1].abs().mean(1)])
    outs = []
    for _ in range(2):
        out = torch.full((n,), float("nan"), device=DEV)
        hip_ops.rel_l1_steps(table, out)
        torch.cuda.synchronize()
        outs.append(out)
    assert outs[0][0] == 0.0
    rel = ((outs[0].double()[1:] - want[1:]).abs() / want[1:]).max()
    assert float(rel) <= 1e-6, f"relative error {float(rel)}"
    assert torch.equal(outs[0], outs[1]), "two runs differ"


def _setup():
    sd, bsd = syn.make_dit_state_dict(CFG), syn.make_buffer_embedder_state_dict(CFG)
    return sd, bsd, syn.make_latent_noise(GRID), syn.make_text_context(CFG, 1), syn.make_text_context(CFG, 2), syn.make_buffer_latents(CFG, GRID)


def test_forced_schedule_loop_matches_restatement(hip_ops, monkeypatch):
    """A 10-step CFG loop whose schedule is forced by the test-only coefficients: the restatement of upstream's loop decides the
    same steps, the latents agree to the bar of test_denoise_loop_psnr, and blocks run on the computed steps only."""
    sd, bsd, noise, c1, c2, bl = _setup()
    m = WanDiT(CFG, sd, hip_ops, bsd).prepare(GRID)
    ck, cu, bt = m.encode_context(c1), m.encode_context(c2), m.embed_buffers(bl)
    sch = FlowMatchScheduler(10)
    plan = teacache.plan(m, sch, FORCED_THRESH, "test-linear", coeffs=LINEAR)
    assert plan.computed == FORCED_COMPUTED
    n_ffn = [0]
    raw = hip_ops.gemm

    def counting(a, w, bias, out, epilogue, **kw):
        n_ffn[0] += int(epilogue == 1 and w.shape[0] == CFG.ffn_dim)
        raw(a, w, bias, out, epilogue, **kw)

    monkeypatch.setattr(hip_ops, "gemm", counting)
    lat = noise.clone().to(DEV)
    m.denoise(lat, ck, cu, bt, sch, 5.0, tea_cache=plan)
    torch.cuda.synchronize()
    monkeypatch.setattr(hip_ops, "gemm", raw)
    assert m._pair is not None and n_ffn[0] == len(FORCED_COMPUTED) * CFG.num_layers, n_ffn[0]   # the pair: one FFN1 per layer
    ref, ref_computed = _tea_cache_reference(R.round_state_dict_to_bf16(sd), R.round_state_dict_to_bf16(bsd), CFG, noise, c1, c2, bl,
                                             10, FORCED_THRESH, LINEAR)
    assert ref_computed == plan.computed
    p = R.psnr(lat.cpu(), ref)
    assert p >= 40.0, f"TeaCache loop vs restatement: {p:.1f} dB"


def test_tea_cache_none_is_the_unchanged_loop(hip_ops):
    sd, bsd, noise, c1, c2, bl = _setup()
    lats = []
    for kw in ({}, dict(tea_cache=None), "all"):
        m = WanDiT(CFG, sd, hip_ops, bsd).prepare(GRID)
        ck, cu, bt = m.encode_context(c1), m.encode_context(c2), m.embed_buffers(bl)
        sch = FlowMatchScheduler(6)
        if kw == "all":                      # threshold 0: every step computed, the residual stores must not change anything
            kw = dict(tea_cache=teacache.plan(m, sch, 0.0, "test-linear", coeffs=LINEAR))
            assert kw["tea_cache"].computed == tuple(range(6))
        lat = noise.clone().to(DEV)
        m.denoise(lat, ck, cu, bt, sch, 5.0, **kw)
        torch.cuda.synchronize()
        if kw.get("tea_cache") is None:
            assert m._tc_res is None, "tea_cache=None must allocate nothing"
        lats.append(lat.cpu())
    assert torch.equal(lats[0], lats[1]) and torch.equal(lats[0], lats[2])


def _tc_loop(hip_ops, sd, bsd, noise, c1, c2, bl, prep=None, setup=None, kw=None):
    m = WanDiT(CFG, sd, hip_ops, bsd, **(kw or {})).prepare(GRID, **(prep or dict(graphs=False)))
    if setup is not None:
        setup(m)
    ck, cu, bt = m.encode_context(c1), m.encode_context(c2), m.embed_buffers(bl)
    sch = FlowMatchScheduler(10)
    plan = teacache.plan(m, sch, FORCED_THRESH, "test-linear", coeffs=LINEAR)
    assert plan.computed == FORCED_COMPUTED
    lat = noise.clone().to(DEV)
    m.denoise(lat, ck, cu, bt, sch, 5.0, tea_cache=plan)
    m.denoise(lat, ck, cu, bt, sch, 5.0, tea_cache=plan)       # a second call: graph replays, a residual left by the first call
    torch.cuda.synchronize()
    if getattr(m, "kv_gather", None) is not None:
        m.check_exchange()
        m.kv_gather.close()
    return m, lat.cpu()


def _sequential(m):
    m.cfg_batch = False


FP8 = dict(gemm_dtype="fp8", attn_dtype="fp8", fp8_weights=WanDiT.FP8_WEIGHTS)


@pytest.mark.parametrize("mode", ["pair", "pair-no-stem", "native", "graphs", "native+graphs", "dual-stream", "fp8-pair", "fp8-native",
                                  "sp-allgather", "sp-allgather-3chunks", "sp-ipc+arrival", "sp-native"])
def test_driver_modes_match_sequential_loop(hip_ops, mode, monkeypatch):
    """Every driver mode honours the schedule: bit-identical to the sequential TeaCache loop where the existing tests demand it
    between those modes (pair, native, graphs, dual stream), to their tolerance for the one-rank sequence-parallel rehearsals."""
    sd, bsd, noise, c1, c2, bl = _setup()
    kw = FP8 if mode.startswith("fp8") else None
    _, ref = _tc_loop(hip_ops, sd, bsd, noise, c1, c2, bl, setup=_sequential, kw=kw)
    prep, setup = dict(graphs=False), None
    if mode == "pair-no-stem":
        setup = lambda m: setattr(m, "share_stem", False)                        # noqa: E731
    elif mode in ("native", "fp8-native"):
        setup = lambda m: setattr(m, "native_forward", True)                     # noqa: E731
    elif mode == "graphs":
        prep = dict(graphs=True)
    elif mode == "native+graphs":
        prep, setup = dict(graphs=True), (lambda m: setattr(m, "native_forward", True))
    elif mode == "dual-stream":
        monkeypatch.setenv("ICV_DUAL_STREAM", "1")
    elif mode.startswith("sp-"):
        kv = mode[3:].replace("-3chunks", "")
        prep = dict(graphs=False, force_sp=True, kv_exchange=kv, sp_chunks=3 if mode.endswith("3chunks") else 1)
        if kv == "native":
            setup = lambda m: setattr(m, "native_forward", True)                 # noqa: E731
    m, got = _tc_loop(hip_ops, sd, bsd, noise, c1, c2, bl, prep=prep, setup=setup, kw=kw)
    assert torch.isfinite(got).all()
    if mode in ("pair", "pair-no-stem", "fp8-pair"):
        assert m._pair is not None
    if "native" in mode:
        assert m._native is not None
    if "graphs" in mode:
        assert m._graphs_on and any(k[4] == 0 for k in m._graphs), "the skipped steps must replay their own graph"
    if mode == "dual-stream":
        assert m.dual_stream and m._twin is not None
    if mode.startswith("sp-"):
        assert m.sp_on
        rel = float((got - ref).norm() / ref.norm())
        assert rel < 2e-3, f"{mode}: rel-L2 {rel} vs the sequential TeaCache loop"
    else:
        assert torch.equal(got, ref), f"{mode}: max |d| {float((got - ref).abs().max())}"


def _pipe():
    from infinicube_amd.videogen.ops import HipOps
    from infinicube_amd.videogen.pipeline import DiTHolder, WanVideoPipeline
    from standins import HashTextEncoder, PoolVAE
    return WanVideoPipeline(DEV, torch.bfloat16, DiTHolder(syn.make_dit_state_dict(CFG), CFG), HashTextEncoder(CFG), PoolVAE(),
                            ops=HipOps(DEV))


def test_pipeline_end_to_end(monkeypatch):
    for k in ("ICV_TEACACHE_L1_THRESH", "ICV_TEACACHE_MODEL_ID"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setitem(teacache.COEFFICIENTS, "test-linear", LINEAR)
    p = _pipe()
    kw = dict(prompt="a street", negative_prompt="bad", height=GRID.height, width=GRID.width, num_frames=GRID.num_frames, seed=3,
              num_inference_steps=6, return_latents=True)
    base = p(**kw).cpu()
    same = p(**kw, tea_cache_l1_thresh=0.0, tea_cache_model_id="test-linear").cpu()      # threshold 0, positive polynomial: every step
    assert p.tea_cache_record["computed"] == list(range(6)) and torch.equal(same, base)
    # the real 1.3B polynomial is negative at these random-init distances: only the forced ends are computed
    cached = p(**kw, tea_cache_l1_thresh=0.1, tea_cache_model_id="Wan2.1-T2V-1.3B").cpu()
    rec = p.tea_cache_record
    assert rec["computed"] == [0, 5] and rec["model_id"] == "Wan2.1-T2V-1.3B" and len(rec["distances"]) == 6
    assert torch.isfinite(cached).all() and not torch.equal(cached, base)
    with pytest.raises(ValueError, match="is not a supported TeaCache model id"):
        p(**kw, tea_cache_l1_thresh=0.1)


def tea_factory(torch_dtype, device, model_configs):
    """Worker-pool factory (ICV_WORKER_FACTORY="test_teacache_gpu:tea_factory"): the tiny pipeline on the shared cuda:0, 6 steps."""
    p = _pipe()
    p.num_inference_steps = 6
    return p


def test_worker_pool_two_ranks_sharing_the_gpu(tmp_path, monkeypatch):
    """The unchanged caller opts in through the environment; behind ICV_WORLD=2 (gloo, both ranks on cuda:0) the plan is built on
    rank 0 and broadcast (every rank reports it back), and the frames equal the single-process TeaCache frames to the rounding of the sharded attention."""
    import torch.distributed as dist
    from safetensors.torch import save_file
    from infinicube.videogen import WanVideoGenerator
    if dist.is_initialized():
        dist.destroy_process_group()
    path = str(tmp_path / "step-1.safetensors")
    save_file({"buffer_embedder." + k: v for k, v in syn.make_buffer_embedder_state_dict(CFG).items()}, path)
    sem, co = syn.make_dummy_buffers(GRID)
    import test_teacache_gpu as me

    def run():
        with contextlib.redirect_stdout(io.StringIO()):
            g = WanVideoGenerator(path, device=DEV, use_wan_1pt3b=True, pipeline_factory=me.tea_factory)
            frames = g.generate(sem, co, seed=3)
        return g, np.stack([np.asarray(f) for f in frames])

    monkeypatch.delenv("ICV_TEACACHE_L1_THRESH", raising=False)
    g0, _ = run()
    assert g0.pipe.tea_cache_record is None
    monkeypatch.setenv("ICV_TEACACHE_L1_THRESH", "0.1")
    monkeypatch.setenv("ICV_TEACACHE_MODEL_ID", "Wan2.1-T2V-1.3B")
    g1, ref = run()
    assert g1.pipe.tea_cache_record["computed"] == [0, 5], "the environment must switch TeaCache on"
    monkeypatch.delenv("GPU_MAX_HW_QUEUES", raising=False)
    monkeypatch.setenv("ICV_WORLD", "2")
    monkeypatch.setenv("ICV_DIST_BACKEND", "gloo")
    monkeypatch.setenv("ICV_WORKER_FACTORY", "test_teacache_gpu:tea_factory")
    monkeypatch.setenv("ICV_WORLD_TIMEOUT_S", "240")
    monkeypatch.setenv("PYTHONPATH", os.pathsep.join([os.path.dirname(HERE), HERE, os.environ.get("PYTHONPATH", "")]))
    g = None
    try:
        g, got = run()
        assert g._pool is not None and g._pool.world == 2
        assert g.pipe.tea_cache_record == g1.pipe.tea_cache_record, "the ranks must run rank 0's schedule"
        d = np.abs(ref.astype(np.int16) - got.astype(np.int16))
        assert d.max() <= 2 and (d > 0).mean() < 0.02, f"2-rank TeaCache frames differ: max {d.max()}, {100 * (d > 0).mean():.2f} % pixels"
    finally:
        if g is not None and g._pool is not None:
            g._pool.close()
    assert not dist.is_initialized()
