"""LoRA merge on the HIP path: icv_lora_merge_bf16 bit-exact on gridded data between guard bands, within half a bf16 ulp (+ f32
accumulation slack) on random data, its host-side contract; WanDiT.apply_lora / restore_lora against engines built from CPU-merged
and pristine state dicts with every weight pointer unchanged; pipe.load_lora in every driver mode, two adapters, clear, re-load at
another alpha, a DiT overlay, ICV_LORA behind the unchanged generator, the e4m3 scope; and one merge at the 14B shapes next to the
time of a copy of the same matrix (the 4 N K byte floor)."""
import contextlib
import io

import pytest
import torch

from infinicube_amd import native
from infinicube_amd.videogen import lora as L
from infinicube_amd.videogen import synthetic as syn
from infinicube_amd.videogen.config import TokenGrid
from infinicube_amd.videogen.dit import WanDiT
from standins import HashTextEncoder, PoolVAE
from test_lora_cpu import CFG, CFG_I2V, cpu_merge, gridded_adapter

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16 = torch.bfloat16
GUARD = 64                      # elements (128 bytes: keeps the 16-byte alignment of what follows)
SENTINEL = 768.0                # 3 * 2^8: exactly representable in bf16, far from every value a merge can produce here


def _guarded(rows_total, ld, r0, N, K):
    """A bf16 buffer of sentinels: guard band, a [rows_total, ld] matrix, guard band.  Returns (whole buffer, the [N, K] view at row
    r0, a mask over the buffer of the [N, K] elements)."""
    buf = torch.full((GUARD + rows_total * ld + GUARD,), SENTINEL, dtype=BF16, device=DEV)
    mat = buf[GUARD: GUARD + rows_total * ld].view(rows_total, ld)
    mask = torch.zeros_like(buf, dtype=torch.bool)
    mask[GUARD: GUARD + rows_total * ld].view(rows_total, ld)[r0: r0 + N, :K] = True
    return buf, mat[r0: r0 + N, :K], mask


def _only_view_written(buf, mask):
    assert bool((buf[~mask].float() == SENTINEL).all()), "guard band, rows outside the range or ldw padding columns were written"


# ---- kernel, exact -----------------------------------------------------------------------------------------------------------------
SHAPES = [(64, 64, 32, 64, 64, 0), (192, 320, 32, 320 + 64, 192 + 128, 64), (128, 256, 128, 256, 128, 0)]   # N, K, R, ldw, rows_total, r0


@pytest.mark.parametrize("N,K,R,ldw,rows_total,r0", SHAPES)
@pytest.mark.parametrize("alpha", [1.0, 0.5, -2.0, 0.0])
def test_merge_kernel_gridded_is_bit_exact(hip_ops, N, K, R, ldw, rows_total, r0, alpha):
    """W = integers in [-255, 255] / 256, factors = integers in [-4, 4] / 8: every product, the rank sum and the f32 addition are
    exact, so the result is bf16(W + alpha * up @ down) whatever the order of the sum.  alpha = 0 leaves W bit-identical."""
    g = torch.Generator().manual_seed(N + K + R)
    W = (torch.randint(-255, 256, (N, K), generator=g).float() / 256).to(BF16)
    up = (torch.randint(-4, 5, (N, R), generator=g).float() / 8).to(BF16)
    down = (torch.randint(-4, 5, (R, K), generator=g).float() / 8).to(BF16)
    buf, view, mask = _guarded(rows_total, ldw, r0, N, K)
    view.copy_(W.to(DEV))
    hip_ops.lora_merge(view, up.to(DEV), down.t().contiguous().to(DEV), alpha)
    torch.cuda.synchronize()
    want = (W.double() + alpha * (up.double() @ down.double())).to(BF16)
    got = view.cpu()
    changed = float((got.view(torch.int16) != W.view(torch.int16)).float().mean())
    print(f"gridded merge N={N} K={K} R={R} ldw={ldw} alpha={alpha}: {changed:.1%} of the elements changed")
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"{int((got != want).sum())} elements differ from bf16(exact)"
    _only_view_written(buf, mask)
    if alpha == 0.0:
        assert changed == 0.0
    else:
        assert changed > 0.9


# ---- kernel, random data -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [32, 128])
@pytest.mark.parametrize("alpha", [1.0, -0.7])
def test_merge_kernel_random_data_is_one_rounding(hip_ops, R, alpha):
    """sigma = 0.02 for W, 0.05 for the factors; x = the f64 result.  Every element within half a bf16 ulp of x plus f32 accumulation
    slack; at most 5e-4 of the elements differ from bf16(x) (a correct kernel differs only where f32 round-off of the sum moves x
    across a bf16 rounding boundary)."""
    N, K = 256, 512
    g = torch.Generator().manual_seed(7 * R)
    W = (torch.randn((N, K), generator=g) * 0.02).to(BF16)
    up = (torch.randn((N, R), generator=g) * 0.05).to(BF16)
    down = (torch.randn((R, K), generator=g) * 0.05).to(BF16)
    buf, view, mask = _guarded(N, K, 0, N, K)
    view.copy_(W.to(DEV))
    hip_ops.lora_merge(view, up.to(DEV), down.t().contiguous().to(DEV), alpha)
    torch.cuda.synchronize()
    x = W.double() + alpha * (up.double() @ down.double())
    got = view.cpu()
    bound = 2.0 ** -8 * x.abs() + 2.0 ** -16 * (W.double().abs() + abs(alpha) * (up.double().abs() @ down.double().abs()))
    err = (got.double() - x).abs()
    share = float((got.view(torch.int16) != x.to(BF16).view(torch.int16)).float().mean())
    print(f"random merge R={R} alpha={alpha}: worst err / bound {float((err / bound).max()):.3f}, share differing from bf16(x) {share:.2e}")
    assert bool((err <= bound).all())
    assert share <= 5e-4
    _only_view_written(buf, mask)


# ---- contract ------------------------------------------------------------------------------------------------------------------------
def test_merge_contract_is_checked_on_the_host(hip_ops):
    lib = hip_ops.lib
    buf = torch.full((4096 + 2 * GUARD + 64,), SENTINEL, dtype=BF16, device=DEV)
    ops = torch.ones((2, 64 * 600 + 64), dtype=BF16, device=DEV)
    w, u, d = buf.data_ptr() + 2 * GUARD, ops[0].data_ptr(), ops[1].data_ptr()
    assert w % 16 == 0 and u % 16 == 0 and d % 16 == 0
    good = dict(W=w, ldw=64, up=u, ldu=32, down=d, ldd=32, N=64, K=64, R=32)
    cases = [(dict(N=96), "multiples of 64"), (dict(K=32), "multiples of 64"), (dict(N=0), "multiples of 64"), (dict(R=16), "rank"),
             (dict(R=48, ldu=48, ldd=48), "rank"), (dict(R=544, ldu=544, ldd=544), "rank"), (dict(W=w + 8), "16-byte aligned"),
             (dict(up=u + 8), "16-byte aligned"), (dict(down=d + 2), "16-byte aligned"), (dict(ldw=68), "row strides"),
             (dict(ldu=36), "row strides"), (dict(ldd=36), "row strides"), (dict(ldw=56), "row strides"), (dict(ldu=24), "row strides"),
             (dict(W=None), "null argument")]
    for change, msg in cases:
        a = dict(good, **change)
        rc = lib.icv_lora_merge_bf16(a["W"], a["ldw"], a["up"], a["ldu"], a["down"], a["ldd"], a["N"], a["K"], a["R"], 1.0, None)
        assert rc != 0 and msg.encode() in lib.icv_last_error(), (change, lib.icv_last_error())
    torch.cuda.synchronize()
    assert bool((buf.float() == SENTINEL).all()), "a refused call wrote to W"
    with pytest.raises(native.NativeError, match="multiples of 64"):
        hip_ops.lora_merge(torch.zeros((32, 64), dtype=BF16, device=DEV), torch.zeros((32, 32), dtype=BF16, device=DEV),
                           torch.zeros((64, 32), dtype=BF16, device=DEV), 1.0)
    with pytest.raises(ValueError, match="up \\[N, R\\] and down_t \\[K, R\\]"):
        hip_ops.lora_merge(torch.zeros((64, 64), dtype=BF16, device=DEV), torch.zeros((64, 32), dtype=BF16, device=DEV),
                           torch.zeros((32, 64), dtype=BF16, device=DEV), 1.0)


# ---- engine --------------------------------------------------------------------------------------------------------------------------
def _matrices(engine):
    return {(i, name): lw[name] for i, lw in enumerate(engine.layers) for name in WanDiT.LAYER_MATRICES if name in lw}


def _assert_same_matrices(a, b, what):
    ma, mb = _matrices(a), _matrices(b)
    assert ma.keys() == mb.keys()
    for key in ma:
        assert torch.equal(ma[key].view(torch.int16), mb[key].view(torch.int16)), f"{what}: {key} differs in {int((ma[key] != mb[key]).sum())} elements"


@pytest.mark.parametrize("cfg", [CFG, CFG_I2V], ids=["t2v", "i2v"])
def test_engine_apply_and_restore(hip_ops, cfg):
    sd = syn.make_dit_state_dict(cfg)
    ad_sd = gridded_adapter(cfg, seed=1)
    adapter = L.load_adapter(ad_sd)
    e = WanDiT(cfg, sd, hip_ops)
    ptrs = {k: t.data_ptr() for k, t in _matrices(e).items()}
    assert e.lora_applied == [] and e.lora_touched == set()
    n = e.apply_lora(adapter, 0.5)
    torch.cuda.synchronize()
    kinds = 12 if cfg.has_image_input else 10
    assert n == kinds * cfg.num_layers and e.lora_applied == [(adapter.id, 0.5)]
    assert e.lora_touched == set((name, i) for i, name in _matrices(e))
    _assert_same_matrices(e, WanDiT(cfg, cpu_merge(sd, ad_sd, 0.5), hip_ops), "after apply_lora vs the CPU-merged state dict")
    fresh = WanDiT(cfg, sd, hip_ops)
    assert not torch.equal(e.layers[0]["wqkv"], fresh.layers[0]["wqkv"])
    # a second adapter on top: one rounding each, in order
    ad2_sd = gridded_adapter(cfg, seed=2, rank=32, spelling="kohya")
    e.apply_lora(L.load_adapter(ad2_sd), -0.25)
    torch.cuda.synchronize()
    _assert_same_matrices(e, WanDiT(cfg, cpu_merge(cpu_merge(sd, ad_sd, 0.5), ad2_sd, -0.25), hip_ops), "two adapters in order")
    e.restore_lora(sd)
    torch.cuda.synchronize()
    _assert_same_matrices(e, fresh, "after restore_lora vs a fresh engine")
    assert e.lora_applied == [] and e.lora_touched == set()
    assert {k: t.data_ptr() for k, t in _matrices(e).items()} == ptrs, "a weight tensor moved"
    for i, (lw, lf) in enumerate(zip(e.layers, fresh.layers)):      # nothing but the projections is ever touched
        assert all(torch.equal(lw[k], lf[k]) for k in lw if k not in WanDiT.LAYER_MATRICES)


def test_engine_refuses_quantised_projections(hip_ops):
    sd = syn.make_dit_state_dict(CFG)
    e = WanDiT(CFG, sd, hip_ops, gemm_dtype="fp8", attn_dtype="fp8")
    before = {k: t.clone() for k, t in _matrices(e).items() if not isinstance(t, tuple)}
    with pytest.raises(ValueError, match="first-version scope.*wqkv"):
        e.apply_lora(L.load_adapter(gridded_adapter(CFG, seed=1)), 0.5)
    torch.cuda.synchronize()
    assert e.lora_applied == [] and e.lora_touched == set()
    assert all(torch.equal(e.layers[i][name], t) for (i, name), t in before.items()), "a refused adapter must merge nothing"


# ---- pipeline ------------------------------------------------------------------------------------------------------------------------
GRID = TokenGrid(5, 64, 96)
A1, A2 = 0.0625, -0.125          # powers of two: alpha * delta stays exact for the gridded adapters


def _pipe(sd, cfg=CFG, dtype=torch.bfloat16):
    from infinicube_amd.videogen.ops import HipOps
    from infinicube_amd.videogen.pipeline import DiTHolder, WanVideoPipeline
    p = WanVideoPipeline(DEV, dtype, DiTHolder(sd, cfg), HashTextEncoder(cfg), PoolVAE(), ops=HipOps(DEV))
    p.num_inference_steps = 2
    return p


def _latents(p, **kw):
    lat = p(prompt="a street", negative_prompt="bad", height=GRID.height, width=GRID.width, num_frames=GRID.num_frames, seed=3,
            return_latents=True, **kw).cpu()
    assert torch.isfinite(lat).all()
    return lat


@pytest.fixture(scope="module")
def adapters():
    return gridded_adapter(CFG, seed=1), gridded_adapter(CFG, seed=2, rank=8, spelling="peft-default", prefix="diffusion_model.")


@pytest.fixture(scope="module")
def base_sd():
    return syn.make_dit_state_dict(CFG)


@pytest.fixture(autouse=True)
def _no_lora_env(monkeypatch):
    for k in ("ICV_LORA", "ICV_CFG_BATCH", "ICV_NATIVE_FORWARD", "ICV_GRAPHS", "ICV_WORLD", "ICV_FP8_WEIGHTS"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("mode", ["pair", "sequential", "native", "graphs"])
def test_load_lora_equals_cpu_merged_state_dict(mode, monkeypatch, adapters, base_sd):
    """Two denoising steps: pipe.load_lora gives the bits of a pipeline whose DiT state dict was merged on the CPU.  graphs: one
    forward per step (cfg_scale 1), so step 0 captures and step 1 replays - one capture, one replay."""
    kw = {}
    if mode == "sequential":
        monkeypatch.setenv("ICV_CFG_BATCH", "0")
    elif mode == "native":
        monkeypatch.setenv("ICV_NATIVE_FORWARD", "1")
    elif mode == "graphs":
        monkeypatch.setenv("ICV_GRAPHS", "1")
        kw = dict(cfg_scale=1.0)
    p = _pipe(base_sd)
    p.load_lora(p.dit, adapters[0], alpha=A1)
    got = _latents(p, **kw)
    eng = p._engine
    assert p.lora_record == [dict(path=None, alpha=A1, matrices=10 * CFG.num_layers, rank=4)]
    if mode == "pair":
        assert eng._pair is not None
    elif mode == "sequential":
        assert eng._pair is None and not eng._graphs_on and eng._native is None
    elif mode == "native":
        assert eng._native is not None
    else:
        assert eng._graphs_on and len(eng._graphs) == 1
    monkeypatch.delenv("ICV_GRAPHS", raising=False)      # the comparison runs eagerly: one capture and one replay in this test
    want = _latents(_pipe(cpu_merge(base_sd, adapters[0], A1)), **kw)
    plain = _latents(_pipe(base_sd), **kw)
    assert torch.equal(got, want), f"{mode}: max |d| {float((got - want).abs().max())}"
    assert not torch.equal(got, plain)


def test_two_adapters_clear_and_reload(adapters, base_sd):
    ad1, ad2 = adapters
    p = _pipe(base_sd)
    never = _latents(p)
    assert p.lora_record is None and p._engine.lora_applied == [] and p._engine.lora_touched == set()
    eng = p._engine
    ptr = eng.layers[1]["f0_w"].data_ptr()
    calls0 = native.N_CALLS[0]
    assert torch.equal(_latents(p), never)
    plain_calls = native.N_CALLS[0] - calls0
    # one adapter, then a second on top: the merged one is a prefix, only the new one is merged
    p.load_lora(p.dit, ad1, alpha=A1)
    one = _latents(p)
    applied = list(eng.lora_applied)
    p.load_lora(p.dit, ad2, alpha=A2)
    two = _latents(p)
    assert eng.lora_applied[:1] == applied and len(eng.lora_applied) == 2
    assert [r["rank"] for r in p.lora_record] == [4, 8] and [r["alpha"] for r in p.lora_record] == [A1, A2]
    merged2 = cpu_merge(cpu_merge(base_sd, ad1, A1), ad2, A2)
    assert torch.equal(two, _latents(_pipe(merged2))) and not torch.equal(two, one)
    # both loaded before the first call: the same bits
    q = _pipe(base_sd)
    q.load_lora(q.dit, ad1, alpha=A1)
    q.load_lora(q.dit, ad2, alpha=A2)
    assert torch.equal(_latents(q), two)
    # clear: the touched matrices are restored in place, and the loop is the plain one again (same bits, same number of C calls)
    p.clear_lora()
    assert torch.equal(_latents(p), never) and p.lora_record is None and eng.lora_applied == []
    calls0 = native.N_CALLS[0]
    assert torch.equal(_latents(p), never)
    assert native.N_CALLS[0] - calls0 == plain_calls
    # the same adapter at another alpha, with the old merge still in HBM: the restore path
    p.load_lora(p.dit, ad1, alpha=A1)
    assert torch.equal(_latents(p), one)
    p.clear_lora()
    p.load_lora(p.dit, ad1, alpha=A2)
    got = _latents(p)
    assert torch.equal(got, _latents(_pipe(cpu_merge(base_sd, ad1, A2)))) and not torch.equal(got, one)
    assert p._engine is eng and eng.layers[1]["f0_w"].data_ptr() == ptr, "no rebuild, no new weight tensors"
    # a DiT overlay bumps dit.version: the engine is rebuilt as before, the list is merged again
    overlay = {k: v * 0.5 for k, v in base_sd.items() if k.startswith("blocks.0.ffn.")}
    p.dit.load_state_dict(overlay, strict=False)
    got = _latents(p)
    assert p._engine is not eng and len(p._engine.lora_applied) == 1
    assert torch.equal(got, _latents(_pipe(cpu_merge(dict(base_sd, **overlay), ad1, A2))))


def test_e4m3_mode_scope(adapters, base_sd):
    """torch_dtype=float8_e4m3fn quantises wqkv (WanDiT.FP8_DEFAULT): an adapter on it raises, one on bf16 projections merges."""
    p = _pipe(base_sd, dtype=torch.float8_e4m3fn)
    p.load_lora(p.dit, adapters[0], alpha=A1)
    with pytest.raises(ValueError, match="first-version scope"):
        _latents(p)
    p.clear_lora()
    ffn = gridded_adapter(CFG, seed=3, kinds=("ffn.0", "ffn.2", "cross_attn.k", "self_attn.o"))
    p.load_lora(p.dit, ffn, alpha=A1)
    got = _latents(p)
    assert p._engine.fp8_set == ("wqkv",) and p.lora_record[0]["matrices"] == 4 * CFG.num_layers
    assert torch.equal(got, _latents(_pipe(cpu_merge(base_sd, ffn, A1), dtype=torch.float8_e4m3fn)))


class RecordingVAE(PoolVAE):
    def decode(self, latent, **kw):
        self.last_latent = latent.detach().float().cpu().clone()
        return super().decode(latent, **kw)


def lora_factory(torch_dtype, device, model_configs):
    from infinicube_amd.videogen.ops import HipOps
    from infinicube_amd.videogen.pipeline import DiTHolder, WanVideoPipeline
    p = WanVideoPipeline(device, torch_dtype, DiTHolder(syn.make_dit_state_dict(CFG), CFG), HashTextEncoder(CFG), RecordingVAE(), ops=HipOps(DEV))
    p.num_inference_steps = 2
    return p


def test_icv_lora_behind_the_unchanged_generator(tmp_path, monkeypatch, adapters):
    from safetensors.torch import save_file
    from infinicube.videogen import WanVideoGenerator
    ckpt, ad_path = str(tmp_path / "step-1.safetensors"), str(tmp_path / "city.safetensors")
    save_file({"buffer_embedder." + k: v for k, v in syn.make_buffer_embedder_state_dict(CFG).items()}, ckpt)
    save_file(adapters[0], ad_path)
    sem, co = syn.make_dummy_buffers(GRID)

    def run(env, load=None):
        if env is None:
            monkeypatch.delenv("ICV_LORA", raising=False)
        else:
            monkeypatch.setenv("ICV_LORA", env)
        with contextlib.redirect_stdout(io.StringIO()):
            g = WanVideoGenerator(ckpt, device=DEV, use_wan_1pt3b=True, pipeline_factory=lora_factory)
            if load is not None:
                g.pipe.load_lora(g.pipe.dit, *load)
            g.generate(sem, co, seed=3)
        return g, g.pipe.vae.last_latent

    g_env, lat_env = run(f"{ad_path}:{A2}")
    assert g_env.pipe.lora_record == [dict(path=ad_path, alpha=A2, matrices=10 * CFG.num_layers, rank=4)]
    g_call, lat_call = run(None, load=(ad_path, A2))
    g_none, lat_none = run(None)
    assert g_none.pipe.lora_record is None
    assert torch.isfinite(lat_env).all() and torch.equal(lat_env, lat_call) and not torch.equal(lat_env, lat_none)


# ---- one real shape ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(5120, 5120), (13824, 5120)])
def test_merge_at_the_14b_shapes(hip_ops, N, K):
    """R = 64 into the 14B model's attention and FFN1 matrices: a 256-row sample against the f64 result (the bound of the random-data
    test), and the time of one merge next to the time of a device copy of the same matrix - the same 4 N K bytes of HBM traffic,
    i.e. the floor at the rate this GPU delivers.  No threshold on the time (DESIGN.md §11 records it)."""
    R, alpha = 64, 0.8
    g = torch.Generator(device=DEV).manual_seed(N)
    W0 = (torch.randn((N, K), generator=g, device=DEV) * 0.02).to(BF16)
    up = (torch.randn((N, R), generator=g, device=DEV) * 0.05).to(BF16)
    down_t = (torch.randn((K, R), generator=g, device=DEV) * 0.05).to(BF16)
    W = W0.clone()
    hip_ops.lora_merge(W, up, down_t, alpha)
    rows = torch.randperm(N, generator=torch.Generator().manual_seed(1))[:256].to(DEV)
    x = W0[rows].double() + alpha * (up[rows].double() @ down_t.double().t())
    bound = 2.0 ** -8 * x.abs() + 2.0 ** -16 * (W0[rows].double().abs() + alpha * (up[rows].double().abs() @ down_t.double().abs().t()))
    err = (W[rows].double() - x).abs()
    share = float((W[rows].view(torch.int16) != x.to(BF16).view(torch.int16)).float().mean())
    assert bool((err <= bound).all()) and share <= 5e-4, f"worst err / bound {float((err / bound).max())}, share {share}"

    def timed(fn, reps=5):
        fn()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return sorted(ts)[len(ts) // 2]

    dst = torch.empty_like(W)
    t_merge = timed(lambda: hip_ops.lora_merge(W, up, down_t, alpha))
    t_copy = timed(lambda: dst.copy_(W0))
    gbs = 4.0 * N * K / (t_copy * 1e-3) / 1e9
    print(f"LoRA merge R={R} into [{N}, {K}]: {t_merge * 1e3:.0f} us per merge; floor = a copy of the matrix (4 N K bytes) "
          f"{t_copy * 1e3:.0f} us = {gbs:.0f} GB/s; merge / floor {t_merge / t_copy:.2f}, worst err / bound {float((err / bound).max()):.3f}, "
          f"share differing from bf16(f64) {share:.1e}")
