"""LoRA adapters, host side (infinicube_amd/videogen/lora.py; no GPU): every accepted key spelling and prefix gives one plan, the
q / k / v and cross-attention k / v row ranges, zero rank padding, the .alpha scale, every ValueError, ICV_LORA parsing, the
pipeline's load_lora argument checks before an engine exists, and a safetensors round trip.  Also the fixtures the GPU tests
share: the gridded adapter and the CPU merge of an adapter into a DiT state dict."""
import pytest
import torch

from infinicube_amd.videogen import lora as L
from infinicube_amd.videogen import synthetic as syn
from infinicube_amd.videogen.config import preset

CFG, CFG_I2V = preset("tiny"), preset("tiny-i2v")
KINDS = ("self_attn.q", "self_attn.k", "self_attn.v", "self_attn.o", "cross_attn.q", "cross_attn.k", "cross_attn.v",
         "cross_attn.o", "ffn.0", "ffn.2")
IMG_KINDS = ("cross_attn.k_img", "cross_attn.v_img")
SPELLINGS = {"peft": (".lora_A.weight", ".lora_B.weight"), "peft-default": (".lora_A.default.weight", ".lora_B.default.weight"),
             "kohya": (".lora_down.weight", ".lora_up.weight")}


def _nk(cfg, kind):
    d, f = cfg.dim, cfg.ffn_dim
    return {"ffn.0": (f, d), "ffn.2": (d, f)}.get(kind, (d, d))


def gridded_adapter(cfg, seed=0, rank=4, spelling="peft", prefix="", kinds=None, layers=None):
    """Adapter state dict touching every target kind of every layer; all factors are integers in [-4, 4] / 8, so every product
    and every rank sum is exact in f32 (and in bf16 operands)."""
    g = torch.Generator().manual_seed(1000 + seed)
    kinds = kinds if kinds is not None else KINDS + (IMG_KINDS if cfg.has_image_input else ())
    a, b = SPELLINGS[spelling]
    sd = {}
    for i in (range(cfg.num_layers) if layers is None else layers):
        for kind in kinds:
            N, K = _nk(cfg, kind)
            sd[f"{prefix}blocks.{i}.{kind}{a}"] = torch.randint(-4, 5, (rank, K), generator=g).float() / 8
            sd[f"{prefix}blocks.{i}.{kind}{b}"] = torch.randint(-4, 5, (N, rank), generator=g).float() / 8
    return sd


def cpu_merge(sd, adapter_sd, alpha):
    """A copy of the DiT state dict ``sd`` with the adapter merged the way the engine states it: operands rounded to bf16,
    delta = B A (exact here: gridded factors), then f32(W + alpha * delta) - one f32 fused multiply-add, computed exactly in f64
    and rounded to f32 - and ONE rounding to bf16.  For the gridded adapter alpha * delta is exact, so this is the correctly
    rounded f32 sum followed by the store rounding, with no dependence on how the rank sum is ordered."""
    ad = L.load_adapter(adapter_sd)
    out = dict(sd)
    for target, (down, up, alpha_key) in ad.pairs.items():
        key = target + ".weight"
        scale = 1.0 if alpha_key is None else alpha_key / down.shape[0]
        w = out[key].to(torch.bfloat16).double()
        delta = up.to(torch.bfloat16).double() @ down.to(torch.bfloat16).double()
        out[key] = (w + float(alpha) * scale * delta).float().to(torch.bfloat16)
    return out


def _same_plan(p, q):
    assert [(e.name, e.layer, e.rows, e.scale) for e in p] == [(e.name, e.layer, e.rows, e.scale) for e in q]
    for e, f in zip(p, q):
        assert torch.equal(e.up, f.up) and torch.equal(e.down_t, f.down_t)


# ---- accepted spellings ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spelling", list(SPELLINGS))
@pytest.mark.parametrize("prefix", ["", "diffusion_model.", "pipe.dit.", "dit."])
def test_every_spelling_and_prefix_gives_the_same_plan(spelling, prefix):
    want = L.load_adapter(gridded_adapter(CFG)).plan(CFG)
    got = L.load_adapter(gridded_adapter(CFG, spelling=spelling, prefix=prefix)).plan(CFG)
    assert len(want) == CFG.num_layers * len(KINDS)
    _same_plan(got, want)


def test_row_ranges_and_shapes():
    d, f = CFG_I2V.dim, CFG_I2V.ffn_dim
    sd = gridded_adapter(CFG_I2V, layers=[1])
    by = {(e.name, e.rows): e for e in L.load_adapter(sd).plan(CFG_I2V)}
    assert len(by) == 12 and all(e.layer == 1 for e in by.values())
    want = {"self_attn.q": ("wqkv", (0, d)), "self_attn.k": ("wqkv", (d, 2 * d)), "self_attn.v": ("wqkv", (2 * d, 3 * d)),
            "self_attn.o": ("wo", (0, d)), "cross_attn.q": ("xq_w", (0, d)), "cross_attn.k": ("xkv_w", (0, d)),
            "cross_attn.v": ("xkv_w", (d, 2 * d)), "cross_attn.o": ("xo_w", (0, d)), "cross_attn.k_img": ("xkv_img_w", (0, d)),
            "cross_attn.v_img": ("xkv_img_w", (d, 2 * d)), "ffn.0": ("f0_w", (0, f)), "ffn.2": ("f2_w", (0, d))}
    for kind, where in want.items():
        e = by[where]
        N, K = _nk(CFG_I2V, kind)
        assert tuple(e.up.shape) == (N, 32) and tuple(e.down_t.shape) == (K, 32) and e.rows[1] - e.rows[0] == N
        # the factors of THIS target, transposed where the kernel wants it
        assert torch.equal(e.up[:, :4], sd[f"blocks.1.{kind}.lora_B.weight"])
        assert torch.equal(e.down_t[:, :4], sd[f"blocks.1.{kind}.lora_A.weight"].t())


@pytest.mark.parametrize("rank,padded", [(4, 32), (32, 32), (33, 64), (96, 96)])
def test_rank_padding_is_zeros(rank, padded):
    sd = gridded_adapter(CFG, rank=rank, kinds=("self_attn.q", "ffn.0"), layers=[0])
    ad = L.load_adapter(sd)
    assert ad.rank == rank
    for e in ad.plan(CFG):
        assert e.up.shape[1] == e.down_t.shape[1] == padded and e.scale == 1.0
        assert not e.up[:, rank:].any() and not e.down_t[:, rank:].any()
        assert e.up[:, :rank].any() and e.down_t[:, :rank].any()


def test_alpha_key_scales_the_pair_by_alpha_over_rank():
    sd = gridded_adapter(CFG, rank=4, spelling="kohya", kinds=("self_attn.q", "self_attn.o"), layers=[0])
    sd["blocks.0.self_attn.q.alpha"] = torch.tensor(2.0)
    by = {e.name: e for e in L.load_adapter(sd).plan(CFG)}
    assert by["wqkv"].scale == 0.5 and by["wo"].scale == 1.0


# ---- errors: nothing is skipped silently -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["patch_embedding.lora_A.weight", "head.head.lora_A.weight", "blocks.0.norm3.lora_A.weight",
                                 "blocks.0.modulation", "blocks.0.self_attn.q.diff", "blocks.0.self_attn.q.diff_b",
                                 "blocks.0.self_attn.norm_q.lora_A.weight", "text_embedding.0.lora_B.weight", "blocks.0.ffn.1.lora_A.weight",
                                 "model.blocks.0.self_attn.q.lora_A.weight", "blocks.0.self_attn.q.weight"])
def test_other_keys_raise(key):
    sd = gridded_adapter(CFG, layers=[0])
    sd[key] = torch.zeros(4, CFG.dim)
    with pytest.raises(ValueError, match="not lora_A / lora_B") as e:
        L.load_adapter(sd)
    assert key in str(e.value)


def test_each_structural_error_raises():
    base = gridded_adapter(CFG, layers=[0])
    sd = dict(base)
    del sd["blocks.0.ffn.0.lora_B.weight"]
    with pytest.raises(ValueError, match="half of a lora_A / lora_B pair is missing.*blocks.0.ffn.0.lora_A.weight"):
        L.load_adapter(sd)
    sd = dict(base, **{"blocks.0.ffn.2.alpha": torch.tensor(1.0)})
    del sd["blocks.0.ffn.2.lora_A.weight"], sd["blocks.0.ffn.2.lora_B.weight"]
    with pytest.raises(ValueError, match="pair is missing"):
        L.load_adapter(sd)
    sd = dict(base, **{"blocks.0.self_attn.k.lora_B.weight": torch.zeros(CFG.dim, 8)})
    with pytest.raises(ValueError, match="rank mismatch.*self_attn.k"):
        L.load_adapter(sd)
    sd = dict(base, **{"blocks.0.self_attn.v.lora_A.weight": torch.zeros(4, CFG.dim + 64)})
    with pytest.raises(ValueError, match="shapes do not fit the model.*self_attn.v"):
        L.load_adapter(sd).plan(CFG)
    sd = dict(base, **{"blocks.0.ffn.0.lora_B.weight": torch.zeros(CFG.dim, 4)})      # ffn.0 is [ffn_dim, dim]
    with pytest.raises(ValueError, match="shapes do not fit"):
        L.load_adapter(sd).plan(CFG)
    with pytest.raises(ValueError, match="beyond the model's 2 layers.*blocks.2"):
        L.load_adapter(gridded_adapter(CFG, layers=[0, 2])).plan(CFG)
    with pytest.raises(ValueError, match="k_img / v_img targets on a text-to-video DiT"):
        L.load_adapter(gridded_adapter(CFG_I2V, layers=[0])).plan(CFG)
    with pytest.raises(ValueError, match="rank above 512"):
        L.load_adapter(gridded_adapter(CFG, rank=520, kinds=("self_attn.q",), layers=[0])).plan(CFG)
    with pytest.raises(ValueError, match="two spellings"):
        L.load_adapter(dict(base, **{"dit.blocks.0.ffn.0.lora_down.weight": torch.zeros(4, CFG.dim)}))
    with pytest.raises(ValueError, match="no keys"):
        L.load_adapter({})
    assert len(L.load_adapter(gridded_adapter(CFG_I2V)).plan(CFG_I2V)) == 2 * 12


# ---- ICV_LORA ------------------------------------------------------------------------------------------------------------------------
def test_parse_env():
    assert L.parse_env(None) == [] and L.parse_env("") == [] and L.parse_env("  ") == []
    assert L.parse_env("a.safetensors") == [("a.safetensors", 1.0)]
    assert L.parse_env("/x/a.safetensors:0.8,b.pth") == [("/x/a.safetensors", 0.8), ("b.pth", 1.0)]
    assert L.parse_env("a:-2, b:1e-1") == [("a", -2.0), ("b", 0.1)]
    for bad in ("a:", ":0.5", "a:x", "a,,b", "a:nan", "a:inf", ",", "a:0.5:"):
        with pytest.raises(ValueError, match="ICV_LORA: malformed entry"):
            L.parse_env(bad)


# ---- the pipeline's host side --------------------------------------------------------------------------------------------------------
def _pipe(monkeypatch, cfg=CFG):
    from infinicube_amd.videogen.pipeline import DiTHolder, WanVideoPipeline
    from standins import HashTextEncoder, PoolVAE
    monkeypatch.delenv("ICV_LORA", raising=False)
    return WanVideoPipeline("cuda:0", torch.bfloat16, DiTHolder(syn.make_dit_state_dict(cfg), cfg), HashTextEncoder(cfg), PoolVAE())


def test_load_lora_validates_before_an_engine_exists(monkeypatch, tmp_path):
    from safetensors.torch import save_file
    p = _pipe(monkeypatch)
    assert p.loras == [] and p.lora_record is None
    sd = gridded_adapter(CFG, prefix="diffusion_model.")
    path = str(tmp_path / "adapter.safetensors")
    save_file(sd, path)
    for module in (p.text_encoder, p.vae, None, "dit", object()):
        with pytest.raises(ValueError, match="DiT only"):
            p.load_lora(module, path)
    p.load_lora(p.dit, path, alpha=0.5)
    p.load_lora(p.dit, sd)                                        # a state dict in memory is accepted too
    assert [(e["path"], e["alpha"]) for e in p.loras] == [(path, 0.5), (None, 1.0)]
    _same_plan(p.loras[0]["adapter"].plan(CFG), L.load_adapter(gridded_adapter(CFG)).plan(CFG))      # the safetensors round trip
    assert p.loras[0]["adapter"].id != p.loras[1]["adapter"].id
    bad = str(tmp_path / "i2v.safetensors")
    save_file(gridded_adapter(CFG_I2V), bad)
    with pytest.raises(ValueError, match="k_img / v_img"):
        p.load_lora(p.dit, bad)
    with pytest.raises(ValueError, match="not lora_A / lora_B"):
        p.load_lora(p.dit, dict(sd, **{"head.head.lora_A.weight": torch.zeros(4, 4)}))
    assert len(p.loras) == 2 and p._engine is None and p._ops is None, "load_lora must do no GPU work"
    p.clear_lora()
    assert p.loras == []
    # the client of a worker pool holds no weights
    p.remote = True
    with pytest.raises(RuntimeError, match="ICV_LORA"):
        p.load_lora(p.dit, path)


def test_icv_lora_is_read_at_construction(monkeypatch):
    from infinicube_amd.videogen.pipeline import WanVideoPipeline
    monkeypatch.setenv("ICV_LORA", "/x/a.safetensors:0.8,b.pth")
    p = WanVideoPipeline("cuda:0")
    assert [(e["path"], e["alpha"], e["adapter"]) for e in p.loras] == [("/x/a.safetensors", 0.8, None), ("b.pth", 1.0, None)]
    monkeypatch.setenv("ICV_LORA", "a:")
    with pytest.raises(ValueError, match="malformed"):
        WanVideoPipeline("cuda:0")


def test_cpu_merge_fixture_is_one_rounding_of_the_exact_sum():
    """The fixture the GPU tests compare against: on the gridded adapter it equals bf16(exact sum) wherever the exact sum fits f32."""
    sd = syn.make_dit_state_dict(CFG)
    ad = gridded_adapter(CFG, layers=[0], kinds=("self_attn.q",))
    m = cpu_merge(sd, ad, -2.0)
    key = "blocks.0.self_attn.q.weight"
    exact = sd[key].to(torch.bfloat16).double() - 2.0 * (ad["blocks.0.self_attn.q.lora_B.weight"].double() @ ad["blocks.0.self_attn.q.lora_A.weight"].double())
    assert m[key].dtype == torch.bfloat16 and (m[key] != exact.to(torch.bfloat16)).float().mean() < 1e-3
    assert (m[key].float() != sd[key].to(torch.bfloat16).float()).float().mean() > 0.8
    assert all(m[k] is sd[k] for k in sd if k != key)
