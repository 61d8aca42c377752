"""The option table and the scope matrix (infinicube_amd/videogen/options.py) on CPU, row by row and cell by cell: where every
setting comes from (default, variable, keyword) and what its variable refuses; that every layer that can observe a refused combination
refuses it in its own pinned words before any operator runs; that every other pair of features runs together; and that the README's
table lists the same variables.  Tiny DiT, three latent frames, the TEST-ONLY operator twins of the feature files."""
import os
import re

import numpy as np
import pytest
import torch
import torch.distributed as dist

from infinicube_amd.videogen import guidance as G
from infinicube_amd.videogen import options as O
from infinicube_amd.videogen import sliding_window as SW
from infinicube_amd.videogen import solver as S
from infinicube_amd.videogen import synthetic as syn
from infinicube_amd.videogen.config import TokenGrid, preset
from infinicube_amd.videogen.dit import WanDiT
from infinicube_amd.videogen.inference import WanVideoGenerator
from infinicube_amd.videogen.pipeline import DiTHolder, WanVideoPipeline
from infinicube_amd.videogen.scheduler import FlowMatchScheduler
from standins import HashTextEncoder, PoolVAE
from test_attn_window_cpu import FramewinOps
from test_cfg_zero_cpu import ZeroOps
from test_v2v_cpu import V2VOps, make_clip

CFG, I2V_CFG, GRID = preset("tiny"), preset("tiny-i2v"), TokenGrid(9, 64, 96)        # 3 latent frames of 4 x 6 tokens
WINDOW_GRID = TokenGrid(5, 64, 96)                                                   # a sliding window of 2 latent frames
T2V_ID = "Wan2.1-T2V-1.3B"
CLIP_A, CLIP_B = make_clip(GRID, 1), make_clip(GRID, 2)
RECORDS = tuple(O.RECORDS.values())


class AllOps(V2VOps, ZeroOps):
    """The twins of every feature's kernels in one operator set; ``calls`` counts every public operator by name (V2VOps)."""

    def __init__(self):
        super().__init__("cpu")
        self.framewin_calls = []

    attention_framewin = FramewinOps.attention_framewin


def _pipe(ops=None, cfg=CFG, dtype=torch.bfloat16):
    return WanVideoPipeline("cpu", dtype, DiTHolder(syn.make_dit_state_dict(cfg), cfg), HashTextEncoder(cfg), PoolVAE(), ops=ops or AllOps())


def _call_kw(**extra):
    return dict(prompt="a street", negative_prompt="bad", height=GRID.height, width=GRID.width, num_frames=GRID.num_frames, seed=3,
                return_latents=True, **extra)


def _clean(monkeypatch):
    for k in O.ENV_NAMES:
        monkeypatch.delenv(k, raising=False)


# ---- 1. every row of the option table ---------------------------------------------------------------------------------------------------
def _bad(name, what, *texts):
    return {t: f"{name} must be {what}, got {t!r}" for t in texts}


FRAMES = ("an integer number of latent frames", "two", "2.5", " ")            # int() semantics: " 2 " and "+2" pass
STRICT = ("2.5", " ", "two", "+2", "02")                                      # ... the step counts take the plain spelling only
# name -> (default, variable's text, its value, a keyword value that differs, other variables the setting needs, {bad text: message})
ROWS = {
    "tea_cache_l1_thresh": (None, "0.3", 0.3, 0.1, dict(ICV_TEACACHE_MODEL_ID=T2V_ID), {"x": "could not convert string to float: 'x'"}),
    "tea_cache_model_id": ("", T2V_ID, T2V_ID, "Wan2.1-T2V-14B", dict(ICV_TEACACHE_L1_THRESH="0.3"), {}),
    "sliding_window_size": (None, "2", 2, 3, dict(ICV_SLIDING_WINDOW_STRIDE="1"), _bad("ICV_SLIDING_WINDOW_SIZE", *FRAMES)),
    "sliding_window_stride": (None, "1", 1, 2, dict(ICV_SLIDING_WINDOW_SIZE="2"), _bad("ICV_SLIDING_WINDOW_STRIDE", *FRAMES)),
    "loras": ([], "a.safetensors:0.5,b.pth", [dict(path="a.safetensors", alpha=0.5, adapter=None), dict(path="b.pth", alpha=1.0, adapter=None)],
              None, {}, {"a:": "ICV_LORA: malformed entry 'a:' in 'a:' (expected 'path' or 'path:alpha', comma separated)"}),
    "input_video": (None, "<clip A>", "<clip A>", CLIP_B, dict(ICV_DENOISING_STRENGTH="0.6"), {}),
    "denoising_strength": (None, "0.6", 0.6, 0.8, dict(ICV_INPUT_VIDEO="<clip A>"), _bad("ICV_DENOISING_STRENGTH", "a number in (0, 1]", "half", " ")),
    "attention_window_frames": (None, "0", 0, 1, {}, _bad("ICV_ATTN_WINDOW_FRAMES", *FRAMES)),
    "attention_sink_frames": (None, "1", 1, 0, dict(ICV_ATTN_WINDOW_FRAMES="0"), _bad("ICV_ATTN_SINK_FRAMES", *FRAMES)),
    "sample_solver": (None, "unipc", "unipc", "euler", {}, {"heun": "sample_solver must be one of 'euler', 'unipc' (or None), got 'heun'"}),
    "num_inference_steps": (50, "3", 3, 2, {}, _bad("ICV_SAMPLE_STEPS", "an integer >= 1", "0", "-1", *STRICT)),
    "cfg_zero_star": (None, "1", True, False, {}, _bad("ICV_CFG_ZERO_STAR", "0 or 1", "2", "true", "yes", " ")),
    "cfg_zero_init_steps": (None, "1", 1, 0, {}, _bad("ICV_CFG_ZERO_INIT_STEPS", "an integer >= 0", "-1", *STRICT)),
}


def _outcome(p, **kw):
    """Everything a call leaves behind: the latent and the seven records."""
    return p(**_call_kw(**kw)), {r: getattr(p, r) for r in RECORDS}


def _same(a, b):
    return torch.equal(a[0], b[0]) and a[1] == b[1]


def test_the_table_is_the_one_this_file_checks():
    assert [o.name for o in O.OPTIONS] == list(ROWS)
    assert O.ENV_NAMES == tuple(o.env for o in O.OPTIONS) + ("ICV_WORLD",) and len(set(O.ENV_NAMES)) == len(O.ENV_NAMES)
    assert O.Call._fields == tuple(n for n in ROWS if n != "loras")
    # the feature modules keep their constants: the same names
    from infinicube_amd.videogen import attn_window, lora, teacache, v2v
    assert set(O.ENV_NAMES) == {teacache.ENV_THRESH, teacache.ENV_MODEL_ID, SW.ENV_SIZE, SW.ENV_STRIDE, lora.ENV, v2v.ENV_VIDEO, v2v.ENV_STRENGTH,
                                attn_window.ENV_WINDOW, attn_window.ENV_SINK, S.ENV_SOLVER, S.ENV_STEPS, G.ENV_STAR, G.ENV_INIT_STEPS, "ICV_WORLD"}


@pytest.mark.parametrize("name", list(ROWS))
def test_option_row(name, monkeypatch, tmp_path):
    _clean(monkeypatch)
    clip = str(tmp_path / "clip_a.npy")
    np.save(clip, CLIP_A)
    opt = next(o for o in O.OPTIONS if o.name == name)
    default, text, value, keyword, others, bad = (clip if isinstance(x, str) and x == "<clip A>" else x for x in ROWS[name])
    assert getattr(_pipe(), name) == default                                      # unset: the default
    monkeypatch.setenv(opt.env, "")
    assert getattr(_pipe(), name) == default                                      # ... and so is the empty string
    monkeypatch.setenv("ICV_SAMPLE_STEPS", "2")                                   # (short calls)
    for k, v in others.items():
        monkeypatch.setenv(k, clip if v == "<clip A>" else v)
    monkeypatch.setenv(opt.env, text)
    p = _pipe()
    assert getattr(p, name) == value and type(getattr(p, name)) is type(value)    # variable -> attribute
    if opt.keyword:
        from_env = _outcome(p)
        from_keyword = _outcome(p, **{name: keyword})
        assert _same(_outcome(p), from_env) and getattr(p, name) == value         # the keyword does not outlive its call
        monkeypatch.delenv(opt.env)
        plain = _pipe()                                                           # the same pipeline without the variable
        assert _same(from_keyword, _outcome(plain, **{name: keyword}))            # the keyword won over the variable ...
        assert not _same(from_keyword, from_env)                                  # ... and the two values do differ
    else:
        assert name not in O.Call._fields
    for spelling, message in bad.items():                                         # refused at construction, in the variable's words
        monkeypatch.setenv(opt.env, spelling)
        with pytest.raises(ValueError) as e:
            _pipe()
        assert str(e.value) == message


# ---- 2. every cell of the scope matrix, in every layer that can observe it ----------------------------------------------------------------
A, F, P = O.ATTN_WINDOW, O.FP8_ATTN, O.PARALLEL
_PIPE_NAMES = {O.SLIDING: "sliding_window_size / sliding_window_stride", A: "attention_window_frames / attention_sink_frames",
               O.SOLVER: "sample_solver='unipc'", O.CFG_ZERO: "cfg_zero_star / cfg_zero_init_steps", O.V2V: "input_video / denoising_strength"}
_I2V_WORDS = "an image-to-video DiT (the first-frame conditioning belongs to window 0 only)"
PIPELINE_WORDS = {
    (A, O.SLIDING): "sliding_window_size in the same call",
    (A, F): "the e4m3 self-attention mode (torch_dtype=float8_e4m3fn)",
    (O.SOLVER, O.SLIDING): "sliding_window_size (more than one window) in the same call",
    (O.CFG_ZERO, O.SLIDING): "sliding_window_size (more than one window) in the same call",
    (O.SLIDING, P): "a process group of 2 ranks", (O.SLIDING, O.I2V): _I2V_WORDS,
    (O.SLIDING, O.TEACACHE): "TeaCache (tea_cache_l1_thresh / ICV_TEACACHE_L1_THRESH) in the same call",
    (A, P): "a process group of 2 ranks", (O.SOLVER, P): "a process group of 2 ranks", (O.CFG_ZERO, P): "a process group of 2 ranks",
    (O.V2V, P): "a process group of 2 ranks",
}
_ENGINE_NAMES = {O.SLIDING: "sliding temporal windows", A: "attention_window_frames", O.SOLVER: "sample_solver='unipc'",
                 O.CFG_ZERO: "cfg_zero_star / cfg_zero_init_steps"}
_ENGINE_PARALLEL = "sequence / CFG-branch parallelism (world > 1)"
ENGINE_WORDS = {
    (A, O.SLIDING): "sliding_window_size in the same call",
    (A, F): "the e4m3 self-attention mode (attn_dtype='fp8')",
    (O.SOLVER, O.SLIDING): "more than one sliding temporal window",
    (O.CFG_ZERO, O.SLIDING): "more than one sliding temporal window",
    (O.SLIDING, P): _ENGINE_PARALLEL, (O.SLIDING, O.I2V): _I2V_WORDS,
    (O.SLIDING, O.TEACACHE): "TeaCache (one residual per window and CFG branch is not implemented)",
    (A, P): "sequence parallelism (world > 1)", (O.SOLVER, P): _ENGINE_PARALLEL,
    (O.CFG_ZERO, P): _ENGINE_PARALLEL + ": the moments would need an all-reduce",
}
GENERATOR_WORDS = {
    (O.SLIDING, P): "sliding_window_size / sliding_window_stride (ICV_SLIDING_WINDOW_SIZE / _STRIDE) cannot be combined with ICV_WORLD > 1 "
                    "(the worker pool's ranks shard ONE forward) yet",
    (A, P): "attention_window_frames / attention_sink_frames (ICV_ATTN_WINDOW_FRAMES / ICV_ATTN_SINK_FRAMES) cannot be combined with "
            "ICV_WORLD > 1 (the frame-windowed launch is single-rank) yet",
    (O.SOLVER, P): "sample_solver (ICV_SAMPLE_SOLVER) cannot be combined with ICV_WORLD > 1 (the multistep update is single-rank) yet",
    (O.CFG_ZERO, P): "cfg_zero_star / cfg_zero_init_steps (ICV_CFG_ZERO_STAR / ICV_CFG_ZERO_INIT_STEPS) cannot be combined with ICV_WORLD > 1 "
                     "(the scale's moments are single-rank) yet",
    (O.V2V, P): "input_video / denoising_strength (ICV_INPUT_VIDEO / ICV_DENOISING_STRENGTH) cannot be combined with ICV_WORLD > 1 "
                "(the start latent is noised in one process) yet",
}
# how a call switches each feature on (three latent frames: two windows of two; a window of 0 frames is not dense)
ON = {O.SLIDING: dict(sliding_window_size=2, sliding_window_stride=1), A: dict(attention_window_frames=0), O.SOLVER: dict(sample_solver="unipc"),
      O.CFG_ZERO: dict(cfg_zero_star=True), O.V2V: dict(input_video=CLIP_A, denoising_strength=0.6),
      O.TEACACHE: dict(tea_cache_l1_thresh=0.1, tea_cache_model_id=T2V_ID)}


def test_every_layer_words_every_cell_it_can_observe():
    cells = set(O.SCOPE)
    assert len(cells) == len(O.SCOPE) and set(PIPELINE_WORDS) == cells
    assert set(ENGINE_WORDS) == {c for c in cells if c[0] != O.V2V}                       # the engine never sees video-to-video
    assert set(GENERATOR_WORDS) == {c for c in cells if c[1] == P}                         # the generator sees its pool, nothing else
    assert all(not (b, a) in cells for a, b in cells)                                      # a pair is stated once


def _two_ranks(mp):
    mp.setattr(dist, "is_initialized", lambda: True)
    mp.setattr(dist, "get_world_size", lambda *a: 2)
    mp.setattr(dist, "get_rank", lambda *a: 0)


@pytest.mark.parametrize("feature,condition", O.SCOPE)
def test_pipeline_refuses(feature, condition, monkeypatch):
    _clean(monkeypatch)
    ops = AllOps()
    p = _pipe(ops, cfg=I2V_CFG if condition == O.I2V else CFG, dtype=torch.float8_e4m3fn if condition == F else torch.bfloat16)
    monkeypatch.setattr(p, "_get_engine", lambda: pytest.fail("the engine was built before the scope was checked"))
    with monkeypatch.context() as mp:
        if condition == P:
            _two_ranks(mp)
        with pytest.raises(ValueError) as e:
            p(**_call_kw(num_inference_steps=2, **ON[feature], **ON.get(condition, {})))
    assert str(e.value) == f"{_PIPE_NAMES[feature]} cannot be combined with {PIPELINE_WORDS[feature, condition]} yet"
    assert not ops.calls


@pytest.mark.parametrize("feature,condition", list(ENGINE_WORDS))
def test_engine_refuses(feature, condition):
    ops = AllOps()
    cfg = I2V_CFG if condition == O.I2V else CFG
    fp8 = dict(gemm_dtype="fp8", attn_dtype="fp8", fp8_weights=WanDiT.FP8_WEIGHTS) if condition == F else {}
    windows = O.SLIDING in (feature, condition)
    m = WanDiT(cfg, syn.make_dit_state_dict(cfg), ops, syn.make_buffer_embedder_state_dict(cfg), **fp8)
    m.prepare(WINDOW_GRID if windows else GRID, force_sp=condition == P)
    sch = FlowMatchScheduler(2)
    kw = {}
    if windows:
        kw["sliding_window"] = SW.plan(GRID.T, 2, 1)
    if feature == O.SOLVER:
        kw["solver"] = S.MultistepPlan("unipc", sch.sigmas)
    if feature == O.CFG_ZERO:
        kw["guidance"] = G.GuidancePlan(True, 0)
    if condition == O.TEACACHE:
        kw["tea_cache"] = object()                    # refused for being there, never looked at
    if feature == A and windows:
        m.set_attention_window(0, 0)
    issued = dict(ops.calls)
    with pytest.raises(ValueError) as e:
        if feature == A and not windows:
            m.set_attention_window(0, 0)              # alone, the window's scope is checked where it is set
        else:
            m.denoise(syn.make_latent_noise(GRID), None, None, None, sch, 5.0, **kw)
    assert str(e.value) == f"{_ENGINE_NAMES[feature]} cannot be combined with {ENGINE_WORDS[feature, condition]} yet"
    assert dict(ops.calls) == issued


@pytest.mark.parametrize("feature,condition", list(GENERATOR_WORDS))
def test_generator_refuses(feature, condition, monkeypatch):
    _clean(monkeypatch)
    sem, co = syn.make_dummy_buffers(GRID)
    for attr, value in ON[feature].items():           # each attribute of the feature switches it on by itself
        ops = AllOps()
        g = WanVideoGenerator.__new__(WanVideoGenerator)
        g._pool, g.pipe = object(), _pipe(ops)        # a pool that cannot run anything
        setattr(g.pipe, attr, value)
        with pytest.raises(ValueError) as e:
            g.generate(sem, co, seed=0)
        assert str(e.value) == GENERATOR_WORDS[feature, condition]
        assert not ops.calls


# ---- 3. every other pair of features runs together ------------------------------------------------------------------------------------------
FEATURES = (O.TEACACHE, O.SLIDING, A, O.SOLVER, O.CFG_ZERO, O.V2V)       # what one rank can switch on with a keyword
FREE_PAIRS = [(a, b) for i, a in enumerate(FEATURES) for b in FEATURES[i + 1:] if (a, b) not in O.SCOPE and (b, a) not in O.SCOPE]


def test_free_pairs_are_the_rest_of_the_matrix():
    assert len(FREE_PAIRS) == 15 - 4 and (O.SOLVER, O.CFG_ZERO) in FREE_PAIRS and (O.SLIDING, O.V2V) in FREE_PAIRS


@pytest.mark.parametrize("a,b", FREE_PAIRS)
def test_free_pair_runs(a, b, monkeypatch):
    _clean(monkeypatch)
    p = _pipe()
    lat = p(**_call_kw(num_inference_steps=2, **ON[a], **ON[b]))
    assert torch.isfinite(lat).all() and tuple(lat.shape) == (16,) + GRID.latent_shape()[1:]
    on = {O.RECORDS[a], O.RECORDS[b]}
    assert all((getattr(p, r) is not None) == (r in on) for r in RECORDS), {r: getattr(p, r) for r in RECORDS}


# ---- 4. the README's table ------------------------------------------------------------------------------------------------------------------
def test_readme_table_lists_the_same_variables():
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "README.md"), encoding="utf-8") as f:
        text = f.read()
    start = text.index("| option | variable | cannot be combined with |")
    table = text[start: text.index("\n\n", start)]
    assert set(re.findall(r"ICV_[A-Z0-9_]+", table)) == set(O.ENV_NAMES)
