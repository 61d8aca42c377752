"""LoRA adapter files for the DiT: parse, validate, and lay out as merges into the engine's packed weights.

Host-only (no GPU): ``load_adapter`` reads a file and groups its keys per target linear, ``Adapter.plan(cfg)`` maps every
pair onto (engine weight name, layer, row range) with the rank zero-padded for the merge kernel (csrc/lora.hip), and
``parse_env`` reads ``ICV_LORA``.  The merge itself is ``dit.WanDiT.apply_lora``; the public call is upstream's
``pipe.load_lora(pipe.dit, path, alpha=1)`` (pipeline.WanVideoPipeline).

The update rule is ``W += alpha * scale * lora_B @ lora_A`` with ``scale = 1`` unless the file carries a ``<target>.alpha``
scalar (kohya / PEFT exports), then ``scale = alpha_key / rank`` — both restated from memory of DiffSynth's general loader and
the kohya convention, unverified against the fork (ORACLE_RISKS.md).  Nothing is skipped silently: a key this loader does not
understand is an error, not a no-op.
"""

from __future__ import annotations

import itertools
import re
from collections import namedtuple
from typing import Dict, List, Optional, Tuple, Union

import torch

from .config import WanDiTConfig

PREFIXES = ("diffusion_model.", "pipe.dit.", "dit.", "")          # longest first; "" = bare keys
RANK_ALIGN, RANK_MAX = 32, 512                                    # icv_lora_merge_bf16's contract
ENV = "ICV_LORA"

_TARGET = re.compile(r"^blocks\.(\d+)\.(self_attn\.(?:q|k|v|o)|cross_attn\.(?:q|k|v|o|k_img|v_img)|ffn\.(?:0|2))$")
# key suffix -> which half of the pair it is
_SUFFIXES = ((".lora_A.default.weight", "down"), (".lora_B.default.weight", "up"), (".lora_A.weight", "down"),
             (".lora_B.weight", "up"), (".lora_down.weight", "down"), (".lora_up.weight", "up"), (".alpha", "alpha"))

# one merge: layers[layer][name][rows[0]:rows[1]] += scale * alpha * up @ down_t.T;  up [N, R], down_t [K, R], R % 32 == 0
PlanEntry = namedtuple("PlanEntry", ["name", "layer", "rows", "up", "down_t", "scale"])

_ids = itertools.count(1)


def _few(keys) -> str:
    keys = list(keys)
    return ", ".join(repr(k) for k in keys[:4]) + (f", ... ({len(keys)} in all)" if len(keys) > 4 else "")


def _split_key(key: str) -> Optional[Tuple[str, str]]:
    """'<prefix><target><suffix>' -> (target, 'down' | 'up' | 'alpha'), or None when the key is not of that form."""
    for pre in PREFIXES:
        if key.startswith(pre):
            rest = key[len(pre):]
            for suf, half in _SUFFIXES:
                if rest.endswith(suf) and _TARGET.match(rest[: -len(suf)]):
                    return rest[: -len(suf)], half
    return None


def _where(cfg: WanDiTConfig, kind: str):
    """Target kind -> (engine weight name, row range, (N, K)): the packing of dit.WanDiT.__init__ (q|k|v rows of wqkv, k|v rows of
    xkv_w / xkv_img_w)."""
    d, f = cfg.dim, cfg.ffn_dim
    table = {
        "self_attn.q": ("wqkv", (0, d), (d, d)), "self_attn.k": ("wqkv", (d, 2 * d), (d, d)), "self_attn.v": ("wqkv", (2 * d, 3 * d), (d, d)),
        "self_attn.o": ("wo", (0, d), (d, d)),
        "cross_attn.q": ("xq_w", (0, d), (d, d)), "cross_attn.k": ("xkv_w", (0, d), (d, d)), "cross_attn.v": ("xkv_w", (d, 2 * d), (d, d)),
        "cross_attn.o": ("xo_w", (0, d), (d, d)),
        "cross_attn.k_img": ("xkv_img_w", (0, d), (d, d)), "cross_attn.v_img": ("xkv_img_w", (d, 2 * d), (d, d)),
        "ffn.0": ("f0_w", (0, f), (f, d)), "ffn.2": ("f2_w", (0, d), (d, f)),
    }
    return table[kind]


class Adapter:
    """The pairs of one adapter file, per target linear: ``pairs[target] = (down [R, K], up [N, R], alpha scalar | None)``."""

    def __init__(self, pairs: Dict[str, tuple], path: Optional[str] = None):
        self.pairs = pairs
        self.path = path
        self.id = next(_ids)          # two loads of one file are two adapters (each load merges once, as upstream)

    @property
    def rank(self) -> int:
        return max(p[0].shape[0] for p in self.pairs.values())

    def plan(self, cfg: WanDiTConfig) -> List[PlanEntry]:
        """The merges of this adapter into an engine of shape ``cfg``, in key order; raises ValueError on anything that does not fit."""
        out, beyond, img, shapes, ranks = [], [], [], [], []
        for target in sorted(self.pairs, key=lambda t: (int(_TARGET.match(t).group(1)), t)):
            down, up, alpha_key = self.pairs[target]
            m = _TARGET.match(target)
            layer, kind = int(m.group(1)), m.group(2)
            if layer >= cfg.num_layers:
                beyond.append(target)
                continue
            if kind.endswith("_img") and not cfg.has_image_input:
                img.append(target)
                continue
            name, rows, (N, K) = _where(cfg, kind)
            r = down.shape[0]
            if tuple(down.shape) != (r, K) or tuple(up.shape) != (N, r):
                shapes.append(f"{target}: lora_A {tuple(down.shape)} / lora_B {tuple(up.shape)} for a [{N}, {K}] weight")
                continue
            if r > RANK_MAX:
                ranks.append(f"{target}: rank {r}")
                continue
            rp = max(RANK_ALIGN, -(-r // RANK_ALIGN) * RANK_ALIGN)
            up_p = torch.zeros((N, rp), dtype=up.dtype)
            up_p[:, :r] = up
            down_t = torch.zeros((K, rp), dtype=down.dtype)
            down_t[:, :r] = down.t()
            out.append(PlanEntry(name, layer, rows, up_p, down_t, 1.0 if alpha_key is None else float(alpha_key) / r))
        if beyond:
            raise ValueError(f"LoRA: layer index beyond the model's {cfg.num_layers} layers: {_few(beyond)}")
        if img:
            raise ValueError(f"LoRA: k_img / v_img targets on a text-to-video DiT (no image branch): {_few(img)}")
        if shapes:
            raise ValueError(f"LoRA: shapes do not fit the model ({cfg.name}): {_few(shapes)}")
        if ranks:
            raise ValueError(f"LoRA: rank above {RANK_MAX} is not supported by the merge kernel: {_few(ranks)}")
        return out


def load_adapter(src: Union[str, Dict[str, torch.Tensor]]) -> Adapter:
    """Adapter from a file (safetensors or torch, through io.load_state_dict) or from a state dict already in memory."""
    path = None
    if isinstance(src, str):
        from .io import load_state_dict
        path, sd = src, load_state_dict(src)
    else:
        sd = dict(src)
    halves: Dict[str, dict] = {}
    unknown, twice = [], []
    for key, t in sd.items():
        hit = _split_key(key)
        if hit is None:
            unknown.append(key)
            continue
        target, half = hit
        slot = halves.setdefault(target, {})
        if half in slot:
            twice.append(key)
        slot[half] = (key, t)
    if unknown:
        raise ValueError("LoRA: keys that are not lora_A / lora_B (lora_down / lora_up, alpha) of a per-block attention or FFN linear "
                         f"(embeddings, head, norms, modulation and diff-style keys are not supported): {_few(unknown)}")
    if twice:
        raise ValueError(f"LoRA: the same target and half under two spellings: {_few(twice)}")
    if not halves:
        raise ValueError("LoRA: the adapter holds no keys")
    lonely = [v[0] for slot in halves.values() if ("down" in slot) != ("up" in slot) or "down" not in slot
              for h, v in slot.items()]
    if lonely:
        raise ValueError(f"LoRA: half of a lora_A / lora_B pair is missing next to: {_few(lonely)}")
    pairs, bad_rank, bad_alpha = {}, [], []
    for target, slot in halves.items():
        down, up = slot["down"][1].detach(), slot["up"][1].detach()
        if down.dim() != 2 or up.dim() != 2 or down.shape[0] != up.shape[1]:
            bad_rank.append(f"{slot['down'][0]} {tuple(down.shape)} vs {slot['up'][0]} {tuple(up.shape)}")
            continue
        alpha_key = None
        if "alpha" in slot:
            if slot["alpha"][1].numel() != 1:
                bad_alpha.append(slot["alpha"][0])
                continue
            alpha_key = float(slot["alpha"][1].reshape(()).item())
        pairs[target] = (down, up, alpha_key)
    if bad_rank:
        raise ValueError(f"LoRA: rank mismatch between lora_A [R, K] and lora_B [N, R]: {_few(bad_rank)}")
    if bad_alpha:
        raise ValueError(f"LoRA: alpha must be one scalar per target: {_few(bad_alpha)}")
    return Adapter(pairs, path)


def parse_env(value: Optional[str]) -> List[Tuple[str, float]]:
    """``ICV_LORA="pathA:0.8,pathB"`` -> [(pathA, 0.8), (pathB, 1.0)]; unset / empty -> [].  What follows the LAST colon of an
    entry is its alpha and must be a finite number: 'path:', 'path:x' and an empty entry raise."""
    if value is None or not value.strip():
        return []
    out = []
    for item in value.split(","):
        item = item.strip()
        path, sep, a = item.rpartition(":")
        if not sep:
            path, a = item, "1"
        try:
            alpha = float(a)
        except ValueError:
            alpha = None
        if not path or alpha is None or alpha != alpha or alpha in (float("inf"), float("-inf")):
            raise ValueError(f"{ENV}: malformed entry {item!r} in {value!r} (expected 'path' or 'path:alpha', comma separated)")
        out.append((path, alpha))
    return out
