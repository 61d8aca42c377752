"""Coarse-to-fine sampling: ``coarse_steps`` / ``coarse_size`` run the first steps of a call at a lower resolution.

A step's cost is superlinear in its tokens (self-attention is quadratic in S, everything else linear), and the early steps of a
flow-match call decide layout, not detail.  Progressive-resolution samplers for video DiTs (Jenga's "ProRes", Bottleneck Sampling)
and the "two-pass / latent upscale" workflows of the common Wan wrappers use that [EXT: restated from memory of the papers,
ORACLE_RISKS.md R32].  The rule here, for a call of N steps over its sigma list sigma_0 .. sigma_{N-1} with ``coarse_steps = K``:

1. coarse stage: noise drawn at the coarse latent shape (the FIRST draw of the call's generator), steps 0 .. K-1 on the coarse
   grid under a scheduler over sigma_0 .. sigma_{K-1} - whose last step goes to 0, so the coarse latent ends as the x0-prediction
   x - sigma_{K-1} v; guidance buffers (and an image-to-video DiT's conditioning) are resized, encoded and embedded at the coarse size;
2. switch: noise drawn at the fine latent shape (the SECOND draw), and one launch (icv_latent_resize_noise_f32) writes
   x_K = (1 - sigma_K) up(x0_hat) + sigma_K noise into the noise's tensor; up is a bilinear resize of every (channel, frame) plane,
   frames are never resized;
3. fine stage: steps K .. N-1 on the call's grid under the call's scheduler; everything that keeps state (a multistep solver's
   history) begins at step K.

N forwards per branch in all, K of them at the coarse size.  ``coarse_steps`` of None or 0 is off: today's launches, allocations,
bits and ONE generator draw.  ``coarse_size`` of None is half of each dimension, rounded down to a multiple of 16.

First-version scope, each refused with a ValueError in the pipeline before any GPU work (``check_call``) and, where the engine can
observe it, in ``WanDiT.coarse_engine``; none falls back: TeaCache, EasyCache, more than one sliding window, ``input_video`` /
``input_mask``, more than one rank.  It composes with the multistep solvers (one plan per stage), CFG-Zero* (zero-init acts in the
coarse stage and must end before K), NAG, Enhance-A-Video, LoRA, the frame window and radial attention, the e4m3 mode and an
image-to-video DiT.

The settings are keywords of the call with pipeline attributes of the same names as their fallback (``gen.pipe.coarse_steps = 25``
for the caller of the unchanged generator); like ``nag_scale`` there is no environment route and no row in ``options.OPTIONS``.

Host logic only: nothing here imports torch.
"""

from __future__ import annotations

from typing import Optional, Tuple


def default_size(height: int, width: int) -> Tuple[int, int]:
    """Half of each dimension, rounded down to a multiple of 16."""
    return (height // 2) // 16 * 16, (width // 2) // 16 * 16


def validate(coarse_steps, coarse_size, num_steps: int, height: int, width: int) -> Optional[Tuple[int, Tuple[int, int]]]:
    """(K, (h_lo, w_lo)) of a call with the coarse stage on, None when it is off (``coarse_steps`` None or 0).  Raises ValueError
    for a K that is not an integer in [1, num_steps - 1] (a bool included), a ``coarse_size`` that is not two integers, each a
    multiple of 16 and at most the call's, with a product strictly smaller than the call's, and a ``coarse_size`` without
    ``coarse_steps``."""
    if isinstance(coarse_steps, bool) or not (coarse_steps is None or isinstance(coarse_steps, int)):
        raise ValueError(f"coarse_steps must be an integer in [1, num_inference_steps - 1] (or None / 0 = off), got {coarse_steps!r}")
    if coarse_steps is None or coarse_steps == 0:
        if coarse_size is not None:
            raise ValueError("coarse_size given without coarse_steps: it only shapes the coarse stage of coarse-to-fine sampling")
        return None
    if not 1 <= coarse_steps <= num_steps - 1:
        raise ValueError(f"coarse_steps must be an integer in [1, num_inference_steps - 1] = [1, {num_steps - 1}] "
                         f"(the fine stage needs a step), got {coarse_steps}")
    if coarse_size is None:
        coarse_size = default_size(height, width)
    try:
        size = tuple(coarse_size)
    except TypeError:
        size = ()
    if len(size) != 2 or any(isinstance(v, bool) or not isinstance(v, int) for v in size):
        raise ValueError(f"coarse_size must be two integers (height, width), got {coarse_size!r}")
    h_lo, w_lo = size
    if h_lo < 16 or w_lo < 16 or h_lo % 16 or w_lo % 16:
        raise ValueError(f"coarse_size must be positive multiples of 16, got {size!r}")
    if h_lo > height or w_lo > width:
        raise ValueError(f"coarse_size {size!r} must be at most the call's size {(height, width)!r} in both dimensions")
    if h_lo * w_lo >= height * width:
        raise ValueError(f"coarse_size {size!r} must be strictly smaller than the call's size {(height, width)!r}")
    return int(coarse_steps), (int(h_lo), int(w_lo))


def check_call(coarse_steps: int, world: int, windows: bool, tea_cache: bool, easy_cache: bool, input_video: bool, input_mask: bool,
               zero_init_steps: int = 0) -> None:
    """The first-version scope of a call with the coarse stage on, in the pipeline's terms."""
    if tea_cache:
        raise ValueError("coarse_steps cannot be combined with TeaCache (tea_cache_l1_thresh / ICV_TEACACHE_L1_THRESH) in the same call yet")
    if easy_cache:
        raise ValueError("coarse_steps cannot be combined with EasyCache (easy_cache_thresh) in the same call yet")
    if windows:
        raise ValueError("coarse_steps cannot be combined with sliding_window_size (more than one window) in the same call yet")
    if input_video or input_mask:
        raise ValueError("coarse_steps cannot be combined with input_video / input_mask in the same call yet")
    if world > 1:
        raise ValueError(f"coarse_steps cannot be combined with a process group of {world} ranks yet")
    if zero_init_steps >= coarse_steps:
        raise ValueError(f"cfg_zero_init_steps={zero_init_steps} must be less than coarse_steps={coarse_steps}: zero-init acts in the coarse stage")


def record(coarse_steps: int, size: Tuple[int, int], sigma: float, tokens: Tuple[int, int]) -> dict:
    """``pipe.coarse_record`` of a call: K, the coarse size, sigma_K and the tokens per forward of the two stages."""
    return dict(steps=int(coarse_steps), size=(int(size[0]), int(size[1])), sigma=float(sigma), tokens=(int(tokens[0]), int(tokens[1])))
