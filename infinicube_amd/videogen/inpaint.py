"""Regenerate part of a clip: ``input_mask`` pins the known latent cells.

``input_video`` / ``denoising_strength`` (v2v.py) re-noise a whole clip and denoise all of it.  With ``input_mask`` part of the clip
is known and comes out as it went in.  The rule is the one of diffusion inpainting (diffusers' inpaint pipelines [EXT], restated as
remembered, not read: ORACLE_RISKS.md R27): after every step the known cells of the latent are put back on the noising
trajectory of the known clip with the SAME noise the call drew,

    x[known] <- (1 - sigma_next) * x0 + sigma_next * noise          (icv_pin_known_f32, one launch per step)

and sigma = 0 after the last step, so the known cells end as the encoded clip exactly.  The mask is given in pixels and frames
(non-zero = regenerate, diffusers' convention); a latent cell is kept only if NOTHING in its stride footprint is to be
regenerated (icv_latent_keep_mask_u8, one launch per call).  This module holds the host side: the mask's forms and validation,
the plan object the engine takes, and ``chain``, which continues a clip past one call's frames by holding each call's first
latent frames to the tail of the call before.
"""

from __future__ import annotations

from collections import namedtuple
from dataclasses import dataclass
from typing import List

import numpy as np
from PIL import Image

FORMS = "a uint8 / bool array [N, H, W], a list of N single-channel PIL images, or N per-frame bools (True = regenerate)"


@dataclass
class KnownPlan:
    """What WanDiT.denoise(known=...) takes: the encoded clip, the noise the call drew and the kept cells, on the device.
    x0, noise: f32, the latent's shape [C, T, H/8, W/8]; keep: u8 [T, H/8, W/8], non-zero = kept."""
    x0: object
    noise: object
    keep: object

    def check(self, latent) -> None:
        if tuple(self.x0.shape) != tuple(latent.shape) or tuple(self.noise.shape) != tuple(latent.shape) or \
                tuple(self.keep.shape) != tuple(latent.shape[1:]):
            raise ValueError(f"known cells: x0 {tuple(self.x0.shape)}, noise {tuple(self.noise.shape)} and keep {tuple(self.keep.shape)} "
                             f"do not fit a latent of {tuple(latent.shape)}")


def frame_mask(num_frames: int, height: int, width: int, keep_frames) -> np.ndarray:
    """uint8 [num_frames, height, width]: 0 (keep) on the frames ``keep_frames`` lists (any iterable of indices, a range or a
    slice), 1 (regenerate) elsewhere."""
    m = np.ones((num_frames, height, width), dtype=np.uint8)
    if isinstance(keep_frames, slice):
        m[keep_frames] = 0
        return m
    idx = [int(i) for i in keep_frames]
    if any(not 0 <= i < num_frames for i in idx):
        raise ValueError(f"frame_mask: keep_frames {idx} outside [0, {num_frames})")
    m[idx] = 0
    return m


def validate(mask, frames, num_frames: int, height: int, width: int):
    """The mask in effect for one call as a uint8 array [N, H, W] (non-zero = regenerate), or None; raises ValueError before
    anything is encoded or launched.  ``frames``: the call's input clip (v2v.validate), None without one.  The size must be the
    call's exactly: masks are not resized."""
    if mask is None:
        return None
    if frames is None:
        raise ValueError("input_mask needs an input_video: the mask says which part of that clip is kept")
    want = (num_frames, height, width)
    if isinstance(mask, np.ndarray):
        a = mask
    else:
        try:
            items = list(mask)
        except TypeError:
            raise ValueError(f"input_mask must be {FORMS}, got {type(mask).__name__}") from None
        if items and all(isinstance(x, Image.Image) for x in items):
            for i, im in enumerate(items):
                if len(im.getbands()) != 1:
                    raise ValueError(f"input_mask: frame {i} is a {im.mode} image, a mask frame has one channel")
                if im.size != (width, height):
                    raise ValueError(f"input_mask: frame {i} is {im.size[0]}x{im.size[1]}, the call is {width}x{height} (masks are not resized)")
            if len(items) != num_frames:
                raise ValueError(f"input_mask has {len(items)} frames, num_frames={num_frames}")
            a = np.stack([np.asarray(im) != 0 for im in items])
        elif items and all(isinstance(x, (bool, np.bool_)) for x in items):
            if len(items) != num_frames:
                raise ValueError(f"input_mask has {len(items)} frames, num_frames={num_frames}")
            a = np.broadcast_to(np.asarray(items, dtype=bool)[:, None, None], want)
        else:
            raise ValueError(f"input_mask must be {FORMS}")
    if a.dtype != np.uint8 and a.dtype != np.bool_:
        raise ValueError(f"input_mask: expected a uint8 or bool array, got {a.dtype}")
    if tuple(a.shape) != want:
        raise ValueError(f"input_mask has shape {tuple(a.shape)}, the call needs {want} (masks are not resized)")
    return np.ascontiguousarray(a != 0, dtype=np.uint8)


def record(keep) -> dict:
    """``pipe.inpaint_record`` from the keep bytes read back once: how much of the latent the call holds."""
    cells, kept = int(keep.size), int(np.count_nonzero(keep))
    return dict(cells=cells, kept_cells=kept, kept_fraction=kept / cells)


# ---- continuing a clip ----------------------------------------------------------------------------------------------------------------
ChainPlan = namedtuple("ChainPlan", "starts overlaps")      # per clip: its first frame, and how many of its first frames are held


def plan(num_frames: int, clip_frames: int = 93, overlap_frames: int = 9) -> ChainPlan:
    """Clip starts 0, s, 2s, ... (s = clip - overlap) while start + clip < N, the last clip at N - clip; ``overlaps[j]`` is how
    many first frames of clip j were generated by the clips before it (0 for clip 0).  Every start is a multiple of 4, so every
    overlap is 4k + 1: whole latent frames."""
    for name, v in (("num_frames", num_frames), ("clip_frames", clip_frames), ("overlap_frames", overlap_frames)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1 or v % 4 != 1:
            raise ValueError(f"chain: {name} must be an integer 4k + 1 >= 1, got {v!r}")
    if overlap_frames >= clip_frames:
        raise ValueError(f"chain: overlap_frames={overlap_frames} must be smaller than clip_frames={clip_frames}")
    if num_frames < clip_frames:
        raise ValueError(f"chain: {num_frames} frames are fewer than one clip of {clip_frames}")
    step, starts = clip_frames - overlap_frames, [0]
    while starts[-1] + clip_frames < num_frames:
        starts.append(min(starts[-1] + step, num_frames - clip_frames))
    overlaps = [0] + [a + clip_frames - b for a, b in zip(starts, starts[1:])]
    return ChainPlan(starts, overlaps)


def chain(pipe, *, semantic_buffer_video, coordinate_buffer_video, clip_frames: int = 93, overlap_frames: int = 9, seed=None,
          **call_kw) -> List[Image.Image]:
    """A clip as long as the guidance buffers, as consecutive calls of ``pipe``: clip 0 is the plain call on its slice of the
    buffers; clip j > 0 is given the already generated frames of its overlap (followed by the last of them repeated) as
    ``input_video`` and a per-frame mask that keeps exactly the overlap, with ``seed + j``.  The VAE encoder is causal in time, so
    the kept latent frames depend on the overlap alone.  Returns clip 0's frames plus each later clip's frames after its overlap."""
    if call_kw.get("return_latents"):
        raise ValueError("chain: return_latents=True is not supported (the next clip continues from decoded frames)")
    for k in ("input_video", "input_mask", "num_frames"):
        if k in call_kw:
            raise ValueError(f"chain sets {k} itself")
    sem, co = list(semantic_buffer_video), list(coordinate_buffer_video)
    if len(sem) != len(co):
        raise ValueError(f"chain: the buffer videos have {len(sem)} and {len(co)} frames")
    p = plan(len(sem), clip_frames, overlap_frames)
    out: List[Image.Image] = []
    for j, (start, ov) in enumerate(zip(p.starts, p.overlaps)):
        kw = dict(call_kw, semantic_buffer_video=sem[start: start + clip_frames], coordinate_buffer_video=co[start: start + clip_frames],
                  num_frames=clip_frames, seed=None if seed is None else seed + j)
        if j > 0:
            held = out[start: start + ov]
            w, h = held[0].size
            kw.update(input_video=held + [held[-1]] * (clip_frames - ov), input_mask=frame_mask(clip_frames, h, w, range(ov)))
        frames = pipe(**kw)
        out.extend(frames[ov:])
    return out


chain.plan = plan

