"""Video-to-video: start the denoising loop from an input clip instead of pure noise.

Upstream DiffSynth-Studio's ``WanVideoPipeline.__call__(input_video=, denoising_strength=)`` [EXT], restated as remembered (not
read: ORACLE_RISKS.md R22).  With strength s in (0, 1]:
  * ``sigmas = linspace(s, 0, N+1)[:-1]`` then the shift warp: all N steps run over the shortened range (scheduler.py);
  * with an input clip ``x0 = VAE.encode(input_video)`` and ``latent = (1 - sigma_0) * x0 + sigma_0 * noise`` with
    ``sigma_0 = sigmas[0]`` and the CPU-generator noise drawn as always (icv_add_noise_f32, on the device); without one the
    latent is the noise;
  * s == 1 gives sigma_0 == 1 exactly for any shift (shift / (1 + (shift - 1))), so the noised latent IS the noise.
Everything behind the start latent - driver modes, graphs, TeaCache, sliding windows, i2v conditioning - sees a scheduler and a
latent and does not change.  This module holds the host side: settings, validation, and reading ``ICV_INPUT_VIDEO``.
"""

from __future__ import annotations

import os
from typing import List, Optional, Tuple

import numpy as np
from PIL import Image

ENV_VIDEO, ENV_STRENGTH = "ICV_INPUT_VIDEO", "ICV_DENOISING_STRENGTH"
FORMS = "a .npy file of uint8 [N, H, W, 3] frames, or a directory of image files (read in sorted order)"


def _frames_of_array(a: np.ndarray, what: str) -> List[Image.Image]:
    if a.ndim != 4 or a.shape[-1] != 3 or a.dtype != np.uint8:
        raise ValueError(f"{what}: expected uint8 frames [N, H, W, 3], got {a.dtype} {tuple(a.shape)}")
    return [Image.fromarray(a[i], mode="RGB") for i in range(a.shape[0])]


def load_clip(path: str) -> List[Image.Image]:
    """The frames a path stands for: a ``.npy`` of uint8 [N, H, W, 3], or a directory of image files in sorted order.  Any other
    path is handed to ``imageio`` when that package is importable; otherwise it raises, naming the two supported forms."""
    path = os.fspath(path)
    if os.path.isdir(path):
        names = sorted(n for n in os.listdir(path) if os.path.isfile(os.path.join(path, n)))
        if not names:
            raise ValueError(f"{ENV_VIDEO}: directory {path!r} holds no files")
        frames = []
        for n in names:
            try:
                with Image.open(os.path.join(path, n)) as im:
                    frames.append(im.convert("RGB"))
            except OSError as e:
                raise ValueError(f"{ENV_VIDEO}: {os.path.join(path, n)!r} is not an image file ({e})") from None
        return frames
    if path.lower().endswith(".npy"):
        return _frames_of_array(np.load(path, allow_pickle=False), f"{ENV_VIDEO}: {path!r}")
    try:
        import imageio
    except ImportError:
        raise ValueError(f"{ENV_VIDEO}: cannot read {path!r}: supported are {FORMS}; any other file needs the `imageio` "
                         f"package, which is not installed") from None
    return _frames_of_array(np.stack([np.asarray(f)[..., :3] for f in imageio.mimread(path, memtest=False)]).astype(np.uint8, copy=False),
                            f"{ENV_VIDEO}: {path!r}")


def as_frames(video) -> List[Image.Image]:
    """``input_video`` as the caller may give it - a list of PIL images (upstream's form), a uint8 [N, H, W, 3] array, or a path
    (what ICV_INPUT_VIDEO holds) - as a list of PIL images."""
    if isinstance(video, (str, os.PathLike)):
        return load_clip(video)
    if isinstance(video, np.ndarray):
        return _frames_of_array(video, "input_video")
    return list(video)


def validate(video, strength, num_frames: int) -> Tuple[Optional[List[Image.Image]], float]:
    """(frames | None, strength) in effect for one call; raises ValueError before anything is encoded or launched.  No strength
    means 1.0, upstream's default.  A strength below 1 without an input video is refused: upstream would silently denoise pure
    noise over the short range, which no caller wants."""
    s = 1.0 if strength is None else strength
    if isinstance(s, bool) or not isinstance(s, (int, float, np.integer, np.floating)) or not (0.0 < float(s) <= 1.0):
        raise ValueError(f"denoising_strength must be a number in (0, 1], got {strength!r}")
    s = float(s)
    if video is None:
        if s < 1.0:
            raise ValueError(f"denoising_strength={s} needs an input_video ({ENV_VIDEO}): without one the loop would denoise pure "
                             f"noise over a shortened sigma range")
        return None, s
    frames = as_frames(video)
    if len(frames) != num_frames:
        raise ValueError(f"input_video has {len(frames)} frames, num_frames={num_frames}")
    return frames, s
