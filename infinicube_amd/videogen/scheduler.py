"""Flow-matching Euler sampler used by the Wan2.1 pipeline.

The reference never touches the sampler: ``WanVideoGenerator.generate`` forwards nine kwargs to
``WanVideoPipeline.__call__`` [R infinicube/videogen/inference.py:216-226] and the fork's
defaults apply.  Those defaults are the upstream DiffSynth ones restated in SURVEY.md
Appendix A.5/A.6 ([EXT]): ``FlowMatchScheduler(shift=5, sigma_min=0, extra_one_step=True)``,
50 steps, cfg_scale 5.
"""

from __future__ import annotations

from typing import List


def flow_match_sigmas(num_steps: int, shift: float = 5.0, sigma_max: float = 1.0,
                      sigma_min: float = 0.0, denoising_strength: float = 1.0) -> List[float]:
    """sigma_i for i in [0, num_steps): linspace(start, min, N+1)[:-1] then the shift warp."""
    start = sigma_min + (sigma_max - sigma_min) * denoising_strength
    out = []
    for i in range(num_steps):
        s = start + (sigma_min - start) * (i / num_steps)
        out.append(shift * s / (1.0 + (shift - 1.0) * s))
    return out


def round_through_bf16(x: float) -> float:
    """The float nearest-even-rounded to bfloat16 (8 significant bits): 937.5 -> 936.0."""
    import struct
    (u,) = struct.unpack("<I", struct.pack("<f", x))
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return struct.unpack("<f", struct.pack("<I", u))[0]


class FlowMatchScheduler:
    """``reference_rounding``: the timestep fed to the DiT is 1000 sigma rounded to bfloat16, as a pipeline that casts
    ``timestep.to(torch_dtype)`` before the sinusoidal embedding does ([EXT], ORACLE_RISKS.md R1); the sigmas of the
    Euler update stay exact either way.
    ``denoising_strength`` s in (0, 1] (video-to-video): the SAME number of steps over the range that starts at
    s instead of 1 - ``linspace(s, 0, N+1)[:-1]``, then the shift warp ([EXT], ORACLE_RISKS.md R22).  1.0 = the full range."""

    def __init__(self, num_inference_steps: int = 50, shift: float = 5.0, reference_rounding: bool = False,
                 denoising_strength: float = 1.0):
        self.reference_rounding = reference_rounding
        self.set_timesteps(num_inference_steps, shift, denoising_strength)

    def set_timesteps(self, num_inference_steps: int, shift: float = 5.0, denoising_strength: float = 1.0):
        self.denoising_strength = denoising_strength
        self.sigmas = flow_match_sigmas(num_inference_steps, shift, denoising_strength=denoising_strength)
        self.timesteps = [s * 1000.0 for s in self.sigmas]
        if self.reference_rounding:
            self.timesteps = [round_through_bf16(t) for t in self.timesteps]

    @classmethod
    def from_sigmas(cls, sigmas, reference_rounding: bool = False) -> "FlowMatchScheduler":
        """A scheduler over an explicit sigma list, e.g. the first K sigmas of a call (coarse-to-fine sampling): the
        floats are kept as they are, the timesteps get the same ``reference_rounding``, and the last step goes to 0 as always."""
        sch = cls.__new__(cls)
        sch.reference_rounding = reference_rounding
        sch.denoising_strength = None                     # not a range this class built
        sch.sigmas = [float(s) for s in sigmas]
        if not sch.sigmas:
            raise ValueError("FlowMatchScheduler.from_sigmas: an empty sigma list")
        sch.timesteps = [s * 1000.0 for s in sch.sigmas]
        if reference_rounding:
            sch.timesteps = [round_through_bf16(t) for t in sch.timesteps]
        return sch

    def dsigma(self, i: int) -> float:
        """sigma_{i+1} - sigma_i with sigma_N = 0 (the Euler step multiplier)."""
        nxt = self.sigmas[i + 1] if i + 1 < len(self.sigmas) else 0.0
        return nxt - self.sigmas[i]
