"""The Wan-VAE's HIP path (vae_hip.VaeHip on icv_conv3d_ndhwc / icv_rmsnorm_act_volume) at the widths of the SHIPPED network
(dim = 96: 96 / 192 / 384 channels, a 768-wide time_conv, a 1152-wide to_qkv, 3x3x3 convolutions over 384 inputs), checked call by
call: every kernel call is recorded and compared with an fp64 reference of that one call computed from the interior of its input
(tests/vae_trace.py; tests/test_vae_trace_cpu.py shows that these checks reject every mutant executor).  ``Vol.POISON`` is on, so
whatever a kernel reads from a halo, margin or padding row that nobody wrote is a NaN, and what it must not write stays one.

Shapes: the smallest that still span two 256-row tiles with a ragged tail (385 padded rows for the single convolutions).

Blocks: with e_host = rel-L2(HostVaeHip on the CPU, stock fp32 module) and d = rel-L2(GPU, HostVaeHip), d <= e_host - both executors
round at the same points and can differ only where fp32 summation order or __expf flips one of those roundings; the attention block
(stock SDPA on either side) is held to rel-L2(GPU, fp32) <= 2 e_host.

Measured on an MI355X (printed per case by the tests; all 32 cases pass, 8.5 s together):
  * single convolutions: largest error 0.32 .. 0.44 of the per-op bar (one bf16 rounding is at most 0.5 of it);
  * blocks without attention: e_host 1.65e-3 .. 2.56e-3, d 0 .. 1.6e-4; largest d / e_host = 0.085 (res_block 384 -> 384:
    d 1.58e-4, e_host 1.84e-3), then 0.045 / 0.044 (res_block 96 -> 192, 192 -> 384), <= 0.033 for the resamplers;
  * attn_block 384: rel-L2(GPU, fp32) 3.84e-3 against e_host 3.87e-3 (bound 7.73e-3); d = 1.21e-3;
  * tile networks, rel-L2 / cosine vs fp32: decode 2x3x4 1.43e-2 / 0.999898 (68 calls), decode 1x2x2 1.49e-2 / 0.999889 (66),
    encode 5x16x24 3.73e-3 / 0.999993 (53), encode 1x8x8 3.81e-3 / 0.999995 (51); HostVaeHip on the CPU: 1.45e-2, 1.61e-2, 4.02e-3,
    3.79e-3.  Every call inside its bar (convolutions <= 0.44 of it, norms <= 0.996: the norm's bar IS one bf16 rounding).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import vae_trace as VT  # noqa: E402
from infinicube_amd.videogen import vae_hip as VH  # noqa: E402

GPU = VT.recording(VH.VaeHip)


@pytest.fixture(autouse=True)
def poisoned(monkeypatch):
    monkeypatch.setattr(VH.Vol, "POISON", True)


def _w(figs):
    return ", ".join(f"{op} {v:.3f}" for op, v in sorted(figs["worst_call"].items()))


def _dev():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch.device("cuda", 0)


@pytest.mark.parametrize("case", VT.CONV_CASES, ids=VT.conv_case_id)
def test_conv_geometries_of_the_shipped_widths(case):
    """One convolution per geometry that only dim = 96 has: every N-tile count and dispatch branch, 162 K-tiles, a padded last
    K-tile half, padded input channels and filters, row ranges that start at frame 1 / 2."""
    worst = VT.run_conv_case(GPU, _dev(), case)
    print(f"{VT.conv_case_id(case)}: largest error {worst:.3f} of the per-op bar")


@pytest.mark.parametrize("case", VT.BLOCK_CASES, ids=VT.block_case_id)
def test_blocks_at_the_shipped_widths(case):
    figs = VT.run_block_case(GPU, _dev(), case)
    print(f"{VT.block_case_id(case)}: {figs['calls']} calls, worst call / bar {_w(figs)}, d {figs['d']:.3g}, e_host {figs['e_host']:.3g}, "
          f"d / e_host {figs['d'] / figs['e_host']:.3f}, rel-L2 vs fp32 {figs['e']:.3g}")


@pytest.mark.parametrize("case", VT.NET_CASES, ids=VT.net_case_id)
def test_tile_networks_of_the_shipped_vae_call_by_call(case):
    figs = VT.run_net_case(GPU, _dev(), case)
    print(f"{VT.net_case_id(case)}: {figs['calls']} calls, worst call / bar {_w(figs)}, rel-L2 vs fp32 {figs['rel']:.3g}, cosine {figs['cos']:.6f}")
