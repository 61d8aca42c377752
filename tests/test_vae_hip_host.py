"""Host logic of the padded-volume VAE executor (infinicube_amd/videogen/vae_hip.py) WITHOUT the GPU: the two libicvideo kernels
are replaced by torch restatements of their CONTRACT (include/icvideo.h: icv_conv3d_ndhwc = out[m] = bias + sum_i x[m + off_i] W_i^T
(+ resid[m]) over a row range with garbage on the halo; icv_rmsnorm_act_volume = norm on the interior, zeros on the padding), so what
is checked here is everything the Python side owns: tap tables and row offsets, the weight re-layout (tap-major, padded channels /
filters / K), row ranges and margins, which volumes need their halo zeroed, the stride-2 / upsampling / temporal-interleave
index arithmetic, the attention block's gather, and the 1x1x1 head / latent convolutions — against the stock fp32 network.
Every new volume is poisoned with NaNs first: a halo or margin read that reaches a real output turns the result non-finite."""
import copy

import pytest
import torch

from infinicube_amd.videogen import vae as V
from infinicube_amd.videogen import vae_hip as VH
from vae_trace import HostVaeHip


@pytest.fixture(scope="module")
def tiny():
    torch.manual_seed(4)
    ref = V.WanVAENet(dim=32, z_dim=16).eval()
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(p.to(torch.bfloat16).float())
    return ref


@pytest.fixture()
def poisoned(monkeypatch):
    monkeypatch.setattr(VH.Vol, "POISON", True)


def _close(got, ref, what, bound=2e-2):
    assert torch.isfinite(got.float()).all(), f"{what}: a halo / margin / padding value reached a real output"
    rel = float((got.float() - ref).norm() / ref.norm())
    assert rel <= bound, f"{what}: rel-L2 {rel}"


def test_decoder_host_logic(tiny, poisoned):
    hip = HostVaeHip(copy.deepcopy(tiny).to(torch.bfloat16))
    z = torch.randn(1, 16, 3, 5, 6).to(torch.bfloat16)
    with torch.no_grad():
        got, ref = hip.decode_tile(z), tiny.decode(z.float())
    assert got.shape == ref.shape == (1, 3, 9, 40, 48)
    _close(got, ref, "decoder")


def test_encoder_host_logic(tiny, poisoned):
    hip = HostVaeHip(copy.deepcopy(tiny).to(torch.bfloat16))
    x = (torch.rand(1, 3, 9, 16, 32) * 2 - 1).to(torch.bfloat16)
    with torch.no_grad():
        got, ref = hip.encode_tile(x), tiny.encode(x.float())
    assert got.shape == ref.shape == (1, 16, 3, 2, 4)
    _close(got, ref, "encoder")


@pytest.mark.parametrize("frames", [1, 5])
def test_single_frame_and_short_clips(tiny, poisoned, frames):
    """T = 1 takes the branches without temporal resampling (the reference's first-frame special cases)."""
    hip = HostVaeHip(copy.deepcopy(tiny).to(torch.bfloat16))
    x = (torch.rand(1, 3, frames, 16, 16) * 2 - 1).to(torch.bfloat16)
    with torch.no_grad():
        _close(hip.encode_tile(x), tiny.encode(x.float()), f"encoder, {frames} frame(s)")
    z = torch.randn(1, 16, (frames - 1) // 4 + 1, 2, 2).to(torch.bfloat16)
    with torch.no_grad():
        _close(hip.decode_tile(z), tiny.decode(z.float()), f"decoder, {frames} frame(s)")


def test_weight_layout_and_tap_offsets():
    mod = V.CausalConv3d(48, 10, 3, padding=1)
    rec = VH._ConvW(mod, "cpu", VH.TAPS_333, 48)
    assert (rec.cin, rec.cout, rec.cout_real) == (64, 12, 10) and rec.w.shape == (12, 27 * 64) and rec.bias.shape == (12,)
    w = rec.w.float().view(12, 27, 64)
    ref = mod.weight.detach().to(torch.bfloat16).float()
    assert torch.equal(w[:10, :, :48], ref.reshape(10, 48, 27).permute(0, 2, 1)) and float(w[10:].abs().sum()) == 0 and float(w[:, :, 48:].abs().sum()) == 0
    offs = list(rec.offsets(9, 11))
    assert offs[0] == (-2 * 9 - 1) * 11 - 1 and offs[13] == (-1 * 9 + 0) * 11 + 0 and offs[26] == (0 * 9 + 1) * 11 + 1
    odd = VH._ConvW(V.CausalConv3d(96, 96, (3, 1, 1), padding=(1, 0, 0)), "cpu", VH.TAPS_311, 96)
    assert odd.w.shape == (96, 320), "3 taps x 96 channels = 288 -> K padded to whole 64-wide tiles"
