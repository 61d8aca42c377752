"""What makes tests/test_vae_widths_gpu.py trustworthy, without a GPU: the per-call fp64 references, bars and layout checks of
tests/vae_trace.py, run with ``Vol.POISON`` on over the torch restatement of the kernel contract (``HostVaeHip``).

  * every case of the GPU file passes every check for this correct executor - the references, the tap order read from the modules'
    own weights, the per-op bars and the layout checks are right;
  * every wrong executor of ``vae_trace.MUTANTS`` is rejected, by the check named next to it here - the checks can see a halo that is
    not zeroed, a swapped or mis-placed frame, a dropped tap or residual, mixed-up channel halves, a write before ``first_frame``,
    a norm that leaves garbage on the halo or skips its activation."""
import pytest
import torch
import torch.nn as nn

import vae_trace as VT
from infinicube_amd.videogen import vae_hip as VH

HOST = VT.recording(VT.HostVaeHip)


@pytest.fixture(autouse=True)
def poisoned(monkeypatch):
    monkeypatch.setattr(VH.Vol, "POISON", True)


@pytest.mark.parametrize("case", VT.CONV_CASES, ids=VT.conv_case_id)
def test_conv_checks_pass_for_the_restated_kernel(case):
    assert VT.run_conv_case(HOST, "cpu", case) <= 1.0


@pytest.mark.parametrize("case", VT.BLOCK_CASES, ids=VT.block_case_id)
def test_block_checks_pass_for_the_restated_kernel(case):
    figs = VT.run_block_case(HOST, "cpu", case)
    print(VT.block_case_id(case), figs)
    assert figs["d"] == 0.0, "the same executor on the same input"
    # e_host is nothing but the bf16 rounding points of a block: a few 1e-3 (the attention block adds its residual in fp32: less)
    assert 1e-4 < figs["e_host"] < 5e-3, figs


@pytest.mark.parametrize("case", VT.NET_CASES, ids=VT.net_case_id)
def test_network_checks_pass_for_the_restated_kernel(case):
    figs = VT.run_net_case(HOST, "cpu", case)
    print(VT.net_case_id(case), figs)
    assert figs["calls"] > 40


def test_recorded_output_is_what_the_call_left():
    """upsample zeroes frame 0 of the volume it is handed AFTER the call that produced it was recorded: the record keeps its own copy."""
    hip = HOST(nn.Identity(), "cpu")
    mod = VT._randomise(VT.CONV_KINDS["111"][0](32, 32))
    out = hip.conv(hip._to_vol(torch.randn(1, 32, 2, 3, 3).to(torch.bfloat16), 32), mod, VH.TAPS_111)
    out.vol()[VH.PT].zero_()
    VT.check_record(hip.records[0])
    assert hip.records[0].x.shape == (2, 3, 3, 32) and float(hip.records[0].out.interior()[0].abs().max()) > 0


# mutant -> the case that must reject it and the check that must fire there
CONV = {VT.conv_case_id(c): c for c in VT.CONV_CASES}
BLOCK = {VT.block_case_id(c): c for c in VT.BLOCK_CASES}
KILLS = [
    ("zero_halo does nothing", BLOCK["upsample2d-192-2x4x6"], "conv.finite"),
    ("zero_halo does nothing", BLOCK["downsample3d-192-3x8x12"], "conv.finite"),
    ("upsample swaps the two interleaved frames", BLOCK["upsample3d-384-2x4x6"], "block.d"),
    ("upsample swaps the two interleaved frames", BLOCK["upsample3d-384-3x4x6"], "block.d"),
    ("downsample takes the odd positions", BLOCK["downsample2d-96-2x8x12"], "block.d"),
    ("conv drops the last tap", CONV["311-96to96"], "conv.value"),
    ("conv drops the last tap", CONV["333-384to384"], "conv.value"),
    ("conv ignores resid", CONV["333-384to384-resid"], "conv.value"),
    ("conv ignores resid", BLOCK["res_block-96to96-3x6x10"], "conv.value"),
    ("conv swaps the first two 32-channel halves of every tap", CONV["311-96to96"], "conv.value"),
    ("conv swaps the first two 32-channel halves of every tap", CONV["111-384to1152"], "conv.value"),
    ("conv writes frame first_frame - 1", CONV["311-192to192-from1"], "conv.untouched"),
    ("conv writes frame first_frame - 1", CONV["311-192to192-from2"], "conv.untouched"),
    ("conv writes frame first_frame - 1", CONV["111-32to96"], "conv.padding"),
    ("norm_act copies the input onto the halo", BLOCK["res_block-96to96-3x6x10"], "norm.layout"),
    ("norm_act skips SiLU", BLOCK["res_block-192to384-3x6x10"], "norm.value"),
]


def test_every_mutant_has_a_kill():
    assert {k[0] for k in KILLS} == set(VT.MUTANTS)


@pytest.mark.parametrize("name,case,check", KILLS, ids=[f"{n} | {c[0]}-{c[1]} | {k}" for n, c, k in KILLS])
def test_mutant_is_rejected(name, case, check):
    run = VT.run_block_case if case in VT.BLOCK_CASES else VT.run_conv_case
    if run is VT.run_block_case:
        VT.block_setup(case)          # the references come from the unpatched executor
    with VT.mutant(name):
        with pytest.raises(VT.CheckError) as err:
            run(HOST, "cpu", case)
    print(f"{name}: rejected by {err.value}")
    assert err.value.check == check, f"{name}: expected {check} to fire, got {err.value}"
    run(HOST, "cpu", case)          # and the patch is gone again
