"""tools/attn_isa_census.py's readers on the staggered long-key kernel of csrc/attn7p.hip, att7p::attn7ps_kernel<UNIT, PRIO, SWAP> (no GPU;
about half a minute of hipcc -S): every instantiation fits its registers - no scratch, at most 256 VGPRs, no AGPRs - and the steady
loop of the unit and the scaled kernel issues per 128 keys what the slim loop's steady interval issues: 128 MFMAs, 64 v_exp_f32,
32 + 64 LDS fragment reads and 8 LDS-DMA requests.  The loop is one program for both wave groups (a group skips the other group's
barrier and request with a scalar branch), so the cheapest walk with 128 MFMAs and 8 requests is one group's way through it."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import attn_isa_census as C  # noqa: E402


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    text = open(C.compile_asm("attn7p", str(tmp_path_factory.mktemp("attn_stagger_isa")))).read()
    res = C.kernel_resources(text)
    names = C.demangle(list(res))
    return text, {names[n]: (n, r) for n, r in res.items() if "attn7ps_kernel" in n}


def test_the_staggered_kernels_fit_their_registers(asm):
    _, kernels = asm
    assert len(kernels) == 8, sorted(kernels)          # UNIT x PRIO x SWAP
    for name, (_, r) in kernels.items():
        assert r["scratch"] == 0 and r["vgpr"] <= 256 and r["agpr"] == 0, f"{name}: {r}"


@pytest.mark.parametrize("unit", ["true", "false"], ids=["unit", "scaled"])
@pytest.mark.parametrize("prio", ["true", "false"], ids=["setprio", "no_setprio"])
@pytest.mark.parametrize("swap", ["true", "false"], ids=["swap", "no_swap"])
def test_the_steady_loop(asm, unit, prio, swap):
    text, kernels = asm
    hits = [m for name, (m, _) in kernels.items() if f"attn7ps_kernel<{unit}, {prio}, {swap}>" in name]
    assert len(hits) == 1, sorted(kernels)
    hot = C.classify(C.hot_path(C.function_blocks(text, hits[0]), any_back_edge=True))
    print(hot)
    needed = {"v_mfma_f32_16x16x32_bf16": 128, "v_exp_f32": 64, "ds_read_b128": 32, "ds_read_b64_tr_b16": 64, "v_cvt_pk_bf16_f32": 32,
              "global_load_lds (DMA)": 8}
    for k, n in needed.items():
        assert hot[k] == n, f"{k}: {hot[k]} in the steady loop, the slim loop's steady interval has {n}"
    assert hot["other v_mfma"] == 0, hot
    if unit == "true":          # the scaled kernel's exponent argument is an fma the compiler may pack; the unit kernel has none
        assert hot["v_pk_*_f32 (packed f32)"] == 0, hot
