"""tools/attn_isa_census.py on the slim key loop of csrc/attn7p.hip (no GPU; about half a minute of hipcc -S): the steady interval of
att7p::attn7p_kernel<true, false, 16, SLIM = true, LEAN = true> issues what the softmax needs and no more of it than the lean loop's
hot path - the same 128 MFMAs, 32 + 64 LDS reads, 64 exponentials, 32 conversions and 8 LDS-DMA requests per 128 keys, no more VALU
instructions - and strictly less of what it was written to remove: scalar instructions, branches and s_nop.  "Other SALU" falls by
at least 16, the eight save-and-restore pairs of M0: the one reduction that follows from the source alone; the measured census is in
profiles/attn_slim_loop/isa_census.txt."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import attn_isa_census as C  # noqa: E402


@pytest.fixture(scope="module")
def census(tmp_path_factory):
    return C.census(str(tmp_path_factory.mktemp("attn_slim_isa")))


def test_the_slim_hot_path(census):
    lean, slim = census["hot"]["lean"], census["hot"]["slim"]
    print({k: (lean[k], slim[k]) for k in lean})
    needed = {"v_mfma_f32_16x16x32_bf16": 128, "ds_read_b128": 32, "ds_read_b64_tr_b16": 64, "v_exp_f32": 64, "v_cvt_pk_bf16_f32": 32,
              "global_load_lds (DMA)": 8}
    for k, n in needed.items():
        assert lean[k] == n and slim[k] == n, f"{k}: lean {lean[k]}, slim {slim[k]}, the arithmetic needs {n}"
    assert slim["VALU total (v_* without MFMA)"] <= lean["VALU total (v_* without MFMA)"], (slim, lean)
    for k in ("other SALU", "branches", "s_nop"):
        assert slim[k] < lean[k], f"{k}: slim {slim[k]}, lean {lean[k]}"
    assert slim["other SALU"] <= lean["other SALU"] - 16, (slim["other SALU"], lean["other SALU"])


def test_the_slim_kernels_fit_their_registers(census):
    """Both SLIM instantiations are there, are counted as lean kernels by name (SLIM stands in front of LEAN) and do not spill."""
    slim = {n: r for n, r in census["resources"]["attn7p"].items() if "attn7p_kernel<" in n and n.split(">(")[0].endswith("16, true, true")}
    assert len(slim) == 2, sorted(slim)
    for n, r in slim.items():
        assert r["scratch"] == 0 and r["vgpr"] <= 256 and r["agpr"] == 0, f"{n}: {r}"


def test_the_walk_finds_a_loop_closed_by_an_unconditional_branch():
    """The steady loop's shape in miniature: a cold block in front of the header, entered by a conditional branch from the loop's end;
    the hot way round closes with an s_branch to the block behind it and falls into the header."""
    text = """
_Z1kv:
; %bb.0:
	s_branch .LBB0_3
.LBB0_1:
	v_pk_mul_f32 v[0:1], v[0:1], v[2:3]
	v_pk_mul_f32 v[4:5], v[4:5], v[2:3]
.LBB0_2:
	s_cmp_le_i32 s0, s1
	s_cbranch_scc0 .LBB0_4
.LBB0_3:
	global_load_lds_dwordx4 v1, s[0:1]
	v_mfma_f32_16x16x32_bf16 v[0:3], v[4:7], v[8:11], v[0:3]
	s_cbranch_vccnz .LBB0_1
	s_branch .LBB0_2
.LBB0_4:
	s_endpgm
.Lfunc_end0:
"""
    blocks = C.function_blocks(text, "_Z1kv")
    old = C.N_MFMA, C.N_DMA
    try:
        C.N_MFMA, C.N_DMA = 1, 1
        hot = C.hot_path(blocks, any_back_edge=True)
        cold = C.hot_path(blocks)
    finally:
        C.N_MFMA, C.N_DMA = old
    assert [x.split()[0] for x in hot] == ["s_cmp_le_i32", "s_cbranch_scc0", "global_load_lds_dwordx4", "v_mfma_f32_16x16x32_bf16",
                                           "s_cbranch_vccnz", "s_branch"]
    assert len(cold) == len(hot) + 1 and C.classify(cold)["v_pk_*_f32 (packed f32)"] == 2
