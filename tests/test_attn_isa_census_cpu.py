"""tools/attn_isa_census.py on the attention sources as they are (no GPU; about a minute of hipcc -S): every instantiation of
attn7.hip / attn7p.hip fits its registers - no scratch, at most 256 VGPRs (amdgpu_waves_per_eu(2): the accumulators of a kernel that
spills go through memory in the key loop) - and the lean body of the 16x16x32 tile keeps what it was written for: no packed f32 VALU
in the hot path of the default long-key kernel, fewer VALU instructions there than under the first body, and the same MFMAs, LDS
reads, exponentials and conversions as the first body (the arithmetic the softmax needs: 128 / 32 + 64 / 64 / 32 per 128 keys)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import attn_isa_census as C  # noqa: E402


@pytest.fixture(scope="module")
def census(tmp_path_factory):
    return C.census(str(tmp_path_factory.mktemp("attn_isa")))


def test_no_attention_instantiation_spills(census):
    bad, n = [], 0
    for src, kernels in census["resources"].items():
        for name, r in kernels.items():
            if "attn7" not in name:
                continue
            n += 1
            if r["scratch"] != 0 or r["vgpr"] > 256 or r["agpr"] != 0:
                bad.append(f"{src}: {name}: {r}")
    lean = [k for ks in census["resources"].values() for k in ks if "attn7" in k and k.split(">(")[0].endswith("true")]
    assert n >= 60 and len(lean) >= 20, f"{n} attention kernels, {len(lean)} of them with the lean body: instantiations are missing"
    assert not bad, "\n".join(bad)


def test_the_lean_hot_path(census):
    first, lean = census["hot"]["first"], census["hot"]["lean"]
    needed = {"v_mfma_f32_16x16x32_bf16": 128, "ds_read_b128": 32, "ds_read_b64_tr_b16": 64, "v_exp_f32": 64, "v_cvt_pk_bf16_f32": 32,
              "global_load_lds (DMA)": 8}
    for k, n in needed.items():
        assert first[k] == n and lean[k] == n, f"{k}: first {first[k]}, lean {lean[k]}, the arithmetic needs {n}"
    assert lean["v_pk_*_f32 (packed f32)"] == 0
    assert lean["VALU total (v_* without MFMA)"] < first["VALU total (v_* without MFMA)"], (lean, first)
    # the count above moves little (a packed add counts once); what the lean body is for shows in these
    assert lean["s_nop"] < first["s_nop"], (lean, first)
    assert lean["integer VALU (v_add_u32, shifts, logic ...)"] < first["integer VALU (v_add_u32, shifts, logic ...)"], (lean, first)
    assert lean["v_cmp / v_cndmask"] < first["v_cmp / v_cndmask"], (lean, first)


def test_the_parser_on_a_known_fragment():
    text = """
_Z1kv:
; %bb.0:
	s_load_dword s0, s[4:5], 0x0
.LBB0_1:                                ; =>This Inner Loop Header: Depth=1
	v_mfma_f32_16x16x32_bf16 v[0:3], v[4:7], v[8:11], v[0:3]
	s_cbranch_scc1 .LBB0_3
; %bb.2:
	v_pk_mul_f32 v[0:1], v[0:1], v[2:3]
.LBB0_3:
	global_load_lds_dwordx4 v1, s[0:1]
	v_add_u32_e32 v1, s0, v1
	s_cbranch_vccnz .LBB0_1
; %bb.4:
	s_endpgm
.Lfunc_end0:
amdhsa.kernels:
  - .agpr_count:     0
    .name:           _Z1kv
    .private_segment_fixed_size: 8
    .vgpr_count:     12
"""
    assert C.kernel_resources(text) == {"_Z1kv": {"vgpr": 12, "agpr": 0, "scratch": 8, "lds": 0}}
    blocks = C.function_blocks(text, "_Z1kv")
    old = C.N_MFMA, C.N_DMA
    try:
        C.N_MFMA, C.N_DMA = 1, 1
        hot = C.hot_path(blocks)
    finally:
        C.N_MFMA, C.N_DMA = old
    assert [x.split()[0] for x in hot] == ["v_mfma_f32_16x16x32_bf16", "s_cbranch_scc1", "global_load_lds_dwordx4", "v_add_u32_e32", "s_cbranch_vccnz"]
    c = C.classify(hot)
    assert c["VALU total (v_* without MFMA)"] == 1 and c["v_pk_*_f32 (packed f32)"] == 0 and c["branches"] == 2
