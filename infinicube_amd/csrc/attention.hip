// Attention entry points of the C ABI (include/icvideo.h) and the kernel-family routing.
//   7 = attn7.hip (default: LDS-DMA ring + lazy max + unit scale), 2 = attn2.hip (the previous default, register-staged
//   128-key tile).  Families 1, 3, 4, 5, 6, 9 are measured-slower (or tying) experiments kept for A/B under experiments/; they are
//   compiled in only when the library is built with ICV_EXPERIMENTS=1 (csrc/build.sh) and otherwise report an error.
#include "icv_common.h"


int icv_attn1_dispatch(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o,
                       int64_t ldo, int64_t Sq, int64_t Skv, int64_t heads, float scale, void* stream);
int icv_attn2_dispatch(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                       void* o, int64_t ldo, float* acc, int64_t ldacc, float* ml, int state_in,
                       int state_out, int64_t Sq, int64_t Skv, int64_t heads, float scale, int var,
                       hipStream_t st);

int icv_attn3_dispatch(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                       void* o, int64_t ldo, float* acc, int64_t ldacc, float* ml, int state_in,
                       int state_out, int64_t Sq, int64_t Skv, int64_t heads, float scale, int var,
                       hipStream_t st);

int icv_attn9_dispatch(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                       void* o, int64_t ldo, float* acc, int64_t ldacc, float* ml, int state_in,
                       int state_out, int64_t Sq, int64_t Skv, int64_t heads, float scale, int var,
                       hipStream_t st);
int icv_attn7p_single(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o, int64_t ldo, float* acc,
                      int64_t ldacc, float* ml, int state_in, int state_out, int64_t Sq, int64_t Skv, int64_t heads, float scale, hipStream_t st);
int icv_attn7q_single(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o, int64_t ldo, float* acc,
                      int64_t ldacc, float* ml, int state_in, int state_out, int64_t Sq, int64_t Skv, int64_t heads, float scale, int variant,
                      hipStream_t st);
int icv_attn7_dispatch(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                       void* o, int64_t ldo, float* acc, int64_t ldacc, float* ml, int state_in,
                       int state_out, int64_t Sq, int64_t Skv, int64_t heads, float scale, int var,
                       hipStream_t st);
int icv_attn6_dispatch(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                       void* o, int64_t ldo, float* acc, int64_t ldacc, float* ml, int state_in,
                       int state_out, int64_t Sq, int64_t Skv, int64_t heads, float scale, int var,
                       hipStream_t st);
int icv_attn5_dispatch(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                       void* o, int64_t ldo, float* acc, int64_t ldacc, float* ml, int state_in,
                       int state_out, int64_t Sq, int64_t Skv, int64_t heads, float scale, int var,
                       hipStream_t st);
int icv_attn4_dispatch(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                       void* o, int64_t ldo, float* acc, int64_t ldacc, float* ml, int state_in,
                       int state_out, int64_t Sq, int64_t Skv, int64_t heads, float scale, int var,
                       hipStream_t st);

// Kernel family selection (icv_set_option("attn_kernel", n)): 7 = attn7.hip (default: LDS-DMA ring + lazy max + unit
// scale), 2 = attn2.hip, 3..6 = the experiments kept for A/B, 1 = experiments/attn1.hip (icv_attention_fwd only).
constexpr int ATTN_KERNEL_DEFAULT = 7;
constexpr int ATTN7_VARIANT_DEFAULT = 132;
constexpr int ATTN7Q_DEFAULT = 0;
static int attn_route(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o,
                      int64_t ldo, float* acc, int64_t ldacc, float* ml, int state_in, int state_out, int64_t Sq,
                      int64_t Skv, int64_t heads, float scale, hipStream_t st) {
#define ATT_ARGS q, ldq, k, ldk, v, ldv, o, ldo, acc, ldacc, ml, state_in, state_out, Sq, Skv, heads, scale
  switch (icv_get_option_int("attn_kernel", ATTN_KERNEL_DEFAULT)) {
    case 7: {
      // default variant 132 = 128-key publish (one vmcnt(0) + barrier per TWO key tiles) + s_setprio around the MFMA
      // clusters: +1.4 % on the 37 440-key self-attention of both model sizes, neutral on the sequence-parallel shard
      // shapes (same-process A/B, profiles/r03/attention_variants.md); a negative option value = this default
      const int var7 = icv_get_option_int("attn7_variant", -1);
      // round 6: the default long-key launch (self-attention, plain or carried-state chunk) runs as ONE piece of the pieces kernel
      // (csrc/attn7p.hip: attn7's variant-132 schedule, bit-identical, 1.5-2.7 % faster at the 14B shapes); an explicit attn7_variant,
      // attn7_plain = 1 (A/B), the ablation switches and the short-key shape (cross-attention) keep attn7.hip
      int short_max = icv_get_option_int("attn7_short", -1);
      if (short_max < 0) short_max = 1024;
      if (var7 < 0 && Skv > short_max && !icv_get_option_int("attn7_plain", 0) && !icv_get_option_int("attn7_ablate", 0) && state_out != 2) {
#ifdef ICV_EXPERIMENTS
        // experiments/attn7q.hip: attn8's software-pipelined loop on the bf16 MFMA (1 / 2 = fragment prefetch distance).  Measured SLOWER than
        // attn7p (1133 vs 1196 TF/s): same MFMA busy (0.58 vs 0.59), 43 % more vector instructions, lower sustained clock (1.89 vs 1.94 GHz) -
        // the bf16 attention sits on the power limit, not on its schedule (profiles/r06/attn7q_pipelined_bf16_negative.txt)
        const int q7 = icv_get_option_int("attn7q", ATTN7Q_DEFAULT);
        if (q7 > 0) {
          const int rc = icv_attn7q_single(ATT_ARGS, q7, st);
          if (rc >= 0) return rc;
        }
#endif
        return icv_attn7p_single(ATT_ARGS, st);
      }
      return icv_attn7_dispatch(ATT_ARGS, var7 < 0 ? ATTN7_VARIANT_DEFAULT : var7, st);
    }
#ifdef ICV_EXPERIMENTS
    case 9: return icv_attn9_dispatch(ATT_ARGS, icv_get_option_int("attn9_variant", 0), st);
    case 6: return icv_attn6_dispatch(ATT_ARGS, icv_get_option_int("attn6_variant", 5), st);
    case 5: return icv_attn5_dispatch(ATT_ARGS, 0, st);
    case 4: return icv_attn4_dispatch(ATT_ARGS, icv_get_option_int("attn4_variant", 4), st);
    case 3: return icv_attn3_dispatch(ATT_ARGS, icv_get_option_int("attn3_variant", 0), st);
#else
    case 9: case 6: case 5: case 4: case 3:
      icv_set_error("attn_kernel 3..6 and 9 are experiments: rebuild libicvideo with ICV_EXPERIMENTS=1");
      return 1;
#endif
    default: return icv_attn2_dispatch(ATT_ARGS, icv_get_option_int("attn2_variant", 12), st);
  }
#undef ATT_ARGS
}

extern "C" int icv_attention_fwd_chunk(const void* q, int64_t ldq, const void* k, int64_t ldk,
                                       const void* v, int64_t ldv, void* o, int64_t ldo, float* acc,
                                       int64_t ldacc, float* ml, int64_t Sq, int64_t Skv,
                                       int64_t heads, float scale, int first, int last, void* stream) {
  ICV_REQUIRE(q && k && v, "icv_attention_fwd_chunk: null pointer");
  ICV_REQUIRE(Sq > 0 && Skv > 0 && heads > 0, "icv_attention_fwd_chunk: empty problem");
  ICV_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0, "icv_attention_fwd_chunk: leading dims must keep 16-byte row alignment");
  ICV_REQUIRE((first && last) || (acc && ml && ldacc % 4 == 0), "icv_attention_fwd_chunk: carried state buffers required unless first && last");
  ICV_REQUIRE(!last || (o && ldo % 4 == 0), "icv_attention_fwd_chunk: output required for the last chunk");
  return attn_route(q, ldq, k, ldk, v, ldv, o, ldo, acc, ldacc, ml, first ? 0 : 1, last ? 0 : 1, Sq, Skv, heads, scale, (hipStream_t)stream);
}

extern "C" int icv_attention_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk,
                                 const void* v, int64_t ldv, void* o, int64_t ldo, int64_t Sq,
                                 int64_t Skv, int64_t heads, float scale, void* stream) {
  ICV_REQUIRE(q && k && v && o, "icv_attention_fwd: null pointer");
  ICV_REQUIRE(Sq > 0 && Skv > 0 && heads > 0, "icv_attention_fwd: empty problem (Sq=%lld Skv=%lld heads=%lld)", (long long)Sq, (long long)Skv, (long long)heads);
  ICV_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 4 == 0, "icv_attention_fwd: leading dims must keep 16-byte row alignment");
  if (icv_get_option_int("attn_kernel", ATTN_KERNEL_DEFAULT) != 1)
    return attn_route(q, ldq, k, ldk, v, ldv, o, ldo, nullptr, 0, nullptr, 0, 0, Sq, Skv, heads, scale, (hipStream_t)stream);
#ifdef ICV_EXPERIMENTS
  return icv_attn1_dispatch(q, ldq, k, ldk, v, ldv, o, ldo, Sq, Skv, heads, scale, stream);
#else
  icv_set_error("attn_kernel 1 is an experiment: rebuild libicvideo with ICV_EXPERIMENTS=1");
  return 1;
#endif
}

extern "C" int icv_attention_fwd_add(const void* q, int64_t ldq, const void* k, int64_t ldk,
                                     const void* v, int64_t ldv, void* o, int64_t ldo, int64_t Sq,
                                     int64_t Skv, int64_t heads, float scale, void* stream) {
  ICV_REQUIRE(q && k && v && o, "icv_attention_fwd_add: null pointer");
  ICV_REQUIRE(Sq > 0 && Skv > 0 && heads > 0, "icv_attention_fwd_add: empty problem (Sq=%lld Skv=%lld heads=%lld)", (long long)Sq, (long long)Skv, (long long)heads);
  ICV_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 4 == 0, "icv_attention_fwd_add: leading dims must keep 16-byte row alignment");
  return attn_route(q, ldq, k, ldk, v, ldv, o, ldo, nullptr, 0, nullptr, 0, 2, Sq, Skv, heads, scale, (hipStream_t)stream);
}

// MFMA shape of the bf16 kernels attn7.hip and attn7p.hip (icv_set_option("attn_mfma", n)): 32 = v_mfma_f32_32x32x16_bf16, 16 =
// v_mfma_f32_16x16x32_bf16 at the same wave tile; a negative value = the default.  The two kernels read it HERE, so the long-key
// launches (attn7p and attn7's 8-wave kernel, pinned to each other bit for bit by tests/test_attn_pieces_gpu.py) always agree.  The
// short-key shape of attn7.hip (cross-attention) has a default of its own; an explicit value applies to it as well.
// Defaults: 16 for both - every round of the 16 arm beat every round of the 32 arm at the 14B self-attention (22.60 vs 23.17 ms), its two
// shard shapes and the 512-key cross-attention (interleaved in one process, tools/attn_mfma_ab.py; profiles/attn_mfma16/README.md).
constexpr int ATTN_MFMA_DEFAULT = 16;
constexpr int ATTN_MFMA_SHORT_DEFAULT = 16;
int icv_attn_mfma(bool short_kv) {
  const int v = icv_get_option_int("attn_mfma", -1);
  if (v < 0) return short_kv ? ATTN_MFMA_SHORT_DEFAULT : ATTN_MFMA_DEFAULT;
  if (v == 16 || v == 32) return v;
  icv_set_error("attn_mfma = %d: the MFMA shape is 16 (16x16x32) or 32 (32x32x16); negative = the default", v);
  return -1;
}

// Body of the MF = 16 tile attc::tile16 (icv_set_option("attn_tile16_lean", n)): 1 = the lean body (K / V fragment addresses formed once per
// work-group and moved with the ring, scalar row sums, the "no reference yet" test folded into the lazy-max limit), 0 = the first body,
// negative = the default.  Same arithmetic in the same order: outputs and carried state are bit-identical (tests/test_attn_lean_tile_gpu.py).
// Read HERE by attn7.hip and attn7p.hip, so the long-key launches always agree; the short-key shape has a default of its own.
// Defaults: 1 for both - every round of the lean arm beat every round of the first body's at the 14B self-attention (22.13 vs 23.29 ms),
// its two shard shapes and the 512-key cross-attention (interleaved in one process, tools/attn_lean_ab.py; profiles/attn_lean_tile/README.md).
constexpr int ATTN_TILE16_LEAN_DEFAULT = 1;
constexpr int ATTN_TILE16_LEAN_SHORT_DEFAULT = 1;
int icv_attn_tile16_lean(bool short_kv) {
  const int v = icv_get_option_int("attn_tile16_lean", -1);
  if (v < 0) return short_kv ? ATTN_TILE16_LEAN_SHORT_DEFAULT : ATTN_TILE16_LEAN_DEFAULT;
  if (v == 0 || v == 1) return v;
  icv_set_error("attn_tile16_lean = %d: 1 = the lean body of the 16x16x32 tile, 0 = the first body; negative = the default", v);
  return -1;
}

// Form of attn7p.hip's key loop around the lean body (icv_set_option("attn7p_slim", n)): 1 = the slim loop (steady intervals without the
// loop-control tests, their DMA requests from running tile pointers with one M0 write per K or V pair), 0 = the one loop, negative = the
// default.  Same tiles and requests in the same order: outputs and carried state are bit-identical (tests/test_attn_slim_loop_gpu.py).
// It applies where the lean body runs (attn_mfma = 16, attn_tile16_lean = 1), to the pieces, chunk and plain launches of attn7p.hip.
// Default: 1 - every round of the slim arm beat every round of the one loop's at the 14B self-attention (23.27 vs 24.34 ms) and its two
// shard shapes (interleaved in one process, tools/attn_slim_ab.py; profiles/attn_slim_loop/README.md).
constexpr int ATTN7P_SLIM_DEFAULT = 1;
int icv_attn7p_slim() {
  const int v = icv_get_option_int("attn7p_slim", -1);
  if (v < 0) return ATTN7P_SLIM_DEFAULT;
  if (v == 0 || v == 1) return v;
  icv_set_error("attn7p_slim = %d: 1 = the slim key loop of attn7p, 0 = the one loop; negative = the default", v);
  return -1;
}

// attn7p.hip's staggered long-key kernel (icv_set_option("attn7p_stagger", n)): 1 = a launch that takes the slim loop with ONE piece
// whose rows are there when it starts (the plain launch and the carried-state chunk launches on long keys, a one-piece pieces launch
// without a flag) runs att7p::attn7ps_kernel - the two waves of a SIMD in opposite phases of the tile, one barrier per 64 keys; 0 = the
// slim loop; negative = the default.  Same arithmetic in the same order per wave: outputs and carried state are bit-identical
// (tests/test_attn_stagger_gpu.py).  Multi-piece and flagged launches, the frame-windowed and radial kernels are not touched by it.
// Two compile-time variants of that kernel, kept for the A/B (tools/attn_stagger_ab.py):
//   "attn7p_stagger_swap": which half of the work-group opens a slot with the softmax (barrier behind QK^T) and which with the QK^T
//     MFMAs (barrier behind PV): 1 = waves 0-3 the softmax, waves 4-7 the MFMAs; 0 = the other way round;
//   "attn7p_stagger_setprio": 1 = s_setprio 1 over softmax + PV, as the tile has it everywhere else, 0 = none.
// Defaults (interleaved in one process, 9 rounds of 0.45 s, tools/attn_stagger_ab.py; profiles/attn_stagger/README.md):
// attn7p_stagger_swap = 1 with attn7p_stagger_setprio = 1 is the one combination of which every round beat every round of the slim loop
// at the 14B self-attention and its two shard shapes; the other three tie with the slim loop.
constexpr int ATTN7P_STAGGER_DEFAULT = 1;
constexpr int ATTN7P_STAGGER_SETPRIO_DEFAULT = 1;
constexpr int ATTN7P_STAGGER_SWAP_DEFAULT = 1;
int icv_attn7p_stagger() {
  const int v = icv_get_option_int("attn7p_stagger", -1);
  if (v < 0) return ATTN7P_STAGGER_DEFAULT;
  if (v == 0 || v == 1) return v;
  icv_set_error("attn7p_stagger = %d: 1 = the staggered long-key kernel of attn7p, 0 = the slim loop; negative = the default", v);
  return -1;
}
int icv_attn7p_stagger_setprio() {
  const int v = icv_get_option_int("attn7p_stagger_setprio", -1);
  if (v < 0) return ATTN7P_STAGGER_SETPRIO_DEFAULT;
  if (v == 0 || v == 1) return v;
  icv_set_error("attn7p_stagger_setprio = %d: 1 = s_setprio over softmax + PV in the staggered kernel, 0 = none; negative = the default", v);
  return -1;
}

int icv_attn7p_stagger_swap() {
  const int v = icv_get_option_int("attn7p_stagger_swap", -1);
  if (v < 0) return ATTN7P_STAGGER_SWAP_DEFAULT;
  if (v == 0 || v == 1) return v;
  icv_set_error("attn7p_stagger_swap = %d: 1 = waves 0-3 open a slot with the softmax and waves 4-7 with QK^T, 0 = the other way round; negative = the default", v);
  return -1;
}

// ---- diagnostics: where and when every work-group of the NEXT attn7 launches runs -----------------------------------------
// icv_attention_trace(buf, capacity): buf = device u64 [capacity][4] (NULL switches tracing off).  While set, every attn7
// work-group b < capacity writes buf[b] = {start, end (s_memrealtime ticks, 100 MHz), HW_ID, XCC_ID} - the round structure and
// the work-group -> XCD placement of a launch (tools/attn_round_trace.py; profiles/r05/attn_round_occupancy.md).
namespace {
unsigned long long* g_trace = nullptr;
int g_trace_cap = 0;
}  // namespace
unsigned long long* icv_attention_trace_buffer(int* capacity) {
  *capacity = g_trace_cap;
  return g_trace;
}
extern "C" int icv_attention_trace(void* buf, int64_t capacity) {
  ICV_REQUIRE(capacity >= 0 && capacity < (1LL << 31), "icv_attention_trace: bad capacity");
  g_trace = (unsigned long long*)buf;
  g_trace_cap = buf ? (int)capacity : 0;
  return 0;
}
