// Pieces shared by the flash-attention kernel variants (attn7.hip default, attn2.hip, and the experiments/ family):
// launch parameters, (head, query-block) work-item mapping, the transposed LDS read, the carried
// online-softmax state (load / init) and the epilogue (state write-back or normalised bf16 output).
// Fragment conventions (see experiments/attn1.hip for the derivation): a wave owns 32 query rows, query = lane&31;
// O^T accumulator ot[d0][r] = O[q][d = d0*32 + (r&3) + 8*(r>>2) + 4*(lane>>5)]; the row sum l is kept as
// two half-lane partials (lanes q and q+32).
#pragma once
#include "icv_common.h"

unsigned long long* icv_attention_trace_buffer(int* capacity);   // attention.hip (icv_attention_trace)
int icv_attn_mfma(bool short_kv);                                // attention.hip: MFMA shape of attn7 / attn7p (16 or 32; -1 = error set)
int icv_attn_tile16_lean(bool short_kv);                         // attention.hip: body of the MF = 16 tile (1 = lean, 0 = the first one)
int icv_attn7p_slim();                                           // attention.hip: attn7p's key loop around the lean body (1 = slim, 0 = the one loop)
int icv_attn7p_stagger();                                        // attention.hip: attn7p's staggered kernel for one piece that is there (1 / 0; -1 = error set)
int icv_attn7p_stagger_setprio();                                // attention.hip: s_setprio over softmax + PV in the staggered kernel (1 / 0; -1 = error set)
int icv_attn7p_stagger_swap();                                   // attention.hip: which half of the work-group opens a slot with the softmax (1 / 0; -1 = error set)

namespace attc {

constexpr int D = 128;
constexpr float NEG_BIG = -1.0e30f;

struct Params {
  const bf16_t* q; int64_t ldq;
  const bf16_t* k; int64_t ldk;
  const bf16_t* v; int64_t ldv;
  bf16_t* o; int64_t ldo;
  float* acc; int64_t ldacc;   // carried O^T state, f32 [Sq, heads*128] (may be NULL)
  float* ml;                   // carried (m, l) per (row, head): f32 [Sq, heads, 2]
  int64_t Sq, Skv;
  int heads, nqb;
  int state_in, state_out;   // state_out: 0 = normalise + store bf16, 1 = write the carried state, 2 = normalise + ADD into bf16 o
  float sc;   // scale * log2(e)
  float thr;  // defer-max threshold, log2 units
  int ablate; // timing ablations (attn7: 1 = no K/V DMA after the prologue, 2 = no per-tile barrier); results are then WRONG
  // diagnostics (icv_attention_trace; attn7 only): per work-group {start, end} in 100 MHz s_memrealtime ticks, HW_ID, XCC_ID
  unsigned long long* trace;
  int trace_cap;
};


inline void fill_params(Params& p, const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v,
                        int64_t ldv, void* o, int64_t ldo, float* acc, int64_t ldacc, float* ml, int state_in,
                        int state_out, int64_t Sq, int64_t Skv, int64_t heads, float scale, int rows_per_block) {
  p.q = (const bf16_t*)q; p.ldq = ldq; p.k = (const bf16_t*)k; p.ldk = ldk;
  p.v = (const bf16_t*)v; p.ldv = ldv; p.o = (bf16_t*)o; p.ldo = ldo;
  p.acc = acc; p.ldacc = ldacc; p.ml = ml; p.state_in = state_in; p.state_out = state_out;
  p.Sq = Sq; p.Skv = Skv; p.heads = (int)heads;
  p.nqb = (int)((Sq + rows_per_block - 1) / rows_per_block);
  p.sc = scale * 1.4426950408889634f;
  if (fabsf(p.sc - 1.0f) < 1e-6f) p.sc = 1.0f;   // "unit scale": the caller folded scale * log2(e) into K (scale = ln 2)
  p.thr = (float)icv_get_option_int("attn_defer_max_log2", 8);
  p.ablate = 0;
  p.trace = nullptr;
  p.trace_cap = 0;
}

typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

// ds_read_b64_tr_b16: within each 16-lane group the 16 x (4 x b16) loaded words are transposed: lane t
// receives element (t&3) of the words loaded by lanes 4j + (t>>2), j = 0..3 (probed: tools/probe_tr.hip).
__device__ __forceinline__ bf16x4 lds_read_tr16(const char* p) {
  s16x4 r = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p));
  return __builtin_bit_cast(bf16x4, r);
}

// (head, query block) of this workgroup: block b runs on XCD b%8, so give each XCD a contiguous run of
// work items (head-major): its 32 CUs then stream the SAME head's K/V through that XCD's L2 together.
__device__ __forceinline__ void work_item(const Params& p, int& head, int& qb) {
  const int nwg = p.heads * p.nqb;
  const int bid = blockIdx.x;
  const int xcd = bid & 7, local = bid >> 3;
  const int qn = nwg >> 3, r = nwg & 7;
  const int wg = (xcd < r ? xcd * (qn + 1) : r * (qn + 1) + (xcd - r) * qn) + local;
  head = wg / p.nqb;
  qb = wg - head * p.nqb;
}

// softmax state of one 32-row sub-block: from the carried buffers (row qr_c, clamped) or empty
__device__ __forceinline__ void load_state(const Params& p, int64_t qr_c, int head, int hi, f32x16 (&ot)[4],
                                           float& m_run, float& l_run) {
  if (p.state_in) {
    const float* ap = p.acc + qr_c * p.ldacc + (int64_t)head * D + 4 * hi;
#pragma unroll
    for (int d0 = 0; d0 < 4; ++d0)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const float4 a = *reinterpret_cast<const float4*>(ap + d0 * 32 + rr * 8);
        ot[d0][rr * 4 + 0] = a.x; ot[d0][rr * 4 + 1] = a.y; ot[d0][rr * 4 + 2] = a.z; ot[d0][rr * 4 + 3] = a.w;
      }
    const float2 mlv = *reinterpret_cast<const float2*>(p.ml + (qr_c * p.heads + head) * 2);
    m_run = mlv.x;
    l_run = hi == 0 ? mlv.y : 0.f;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) ot[i][r] = 0.f;
    m_run = NEG_BIG;
    l_run = 0.f;
  }
}

// epilogue of one 32-row sub-block: write the state back, or normalise and store bf16 (8-byte stores)
__device__ __forceinline__ void store_result(const Params& p, int64_t qr, int head, int hi, const f32x16 (&ot)[4],
                                             float m_run, float l_run) {
  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  if (qr >= p.Sq) return;
  if (p.state_out == 1) {
    float* ap = p.acc + qr * p.ldacc + (int64_t)head * D + 4 * hi;
#pragma unroll
    for (int d0 = 0; d0 < 4; ++d0)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr)
        *reinterpret_cast<float4*>(ap + d0 * 32 + rr * 8) =
            make_float4(ot[d0][rr * 4 + 0], ot[d0][rr * 4 + 1], ot[d0][rr * 4 + 2], ot[d0][rr * 4 + 3]);
    if (hi == 0) *reinterpret_cast<float2*>(p.ml + (qr * p.heads + head) * 2) = make_float2(m_run, l_tot);
  } else {
    const float inv = 1.0f / l_tot;
    bf16_t* op = p.o + qr * p.ldo + (int64_t)head * D + 4 * hi;
#pragma unroll
    for (int d0 = 0; d0 < 4; ++d0)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        float a = ot[d0][rr * 4 + 0] * inv, b = ot[d0][rr * 4 + 1] * inv;
        float c = ot[d0][rr * 4 + 2] * inv, d = ot[d0][rr * 4 + 3] * inv;
        if (p.state_out == 2) {   // o += result (i2v: image cross-attention summed with the text one)
          const uint2 prev = *reinterpret_cast<const uint2*>(op + d0 * 32 + rr * 8);
          a += __uint_as_float(prev.x << 16); b += __uint_as_float(prev.x & 0xFFFF0000u);
          c += __uint_as_float(prev.y << 16); d += __uint_as_float(prev.y & 0xFFFF0000u);
        }
        *reinterpret_cast<uint2*>(op + d0 * 32 + rr * 8) = make_uint2(pack_bf16x2(a, b), pack_bf16x2(c, d));
      }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// MF = 16: the same wave tile (32 query rows x 64 keys) on v_mfma_f32_16x16x32_bf16 (attn7.hip / attn7p.hip, option "attn_mfma").
// Both kernels run THIS tile, so they stay bit-identical to each other.  Lane maps, g = lane >> 4, t = lane & 15 (restated in plain
// Python and checked against each other in tests/test_attn_mfma16_layout_cpu.py - change both together):
//   q-block qb (0, 1):  query row = 16 qb + t;  m_run, l_run, m_base and the reference in the C operand exist once per q-block
//   Q fragment (B of S^T = K Q^T)   qf[qb][ks][j] = Q[16 qb + t][d = 32 ks + 8 g + j],  ks = 0..3, j = 0..7
//   K fragment (A), one ds_read_b128:        kf[j] = K[key = 16 kb + t][d = 32 ks + 8 g + j],  kb = 0..3; the K image is the 32 form's
//                                                    (16-byte chunk c of row `key` sits at chunk c ^ (key & 15)), here c = 4 ks + g
//   S^T accumulator                 st[kb][qb][r] = S[16 qb + t][key = 16 kb + 4 g + r],  r = 0..3 (the tail mask's key index)
//   P -> B of O^T += V^T P^T, k-step kk (0, 1):  pf[qb][j] = P[16 qb + t][key = 32 kk + 16 (j >> 2) + 4 g + (j & 3)]: the MFMA's k = 8 g + j
//   V fragment (A), two ds_read_b64_tr_b16:  vf[j] = V[key = 32 kk + 16 (j >> 2) + 4 g + (j & 3)][d = 16 db + t],  db = 0..7: the SAME
//                                                    key for (g, j) as pf.  Read jh = j >> 2: lane 4 q + p of a 16-lane group supplies the
//                                                    address of row 32 kk + 16 jh + 4 g + q, columns 16 db + 4 p ... + 3, and receives
//                                                    element (t & 3) of the rows q = 0..3 of column group t >> 2 (lds_read_tr16 above)
//   V image (MF = 16 only):  32-byte segment s (0..7) of row `key` sits at segment s ^ (key & 7).  A 32-lane half of the transposed
//                            read takes rows 4 g + q, g in {0, 1} or {2, 3}: 8 rows with key & 7 = 0..7 in ONE 32-byte column, which the
//                            XOR spreads over the 8 segments of the 256-byte bank row (the 32 form's chunk ^ ((key & 3) << 2) image
//                            would leave rows key and key + 4 on the same banks: 2-way).  The DMA applies it on the source side.
//   O^T accumulator                 ot[db][qb][r] = O[16 qb + t][d = 16 db + 4 g + r];  the row sum l is four lane-group partials
// The carried state in memory (acc, ml) and the output are the 32 form's: a chunk written by one shape is read by the other.
struct Tile16 {
  f32x4 ot[8][2];
  float m_run[2], l_run[2], m_base[2];
  f32x4 cinit[2];     // UNIT: -m_base, the C operand of the first MFMA of every S^T chain
  bf16x8 qf[2][4];
};

// softmax state of the wave's two 16-row q-blocks (rows qr_c[qb], clamped): from the carried buffers or empty
__device__ __forceinline__ void load_state(const Params& p, const int64_t (&qr_c)[2], int head, int g, f32x4 (&ot)[8][2],
                                           float (&m_run)[2], float (&l_run)[2]) {
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    if (p.state_in) {
      const float* ap = p.acc + qr_c[qb] * p.ldacc + (int64_t)head * D + 4 * g;
#pragma unroll
      for (int db = 0; db < 8; ++db) {
        const float4 a = *reinterpret_cast<const float4*>(ap + db * 16);
        ot[db][qb][0] = a.x; ot[db][qb][1] = a.y; ot[db][qb][2] = a.z; ot[db][qb][3] = a.w;
      }
      const float2 mlv = *reinterpret_cast<const float2*>(p.ml + (qr_c[qb] * p.heads + head) * 2);
      m_run[qb] = mlv.x;
      l_run[qb] = g == 0 ? mlv.y : 0.f;
    } else {
#pragma unroll
      for (int db = 0; db < 8; ++db)
#pragma unroll
        for (int r = 0; r < 4; ++r) ot[db][qb][r] = 0.f;
      m_run[qb] = NEG_BIG;
      l_run[qb] = 0.f;
    }
  }
}

// epilogue of the two q-blocks (rows qr[qb]; a row >= p.Sq is not stored): write the state back, or normalise and store bf16
__device__ __forceinline__ void store_result(const Params& p, const int64_t (&qr)[2], int head, int g, const f32x4 (&ot)[8][2],
                                             const float (&m_run)[2], const float (&l_run)[2]) {
  float l_tot[2];
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    const float l2 = l_run[qb] + __shfl_xor(l_run[qb], 16, 64);
    l_tot[qb] = l2 + __shfl_xor(l2, 32, 64);
  }
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    if (qr[qb] >= p.Sq) continue;
    if (p.state_out == 1) {
      float* ap = p.acc + qr[qb] * p.ldacc + (int64_t)head * D + 4 * g;
#pragma unroll
      for (int db = 0; db < 8; ++db)
        *reinterpret_cast<float4*>(ap + db * 16) = make_float4(ot[db][qb][0], ot[db][qb][1], ot[db][qb][2], ot[db][qb][3]);
      if (g == 0) *reinterpret_cast<float2*>(p.ml + (qr[qb] * p.heads + head) * 2) = make_float2(m_run[qb], l_tot[qb]);
    } else {
      const float inv = 1.0f / l_tot[qb];
      bf16_t* op = p.o + qr[qb] * p.ldo + (int64_t)head * D + 4 * g;
#pragma unroll
      for (int db = 0; db < 8; ++db) {
        float a = ot[db][qb][0] * inv, b = ot[db][qb][1] * inv;
        float c = ot[db][qb][2] * inv, d = ot[db][qb][3] * inv;
        if (p.state_out == 2) {   // o += result
          const uint2 prev = *reinterpret_cast<const uint2*>(op + db * 16);
          a += __uint_as_float(prev.x << 16); b += __uint_as_float(prev.x & 0xFFFF0000u);
          c += __uint_as_float(prev.y << 16); d += __uint_as_float(prev.y & 0xFFFF0000u);
        }
        *reinterpret_cast<uint2*>(op + db * 16) = make_uint2(pack_bf16x2(a, b), pack_bf16x2(c, d));
      }
    }
  }
}

// state, reference and Q fragments of a wave whose q-block rows are qr_c[qb] (clamped); issues the Q loads, waits for nothing
__device__ __forceinline__ void tile16_load_q(const Params& p, const int64_t (&qr_c)[2], int head, int g, Tile16& s) {
  const bf16_t* qh = p.q + (int64_t)head * D + g * 8;
#pragma unroll
  for (int qb = 0; qb < 2; ++qb)
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) s.qf[qb][ks] = *reinterpret_cast<const bf16x8*>(qh + qr_c[qb] * p.ldq + ks * 32);
}

template <bool UNIT>
__device__ __forceinline__ void tile16_init(const Params& p, const int64_t (&qr_c)[2], int head, int g, Tile16& s) {
  load_state(p, qr_c, head, g, s.ot, s.m_run, s.l_run);
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    s.m_base[qb] = s.m_run[qb] < -1.0e29f ? 0.f : s.m_run[qb];
#pragma unroll
    for (int r = 0; r < 4; ++r) s.cinit[qb][r] = UNIT ? -s.m_base[qb] : 0.f;
  }
}

// source column (elements) of the 16-byte LDS chunk pc of V row `key`: the DMA side of the MF = 16 V image
__device__ __forceinline__ int tile16_vcol(int pc, int key) { return (pc ^ ((key & 7) << 1)) * 8; }

// LEAN body of the tile (option "attn_tile16_lean"; profiles/attn_lean_tile/README.md): the same arithmetic in the same order, with less
// vector work that is not softmax.  The per-lane K / V fragment addresses (one per d-step of K, one per d-block of V) are formed ONCE per
// work-group and FOLLOW the ring: the kernel moves them on by a wave-uniform byte count when it moves to another part of the ring (12
// adds per step) instead of adding a fresh stage base to per-lane constants in every 32-key half.  What is known at compile time - the
// tile's place STG (0, 1) inside a step of two stages, kb * 4096, kk * 8192, + 4096 - sits in the offset: field of the ds_reads.  The
// lane's two row sums stay two scalar chains (hipcc's SLP vectoriser otherwise packs them into v_pk_add_f32, which is slow beside MFMAs),
// and the first body's per-tile "no reference yet" compares are state (Tile16Addr::lim).  22.13 vs 23.29 ms at the 14B self-attention.
typedef __attribute__((address_space(3))) bf16x8 lds_bf16x8;
struct Tile16Addr {               // the lean body's own per-lane state
  unsigned k[4], v[8];             // LDS byte addresses of this lane's fragments in the K image / the V image of the current stage
  // UNIT: the lazy-max test's limit on the lane's partial row sum of q-block qb, with "this q-block has no reference yet" folded in: -1
  // (no sum of P is <= -1, so the test fires) while m_run was empty when the CURRENT tile began, p_lim after that.  The first body
  // evaluates that condition at the top of every tile; here it is state, renewed where m_run changes for the last time in a tile.
  float lim[2];
};
template <bool UNIT>
__device__ __forceinline__ void tile16_lean_lim(const Tile16& s, const float p_lim, Tile16Addr& a) {
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) a.lim[qb] = UNIT && s.m_run[qb] < -1.0e29f ? -1.0f : p_lim;
}
__device__ __forceinline__ void tile16_lean_addr(const unsigned lds_base, const int lane, Tile16Addr& a) {
  const int g = lane >> 4, t = lane & 15;
  const int v_row_off = (4 * g + (t >> 2)) * 256;
  const int v_sw = (4 * (g & 1) + (t >> 2)) << 5;
  const int v_byte_lo = (t & 3) * 8;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) a.k[ks] = lds_base + t * 256 + (((ks * 4 + g) ^ t) << 4);
#pragma unroll
  for (int db = 0; db < 8; ++db) a.v[db] = lds_base + 16384 + v_row_off + ((db * 32 + v_byte_lo) ^ v_sw);
}
// move the addresses on by `bytes` (wave-uniform, may be negative: the ring wraps)
__device__ __forceinline__ void tile16_lean_advance(Tile16Addr& a, const int bytes) {
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) a.k[ks] += (unsigned)bytes;
#pragma unroll
  for (int db = 0; db < 8; ++db) a.v[db] += (unsigned)bytes;
}

// a + b as fma(b, one, a), one = 1.0 the compiler cannot see through: one rounding of the exact sum, so the SAME bits as a + b, but not an
// fadd - the lane's two row-sum chains are isomorphic, and the SLP vectoriser packs two fadd chains into v_pk_add_f32, which cost more
// beside MFMAs than scalar adds.  The first chain stays plain C++ (alone it has nothing to pair with).  Not inline assembly: the
// compiler must see the instruction to keep the wait state between a v_exp_f32 and its consumer.
__device__ __forceinline__ float t16_add_opaque(const float a, const float b, const float one) { return __builtin_fmaf(b, one, a); }

// one 64-key tile: keys [key0, key0 + 64) of a key axis of skv rows, K image at ks, V image at vs (LDS).  The 32 form's order of work:
// K reads -> 32 QK^T MFMAs -> per 32-key half: softmax (lazy max, re-base decided on the lane's partial sums), V tr-reads, 16 PV MFMAs.
// KPREFETCH / DSMAJOR / SETPRIO: attn7.hip's variant bits 2, !32 and 4.
// LEAN: the tile lies STG stages (32 KiB each) past the one the addresses `la` point at; ks / vs are not used.
template <bool UNIT, bool KPREFETCH, bool DSMAJOR, bool SETPRIO, bool LEAN = false, int STG = 0>
__device__ __forceinline__ void tile16(const Params& p, const float p_lim, const char* ks, const char* vs, const int64_t key0,
                                       const int64_t skv, const int lane, Tile16& s, Tile16Addr* la = nullptr) {
  static_assert(STG == 0 || (LEAN && STG == 1), "STG: the tile's place in a step of two stages (lean body only)");
  static_assert(STG * 32768 + 8192 + 4096 < 65536, "the ds_read offset: field holds 16 bits");
  const int g = lane >> 4, t = lane & 15;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  const int k_row_off = t * 256;
  const int v_row_off = (4 * g + (t >> 2)) * 256;
  const int v_sw = (4 * (g & 1) + (t >> 2)) << 5;        // (key & 7) << 5: 32 kk + 16 jh drop out
  const int v_byte_lo = (t & 3) * 8;
  f32x4 st[4][2];
  const bool no_ref = UNIT && !LEAN && (s.m_run[0] < -1.0e29f || s.m_run[1] < -1.0e29f);     // LEAN: folded into la->lim
#define T16_KADDR(KB_, KS_) (ks + (KB_) * 4096 + k_row_off + ((((KS_) * 4 + g) ^ t) << 4))
#define T16_KLOAD(DST_, KB_, KS_)                                                                                   \
  do {                                                                                                              \
    if constexpr (LEAN) DST_ = *(const lds_bf16x8*)(la->k[KS_] + (unsigned)(STG * 32768 + (KB_) * 4096));           \
    else DST_ = *reinterpret_cast<const bf16x8*>(T16_KADDR(KB_, KS_));                                              \
  } while (0)
#define T16_QK(KB_, KS_, KF_)                                                                                       \
  _Pragma("unroll") for (int qb = 0; qb < 2; ++qb) st[KB_][qb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(           \
      KF_, s.qf[qb][KS_], (KS_) == 0 ? (UNIT ? s.cinit[qb] : zero4) : st[KB_][qb], 0, 0, 0)
  if (KPREFETCH) {
    bf16x8 kf[4][4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int kq = 0; kq < 4; ++kq) T16_KLOAD(kf[kb][kq], kb, kq);
    __builtin_amdgcn_sched_barrier(0);
    if (SETPRIO) __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kq = 0; kq < 4; ++kq)
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) { T16_QK(kb, kq, kf[kb][kq]); }
    if (SETPRIO) __builtin_amdgcn_s_setprio(0);
  } else if (DSMAJOR) {
    // software-pipelined by hand, KD fragments ahead, and pinned with sched_group_barrier: left alone, hipcc issues one read, waits
    // lgkmcnt(0) and issues its two MFMAs - two 16-cycle MFMAs cover a quarter of the read's latency, sixteen times per tile
    constexpr int KD = 3;
    bf16x8 kf[16];
#pragma unroll
    for (int i = 0; i < KD; ++i) T16_KLOAD(kf[i], i & 3, i >> 2);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if (i + KD < 16) T16_KLOAD(kf[i + KD], (i + KD) & 3, (i + KD) >> 2);
      T16_QK(i & 3, i >> 2, kf[i]);
    }
    __builtin_amdgcn_sched_group_barrier(0x100, KD, 0);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if (i + KD < 16) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
    }
  } else {
    if (SETPRIO) __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int kq = 0; kq < 4; ++kq) {
        bf16x8 kf;
        T16_KLOAD(kf, kb, kq);
        T16_QK(kb, kq, kf);
      }
    if (SETPRIO) __builtin_amdgcn_s_setprio(0);
  }
#undef T16_KADDR
#undef T16_KLOAD
#undef T16_QK
  if (key0 + 64 > skv) {
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t key = key0 + kb * 16 + 4 * g + r;
        if (key >= skv) { st[kb][0][r] = NEG_BIG; st[kb][1][r] = NEG_BIG; }
      }
  }
  float one = 1.0f;                          // LEAN: see t16_add_opaque
  if (LEAN) asm("" : "+s"(one));
  float mb[2] = {-s.m_run[0] * p.sc, -s.m_run[1] * p.sc};
  float psum[2] = {0.f, 0.f};
  if (SETPRIO) __builtin_amdgcn_s_setprio(1);
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {          // a 32-key half = key blocks 2 kk and 2 kk + 1 = one k-step of the PV MFMAs
    bf16x8 pf[2];
    float ps[2];
#define T16_EXP()                                                                                                   \
  _Pragma("unroll") for (int qb = 0; qb < 2; ++qb) {                                                                \
    ps[qb] = 0.f;                                                                                                   \
    _Pragma("unroll") for (int j = 0; j < 8; ++j) {                                                                 \
      const float sv = st[2 * kk + (j >> 2)][qb][j & 3];                                                            \
      const float pv = UNIT ? __builtin_amdgcn_exp2f(sv) : __builtin_amdgcn_exp2f(fmaf(sv, p.sc, mb[qb]));          \
      if (LEAN && j == 0) ps[qb] = pv; /* 0 + pv, exactly */                                                        \
      else if (LEAN && qb == 1) ps[qb] = t16_add_opaque(ps[qb], pv, one);                                           \
      else ps[qb] += pv;                                                                                            \
      pf[qb][j] = (__bf16)pv;                                                                                       \
    }                                                                                                               \
  }
    T16_EXP();
    // lazy max (attn2.hip): the lane's partial row sum bounds every P it holds
    if (__any(LEAN && UNIT ? !(ps[0] <= la->lim[0]) || !(ps[1] <= la->lim[1]) : !(ps[0] <= p_lim) || !(ps[1] <= p_lim) || no_ref)) {
#pragma unroll
      for (int qb = 0; qb < 2; ++qb) {
        float mloc = st[2 * kk][qb][0];
#pragma unroll
        for (int j = 1; j < 8; ++j) mloc = fmaxf(mloc, st[2 * kk + (j >> 2)][qb][j & 3]);
        mloc = fmaxf(mloc, __shfl_xor(mloc, 16, 64));
        mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
        if (UNIT) mloc += s.m_base[qb];                      // st = s - m_base
        const float m_new = fmaxf(s.m_run[qb], mloc);
        const float alpha = __builtin_amdgcn_exp2f((s.m_run[qb] - m_new) * p.sc);
        s.m_run[qb] = m_new;
        // an empty m_run at the top of the tile forces the re-base in BOTH halves (as no_ref does), so the second half's sees the final one
        if (LEAN && UNIT && kk == 1) la->lim[qb] = m_new < -1.0e29f ? -1.0f : p_lim;
        s.l_run[qb] = (s.l_run[qb] + psum[qb]) * alpha;
        psum[qb] = 0.f;
#pragma unroll
        for (int db = 0; db < 8; ++db)
#pragma unroll
          for (int r = 0; r < 4; ++r) s.ot[db][qb][r] *= alpha;
        mb[qb] = -m_new * p.sc;
        if (UNIT) {                                          // re-base this and the later half of the tile, and cinit
          const float dm = m_new - s.m_base[qb];
          s.m_base[qb] = m_new;
#pragma unroll
          for (int kb = 0; kb < 4; ++kb)
            if (kb >= 2 * kk) {
#pragma unroll
              for (int r = 0; r < 4; ++r) st[kb][qb][r] -= dm;
            }
#pragma unroll
          for (int r = 0; r < 4; ++r) s.cinit[qb][r] = -m_new;
        }
      }
      T16_EXP();
    }
#undef T16_EXP
    if (LEAN) {                              // ps >= +0, so 0 + ps = ps exactly
      psum[0] = kk == 0 ? ps[0] : psum[0] + ps[0];
      psum[1] = kk == 0 ? ps[1] : t16_add_opaque(psum[1], ps[1], one);
    } else {
      psum[0] += ps[0];
      psum[1] += ps[1];
    }
    // the V fragments VD d-blocks ahead of their MFMAs, pinned the same way (the next half's exp / convert work floats between them)
    constexpr int VD = 2;
    bf16x4 va[8], vb[8];
#define T16_VREAD(DB_)                                                                                  \
  {                                                                                                     \
    if constexpr (LEAN) {                                                                               \
      const unsigned va_a = la->v[DB_] + (unsigned)(STG * 32768 + kk * 8192);                           \
      va[DB_] = __builtin_bit_cast(bf16x4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(va_a))); \
      vb[DB_] = __builtin_bit_cast(bf16x4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(va_a + 4096u))); \
    } else {                                                                                            \
      const char* va_p = vs + kk * 8192 + v_row_off + (((DB_) * 32 + v_byte_lo) ^ v_sw);                 \
      va[DB_] = lds_read_tr16(va_p);                                                                    \
      vb[DB_] = lds_read_tr16(va_p + 4096); /* 16 rows further on: the same key & 7, the same swizzle */ \
    }                                                                                                   \
  }
#pragma unroll
    for (int db = 0; db < VD; ++db) T16_VREAD(db);
#pragma unroll
    for (int db = 0; db < 8; ++db) {
      if (db + VD < 8) T16_VREAD(db + VD);
      bf16x8 vf;
      vf[0] = va[db][0]; vf[1] = va[db][1]; vf[2] = va[db][2]; vf[3] = va[db][3];
      vf[4] = vb[db][0]; vf[5] = vb[db][1]; vf[6] = vb[db][2]; vf[7] = vb[db][3];
#pragma unroll
      for (int qb = 0; qb < 2; ++qb) s.ot[db][qb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[qb], s.ot[db][qb], 0, 0, 0);
    }
#undef T16_VREAD
    __builtin_amdgcn_sched_group_barrier(0x100, 2 * VD, 0);
#pragma unroll
    for (int db = 0; db < 8; ++db) {
      if (db + VD < 8) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
    }
  }
  if (SETPRIO) __builtin_amdgcn_s_setprio(0);
  s.l_run[0] += psum[0];
  if (LEAN) s.l_run[1] = t16_add_opaque(s.l_run[1], psum[1], one);
  else s.l_run[1] += psum[1];
}

// The lean body of tile16<UNIT, false, true, SETPRIO, true, STG> cut in two, for a key loop that may put a barrier between the halves
// (attn7p.hip's staggered kernel): tile16_qk is the K fragment reads and the 32 QK^T MFMAs into st, tile16_sv everything behind them -
// tail mask, both 32-key halves of softmax with lazy max and re-base, the V tr-reads and the 32 PV MFMAs.  The lean body's code in the
// lean body's order, statement for statement: tile16_qk + tile16_sv on one tile IS tile16's lean body, so outputs and carried state are
// bit-identical whichever loop runs them (tests/test_attn_stagger_gpu.py).  st (32 VGPRs) is the caller's, so that it can outlive a
// barrier.  Change tile16's lean body and these two together.
template <bool UNIT, int STG>
__device__ __forceinline__ void tile16_qk(const Tile16& s, const Tile16Addr& la, f32x4 (&st)[4][2]) {
  static_assert(STG == 0 || STG == 1, "STG: the tile's place in a step of two stages");
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
#define T16_KLOAD(DST_, KB_, KS_) DST_ = *(const lds_bf16x8*)(la.k[KS_] + (unsigned)(STG * 32768 + (KB_) * 4096))
#define T16_QK(KB_, KS_, KF_)                                                                                       \
  _Pragma("unroll") for (int qb = 0; qb < 2; ++qb) st[KB_][qb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(           \
      KF_, s.qf[qb][KS_], (KS_) == 0 ? (UNIT ? s.cinit[qb] : zero4) : st[KB_][qb], 0, 0, 0)
  constexpr int KD = 3;
  bf16x8 kf[16];
#pragma unroll
  for (int i = 0; i < KD; ++i) T16_KLOAD(kf[i], i & 3, i >> 2);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    if (i + KD < 16) T16_KLOAD(kf[i + KD], (i + KD) & 3, (i + KD) >> 2);
    T16_QK(i & 3, i >> 2, kf[i]);
  }
  __builtin_amdgcn_sched_group_barrier(0x100, KD, 0);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    if (i + KD < 16) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
  }
#undef T16_KLOAD
#undef T16_QK
}

template <bool UNIT, bool SETPRIO, int STG>
__device__ __forceinline__ void tile16_sv(const Params& p, const float p_lim, const int64_t key0, const int64_t skv, const int lane, Tile16& s,
                                          Tile16Addr& la, f32x4 (&st)[4][2]) {
  static_assert(STG == 0 || STG == 1, "STG: the tile's place in a step of two stages");
  const int g = lane >> 4;
  if (key0 + 64 > skv) {
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t key = key0 + kb * 16 + 4 * g + r;
        if (key >= skv) { st[kb][0][r] = NEG_BIG; st[kb][1][r] = NEG_BIG; }
      }
  }
  float one = 1.0f;                          // see t16_add_opaque
  asm("" : "+s"(one));
  float mb[2] = {-s.m_run[0] * p.sc, -s.m_run[1] * p.sc};
  float psum[2] = {0.f, 0.f};
  if (SETPRIO) __builtin_amdgcn_s_setprio(1);
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {          // a 32-key half = key blocks 2 kk and 2 kk + 1 = one k-step of the PV MFMAs
    bf16x8 pf[2];
    float ps[2];
#define T16_EXP()                                                                                                   \
  _Pragma("unroll") for (int qb = 0; qb < 2; ++qb) {                                                                \
    ps[qb] = 0.f;                                                                                                   \
    _Pragma("unroll") for (int j = 0; j < 8; ++j) {                                                                 \
      const float sv = st[2 * kk + (j >> 2)][qb][j & 3];                                                            \
      const float pv = UNIT ? __builtin_amdgcn_exp2f(sv) : __builtin_amdgcn_exp2f(fmaf(sv, p.sc, mb[qb]));          \
      if (j == 0) ps[qb] = pv; /* 0 + pv, exactly */                                                                \
      else if (qb == 1) ps[qb] = t16_add_opaque(ps[qb], pv, one);                                                   \
      else ps[qb] += pv;                                                                                            \
      pf[qb][j] = (__bf16)pv;                                                                                       \
    }                                                                                                               \
  }
    T16_EXP();
    // lazy max (attn2.hip): the lane's partial row sum bounds every P it holds
    if (__any(UNIT ? !(ps[0] <= la.lim[0]) || !(ps[1] <= la.lim[1]) : !(ps[0] <= p_lim) || !(ps[1] <= p_lim))) {
#pragma unroll
      for (int qb = 0; qb < 2; ++qb) {
        float mloc = st[2 * kk][qb][0];
#pragma unroll
        for (int j = 1; j < 8; ++j) mloc = fmaxf(mloc, st[2 * kk + (j >> 2)][qb][j & 3]);
        mloc = fmaxf(mloc, __shfl_xor(mloc, 16, 64));
        mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
        if (UNIT) mloc += s.m_base[qb];                      // st = s - m_base
        const float m_new = fmaxf(s.m_run[qb], mloc);
        const float alpha = __builtin_amdgcn_exp2f((s.m_run[qb] - m_new) * p.sc);
        s.m_run[qb] = m_new;
        // an empty m_run at the top of the tile forces the re-base in BOTH halves, so the second half's sees the final one
        if (UNIT && kk == 1) la.lim[qb] = m_new < -1.0e29f ? -1.0f : p_lim;
        s.l_run[qb] = (s.l_run[qb] + psum[qb]) * alpha;
        psum[qb] = 0.f;
#pragma unroll
        for (int db = 0; db < 8; ++db)
#pragma unroll
          for (int r = 0; r < 4; ++r) s.ot[db][qb][r] *= alpha;
        mb[qb] = -m_new * p.sc;
        if (UNIT) {                                          // re-base this and the later half of the tile, and cinit
          const float dm = m_new - s.m_base[qb];
          s.m_base[qb] = m_new;
#pragma unroll
          for (int kb = 0; kb < 4; ++kb)
            if (kb >= 2 * kk) {
#pragma unroll
              for (int r = 0; r < 4; ++r) st[kb][qb][r] -= dm;
            }
#pragma unroll
          for (int r = 0; r < 4; ++r) s.cinit[qb][r] = -m_new;
        }
      }
      T16_EXP();
    }
#undef T16_EXP
    psum[0] = kk == 0 ? ps[0] : psum[0] + ps[0];             // ps >= +0, so 0 + ps = ps exactly
    psum[1] = kk == 0 ? ps[1] : t16_add_opaque(psum[1], ps[1], one);
    // the V fragments VD d-blocks ahead of their MFMAs, pinned the same way (the next half's exp / convert work floats between them)
    constexpr int VD = 2;
    bf16x4 va[8], vb[8];
#define T16_VREAD(DB_)                                                                                  \
  {                                                                                                     \
    const unsigned va_a = la.v[DB_] + (unsigned)(STG * 32768 + kk * 8192);                              \
    va[DB_] = __builtin_bit_cast(bf16x4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(va_a)));  \
    vb[DB_] = __builtin_bit_cast(bf16x4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(va_a + 4096u))); \
  }
#pragma unroll
    for (int db = 0; db < VD; ++db) T16_VREAD(db);
#pragma unroll
    for (int db = 0; db < 8; ++db) {
      if (db + VD < 8) T16_VREAD(db + VD);
      bf16x8 vf;
      vf[0] = va[db][0]; vf[1] = va[db][1]; vf[2] = va[db][2]; vf[3] = va[db][3];
      vf[4] = vb[db][0]; vf[5] = vb[db][1]; vf[6] = vb[db][2]; vf[7] = vb[db][3];
#pragma unroll
      for (int qb = 0; qb < 2; ++qb) s.ot[db][qb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[qb], s.ot[db][qb], 0, 0, 0);
    }
#undef T16_VREAD
    __builtin_amdgcn_sched_group_barrier(0x100, 2 * VD, 0);
#pragma unroll
    for (int db = 0; db < 8; ++db) {
      if (db + VD < 8) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
    }
  }
  if (SETPRIO) __builtin_amdgcn_s_setprio(0);
  s.l_run[0] += psum[0];
  s.l_run[1] = t16_add_opaque(s.l_run[1], psum[1], one);
}

}  // namespace attc
