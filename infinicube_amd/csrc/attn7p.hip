// K6 for the sequence-parallel schedule ("process K/V chunks in arrival order (own shard first) with online-softmax
// merging"): ONE launch per layer whose work-groups walk a list of K|V PIECES - this rank's own rows first, then every (peer, row
// chunk) in the order the exchange delivers them - and gate on an ARRIVAL FLAG per piece instead of the host launching one
// carried-state kernel per chunk.  What that removes, per layer and forward: C - 1 launches with their per-XCD tails, the
// C - 1 round trips of the carried (O, m, l) state through HBM, and the all-peers barrier in front of every chunk
// (profiles/r05/attn_round_occupancy.md; chunks 4 -> 2 alone was worth 2 % of a sequence-parallel step).
//
// The inner loop is attn7.hip's default schedule (variant 148/132: 8 waves x 32 query rows, 64-key tiles, LDS-DMA ring used as two
// halves of two tiles, ONE vmcnt(0) + barrier per 128 keys, lazy max, unit scale, s_setprio) - see there for the fragment / swizzle
// conventions.  New here:
//   * the key axis is a list of pieces {k, v, rows, flag, value} carried in the kernel arguments; the softmax state (O, m, l and
//     the reference baked into the MFMA's C operand) stays in registers across pieces;
//   * the ring runs THROUGH a piece boundary when the next piece is already there: wave 0 samples the next piece's flag once per
//     128-key interval (one uncached dword load whose latency hides behind the interval's own vmcnt(0)), publishes the verdict
//     through an LDS word in front of the interval's barrier, and the last interval of a piece requests the next piece's first two
//     tiles instead of its own (dead) past-the-end tiles.  The verdict is taken by ONE lane and read by all waves after a barrier:
//     every wave issues its share of a tile's DMA, so a per-wave opinion about "ready" would tear a tile;
//   * a piece that has NOT arrived when its predecessor ends costs a bubble: wave 0 spins on the flag (s_sleep between polls, bounded
//     by a time-out that sets an error word and lets the kernel finish with garbage rather than hang the queue; once the word is set no
//     waiter of this or a later launch waits out the deadline again), then the ring is refilled;
//   * no cache maintenance is needed for the late rows: the rows of a piece are first read after its flag was seen, the launch's own
//     acquire invalidated whatever an earlier launch left in L2 / L1, and pieces are whole rows (no cache line straddles two pieces),
//     so no stale line of a piece can exist; the flag itself is polled with system-scope (uncached) loads.
// FRAME-WINDOWED instantiation (attn7p_kernel<UNIT, true>, icv_attention_fwd_framewin): the same ring and tile, but every
// work-group derives its OWN one or two pieces from the latent frame its query rows lie in.  Tokens are ordered (frame, row, column),
// so a frame is F contiguous rows; a query of frame f reads the frames [f - window, f + window] plus the first `sink` frames: one or
// two contiguous key ranges, computed from four scalars in the kernel arguments (no table in memory).  Work-groups are (head, frame,
// block of 256 rows of that frame): a block never straddles a frame, rows past the frame's end are clamped for reads and never stored
// - what happens at Sq in the other instantiations.  Pieces are always there (no flags, no time-out, no error word): the ring runs
// through the boundary between the two pieces as it does for a piece with flag < 0.
// MFMA shape (template MF, option "attn_mfma", default 16): the tile in this file is the 32x32x16 form; MF = 16 runs attc::tile16
// (attn_common.h) on v_mfma_f32_16x16x32_bf16 in every instantiation - same ring, pieces, flags and softmax; the carried state in memory
// is one format for both.  22.60 vs 23.17 ms at the 14B self-attention (profiles/attn_mfma16/README.md).
// Replaces: the chunked icv_attention_fwd_chunk sequence of the sequence-parallel self-attention (the fork's / xDiT-USP's gather-then-
// flash_attention [EXT]); the reference itself has no such path (one GPU, [R infinicube/inference/guidance_buffer_generation.py:759-766]).
#include <type_traits>
#include "attn_common.h"

namespace att7p {

using attc::D;
using attc::NEG_BIG;
using attc::lds_read_tr16;
constexpr int KVB = 64;
constexpr int TILE_BYTES = KVB * D * 2;      // 16 KiB (K or V)
constexpr int STAGE_BYTES = 2 * TILE_BYTES;  // 32 KiB
constexpr int NST = 4, NW = 8, NI = 16 / NW, QB = NW * 32;
constexpr int LDS_BYTES = NST * STAGE_BYTES + 64;   // ring + the verdict words
constexpr int MAX_PIECES = ICV_ATTN_MAX_PIECES;

struct Piece {
  const bf16_t* k;
  const bf16_t* v;
  int rows;
  int flag;          // index into Params::flags; < 0: the rows are there when the launch starts
  unsigned value;    // arrived when (int)(flags[flag] - value) >= 0
  int pad;
};

struct Params {
  attc::Params a;                      // q / o / strides / heads / nqb / scale / trace (k, v, Skv unused)
  const unsigned* flags;
  unsigned* err;                       // first time-out wins: 0x80000000 | piece index
  unsigned long long timeout_ticks;    // 100 MHz s_memrealtime ticks; 0 = wait for ever
  unsigned long long* ptrace;          // diagnostics: [work-group][piece] tick at which the piece's first tile was started
  int n_pieces;
  Piece piece[MAX_PIECES];
  // frame-windowed instantiation only (keys / values: a.k, a.v; a.Sq = frames * frame_rows); behind the pieces, so that nothing the
  // other instantiations read moves
  int fw_frames, fw_frame_rows, fw_window, fw_sink;
};

__device__ __forceinline__ void dma16(const void* gsrc, unsigned lds_dst) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, off\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(gsrc), "s"(lds_dst)
      : "memory");
}

__device__ __forceinline__ void dma16s(const void* base, unsigned off, unsigned lds_dst) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %3\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, %2\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(off), "s"(base), "s"(lds_dst)
      : "memory");
}

// SLIM: one FULL tile of the ring, this wave's share of it - K pieces j = 0, 1 to lds_dst and lds_dst + 1 KiB, the V pieces TILE_BYTES
// further on.  M0 is written and read inside the statement and NOT put back (the compiler keeps nothing in it: the clobber says so);
// the instruction's offset: field moves the LDS address AND the global address, so piece 1 shares piece 0's M0 and its lane offset
// comes in 1 KiB short (ko1 / vo1: ko[1] / vo[1] of a SLIM kernel).  The s_nop is the wait state between an SALU write of M0 and the
// LDS-DMA that reads it: the compiler pads nothing inside a string.  Two M0 writes and two wait states per tile, where dma16s has
// twelve moves and four.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"      // "clobber list contains reserved registers: m0" - reserved, and still to be named
__device__ __forceinline__ void dma_tile_slim(const void* kt, const void* vt, unsigned ko0, unsigned ko1, unsigned vo0, unsigned vo1,
                                              unsigned lds_dst) {
  asm volatile(
      "s_mov_b32 m0, %6\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %0, %4\n\t"
      "global_load_lds_dwordx4 %1, %4 offset:1024\n\t"
      "s_add_u32 m0, %6, %7\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %2, %5\n\t"
      "global_load_lds_dwordx4 %3, %5 offset:1024"
      :
      : "v"(ko0), "v"(ko1), "v"(vo0), "v"(vo1), "s"(kt), "s"(vt), "s"(lds_dst), "i"(TILE_BYTES)
      : "memory", "m0", "scc");
}
#pragma clang diagnostic pop

// uncached (system-scope) dword load WITHOUT a compiler-inserted wait: the caller consumes the value after its own s_waitcnt vmcnt(0)
__device__ __forceinline__ unsigned load_flag_async(const unsigned* f) {
  unsigned v;
  asm volatile("global_load_dword %0, %1, off sc0 sc1" : "=v"(v) : "v"(f) : "memory");
  return v;
}

// FW: the frame-windowed instantiation (see the head of this file)
// MF (option "attn_mfma"): 32 = v_mfma_f32_32x32x16_bf16, the tile below; 16 = v_mfma_f32_16x16x32_bf16 at the same wave tile, ring and
// softmax: attc::tile16 (attn_common.h, lane maps there), the tile attn7.hip runs at MF = 16 - the two stay bit-identical at either shape
// LEAN (MF = 16 only, option "attn_tile16_lean", default on): attc::tile16's lean body - K / V fragment addresses formed once and moved with the ring
// SLIM (LEAN only, option "attn7p_slim"): a third form of the key loop.  Every interval whose two tiles and two requested tiles are full
// tiles of the current piece, with two more intervals of the piece behind it, runs a STEADY body: no last-interval, second-tile, clamp,
// ragged-tile, tail-mask or poll test, the two requests through dma_tile_slim from running K / V tile pointers and a ring destination
// that alternates between its two values.  The last intervals of a piece (ragged tile, odd count, the run through a boundary, the
// poll, a bubble) are the loop below, unchanged.  Same tiles, same requests in the same order between the same barriers, same LDS
// bytes: outputs and carried state are bit-identical (tests/test_attn_slim_loop_gpu.py).  SLIM stands in front of LEAN so that an
// instantiation's name still ends in its LEAN value.
template <bool UNIT, bool FW, int MF, bool SLIM = false, bool LEAN = false>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(2))) void attn7p_kernel(Params pp) {
  static_assert(MF == 16 || MF == 32, "MF: 16 (16x16x32 MFMAs) or 32 (32x32x16)");
  static_assert(MF == 16 || !LEAN, "the lean body is a body of the MF = 16 tile");
  static_assert(LEAN || !SLIM, "the slim loop is a loop around the lean body");
  const attc::Params& p = pp.a;
  const float p_lim = __builtin_amdgcn_exp2f(p.thr);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  volatile unsigned* verdict = reinterpret_cast<volatile unsigned*>(smem + NST * STAGE_BYTES);   // [2]: double-buffered by interval parity
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5;
  const int l31 = lane & 31;

  int head, qb;
  attc::work_item(p, head, qb);
  int64_t q0 = (int64_t)qb * QB + wave * 32;
  int64_t q_end = 0;                    // FW: first row this work-group may neither read as a query nor store (the others: p.Sq)
  // FW: this work-group's pieces, in frames [fw_a, fw_b) (wave-uniform scalars), and how many of them.  They derive from blockIdx and
  // kernel arguments ONLY, so they - and P_ROWS / skv_d / nt_d, the loop bounds made of them - live in SGPRs without a readfirstlane;
  // mix in nothing per-lane (tid, lane, a loaded value) or those bounds turn into VGPR values and the loops into divergent ones.
  int fw_np = 1, fw_a0 = 0, fw_b0 = 0, fw_a1 = 0, fw_b1 = 0;
  if constexpr (FW) {
    const int T = pp.fw_frames, F = pp.fw_frame_rows, W = pp.fw_window, sink = pp.fw_sink;
    const int bpf = (F + QB - 1) / QB;  // q-blocks per frame
    const int f = qb / bpf;
    q0 = (int64_t)f * F + (qb - f * bpf) * QB + wave * 32;
    q_end = (int64_t)(f + 1) * F;
    const int lo = f - W > 0 ? f - W : 0;
    const int hi = f + W + 1 < T ? f + W + 1 : T;
    if (sink == 0) {
      fw_a0 = lo; fw_b0 = hi;
    } else if (lo <= sink) {            // the window touches or overlaps the sink: one piece
      fw_a0 = 0; fw_b0 = hi > sink ? hi : sink;
    } else {
      fw_np = 2;
      fw_a0 = 0; fw_b0 = sink;
      fw_a1 = lo; fw_b1 = hi;
    }
  }
  const unsigned long long t_start = p.trace ? __builtin_amdgcn_s_memrealtime() : 0ull;
  const bf16_t* qh = p.q + (int64_t)head * D;
  int64_t qr_c = q0 + l31;
  if constexpr (FW) qr_c = qr_c < q_end ? qr_c : q_end - 1;
  else qr_c = qr_c < p.Sq ? qr_c : p.Sq - 1;

  // ---- softmax state (registers, across all pieces) ----
  f32x16 ot[4];
  float m_run = NEG_BIG, l_run = 0.f;
  attc::Tile16 s16;                  // MF == 16: state, reference and Q fragments of the wave's two 16-row q-blocks
  int64_t qr16[2] = {0, 0};
  if constexpr (MF == 16) {
    const int64_t q_lim = FW ? q_end : p.Sq;
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      const int64_t r = q0 + qb * 16 + (lane & 15);
      qr16[qb] = r < q_lim ? r : q_lim - 1;
    }
    attc::tile16_init<UNIT>(p, qr16, head, lane >> 4, s16);
  } else {
    attc::load_state(p, qr_c, head, hi, ot, m_run, l_run);
  }
  float m_base = m_run < -1.0e29f ? 0.f : m_run;
  f32x16 cinit;
  const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int r = 0; r < 16; ++r) cinit[r] = UNIT ? -m_base : 0.f;

  bf16x8 qf[8];
  if constexpr (MF == 16) attc::tile16_load_q(p, qr16, head, lane >> 4, s16);
  else {
    const bf16_t* qp = qh + qr_c * p.ldq + hi * 8;
#pragma unroll
    for (int ds = 0; ds < 8; ++ds) qf[ds] = *reinterpret_cast<const bf16x8*>(qp + ds * 16);
  }
  __builtin_amdgcn_s_waitcnt(0x0F70);     // retire the VGPR-destination loads before any LDS-DMA is in flight (cdna guide §5 trap (b))

  // ---- LDS-DMA lane mapping (attn7.hip) ----
  const int pc = lane & 15;
  const unsigned lds_base = (unsigned)(uintptr_t)((__attribute__((address_space(3))) char*)smem);
  int dkey[NI], kcol[NI], vcol[NI];
  unsigned ko[NI], vo[NI];
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    dkey[j] = (wave * NI + j) * 4 + (lane >> 4);
    kcol[j] = (pc ^ (dkey[j] & 15)) * 8;
    vcol[j] = MF == 16 ? attc::tile16_vcol(pc, dkey[j]) : (pc ^ ((dkey[j] & 3) << 2)) * 8;
    // SLIM: piece j's lane offset comes in j KiB short, and its requests make that up in the offset: field (dma_tile_slim) or in the
    // base (P_DMA_TILE).  It stays >= 0: piece 1 starts at row >= 4 and launch() takes SLIM only for rows of 256 B or more
    ko[j] = (unsigned)(((int64_t)dkey[j] * p.ldk + kcol[j]) * 2) - (SLIM ? j * 1024u : 0u);
    vo[j] = (unsigned)(((int64_t)dkey[j] * p.ldv + vcol[j]) * 2) - (SLIM ? j * 1024u : 0u);
  }

  // ---- the piece the DMA side reads (wave-uniform) ----
  const bf16_t* kh_d = nullptr;
  const bf16_t* vh_d = nullptr;
  int skv_d = 0, nt_d = 0;
#define P_ROWS(J_) (FW ? ((J_) ? fw_b1 - fw_a1 : fw_b0 - fw_a0) * pp.fw_frame_rows : __builtin_amdgcn_readfirstlane(pp.piece[FW ? 0 : (J_)].rows))
#define P_SET_DMA_PIECE(J_)                                              \
  {                                                                      \
    if constexpr (FW) {                                                  \
      const int64_t r0_ = (int64_t)((J_) ? fw_a1 : fw_a0) * pp.fw_frame_rows; \
      kh_d = p.k + r0_ * p.ldk + (int64_t)head * D;                      \
      vh_d = p.v + r0_ * p.ldv + (int64_t)head * D;                      \
      skv_d = P_ROWS(J_);                                                \
    } else {                                                             \
      const Piece& pc_ = pp.piece[(J_)];                                 \
      kh_d = pc_.k + (int64_t)head * D;                                  \
      vh_d = pc_.v + (int64_t)head * D;                                  \
      skv_d = __builtin_amdgcn_readfirstlane(pc_.rows);                  \
    }                                                                    \
    nt_d = (skv_d + KVB - 1) / KVB;                                      \
  }
  // tile T_ of the DMA piece (clamped to its last tile: a request past the end re-reads that tile into a dead stage) -> ring stage STG_
#define P_DMA_TILE(T_, STG_)                                                                         \
  {                                                                                                  \
    const int tt_ = (T_) < nt_d ? (T_) : nt_d - 1;                                                   \
    const unsigned l0_ = lds_base + (unsigned)(((STG_) & (NST - 1)) * STAGE_BYTES + (wave * NI) * 1024); \
    if ((tt_ + 1) * KVB <= skv_d) {                                                                  \
      const bf16_t* kt_ = kh_d + (int64_t)tt_ * KVB * p.ldk;                                         \
      const bf16_t* vt_ = vh_d + (int64_t)tt_ * KVB * p.ldv;                                         \
      _Pragma("unroll") for (int j_ = 0; j_ < NI; ++j_) dma16s(kt_ + (SLIM ? j_ * 512 : 0), ko[j_], l0_ + j_ * 1024); \
      _Pragma("unroll") for (int j_ = 0; j_ < NI; ++j_) dma16s(vt_ + (SLIM ? j_ * 512 : 0), vo[j_], l0_ + TILE_BYTES + j_ * 1024); \
    } else {                                                                                         \
      _Pragma("unroll") for (int j_ = 0; j_ < NI; ++j_) {                                            \
        int64_t r_ = (int64_t)tt_ * KVB + dkey[j_];                                                  \
        r_ = r_ < skv_d ? r_ : skv_d - 1;                                                            \
        dma16(kh_d + r_ * p.ldk + kcol[j_], l0_ + j_ * 1024);                                        \
        dma16(vh_d + r_ * p.ldv + vcol[j_], l0_ + TILE_BYTES + j_ * 1024);                           \
      }                                                                                              \
    }                                                                                                \
  }
#define P_BARRIER()                                           \
  do {                                                        \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");        \
    __builtin_amdgcn_s_barrier();                             \
    asm volatile("" ::: "memory");                            \
    __builtin_amdgcn_sched_barrier(0);                        \
  } while (0)
  // blocking wait for piece J_ (a bubble): ONE lane polls, everybody else parks at the barrier; bounded by the time-out
#define P_WAIT_PIECE(J_)                                                                                          \
  if constexpr (!FW) {                                                                                            \
    const int fi_ = __builtin_amdgcn_readfirstlane(pp.piece[(J_)].flag);                                          \
    if (fi_ >= 0) {                                                                                               \
      if (tid == 0) {                                                                                             \
        const unsigned want_ = pp.piece[(J_)].value;                                                              \
        const unsigned long long t0_ = __builtin_amdgcn_s_memrealtime();                                          \
        while ((int)(__hip_atomic_load(pp.flags + fi_, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) - want_) < 0) { \
          __builtin_amdgcn_s_sleep(16);                                                                           \
          /* fail fast: once ANY work-group of any launch has given up, nobody waits out the deadline again */    \
          if (pp.err && __hip_atomic_load(pp.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) break;       \
          if (pp.timeout_ticks && __builtin_amdgcn_s_memrealtime() - t0_ > pp.timeout_ticks) {                    \
            if (pp.err) atomicCAS(pp.err, 0u, 0x80000000u | (unsigned)(J_));                                      \
            break;                                                                                                \
          }                                                                                                       \
        }                                                                                                         \
      }                                                                                                           \
      P_BARRIER();                                                                                                \
    }                                                                                                             \
  }

  const int k_row_off = l31 * 256;
  const int k_sw = l31 & 15;
  const int g = lane >> 4, t16 = lane & 15;
  const int v_key_lo = 4 * hi + (t16 >> 2);
  const int v_byte_lo = (g & 1) * 32 + (t16 & 3) * 8;
  const int v_sw = (t16 >> 2) << 6;

  // one 64-key tile from ring stage `stg`: keys [key0, key0 + 64) of a piece with `skv` rows (attn7.hip's tile, variant 148 / 132)
  // par: stg's parity as a std::integral_constant (an interval takes an even and an odd stage per barrier).  LEAN: la16 points at
  // the even stage of the interval's half of the ring and is moved to the other half once per interval.
  attc::Tile16Addr la16;
  int la16_step = 2 * STAGE_BYTES;
  if constexpr (LEAN) {
    attc::tile16_lean_addr(lds_base, lane, la16);
    attc::tile16_lean_lim<UNIT>(s16, p_lim, la16);
  }
  auto tile = [&](const auto par, const int stg, const int key0, const int skv) __attribute__((always_inline)) {
    if constexpr (LEAN) {
      attc::tile16<UNIT, false, true, true, true, decltype(par)::value>(p, p_lim, nullptr, nullptr, key0, skv, lane, s16, &la16);
      return;
    }
    const char* ks = smem + (stg & (NST - 1)) * STAGE_BYTES;
    const char* vs = ks + TILE_BYTES;
    if constexpr (MF == 16) {
      attc::tile16<UNIT, false, true, true>(p, p_lim, ks, vs, key0, skv, lane, s16);
      return;
    }
    f32x16 st[2];
    const bool no_ref = UNIT && m_run < -1.0e29f;
#pragma unroll
    for (int ds = 0; ds < 8; ++ds)
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        const int c = ds * 2 + hi;
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(ks + kb * 8192 + k_row_off + ((c ^ k_sw) << 4));
        st[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ds], ds == 0 ? (UNIT ? cinit : zero16) : st[kb], 0, 0, 0);
      }
    if (key0 + KVB > skv) {
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = key0 + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
          if (key >= skv) st[kb][r] = NEG_BIG;
        }
    }
    float mb = -m_run * p.sc;
    float psum = 0.f;
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      bf16x8 pf[2];
      float ps = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float pv = UNIT ? __builtin_amdgcn_exp2f(st[kb][r]) : __builtin_amdgcn_exp2f(fmaf(st[kb][r], p.sc, mb));
        ps += pv;
        pf[r >> 3][r & 7] = (__bf16)pv;
      }
      if (__any(!(ps <= p_lim) || no_ref)) {      // lazy max (attn2.hip): the partial row sum bounds every P of the block
        float mloc = st[kb][0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mloc = fmaxf(mloc, st[kb][r]);
        mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
        if (UNIT) mloc += m_base;
        const float m_new = fmaxf(m_run, mloc);
        const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * p.sc);
        m_run = m_new;
        l_run = (l_run + psum) * alpha;
        psum = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) ot[i][r] *= alpha;
        mb = -m_run * p.sc;
        if (UNIT) {
          const float dm = m_new - m_base;
          m_base = m_new;
#pragma unroll
          for (int j = 0; j < 2; ++j)
            if (j >= kb) {
#pragma unroll
              for (int r = 0; r < 16; ++r) st[j][r] -= dm;
            }
#pragma unroll
          for (int r = 0; r < 16; ++r) cinit[r] = -m_new;
        }
        ps = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float pv = UNIT ? __builtin_amdgcn_exp2f(st[kb][r]) : __builtin_amdgcn_exp2f(fmaf(st[kb][r], p.sc, mb));
          ps += pv;
          pf[r >> 3][r & 7] = (__bf16)pv;
        }
      }
      psum += ps;
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        const int kk = kb * 2 + hf;
#pragma unroll
        for (int d0 = 0; d0 < 4; ++d0) {
          const int key_l = kk * 16 + v_key_lo;
          const int byte = (d0 * 64 + v_byte_lo) ^ v_sw;
          const bf16x4 va = lds_read_tr16(vs + key_l * 256 + byte);
          const bf16x4 vb = lds_read_tr16(vs + (key_l + 8) * 256 + byte);
          bf16x8 vf;
          vf[0] = va[0]; vf[1] = va[1]; vf[2] = va[2]; vf[3] = va[3];
          vf[4] = vb[0]; vf[5] = vb[1]; vf[6] = vb[2]; vf[7] = vb[3];
          ot[d0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[hf], ot[d0], 0, 0, 0);
        }
      }
    }
    __builtin_amdgcn_s_setprio(0);
    l_run += psum;
  };

  // ---- walk the pieces ----
  const int np = FW ? fw_np : __builtin_amdgcn_readfirstlane(pp.n_pieces);
  // the host passes no empty list and no empty piece: without the path that skips the loops the register allocator no longer parks
  // accumulators in scratch between prologue and epilogue (MF = 16 only: the 32 form's instruction stream stays what it was)
  if constexpr (MF == 16) __builtin_assume(np >= 1);
  unsigned gt = 0;                 // ring position of the current piece's tile 0 (always even)
  unsigned iv = 0;                 // interval counter (verdict word parity)
  P_WAIT_PIECE(0);
  P_SET_DMA_PIECE(0);
  P_DMA_TILE(0, gt);
  P_DMA_TILE(1, gt + 1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  P_BARRIER();
  for (int pj = 0; pj < np; ++pj) {
    const int skv = P_ROWS(pj);
    const int nt = (skv + KVB - 1) / KVB;
    if constexpr (MF == 16) __builtin_assume(nt >= 1);
    const unsigned g_next = gt + (unsigned)((nt + 1) & ~1);
    const bool has_next = pj + 1 < np;
    const int nflag = has_next && !FW ? __builtin_amdgcn_readfirstlane(pp.piece[has_next ? pj + 1 : pj].flag) : -1;
    const unsigned nvalue = has_next && !FW ? pp.piece[has_next ? pj + 1 : pj].value : 0u;
    bool next_ready = has_next && nflag < 0;      // wave-uniform
    bool next_issued = false;
    if (!FW && pp.ptrace && tid == 0) pp.ptrace[(size_t)blockIdx.x * np + pj] = __builtin_amdgcn_s_memrealtime();
    int t_steady = 0;                 // SLIM: the first tile the loop below takes
    if constexpr (SLIM) {
      int t = 0;
      // steady intervals: tiles t .. t + 5 are full tiles of this piece, so two intervals of the loop below always follow - the first of
      // them takes the flag sample that the last one's verdict comes from, as it does without SLIM (a flag, once there, stays)
      const int t_last = (skv >> 6) - 6;
      if (t_last >= 0) {
        const int64_t kstep = (int64_t)KVB * p.ldk, vstep = (int64_t)KVB * p.ldv;     // the DMA piece is this piece (see P_SET_DMA_PIECE's callers)
        const bf16_t* kt_d = kh_d + 2 * kstep;                                       // tile t + 2
        const bf16_t* vt_d = vh_d + 2 * vstep;
        const unsigned l_w = lds_base + (unsigned)(wave * NI * 1024);
        unsigned l0_d = l_w + (unsigned)(((gt + 2) & (NST - 1)) * STAGE_BYTES);      // gt is even: stage 0 or 2, and the other one next time
        const unsigned l_sum = 2 * l_w + 2 * STAGE_BYTES;
        // the second tile stands behind a test the compiler cannot see through (always taken: one s_cmp and one branch per interval).
        // Without the join behind it the allocator lets the PV accumulators wander (D != C), pads 12 wait states per interval in front
        // of the LDS reads that reuse a C register, and takes 251 VGPRs at UNIT = false; with it: none, 209 / 197 VGPRs
        // (profiles/attn_slim_loop/README.md)
        int yes = 1;
        asm volatile("" : "+s"(yes));
        static_assert(NI == 2, "dma_tile_slim issues two K and two V pieces per wave");
        for (; t <= t_last; t += 2) {
          dma_tile_slim(kt_d, vt_d, ko[0], ko[1], vo[0], vo[1], l0_d);
          dma_tile_slim(kt_d + kstep, vt_d + vstep, ko[0], ko[1], vo[0], vo[1], l0_d + STAGE_BYTES);
          kt_d += 2 * kstep;
          vt_d += 2 * vstep;
          l0_d = l_sum - l0_d;
          tile(std::integral_constant<int, 0>{}, 0, 0, KVB);                        // a full tile: key0 + KVB > skv is false where it is written
          if (yes) tile(std::integral_constant<int, 1>{}, 0, 0, KVB);
          attc::tile16_lean_advance(la16, la16_step);
          la16_step = -la16_step;
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          P_BARRIER();
        }
        t_steady = t;
      }
    }
    for (int t = SLIM ? t_steady : 0; t < nt; t += 2) {
      const bool last_iv = t + 2 >= nt;
      if (!last_iv) {                                    // the other half of the ring: last read in the previous interval
        P_DMA_TILE(t + 2, gt + t + 2);
        P_DMA_TILE(t + 3, gt + t + 3);
      } else if (has_next && next_ready) {               // run through the boundary: the next piece's first interval
        P_SET_DMA_PIECE(pj + 1);
        P_DMA_TILE(0, g_next);
        P_DMA_TILE(1, g_next + 1);
        next_issued = true;
      }
      const bool poll = has_next && !next_ready;         // wave-uniform
      unsigned fv = 0;
      if (poll && wave == 0) fv = load_flag_async(pp.flags + nflag);
      tile(std::integral_constant<int, 0>{}, (int)(gt + t), t * KVB, skv);
      if (t + 1 < nt) tile(std::integral_constant<int, 1>{}, (int)(gt + t + 1), (t + 1) * KVB, skv);
      if constexpr (LEAN) {                              // the next interval reads the other half: gt + t is 2 (mod 4) further on
        attc::tile16_lean_advance(la16, la16_step);
        la16_step = -la16_step;
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this interval's DMA requests and the flag sample
      if (poll && tid == 0) verdict[iv & 1] = (int)(fv - nvalue) >= 0 ? 1u : 0u;
      P_BARRIER();
      if (poll) next_ready = __builtin_amdgcn_readfirstlane(verdict[iv & 1]) != 0;
      ++iv;
    }
    if (!has_next) break;
    if (!next_issued) {                                  // bubble: the next piece was not known to be there in time
      if (!next_ready) P_WAIT_PIECE(pj + 1);
      P_SET_DMA_PIECE(pj + 1);
      P_DMA_TILE(0, g_next);
      P_DMA_TILE(1, g_next + 1);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      P_BARRIER();
    }
    gt = g_next;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  // FW: a row past the frame's end belongs to the next frame's work-group - hand store_result a row it does not store
  if constexpr (MF == 16) {
    int64_t qr[2];
    int t16 = lane & 15;
    asm volatile("" : "+v"(t16));      // recompute the rows here: carried from the prologue they cost four VGPRs through the whole loop
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      const int64_t r = q0 + qb * 16 + t16;
      qr[qb] = !FW || r < q_end ? r : p.Sq;
    }
    attc::store_result(p, qr, head, lane >> 4, s16.ot, s16.m_run, s16.l_run);
  } else {
    attc::store_result(p, !FW || q0 + l31 < q_end ? q0 + l31 : p.Sq, head, hi, ot, m_run, l_run);
  }
  if (p.trace && tid == 0 && (int)blockIdx.x < p.trace_cap) {
    unsigned hwid, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    unsigned long long* t = p.trace + (size_t)blockIdx.x * 4;
    t[0] = t_start; t[1] = __builtin_amdgcn_s_memrealtime(); t[2] = hwid; t[3] = xcc;
  }
#undef P_ROWS
#undef P_SET_DMA_PIECE
#undef P_DMA_TILE
#undef P_BARRIER
#undef P_WAIT_PIECE
}

// STAGGERED long-key kernel (option "attn7p_stagger"; profiles/attn_stagger/README.md): ONE piece that is there when the launch starts
// (flag < 0), the lean body of the 16x16x32 tile cut in two (attc::tile16_qk, attc::tile16_sv) and the slim loop's DMA requests.  The
// two waves of a SIMD - wave w and wave w + 4 - run in OPPOSITE phases of the tile, so that one is in its 32 exps while the other is in
// a 32-MFMA run: in attn7p_kernel every wave leaves every barrier into the same QK^T MFMAs and meets its partner again at the exps,
// where the matrix pipe has nothing to do.  (The STAGGER bit of attn1 / 2 / 4 / 7 / 8 delays waves 4-7 by a WHOLE tile, the period of
// the work: the partners are back in phase, on different tiles.)  Every wave still executes QK(0) SV(0) QK(1) SV(1) ... on its own rows
// with the arithmetic of tile16's lean body, so outputs and carried state are bit-identical to attn7p_kernel's
// (tests/test_attn_stagger_gpu.py); only the barriers and the DMA issue are placed differently.  nt tiles, nt + 1 slots, a barrier
// between two slots (nt barriers per wave); tile t lives in ring stage t & 3; slot h is
//     group A:  QK(h) SV(h)                      (nothing in slot nt)
//     group B:  SV(h - 1) QK(h), st carried across the barrier       (QK(0) only in slot 0, SV(nt - 1) only in slot nt)
// SWAP (option "attn7p_stagger_swap"): false = waves 0-3 are A and waves 4-7 B, true = waves 0-3 are B and waves 4-7 A.  true is the
// default and what won: the older half (waves 0-3), whose VALU issue the arbiter favours, opens its slot with the softmax and the
// younger half opens it with MFMAs, which issue at full rate behind a barrier for either (20.79 vs 21.33 ms of the slim loop at the 14B
// self-attention, interleaved; false: 21.34 - 21.60 ms, a tie, with LESS VALU / MFMA co-execution than the slim loop has).
// INVARIANTS OF THE RING
//   (1) Slot h reads K of tile h (A and B), V of tile h (A) and V of tile h - 1 (B): stages h & 3 and (h - 1) & 3.
//   (2) At the START of slot h every wave requests its share (2 K + 2 V requests) of tile h + 2, if there is one, into stage
//       (h + 2) & 3 = the stage of tile h - 2, whose K was last read in slot h - 2 and whose V in slot h - 1 (B): both behind the
//       barrier that ended slot h - 1, and every wave drains lgkmcnt in front of a barrier.  No request goes to a stage of (1).
//   (3) A slot ends with s_waitcnt vmcnt(4) + barrier when it requested a tile and vmcnt(0) + barrier when it did not: requests retire
//       in order and the key loop issues no other vector memory instruction, so behind the wait this wave's four requests of tile
//       h + 1 have landed (only tile h + 2's four may be in flight: LDS-DMA survives s_barrier), and behind the barrier every wave's.
//       Tile h + 1 is what slot h + 1 reads first; tile h landed one barrier earlier.  Tiles 0 and 1 are requested in front of slot 0
//       and waited for together.
//   (4) A ragged last tile takes four requests per wave as a full one does (rows clamped to the last one), so (3) counts the same.
//   (5) A and B execute the same number of barriers (one per slot 0 .. nt - 1) and the same requests in the same slots; B's SV(nt - 1)
//       behind the last barrier reads a tile that landed two barriers earlier, and nothing is requested behind it.
// Cost against attn7p_kernel: one barrier per 64 keys instead of one per 128.  PRIO (option "attn7p_stagger_setprio"): s_setprio 1 over
// softmax + PV, as tile16 has it - with SWAP it is what makes the difference (21.56 ms without).
template <bool UNIT, bool PRIO, bool SWAP>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(2))) void attn7ps_kernel(Params pp) {
  const attc::Params& p = pp.a;
  const float p_lim = __builtin_amdgcn_exp2f(p.thr);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  int head, qb;
  attc::work_item(p, head, qb);
  const int64_t q0 = (int64_t)qb * QB + wave * 32;
  const unsigned long long t_start = p.trace ? __builtin_amdgcn_s_memrealtime() : 0ull;

  // ---- softmax state, reference and Q fragments of the wave's two 16-row q-blocks (registers) ----
  attc::Tile16 s16;
  int64_t qr16[2];
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    const int64_t r = q0 + qb * 16 + (lane & 15);
    qr16[qb] = r < p.Sq ? r : p.Sq - 1;
  }
  attc::tile16_init<UNIT>(p, qr16, head, lane >> 4, s16);
  attc::tile16_load_q(p, qr16, head, lane >> 4, s16);
  __builtin_amdgcn_s_waitcnt(0x0F70);     // retire the VGPR-destination loads before any LDS-DMA is in flight: invariant (3) counts requests only

  // ---- LDS-DMA lane mapping (attn7p_kernel's, SLIM: piece 1's lane offset comes in 1 KiB short) ----
  static_assert(NI == 2, "dma_tile_slim issues two K and two V pieces per wave");
  const int pc = lane & 15;
  const unsigned lds_base = (unsigned)(uintptr_t)((__attribute__((address_space(3))) char*)smem);
  int dkey[NI], kcol[NI], vcol[NI];
  unsigned ko[NI], vo[NI];
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    dkey[j] = (wave * NI + j) * 4 + (lane >> 4);
    kcol[j] = (pc ^ (dkey[j] & 15)) * 8;
    vcol[j] = attc::tile16_vcol(pc, dkey[j]);
    ko[j] = (unsigned)(((int64_t)dkey[j] * p.ldk + kcol[j]) * 2) - j * 1024u;
    vo[j] = (unsigned)(((int64_t)dkey[j] * p.ldv + vcol[j]) * 2) - j * 1024u;
  }
  const bf16_t* kh = pp.piece[0].k + (int64_t)head * D;
  const bf16_t* vh = pp.piece[0].v + (int64_t)head * D;
  const int skv = __builtin_amdgcn_readfirstlane(pp.piece[0].rows);
  const int nt = (skv + KVB - 1) / KVB;
  __builtin_assume(nt >= 1);
  const int64_t kstep = (int64_t)KVB * p.ldk, vstep = (int64_t)KVB * p.ldv;
  const unsigned l_w = lds_base + (unsigned)(wave * NI * 1024);
  // this wave's share of tile T_ (< nt) -> stage T_ & 3: four requests, ragged or not
  auto dma_tile = [&](const int t) __attribute__((always_inline)) {
    const unsigned l0 = l_w + (unsigned)((t & (NST - 1)) * STAGE_BYTES);
    if ((t + 1) * KVB <= skv) {
      dma_tile_slim(kh + (int64_t)t * kstep, vh + (int64_t)t * vstep, ko[0], ko[1], vo[0], vo[1], l0);
    } else {
#pragma unroll
      for (int j = 0; j < NI; ++j) {
        int64_t r = (int64_t)t * KVB + dkey[j];
        r = r < skv ? r : skv - 1;
        dma16(kh + r * p.ldk + kcol[j], l0 + j * 1024);
        dma16(vh + r * p.ldv + vcol[j], l0 + TILE_BYTES + j * 1024);
      }
    }
  };
#define S_END_SLOT(N_)                                              \
  do {                                                              \
    asm volatile("s_waitcnt vmcnt(" #N_ ") lgkmcnt(0)" ::: "memory"); \
    __builtin_amdgcn_s_barrier();                                   \
    asm volatile("" ::: "memory");                                  \
    __builtin_amdgcn_sched_barrier(0);                              \
  } while (0)
  // end of a slot of the tail: tile U_ was requested in this slot if it exists
#define S_END_SLOT_TAIL(U_)          \
  do {                               \
    if ((U_) < nt) S_END_SLOT(4);    \
    else S_END_SLOT(0);              \
  } while (0)

  attc::Tile16Addr la16;
  attc::tile16_lean_addr(lds_base, lane, la16);
  attc::tile16_lean_lim<UNIT>(s16, p_lim, la16);
  int la_step = 2 * STAGE_BYTES;
  f32x4 st[4][2];

  if (pp.ptrace && tid == 0) pp.ptrace[blockIdx.x] = __builtin_amdgcn_s_memrealtime();
  dma_tile(0);
  if (nt > 1) dma_tile(1);
  S_END_SLOT(0);
  // ONE program for both groups: every wave runs QK(t) SV(t) for t = 0 .. nt - 1; A ends its slot (and begins the next: the request)
  // behind SV(t), B behind QK(t).  is_b is wave-uniform: the branches round the barriers are scalar.
  const bool is_b = SWAP ? wave < NW / 2 : wave >= NW / 2;
  if (is_b && nt > 2) dma_tile(2);                        // B's slot 0 is QK(0) alone
  // steady pair of tiles t, t + 1 (t even): tiles t .. t + 4 are full.  A requests tiles t + 2 and t + 3 in front of QK(t) and
  // QK(t + 1), B tiles t + 3 and t + 4 in front of SV(t) and SV(t + 1): kt_d / vt_d point at the first of the two, d0 / d1 are the
  // two ring destinations - stages {2, 3} <-> {0, 1} for A, {3, 0} <-> {1, 2} for B, each alternating between its two values
  const int lead = is_b ? 3 : 2;
  const bf16_t* kt_d = kh + lead * kstep;
  const bf16_t* vt_d = vh + lead * vstep;
  unsigned d0 = l_w + (unsigned)(lead * STAGE_BYTES);
  unsigned d1 = l_w + (unsigned)(((lead + 1) & (NST - 1)) * STAGE_BYTES);
  const unsigned d0_sum = 2 * d0 - 2 * STAGE_BYTES, d1_sum = 2 * l_w + (is_b ? 2 : 4) * STAGE_BYTES;
  const int nfull = skv >> 6;        // full tiles
  int t = 0;
  for (; t <= nfull - 5; t += 2) {
    if (!is_b) dma_tile_slim(kt_d, vt_d, ko[0], ko[1], vo[0], vo[1], d0);
    attc::tile16_qk<UNIT, 0>(s16, la16, st);
    if (is_b) {
      S_END_SLOT(4);
      dma_tile_slim(kt_d, vt_d, ko[0], ko[1], vo[0], vo[1], d0);
    }
    attc::tile16_sv<UNIT, PRIO, 0>(p, p_lim, 0, KVB, lane, s16, la16, st);        // a full tile: no tail mask
    if (!is_b) {
      S_END_SLOT(4);
      dma_tile_slim(kt_d + kstep, vt_d + vstep, ko[0], ko[1], vo[0], vo[1], d1);
    }
    attc::tile16_qk<UNIT, 1>(s16, la16, st);
    if (is_b) {
      S_END_SLOT(4);
      dma_tile_slim(kt_d + kstep, vt_d + vstep, ko[0], ko[1], vo[0], vo[1], d1);
    }
    attc::tile16_sv<UNIT, PRIO, 1>(p, p_lim, 0, KVB, lane, s16, la16, st);
    attc::tile16_lean_advance(la16, la_step);
    la_step = -la_step;
    kt_d += 2 * kstep;
    vt_d += 2 * vstep;
    d0 = d0_sum - d0;
    d1 = d1_sum - d1;
    if (!is_b) S_END_SLOT(4);
  }
  // the last slots (ragged tile, odd count, drain), t even.  B's SV(nt - 1) stands behind the last barrier
  for (; t < nt; t += 2) {
    if (!is_b && t + 2 < nt) dma_tile(t + 2);
    attc::tile16_qk<UNIT, 0>(s16, la16, st);
    if (is_b) {
      S_END_SLOT_TAIL(t + 2);
      if (t + 3 < nt) dma_tile(t + 3);
    }
    attc::tile16_sv<UNIT, PRIO, 0>(p, p_lim, (int64_t)t * KVB, skv, lane, s16, la16, st);
    if (!is_b) S_END_SLOT_TAIL(t + 2);
    if (t + 1 >= nt) break;
    if (!is_b && t + 3 < nt) dma_tile(t + 3);
    attc::tile16_qk<UNIT, 1>(s16, la16, st);
    if (is_b) {
      S_END_SLOT_TAIL(t + 3);
      if (t + 4 < nt) dma_tile(t + 4);
    }
    attc::tile16_sv<UNIT, PRIO, 1>(p, p_lim, (int64_t)(t + 1) * KVB, skv, lane, s16, la16, st);
    attc::tile16_lean_advance(la16, la_step);
    la_step = -la_step;
    if (!is_b) S_END_SLOT_TAIL(t + 3);
  }
#undef S_END_SLOT
#undef S_END_SLOT_TAIL
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  {
    int64_t qr[2];
    int t16 = lane & 15;
    asm volatile("" : "+v"(t16));      // recompute the rows here: carried from the prologue they cost four VGPRs through the whole loop
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) qr[qb] = q0 + qb * 16 + t16;
    attc::store_result(p, qr, head, lane >> 4, s16.ot, s16.m_run, s16.l_run);
  }
  if (p.trace && tid == 0 && (int)blockIdx.x < p.trace_cap) {
    unsigned hwid, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    unsigned long long* tr = p.trace + (size_t)blockIdx.x * 4;
    tr[0] = t_start; tr[1] = __builtin_amdgcn_s_memrealtime(); tr[2] = hwid; tr[3] = xcc;
  }
}

template <bool UNIT, bool PRIO, bool SWAP>
int launch_stagger(const Params& pp, hipStream_t st) {
  static icv_dev_flags attr_set = {};
  if (int rc = icv_ensure_dynamic_lds((const void*)attn7ps_kernel<UNIT, PRIO, SWAP>, NST * STAGE_BYTES, &attr_set, "attn7ps")) return rc;
  const int64_t nwg = (int64_t)pp.a.heads * pp.a.nqb;
  hipLaunchKernelGGL((attn7ps_kernel<UNIT, PRIO, SWAP>), dim3((unsigned)nwg), dim3(NW * 64), NST * STAGE_BYTES, st, pp);
  return icv_check_launch("icv_attention_fwd (staggered)");
}

template <bool UNIT, bool FW, int MF, bool SLIM = false, bool LEAN = false>
int launch_mf(const Params& pp, hipStream_t st) {
  static icv_dev_flags attr_set = {};
  if (int rc = icv_ensure_dynamic_lds((const void*)attn7p_kernel<UNIT, FW, MF, SLIM, LEAN>, LDS_BYTES, &attr_set, "attn7p")) return rc;
  const int64_t nwg = (int64_t)pp.a.heads * pp.a.nqb;
  hipLaunchKernelGGL((attn7p_kernel<UNIT, FW, MF, SLIM, LEAN>), dim3((unsigned)nwg), dim3(NW * 64), LDS_BYTES, st, pp);
  return icv_check_launch(FW ? "icv_attention_fwd_framewin" : "icv_attention_fwd_pieces");
}

// the MFMA shape follows option "attn_mfma" (attention.hip: icv_attn_mfma), as attn7.hip's long-key kernel does
template <bool UNIT, bool FW = false>
int launch(const Params& pp, hipStream_t st) {
  const int mf = icv_attn_mfma(false);
  if (mf < 0) return 1;
  if (mf != 16) return launch_mf<UNIT, FW, 32>(pp, st);
  const int lean = icv_attn_tile16_lean(false);     // body of the MF = 16 tile (option "attn_tile16_lean")
  if (lean < 0) return 1;
  if (!lean) return launch_mf<UNIT, FW, 16>(pp, st);
  if constexpr (!FW) {
    const int slim = icv_attn7p_slim();             // form of the key loop around the lean body (option "attn7p_slim")
    if (slim < 0) return 1;
    // dma_tile_slim takes a lane offset 1 KiB short of a row >= 4: rows of 256 B or more, which is every layout but a degenerate one
    if (slim && pp.a.ldk >= D && pp.a.ldv >= D) {
      const int stagger = icv_attn7p_stagger();     // one piece that is there: the staggered kernel (option "attn7p_stagger")
      const int prio = icv_attn7p_stagger_setprio(), swap = icv_attn7p_stagger_swap();
      if (stagger < 0 || prio < 0 || swap < 0) return 1;
      if (stagger && pp.n_pieces == 1 && pp.piece[0].flag < 0) {
        if (swap) return prio ? launch_stagger<UNIT, true, true>(pp, st) : launch_stagger<UNIT, false, true>(pp, st);
        return prio ? launch_stagger<UNIT, true, false>(pp, st) : launch_stagger<UNIT, false, false>(pp, st);
      }
      return launch_mf<UNIT, FW, 16, true, true>(pp, st);
    }
  }
  return launch_mf<UNIT, FW, 16, false, true>(pp, st);
}

}  // namespace att7p

extern "C" int icv_attention_fwd_pieces(const void* q, int64_t ldq, const icv_kv_piece* pieces, int64_t n_pieces, int64_t ldk, int64_t ldv,
                                        void* o, int64_t ldo, int64_t Sq, int64_t heads, float scale, const uint32_t* flags, uint32_t* err,
                                        int64_t timeout_us, void* trace, void* stream) {
  ICV_REQUIRE(q && pieces && o, "icv_attention_fwd_pieces: null pointer");
  ICV_REQUIRE(Sq > 0 && heads > 0 && n_pieces > 0, "icv_attention_fwd_pieces: empty problem (Sq=%lld heads=%lld pieces=%lld)", (long long)Sq,
              (long long)heads, (long long)n_pieces);
  ICV_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 4 == 0, "icv_attention_fwd_pieces: leading dims must keep 16-byte row alignment");
  att7p::Params pp;
  int64_t total = 0;
  int n = 0;
  for (int64_t i = 0; i < n_pieces; ++i) {
    const icv_kv_piece& s = pieces[i];
    ICV_REQUIRE(s.rows >= 0 && s.rows < (1LL << 31) / 64, "icv_attention_fwd_pieces: piece %lld has %lld rows", (long long)i, (long long)s.rows);
    if (s.rows == 0) continue;
    ICV_REQUIRE(n < att7p::MAX_PIECES, "icv_attention_fwd_pieces: more than %d non-empty pieces", att7p::MAX_PIECES);
    ICV_REQUIRE(s.k && s.v, "icv_attention_fwd_pieces: piece %lld has a null pointer", (long long)i);
    ICV_REQUIRE(s.flag < 0 || flags, "icv_attention_fwd_pieces: piece %lld waits for flag %d but no flag array was given", (long long)i, s.flag);
    // the LDS-DMA addresses keep 32-bit per-lane byte offsets from a tile base: a tile spans 64 rows
    ICV_REQUIRE(64 * ldk * 2 < (1LL << 32) && 64 * ldv * 2 < (1LL << 32), "icv_attention_fwd_pieces: row stride too large");
    att7p::Piece& d = pp.piece[n++];
    d.k = (const bf16_t*)s.k; d.v = (const bf16_t*)s.v; d.rows = (int)s.rows; d.flag = s.flag; d.value = s.value; d.pad = 0;
    total += s.rows;
  }
  ICV_REQUIRE(n > 0, "icv_attention_fwd_pieces: every piece is empty");
  attc::fill_params(pp.a, q, ldq, nullptr, ldk, nullptr, ldv, o, ldo, nullptr, 0, nullptr, 0, 0, Sq, total, heads, scale, 256);
  pp.a.trace = icv_attention_trace_buffer(&pp.a.trace_cap);
  pp.flags = flags;
  pp.err = err;
  pp.timeout_ticks = timeout_us > 0 ? (unsigned long long)timeout_us * 100ull : 0ull;
  pp.ptrace = (unsigned long long*)trace;
  pp.n_pieces = n;
  hipStream_t st = (hipStream_t)stream;
  return (pp.a.sc == 1.0f && icv_get_option_int("attn_unit_scale", 1)) ? att7p::launch<true>(pp, st) : att7p::launch<false>(pp, st);
}

// The plain launch and the carried-state chunk launch as ONE piece of this kernel: the same tiles in the same order through the same
// arithmetic as attn7.hip's default variant (bit-identical: tests/test_attn_pieces_gpu.py), measured 1.5-2.7 % faster at the 14B shapes
// (23.36 vs 24.01 ms at S = 37 440, interleaved, profiles/r06/attn7p_vs_attn7.txt) - so attention.hip routes its default there.
int icv_attn7p_single(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o, int64_t ldo, float* acc,
                      int64_t ldacc, float* ml, int state_in, int state_out, int64_t Sq, int64_t Skv, int64_t heads, float scale, hipStream_t st) {
  ICV_REQUIRE(Skv > 0 && Skv < (1LL << 31) / 64 && 64 * ldk * 2 < (1LL << 32) && 64 * ldv * 2 < (1LL << 32), "icv_attention: key axis / row stride too large");
  att7p::Params pp;
  attc::fill_params(pp.a, q, ldq, nullptr, ldk, nullptr, ldv, o, ldo, acc, ldacc, ml, state_in, state_out, Sq, Skv, heads, scale, 256);
  pp.a.trace = icv_attention_trace_buffer(&pp.a.trace_cap);
  pp.flags = nullptr; pp.err = nullptr; pp.timeout_ticks = 0; pp.ptrace = nullptr;
  pp.n_pieces = 1;
  att7p::Piece& d = pp.piece[0];
  d.k = (const bf16_t*)k; d.v = (const bf16_t*)v; d.rows = (int)Skv; d.flag = -1; d.value = 0; d.pad = 0;
  return (pp.a.sc == 1.0f && icv_get_option_int("attn_unit_scale", 1)) ? att7p::launch<true>(pp, st) : att7p::launch<false>(pp, st);
}

// Frame-windowed self-attention in ONE launch (see the head of this file and include/icvideo.h)
extern "C" int icv_attention_fwd_framewin(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o, int64_t ldo,
                                          int64_t frames, int64_t frame_rows, int64_t heads, int64_t window, int64_t sink, float scale, void* stream) {
  ICV_REQUIRE(q && k && v && o, "icv_attention_fwd_framewin: null pointer");
  ICV_REQUIRE(frames > 0 && frame_rows > 0 && heads > 0, "icv_attention_fwd_framewin: empty problem (frames=%lld frame_rows=%lld heads=%lld)",
              (long long)frames, (long long)frame_rows, (long long)heads);
  ICV_REQUIRE(window >= 0 && sink >= 0, "icv_attention_fwd_framewin: window (%lld) and sink (%lld) must be >= 0", (long long)window, (long long)sink);
  ICV_REQUIRE(sink <= frames, "icv_attention_fwd_framewin: sink (%lld) exceeds the %lld frames", (long long)sink, (long long)frames);
  ICV_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 4 == 0, "icv_attention_fwd_framewin: leading dims must keep 16-byte row alignment");
  // a piece is at most every row; the LDS-DMA addresses keep 32-bit per-lane byte offsets from a tile base: a tile spans 64 rows
  ICV_REQUIRE(frames < (1LL << 31) / 64 && frame_rows < (1LL << 31) / 64 && frames * frame_rows < (1LL << 31) / 64,
              "icv_attention_fwd_framewin: %lld frames of %lld rows: key axis too large", (long long)frames, (long long)frame_rows);
  ICV_REQUIRE(64 * ldk * 2 < (1LL << 32) && 64 * ldv * 2 < (1LL << 32), "icv_attention_fwd_framewin: row stride too large");
  const int64_t nqb = frames * ((frame_rows + att7p::QB - 1) / att7p::QB);
  ICV_REQUIRE(heads * nqb < (1LL << 31), "icv_attention_fwd_framewin: %lld work-groups", (long long)(heads * nqb));
  att7p::Params pp;
  attc::fill_params(pp.a, q, ldq, k, ldk, v, ldv, o, ldo, nullptr, 0, nullptr, 0, 0, frames * frame_rows, frames * frame_rows, heads, scale, 256);
  pp.a.nqb = (int)nqb;                 // q-blocks never straddle a frame
  pp.a.trace = icv_attention_trace_buffer(&pp.a.trace_cap);
  pp.flags = nullptr; pp.err = nullptr; pp.timeout_ticks = 0; pp.ptrace = nullptr;
  pp.n_pieces = 0;
  pp.fw_frames = (int)frames;
  pp.fw_frame_rows = (int)frame_rows;
  pp.fw_window = (int)(window < frames ? window : frames);      // beyond frames - 1 every range is [0, frames)
  pp.fw_sink = (int)sink;
  hipStream_t st = (hipStream_t)stream;
  return (pp.a.sc == 1.0f && icv_get_option_int("attn_unit_scale", 1)) ? att7p::launch<true, true>(pp, st) : att7p::launch<false, true>(pp, st);
}

namespace {
__global__ void flag_write_kernel(uint32_t* flag, uint32_t value, unsigned long long delay_ticks) {
  if (delay_ticks) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0 < delay_ticks) __builtin_amdgcn_s_sleep(32);
  }
  __hip_atomic_store(flag, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
}  // namespace

extern "C" int icv_flag_write(uint32_t* flags, int64_t index, uint32_t value, int64_t delay_us, void* stream) {
  ICV_REQUIRE(flags && index >= 0, "icv_flag_write: bad argument");
  ICV_REQUIRE(delay_us >= 0 && delay_us <= 10000000, "icv_flag_write: delay_us out of range");
  hipLaunchKernelGGL(flag_write_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, flags + index, value, (unsigned long long)delay_us * 100ull);
  return icv_check_launch("icv_flag_write");
}
