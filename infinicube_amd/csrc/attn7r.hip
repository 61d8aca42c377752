// K6, RADIAL self-attention in ONE launch (icv_attention_fwd_radial; DESIGN.md §19, the rule: videogen/attn_window.py): attn7p.hip's
// frame-windowed instantiation with a piece LIST per work-group instead of one or two pieces.  Tokens are ordered (frame, row, column),
// a frame is F contiguous rows, work-groups are (head, frame f, block b of 256 rows of that frame) - a block never straddles a frame,
// rows past the frame's end are clamped for reads and never stored.  With the block's in-frame rows [p0, p1), window W and sink S,
// the work-group reads of key frame g the in-frame rows
//     g < S or |g - f| <= W:   [0, F)
//     otherwise:               e = |g - f| - W, lvl = floor(log2 e) + 1, h = F >> (lvl + 1):   [max(0, p0 - h), min(F, p1 + h))
// for g ascending; ranges that are adjacent in memory merge into one piece (the dense run, the sink).  Every frame contributes a
// non-empty range, so a work-group has at most T <= ICV_ATTN_MAX_PIECES pieces; they start and end at arbitrary rows.
// No table in memory, no flags: ONE cursor (the next key frame, a wave-uniform scalar made of blockIdx and kernel arguments ONLY - see
// attn7p.hip on why nothing per-lane may be mixed in) produces the pieces.  The DMA side is one piece ahead of the compute side for
// exactly one interval - the last interval of a piece requests the next piece's first two tiles, as attn7p's ring does when it runs
// through a boundary - so the compute side takes the row count the DMA side left behind instead of walking the frames a second time.
// The level is 32 - clz(e); nothing is re-walked.
// Ring, lane maps, tile and softmax are attn7p.hip's at its default (MF = 16, lean body; that file's key loop without the slim steady
// form, which the frame window does not take either): the same tiles in the same order between the same barriers, so a work-group's rows
// are bit-identical to icv_attention_fwd_pieces on those rows with those pieces (tests/test_attn_radial_gpu.py).  This file is the
// tree's third copy of that ring; attn7p.hip is untouched.
// Replaces: nothing in the reference (it attends densely, [R infinicube/inference/guidance_buffer_generation.py:759-766]); the rule is
// Radial Attention's (Li et al. 2025 [EXT]), restated and simplified - ORACLE_RISKS.md.
#include <type_traits>
#include "attn_common.h"

namespace att7r {

using attc::D;
constexpr int KVB = 64;
constexpr int TILE_BYTES = KVB * D * 2;      // 16 KiB (K or V)
constexpr int STAGE_BYTES = 2 * TILE_BYTES;  // 32 KiB
constexpr int NST = 4, NW = 8, NI = 16 / NW, QB = NW * 32;
constexpr int LDS_BYTES = NST * STAGE_BYTES;
static_assert(QB == 256, "RADIAL_QBLOCK (attn_window.py) is this kernel's query block");

struct Params {
  attc::Params a;                      // q / k / v / o / strides / heads / nqb / scale (a.Sq = frames * frame_rows)
  int frames, frame_rows, window, sink;
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

template <bool UNIT>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(2))) void attn7r_kernel(Params pp) {
  const attc::Params& p = pp.a;
  const float p_lim = __builtin_amdgcn_exp2f(p.thr);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  int head, qb;
  attc::work_item(p, head, qb);
  // this work-group's frame and block, and the walk's scalars: blockIdx and kernel arguments only (SGPRs)
  const int T = pp.frames, F = pp.frame_rows, W = pp.window, S = pp.sink;
  const int bpf = (F + QB - 1) / QB;    // q-blocks per frame
  const int f = qb / bpf;
  const int p0 = (qb - f * bpf) * QB;   // the block's in-frame rows [p0, p1)
  const int p1 = p0 + QB < F ? p0 + QB : F;
  const int64_t q0 = (int64_t)f * F + p0 + wave * 32;
  const int64_t q_end = (int64_t)(f + 1) * F;   // first row this work-group may neither read as a query nor store

  // ---- softmax state (registers, across all pieces) ----
  attc::Tile16 s16;
  int64_t qr16[2] = {0, 0};
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int64_t r = q0 + i * 16 + (lane & 15);
    qr16[i] = r < q_end ? r : q_end - 1;
  }
  attc::tile16_init<UNIT>(p, qr16, head, lane >> 4, s16);
  attc::tile16_load_q(p, qr16, head, lane >> 4, s16);
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
    vcol[j] = attc::tile16_vcol(pc, dkey[j]);
    ko[j] = (unsigned)(((int64_t)dkey[j] * p.ldk + kcol[j]) * 2);
    vo[j] = (unsigned)(((int64_t)dkey[j] * p.ldv + vcol[j]) * 2);
  }

  // ---- the piece cursor (wave-uniform): g_cur is the first key frame that no piece has taken yet ----
  int g_cur = 0;
  const bf16_t* kh_d = nullptr;        // the piece the DMA side reads
  const bf16_t* vh_d = nullptr;
  int skv_d = 0, nt_d = 0;
  // in-frame rows [LO_, HI_) of key frame G_
#define R_BAND(G_, LO_, HI_)                                                  \
  {                                                                           \
    const int dist_ = (G_) > f ? (G_) - f : f - (G_);                         \
    if ((G_) < S || dist_ <= W) {                                             \
      LO_ = 0; HI_ = F;                                                       \
    } else {                                                                  \
      const int lvl_ = 32 - __builtin_clz((unsigned)(dist_ - W));             \
      const int h_ = F >> (lvl_ + 1);      /* frames <= 64: lvl_ <= 6 */      \
      LO_ = p0 - h_ > 0 ? p0 - h_ : 0;                                        \
      HI_ = p1 + h_ < F ? p1 + h_ : F;                                        \
    }                                                                         \
  }
  // the next piece: frame g_cur's range, grown over every following frame whose range starts where this one ends (requires g_cur < T)
#define R_NEXT_PIECE()                                                        \
  {                                                                           \
    int lo_, hi_;                                                             \
    R_BAND(g_cur, lo_, hi_);                                                  \
    const int r0_ = g_cur * F + lo_;                                          \
    int r1_ = g_cur * F + hi_;                                                \
    ++g_cur;                                                                  \
    while (g_cur < T && hi_ == F) {                                           \
      int lo2_, hi2_;                                                         \
      R_BAND(g_cur, lo2_, hi2_);                                              \
      if (lo2_ != 0) break;                                                   \
      hi_ = hi2_;                                                             \
      r1_ = g_cur * F + hi2_;                                                 \
      ++g_cur;                                                                \
    }                                                                         \
    kh_d = p.k + (int64_t)r0_ * p.ldk + (int64_t)head * D;                    \
    vh_d = p.v + (int64_t)r0_ * p.ldv + (int64_t)head * D;                    \
    skv_d = r1_ - r0_;                                                        \
    nt_d = (skv_d + KVB - 1) / KVB;                                           \
  }
  // tile T_ of the DMA piece (clamped to its last tile: a request past the end re-reads that tile into a dead stage) -> ring stage STG_
#define R_DMA_TILE(T_, STG_)                                                                         \
  {                                                                                                  \
    const int tt_ = (T_) < nt_d ? (T_) : nt_d - 1;                                                   \
    const unsigned l0_ = lds_base + (unsigned)(((STG_) & (NST - 1)) * STAGE_BYTES + (wave * NI) * 1024); \
    if ((tt_ + 1) * KVB <= skv_d) {                                                                  \
      const bf16_t* kt_ = kh_d + (int64_t)tt_ * KVB * p.ldk;                                         \
      const bf16_t* vt_ = vh_d + (int64_t)tt_ * KVB * p.ldv;                                         \
      _Pragma("unroll") for (int j_ = 0; j_ < NI; ++j_) dma16s(kt_, ko[j_], l0_ + j_ * 1024);        \
      _Pragma("unroll") for (int j_ = 0; j_ < NI; ++j_) dma16s(vt_, vo[j_], l0_ + TILE_BYTES + j_ * 1024); \
    } else {                                                                                         \
      _Pragma("unroll") for (int j_ = 0; j_ < NI; ++j_) {                                            \
        int64_t r_ = (int64_t)tt_ * KVB + dkey[j_];                                                  \
        r_ = r_ < skv_d ? r_ : skv_d - 1;        /* a ragged tile: rows past the piece's end re-read its last row */ \
        dma16(kh_d + r_ * p.ldk + kcol[j_], l0_ + j_ * 1024);                                        \
        dma16(vh_d + r_ * p.ldv + vcol[j_], l0_ + TILE_BYTES + j_ * 1024);                           \
      }                                                                                              \
    }                                                                                                \
  }
#define R_BARRIER()                                           \
  do {                                                        \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");        \
    __builtin_amdgcn_s_barrier();                             \
    asm volatile("" ::: "memory");                            \
    __builtin_amdgcn_sched_barrier(0);                        \
  } while (0)

  // the lean tile's fragment addresses: they point at the even stage of the interval's half of the ring and move to the other half once
  // per interval
  attc::Tile16Addr la16;
  int la16_step = 2 * STAGE_BYTES;
  attc::tile16_lean_addr(lds_base, lane, la16);
  attc::tile16_lean_lim<UNIT>(s16, p_lim, la16);
  auto tile = [&](const auto par, const int key0, const int skv) __attribute__((always_inline)) {
    attc::tile16<UNIT, false, true, true, true, decltype(par)::value>(p, p_lim, nullptr, nullptr, key0, skv, lane, s16, &la16);
  };

  // ---- walk the pieces ----
  unsigned gt = 0;                 // ring position of the current piece's tile 0 (always even)
  R_NEXT_PIECE();
  R_DMA_TILE(0, gt);
  R_DMA_TILE(1, gt + 1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  R_BARRIER();
  for (;;) {
    const int skv = skv_d;                            // the DMA piece is this piece until this piece's last interval
    const int nt = (skv + KVB - 1) / KVB;
    __builtin_assume(nt >= 1);
    const unsigned g_next = gt + (unsigned)((nt + 1) & ~1);
    const bool has_next = g_cur < T;                  // every frame has a range: frames left = pieces left
    for (int t = 0; t < nt; t += 2) {
      if (t + 2 < nt) {                               // the other half of the ring: last read in the previous interval
        R_DMA_TILE(t + 2, gt + t + 2);
        R_DMA_TILE(t + 3, gt + t + 3);
      } else if (has_next) {                          // run through the boundary: the next piece's first interval
        R_NEXT_PIECE();
        R_DMA_TILE(0, g_next);
        R_DMA_TILE(1, g_next + 1);
      }
      tile(std::integral_constant<int, 0>{}, t * KVB, skv);
      if (t + 1 < nt) tile(std::integral_constant<int, 1>{}, (t + 1) * KVB, skv);
      attc::tile16_lean_advance(la16, la16_step);     // the next interval reads the other half: gt + t is 2 (mod 4) further on
      la16_step = -la16_step;
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      R_BARRIER();
    }
    if (!has_next) break;
    gt = g_next;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  // a row past the frame's end belongs to the next frame's work-group - hand store_result a row it does not store
  int64_t qr[2];
  int t16 = lane & 15;
  asm volatile("" : "+v"(t16));      // recompute the rows here: carried from the prologue they cost four VGPRs through the whole loop
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int64_t r = q0 + i * 16 + t16;
    qr[i] = r < q_end ? r : p.Sq;
  }
  attc::store_result(p, qr, head, lane >> 4, s16.ot, s16.m_run, s16.l_run);
#undef R_BAND
#undef R_NEXT_PIECE
#undef R_DMA_TILE
#undef R_BARRIER
}

template <bool UNIT>
int launch(const Params& pp, hipStream_t st) {
  static icv_dev_flags attr_set = {};
  if (int rc = icv_ensure_dynamic_lds((const void*)attn7r_kernel<UNIT>, LDS_BYTES, &attr_set, "attn7r")) return rc;
  const int64_t nwg = (int64_t)pp.a.heads * pp.a.nqb;
  hipLaunchKernelGGL((attn7r_kernel<UNIT>), dim3((unsigned)nwg), dim3(NW * 64), LDS_BYTES, st, pp);
  return icv_check_launch("icv_attention_fwd_radial");
}

}  // namespace att7r

// Radial self-attention in ONE launch (see the head of this file and include/icvideo.h)
extern "C" int icv_attention_fwd_radial(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o, int64_t ldo,
                                        int64_t frames, int64_t frame_rows, int64_t heads, int64_t window, int64_t sink, float scale, void* stream) {
  ICV_REQUIRE(q && k && v && o, "icv_attention_fwd_radial: null pointer");
  ICV_REQUIRE(frames > 0 && frame_rows > 0 && heads > 0, "icv_attention_fwd_radial: empty problem (frames=%lld frame_rows=%lld heads=%lld)",
              (long long)frames, (long long)frame_rows, (long long)heads);
  ICV_REQUIRE(frames <= ICV_ATTN_MAX_PIECES, "icv_attention_fwd_radial: %lld frames: a work-group walks at most %d pieces, one per frame",
              (long long)frames, ICV_ATTN_MAX_PIECES);
  ICV_REQUIRE(window >= 0 && sink >= 0, "icv_attention_fwd_radial: window (%lld) and sink (%lld) must be >= 0", (long long)window, (long long)sink);
  ICV_REQUIRE(sink <= frames, "icv_attention_fwd_radial: sink (%lld) exceeds the %lld frames", (long long)sink, (long long)frames);
  ICV_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 4 == 0, "icv_attention_fwd_radial: leading dims must keep 16-byte row alignment");
  // a piece is at most every row; the LDS-DMA addresses keep 32-bit per-lane byte offsets from a tile base: a tile spans 64 rows
  ICV_REQUIRE(frame_rows < (1LL << 31) / 64 && frames * frame_rows < (1LL << 31) / 64,
              "icv_attention_fwd_radial: %lld frames of %lld rows: key axis too large", (long long)frames, (long long)frame_rows);
  ICV_REQUIRE(64 * ldk * 2 < (1LL << 32) && 64 * ldv * 2 < (1LL << 32), "icv_attention_fwd_radial: row stride too large");
  const int64_t nqb = frames * ((frame_rows + att7r::QB - 1) / att7r::QB);
  ICV_REQUIRE(heads * nqb < (1LL << 31), "icv_attention_fwd_radial: %lld work-groups", (long long)(heads * nqb));
  hipStream_t st = (hipStream_t)stream;
  // every band is the whole frame: dense attention, which is the plain launch (its q-blocks tile all rows, not a frame's)
  if (window >= frames - 1 || sink >= frames)
    return icv_attention_fwd(q, ldq, k, ldk, v, ldv, o, ldo, frames * frame_rows, frames * frame_rows, heads, scale, stream);
  att7r::Params pp;
  attc::fill_params(pp.a, q, ldq, k, ldk, v, ldv, o, ldo, nullptr, 0, nullptr, 0, 0, frames * frame_rows, frames * frame_rows, heads, scale, 256);
  pp.a.nqb = (int)nqb;                 // q-blocks never straddle a frame
  pp.frames = (int)frames;
  pp.frame_rows = (int)frame_rows;
  pp.window = (int)window;
  pp.sink = (int)sink;
  return (pp.a.sc == 1.0f && icv_get_option_int("attn_unit_scale", 1)) ? att7r::launch<true>(pp, st) : att7r::launch<false>(pp, st);
}
