// EasyCache runtime-adaptive step skipping (videogen/easycache.py): the device side of the rule.
//   icv_l1_change_f64           out2 = (sum |a - b|, sum |a|) over [rows, cols] in fp64;  optionally b <- a in the same pass
//   icv_easycache_predict_f32   a skipped step's head outputs: h = h_last + P(x - x_last), both CFG branches in one launch
// The reduction follows icv_cfg_zero_scale_f32 (guidance.hip): two launches on one stream, one pair of fp64 partial sums per
// block in the caller's workspace, then ONE block adds them in a fixed tree.  No atomics, no "last block done" counter, no host
// read; the same inputs give the same bits.
#include "icv_common.h"

// Plain f32 adds and subtractions, as written.
#pragma clang fp contract(off)

#define L1C_THREADS 256
#define L1C_MAX_BLOCKS 256                     // one per CU; 2 * L1C_MAX_BLOCKS == ICV_L1_CHANGE_WORKSPACE_DOUBLES
static_assert(2 * L1C_MAX_BLOCKS == ICV_L1_CHANGE_WORKSPACE_DOUBLES, "workspace: one pair of partial sums per block");
static_assert(L1C_MAX_BLOCKS <= L1C_THREADS, "the final launch reads one pair per thread");

// The work unit is a QUAD: four consecutive elements of the flattened [rows, cols] index space, quad q going to thread
// q % (blocks * 256) - a function of (rows, cols) alone.  The 16-byte path (VEC: cols, lda and ldb multiples of 4, both pointers
// 16-byte aligned, so a quad lies in one row at an aligned address of either operand) and the scalar path walk the same quads in
// the same order and add a quad's terms in the same order, so alignment and strides change the loads, not the bits.
template <bool VEC>
__device__ __forceinline__ int l1c_quad(int64_t q, int64_t lda, int64_t ldb, int64_t cols, int64_t total, int64_t oa[4], int64_t ob[4]) {
  if (VEC) {
    const int64_t per_row = cols >> 2;
    const int64_t row = q / per_row;
    const int64_t col = (q - row * per_row) << 2;
    oa[0] = row * lda + col;
    ob[0] = row * ldb + col;
    return 4;
  }
  const int64_t e0 = q << 2;
  const int n = total - e0 < 4 ? (int)(total - e0) : 4;
  for (int j = 0; j < n; ++j) {
    const int64_t row = (e0 + j) / cols;
    const int64_t col = e0 + j - row * cols;
    oa[j] = row * lda + col;
    ob[j] = row * ldb + col;
  }
  return n;
}

// Fixed-shape tree over the block's 256 pairs (as cfgz_tree, guidance.hip); the sums end in s_d[0] / s_a[0].
__device__ __forceinline__ void l1c_tree(double* s_d, double* s_a, int tid) {
  __syncthreads();
  for (int w = L1C_THREADS / 2; w > 0; w >>= 1) {
    if (tid < w) {
      s_d[tid] += s_d[tid + w];
      s_a[tid] += s_a[tid + w];
    }
    __syncthreads();
  }
}

// Launch 1: per thread sum |a - b| and sum |a|, every term formed in fp64 from the f32 values (the difference of two f32 values is
// rounded once, in fp64); one pair per block.  With UPDATE the thread stores the a it just read over the b it just read.
template <bool VEC, bool UPDATE>
__global__ __launch_bounds__(L1C_THREADS) void l1_change_partial_kernel(const float* __restrict__ a, int64_t lda, float* __restrict__ b,
                                                                        int64_t ldb, int64_t cols, int64_t total, int64_t n_quads,
                                                                        double* __restrict__ partial) {
  const int tid = threadIdx.x;
  double sd = 0.0, sa = 0.0;
  for (int64_t q = (int64_t)blockIdx.x * L1C_THREADS + tid; q < n_quads; q += (int64_t)gridDim.x * L1C_THREADS) {
    int64_t oa[4], ob[4];
    float av[4], bv[4];
    const int n = l1c_quad<VEC>(q, lda, ldb, cols, total, oa, ob);
    if (VEC) {
      const f32x4 a4 = *reinterpret_cast<const f32x4*>(a + oa[0]);
      const f32x4 b4 = *reinterpret_cast<const f32x4*>(b + ob[0]);
      for (int j = 0; j < 4; ++j) { av[j] = a4[j]; bv[j] = b4[j]; }
      if (UPDATE) *reinterpret_cast<f32x4*>(b + ob[0]) = a4;
    } else {
      for (int j = 0; j < n; ++j) { av[j] = a[oa[j]]; bv[j] = b[ob[j]]; }
      if (UPDATE)
        for (int j = 0; j < n; ++j) b[ob[j]] = av[j];
    }
    for (int j = 0; j < n; ++j) {
      sd += fabs((double)av[j] - (double)bv[j]);
      sa += fabs((double)av[j]);
    }
  }
  __shared__ double s_d[L1C_THREADS], s_a[L1C_THREADS];
  s_d[tid] = sd;
  s_a[tid] = sa;
  l1c_tree(s_d, s_a, tid);
  if (tid == 0) {
    partial[2 * blockIdx.x] = s_d[0];
    partial[2 * blockIdx.x + 1] = s_a[0];
  }
}

// Launch 2 (one block): the ``blocks`` pairs of launch 1 through the same tree, into out2.
__global__ __launch_bounds__(L1C_THREADS) void l1_change_final_kernel(const double* __restrict__ partial, int blocks, double* __restrict__ out2) {
  const int tid = threadIdx.x;
  __shared__ double s_d[L1C_THREADS], s_a[L1C_THREADS];
  const bool have = tid < blocks;
  s_d[tid] = have ? partial[2 * tid] : 0.0;
  s_a[tid] = have ? partial[2 * tid + 1] : 0.0;
  l1c_tree(s_d, s_a, tid);
  if (tid == 0) {
    out2[0] = s_d[0];
    out2[1] = s_a[0];
  }
}

static bool l1c_overlap(const void* p, int64_t n_p, const void* q, int64_t n_q) {
  const uintptr_t p0 = (uintptr_t)p, q0 = (uintptr_t)q;
  return p0 < q0 + (uintptr_t)n_q && q0 < p0 + (uintptr_t)n_p;
}

extern "C" int icv_l1_change_f64(const float* a, int64_t lda, float* b, int64_t ldb, int64_t rows, int64_t cols, int update_b,
                                 double* workspace, double* out2, void* stream) {
  ICV_REQUIRE(a && b && workspace && out2, "icv_l1_change_f64: null argument");
  ICV_REQUIRE(rows > 0 && cols > 0 && rows < (1ll << 31) && cols < (1ll << 31), "icv_l1_change_f64: bad shape (rows %lld, cols %lld)",
              (long long)rows, (long long)cols);
  ICV_REQUIRE(lda >= cols && ldb >= cols, "icv_l1_change_f64: lda (%lld) or ldb (%lld) is less than the %lld columns of a row",
              (long long)lda, (long long)ldb, (long long)cols);
  ICV_REQUIRE(lda < (1ll << 40) && ldb < (1ll << 40), "icv_l1_change_f64: leading dimension out of range");
  ICV_REQUIRE((((uintptr_t)a | (uintptr_t)b) & 3) == 0, "icv_l1_change_f64: a and b must be 4-byte aligned");
  ICV_REQUIRE((((uintptr_t)workspace | (uintptr_t)out2) & 7) == 0, "icv_l1_change_f64: workspace and out2 must be 8-byte aligned");
  const int64_t span_a = ((rows - 1) * lda + cols) * 4, span_b = ((rows - 1) * ldb + cols) * 4;
  ICV_REQUIRE(!l1c_overlap(a, span_a, b, span_b), "icv_l1_change_f64: a and b must not overlap");
  ICV_REQUIRE(!l1c_overlap(out2, 16, workspace, ICV_L1_CHANGE_WORKSPACE_DOUBLES * 8), "icv_l1_change_f64: out2 lies inside the workspace");
  const int64_t total = rows * cols;
  const int64_t n_quads = (total + 3) / 4;
  const int64_t want = (n_quads + L1C_THREADS - 1) / L1C_THREADS;
  const unsigned blocks = (unsigned)(want < L1C_MAX_BLOCKS ? want : L1C_MAX_BLOCKS);         // of (rows, cols) only
  const bool vec = cols % 4 == 0 && lda % 4 == 0 && ldb % 4 == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0;
  const hipStream_t st = (hipStream_t)stream;
#define L1C_LAUNCH(V, U) \
  hipLaunchKernelGGL((l1_change_partial_kernel<V, U>), dim3(blocks), dim3(L1C_THREADS), 0, st, a, lda, b, ldb, cols, total, n_quads, workspace)
  if (vec) {
    if (update_b) L1C_LAUNCH(true, true); else L1C_LAUNCH(true, false);
  } else {
    if (update_b) L1C_LAUNCH(false, true); else L1C_LAUNCH(false, false);
  }
#undef L1C_LAUNCH
  hipLaunchKernelGGL(l1_change_final_kernel, dim3(1), dim3(L1C_THREADS), 0, st, (const double*)workspace, (int)blocks, out2);
  return icv_check_launch("icv_l1_change_f64");
}

// ---------------------------------------------------------------------------------------------------------------------------------
// A skipped step's head outputs.  The index map is icv_unpatchify_cfg_euler's (elementwise.hip) read in the other direction: local
// token r = token tok0 + r = (f, hp, wp), head column (y*2+z)*C + c  <->  latent element [c, f, 2hp+y, 2wp+z].  One thread per
// (token, y, group of CV channels) handles z = 0, 1: two latent elements of a row (8 bytes) per channel, CV head columns in a row
// per z.  CV = 4: 16-byte head accesses (C, ldh multiples of 4 and 16-byte-aligned head pointers); CV = 1 otherwise.  Elementwise,
// so the two paths give the same bits.
template <int CV>
__global__ __launch_bounds__(256) void easycache_predict_kernel(const float* __restrict__ x, const float* __restrict__ xl,
                                                                const float* __restrict__ hcl, const float* __restrict__ hul,
                                                                float* __restrict__ hc, float* __restrict__ hu, int64_t ldh, int C,
                                                                int T, int H8, int W8, int64_t tok0, int64_t n_tok) {
  const int G = C / CV;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n_tok * 2 * G) return;
  const int c0 = (int)(idx % G) * CV;
  const int y = (int)((idx / G) & 1);
  const int64_t r = idx / (2 * G);
  const int64_t tok = tok0 + r;
  const int Wp = W8 >> 1, Hp = H8 >> 1;
  const int wp = (int)(tok % Wp);
  const int hp = (int)((tok / Wp) % Hp);
  const int f = (int)(tok / ((int64_t)Wp * Hp));
  float d[2][CV];
  for (int j = 0; j < CV; ++j) {
    const int64_t li = (((int64_t)(c0 + j) * T + f) * H8 + 2 * hp + y) * W8 + 2 * wp;     // even: W8 is even
    const float2 a = *reinterpret_cast<const float2*>(x + li);
    const float2 b = *reinterpret_cast<const float2*>(xl + li);
    d[0][j] = a.x - b.x;
    d[1][j] = a.y - b.y;
  }
  for (int z = 0; z < 2; ++z) {
    const int64_t h0 = r * ldh + (int64_t)(y * 2 + z) * C + c0;
    if (CV == 4) {
      f32x4 v = *reinterpret_cast<const f32x4*>(hcl + h0);
      for (int j = 0; j < 4; ++j) v[j] = v[j] + d[z][j];
      *reinterpret_cast<f32x4*>(hc + h0) = v;
      if (hu) {
        f32x4 u = *reinterpret_cast<const f32x4*>(hul + h0);
        for (int j = 0; j < 4; ++j) u[j] = u[j] + d[z][j];
        *reinterpret_cast<f32x4*>(hu + h0) = u;
      }
    } else {
      for (int j = 0; j < CV; ++j) {
        hc[h0 + j] = hcl[h0 + j] + d[z][j];
        if (hu) hu[h0 + j] = hul[h0 + j] + d[z][j];
      }
    }
  }
}

extern "C" int icv_easycache_predict_f32(const float* x, const float* x_last, const float* hc_last, const float* hu_last, float* hc,
                                         float* hu, int64_t ldh, int64_t C, int64_t T, int64_t H8, int64_t W8, int64_t tok0,
                                         int64_t n_tok, void* stream) {
  ICV_REQUIRE(x && x_last && hc_last && hc, "icv_easycache_predict_f32: null argument");
  ICV_REQUIRE((hu_last == nullptr) == (hu == nullptr), "icv_easycache_predict_f32: hu_last and hu must be given together");
  ICV_REQUIRE(hc != hc_last && hc != hu_last && (!hu || (hu != hu_last && hu != hc_last && hu != hc)),
              "icv_easycache_predict_f32: the head outputs must be buffers of their own (not in place)");
  ICV_REQUIRE(C > 0 && T > 0 && H8 > 0 && W8 > 0 && H8 % 2 == 0 && W8 % 2 == 0 && C < (1 << 20) && T < (1 << 20) && H8 < (1 << 20) &&
                  W8 < (1 << 20) && C * T * H8 * W8 < (1ll << 40),
              "icv_easycache_predict_f32: bad latent shape [%lld, %lld, %lld, %lld]", (long long)C, (long long)T, (long long)H8, (long long)W8);
  ICV_REQUIRE(ldh >= 4 * C && ldh < (1ll << 31), "icv_easycache_predict_f32: ldh (%lld) is less than the %lld columns of a row",
              (long long)ldh, (long long)(4 * C));
  ICV_REQUIRE(n_tok > 0 && tok0 >= 0 && tok0 + n_tok <= T * (H8 / 2) * (W8 / 2), "icv_easycache_predict_f32: token range [%lld, %lld)",
              (long long)tok0, (long long)(tok0 + n_tok));
  ICV_REQUIRE((((uintptr_t)x | (uintptr_t)x_last) & 7) == 0, "icv_easycache_predict_f32: x and x_last must be 8-byte aligned");
  ICV_REQUIRE((((uintptr_t)hc_last | (uintptr_t)hu_last | (uintptr_t)hc | (uintptr_t)hu) & 3) == 0,
              "icv_easycache_predict_f32: the head outputs must be 4-byte aligned");
  const bool vec = C % 4 == 0 && ldh % 4 == 0 && (((uintptr_t)hc_last | (uintptr_t)hu_last | (uintptr_t)hc | (uintptr_t)hu) & 15) == 0;
  const int64_t total = n_tok * 2 * (vec ? C / 4 : C);
  ICV_REQUIRE((total + 255) / 256 < (1ll << 31), "icv_easycache_predict_f32: too many tokens");
  const dim3 grid((unsigned)((total + 255) / 256));
  if (vec)
    hipLaunchKernelGGL(easycache_predict_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, x, x_last, hc_last, hu_last, hc, hu, ldh,
                       (int)C, (int)T, (int)H8, (int)W8, tok0, n_tok);
  else
    hipLaunchKernelGGL(easycache_predict_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, x, x_last, hc_last, hu_last, hc, hu, ldh,
                       (int)C, (int)T, (int)H8, (int)W8, tok0, n_tok);
  return icv_check_launch("icv_easycache_predict_f32");
}
