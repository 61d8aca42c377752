// CFG-Zero* guidance: the optimised scale of the unconditional head output, on the device.
//   icv_cfg_zero_scale_f32   s = <hc, hu> / (|hu|^2 + 1e-8) over [rows, cols];  hu <- s * hu;  s -> scale_out
// Two launches on one stream, the reduction at the launch boundary: launch 1 leaves one pair of fp64 partial sums per block in
// the workspace, launch 2 lets EVERY block add them up in one fixed order (so every block holds the same s) and scale its share
// of hu.  No atomics, no "last block done" counter, no host read; the same inputs give the same bits.
#include "icv_common.h"

// One multiply per stored element, as written (nothing here may be contracted into a fused multiply-add).
#pragma clang fp contract(off)

#define CFGZ_THREADS 256
#define CFGZ_MAX_BLOCKS 256                    // one per CU; 2 * CFGZ_MAX_BLOCKS == ICV_CFG_ZERO_WORKSPACE_DOUBLES
static_assert(2 * CFGZ_MAX_BLOCKS == ICV_CFG_ZERO_WORKSPACE_DOUBLES, "workspace: one pair of partial sums per block");

__device__ __forceinline__ float cfgz_rb(float x) { return bf16_to_f32((bf16_t)f32_to_bf16_bits(x)); }

// The work unit of both launches is a QUAD: four consecutive elements of the flattened [rows, cols] index space, quad q going to
// thread q % (blocks * 256) - a function of (rows, cols) alone.  The 16-byte path (VEC: cols and ldh multiples of 4, both
// pointers 16-byte aligned, so a quad lies in one row at an aligned address) and the scalar path walk the same quads in the same
// order, so a buffer's alignment changes the loads, not the bits.
template <bool VEC>
__device__ __forceinline__ int cfgz_quad_offsets(int64_t q, int64_t ldh, int64_t cols, int64_t total, int64_t off[4]) {
  if (VEC) {
    const int64_t per_row = cols >> 2;
    const int64_t row = q / per_row;
    off[0] = row * ldh + ((q - row * per_row) << 2);
    return 4;
  }
  const int64_t e0 = q << 2;
  const int n = total - e0 < 4 ? (int)(total - e0) : 4;
  for (int j = 0; j < n; ++j) {
    const int64_t row = (e0 + j) / cols;
    off[j] = row * ldh + (e0 + j - row * cols);
  }
  return n;
}

// Fixed-shape tree over the block's 256 pairs (as rel_l1_steps_kernel, teacache.hip); the sums end in s_num[0] / s_den[0].
__device__ __forceinline__ void cfgz_tree(double* s_num, double* s_den, int tid) {
  __syncthreads();
  for (int w = CFGZ_THREADS / 2; w > 0; w >>= 1) {
    if (tid < w) {
      s_num[tid] += s_num[tid + w];
      s_den[tid] += s_den[tid + w];
    }
    __syncthreads();
  }
}

// Launch 1: per thread sum c u and sum u u in fp64 (the product of two f32 values is exact in fp64), one pair per block.
template <bool VEC>
__global__ __launch_bounds__(CFGZ_THREADS) void cfg_zero_moments_kernel(const float* __restrict__ hc, const float* __restrict__ hu,
                                                                        int64_t ldh, int64_t cols, int64_t total, int64_t n_quads,
                                                                        double* __restrict__ partial, int round_bf16) {
  const int tid = threadIdx.x;
  double num = 0.0, den = 0.0;
  for (int64_t q = (int64_t)blockIdx.x * CFGZ_THREADS + tid; q < n_quads; q += (int64_t)gridDim.x * CFGZ_THREADS) {
    int64_t off[4];
    float c[4], u[4];
    const int n = cfgz_quad_offsets<VEC>(q, ldh, cols, total, off);
    if (VEC) {
      const f32x4 cv = *reinterpret_cast<const f32x4*>(hc + off[0]);
      const f32x4 uv = *reinterpret_cast<const f32x4*>(hu + off[0]);
      for (int j = 0; j < 4; ++j) { c[j] = cv[j]; u[j] = uv[j]; }
    } else {
      for (int j = 0; j < n; ++j) { c[j] = hc[off[j]]; u[j] = hu[off[j]]; }
    }
    for (int j = 0; j < n; ++j) {
      const float cj = round_bf16 ? cfgz_rb(c[j]) : c[j], uj = round_bf16 ? cfgz_rb(u[j]) : u[j];
      num += (double)cj * (double)uj;
      den += (double)uj * (double)uj;
    }
  }
  __shared__ double s_num[CFGZ_THREADS], s_den[CFGZ_THREADS];
  s_num[tid] = num;
  s_den[tid] = den;
  cfgz_tree(s_num, s_den, tid);
  if (tid == 0) {
    partial[2 * blockIdx.x] = s_num[0];
    partial[2 * blockIdx.x + 1] = s_den[0];
  }
}

// Launch 2 (the grid of launch 1): every block adds the gridDim.x pairs in the same tree, forms s, scales its quads of hu in
// place with one f32 rounding per element; block 0 stores s.
template <bool VEC>
__global__ __launch_bounds__(CFGZ_THREADS) void cfg_zero_apply_kernel(float* __restrict__ hu, int64_t ldh, int64_t cols, int64_t total,
                                                                      int64_t n_quads, const double* __restrict__ partial,
                                                                      float* __restrict__ scale_out, int round_bf16) {
  const int tid = threadIdx.x;
  __shared__ double s_num[CFGZ_THREADS], s_den[CFGZ_THREADS];
  const bool have = tid < (int)gridDim.x;                      // gridDim.x <= CFGZ_MAX_BLOCKS == CFGZ_THREADS
  s_num[tid] = have ? partial[2 * tid] : 0.0;
  s_den[tid] = have ? partial[2 * tid + 1] : 0.0;
  cfgz_tree(s_num, s_den, tid);
  float s = (float)(s_num[0] / (s_den[0] + 1e-8));             // sum u u == 0: 0 / 1e-8 = 0
  if (round_bf16) s = cfgz_rb(s);
  if (blockIdx.x == 0 && tid == 0) scale_out[0] = s;
  for (int64_t q = (int64_t)blockIdx.x * CFGZ_THREADS + tid; q < n_quads; q += (int64_t)gridDim.x * CFGZ_THREADS) {
    int64_t off[4];
    const int n = cfgz_quad_offsets<VEC>(q, ldh, cols, total, off);
    if (VEC) {
      f32x4 uv = *reinterpret_cast<const f32x4*>(hu + off[0]);
      for (int j = 0; j < 4; ++j) uv[j] = round_bf16 ? cfgz_rb(s * cfgz_rb(uv[j])) : s * uv[j];
      *reinterpret_cast<f32x4*>(hu + off[0]) = uv;
    } else {
      for (int j = 0; j < n; ++j) {
        const float u = hu[off[j]];
        hu[off[j]] = round_bf16 ? cfgz_rb(s * cfgz_rb(u)) : s * u;
      }
    }
  }
}

extern "C" int icv_cfg_zero_scale_f32(const float* hc, float* hu, int64_t ldh, int64_t rows, int64_t cols, double* workspace,
                                      float* scale_out, int round_bf16, void* stream) {
  ICV_REQUIRE(hc && hu && workspace && scale_out, "icv_cfg_zero_scale_f32: null argument");
  ICV_REQUIRE(rows > 0 && cols > 0 && rows < (1ll << 31) && cols < (1ll << 31), "icv_cfg_zero_scale_f32: bad shape (rows %lld, cols %lld)",
              (long long)rows, (long long)cols);
  ICV_REQUIRE(ldh >= cols, "icv_cfg_zero_scale_f32: ldh (%lld) is less than the %lld columns of a row", (long long)ldh, (long long)cols);
  ICV_REQUIRE(hc != (const float*)hu, "icv_cfg_zero_scale_f32: hc and hu must differ (hu is scaled in place)");
  ICV_REQUIRE((((uintptr_t)hc | (uintptr_t)hu | (uintptr_t)scale_out) & 3) == 0, "icv_cfg_zero_scale_f32: hc, hu and scale_out must be 4-byte aligned");
  ICV_REQUIRE(((uintptr_t)workspace & 7) == 0, "icv_cfg_zero_scale_f32: workspace must be 8-byte aligned");
  const int64_t total = rows * cols;
  const int64_t n_quads = (total + 3) / 4;
  const int64_t want = (n_quads + CFGZ_THREADS - 1) / CFGZ_THREADS;
  const unsigned blocks = (unsigned)(want < CFGZ_MAX_BLOCKS ? want : CFGZ_MAX_BLOCKS);       // of (rows, cols) only
  const bool vec = cols % 4 == 0 && ldh % 4 == 0 && (((uintptr_t)hc | (uintptr_t)hu) & 15) == 0;
  const hipStream_t st = (hipStream_t)stream;
  if (vec) {
    hipLaunchKernelGGL(cfg_zero_moments_kernel<true>, dim3(blocks), dim3(CFGZ_THREADS), 0, st, hc, hu, ldh, cols, total, n_quads, workspace, round_bf16);
    hipLaunchKernelGGL(cfg_zero_apply_kernel<true>, dim3(blocks), dim3(CFGZ_THREADS), 0, st, hu, ldh, cols, total, n_quads, workspace, scale_out, round_bf16);
  } else {
    hipLaunchKernelGGL(cfg_zero_moments_kernel<false>, dim3(blocks), dim3(CFGZ_THREADS), 0, st, hc, hu, ldh, cols, total, n_quads, workspace, round_bf16);
    hipLaunchKernelGGL(cfg_zero_apply_kernel<false>, dim3(blocks), dim3(CFGZ_THREADS), 0, st, hu, ldh, cols, total, n_quads, workspace, scale_out, round_bf16);
  }
  return icv_check_launch("icv_cfg_zero_scale_f32");
}
