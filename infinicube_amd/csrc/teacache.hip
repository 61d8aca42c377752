// TeaCache step skipping: the two small kernels the host schedule needs.
//   icv_sub_rows_f32      r = x - r over [rows, d] f32 (row strides): the residual store of a computed forward
//   icv_rel_l1_steps_f32  mean|a_i - a_{i-1}| / mean|a_{i-1}| for every row i >= 1 of a [N, cols] table of t_mod rows
#include "icv_common.h"

// One thread per element; pure fp32 subtraction, so the result is bit-exact against torch.
__global__ __launch_bounds__(256) void sub_rows_kernel(const float* __restrict__ x, int64_t ldx, float* __restrict__ r,
                                                       int64_t ldr, int64_t rows, int64_t d) {
  const int64_t total = rows * d;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t i = e / d, j = e - i * d;
    r[i * ldr + j] = x[i * ldx + j] - r[i * ldr + j];
  }
}

extern "C" int icv_sub_rows_f32(const float* x, int64_t ldx, float* r, int64_t ldr, int64_t rows, int64_t d, void* stream) {
  ICV_REQUIRE(x && r, "icv_sub_rows_f32: null argument");
  ICV_REQUIRE(rows > 0 && d > 0 && ldx >= d && ldr >= d, "icv_sub_rows_f32: bad shape (rows %lld, d %lld, ldx %lld, ldr %lld)",
              (long long)rows, (long long)d, (long long)ldx, (long long)ldr);
  const int64_t total = rows * d;
  const int64_t blocks = (total + 255) / 256 < 65536 ? (total + 255) / 256 : 65536;   // grid-stride beyond that
  hipLaunchKernelGGL(sub_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, ldx, r, ldr, rows, d);
  return icv_check_launch("icv_sub_rows_f32");
}

// One work-group per row i.  Deterministic by construction: every thread sums a fixed, strided subset of the columns in
// fp64, then a fixed-shape tree in LDS combines the 256 partial sums; no atomics, so every rank gets the same bits.
__global__ __launch_bounds__(256) void rel_l1_steps_kernel(const float* __restrict__ tab, int64_t ldt, int64_t cols,
                                                           float* __restrict__ out) {
  const int64_t i = blockIdx.x;
  const int tid = threadIdx.x;
  if (i == 0) {
    if (tid == 0) out[0] = 0.0f;
    return;
  }
  const float* a = tab + i * ldt;
  const float* b = tab + (i - 1) * ldt;
  double num = 0.0, den = 0.0;
  for (int64_t j = tid; j < cols; j += 256) {
    num += fabs((double)a[j] - (double)b[j]);
    den += fabs((double)b[j]);
  }
  __shared__ double s_num[256], s_den[256];
  s_num[tid] = num;
  s_den[tid] = den;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) {
      s_num[tid] += s_num[tid + w];
      s_den[tid] += s_den[tid + w];
    }
    __syncthreads();
  }
  if (tid == 0) out[i] = (float)(s_num[0] / s_den[0]);      // the 1/cols of both means cancels
}

extern "C" int icv_rel_l1_steps_f32(const float* table, int64_t n, int64_t cols, int64_t ldt, float* out, void* stream) {
  ICV_REQUIRE(table && out, "icv_rel_l1_steps_f32: null argument");
  ICV_REQUIRE(n > 0 && n < (1ll << 31) && cols > 0 && ldt >= cols, "icv_rel_l1_steps_f32: bad shape (n %lld, cols %lld, ldt %lld)",
              (long long)n, (long long)cols, (long long)ldt);
  hipLaunchKernelGGL(rel_l1_steps_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, table, ldt, cols, out);
  return icv_check_launch("icv_rel_l1_steps_f32");
}
