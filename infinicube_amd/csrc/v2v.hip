// Video-to-video start latent: the one noising of the VAE-encoded input clip at the first sigma of a shortened range.
//   icv_add_noise_f32   out[i] = (1 - sigma) * x0[i] + sigma * noise[i]
// Elementwise, HBM-bound, once per call.  out may be noise or x0 (a thread reads its elements before it writes them); any other
// overlap is the caller's error.  Any n and any 4-byte-aligned pointers: where x0, noise and out sit at the SAME offset from a
// 16-byte boundary the body moves 16-byte vectors and the up-to-3 elements before and after it go one by one; where the offsets
// differ no element index is 16-byte aligned for all three, and every element goes one by one.
#include "icv_common.h"

// No fused multiply-add contraction in this file: the result is compared bit for bit against a restatement with one tensor
// operation per product and one for the sum, in both rounding modes.  The element's arithmetic is add_noise_one (icv_common.h),
// shared with icv_pin_known_f32.
#pragma clang fp contract(off)

// Threads [0, n_vec): one 16-byte vector each, elements [head + 4 idx, head + 4 idx + 4).  Threads [n_vec, n_vec + n - 4 n_vec):
// one element each - first the `head` elements in front of the vector body, then the ones behind it.
__global__ __launch_bounds__(256) void add_noise_kernel(const float* x0, const float* noise, float* out, int64_t n, int64_t head,
                                                        int64_t n_vec, float sigma, int round_bf16) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const float one_minus = 1.0f - sigma;
  if (idx < n_vec) {
    const int64_t i = head + 4 * idx;
    const f32x4 x = *reinterpret_cast<const f32x4*>(x0 + i);
    const f32x4 z = *reinterpret_cast<const f32x4*>(noise + i);
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = add_noise_one(x[j], z[j], one_minus, sigma, round_bf16);
    *reinterpret_cast<f32x4*>(out + i) = o;
    return;
  }
  const int64_t k = idx - n_vec;
  const int64_t i = k < head ? k : 4 * n_vec + k;
  if (i < n) out[i] = add_noise_one(x0[i], noise[i], one_minus, sigma, round_bf16);
}

extern "C" int icv_add_noise_f32(const float* x0, const float* noise, float* out, int64_t n, float sigma, int round_bf16,
                                 void* stream) {
  ICV_REQUIRE(n >= 0, "icv_add_noise_f32: negative element count %lld", (long long)n);
  if (n == 0) return 0;
  ICV_REQUIRE(x0 && noise && out, "icv_add_noise_f32: null argument");
  ICV_REQUIRE(((uintptr_t)x0 | (uintptr_t)noise | (uintptr_t)out) % 4 == 0, "icv_add_noise_f32: x0, noise and out must be 4-byte aligned");
  const uintptr_t mis = (uintptr_t)out % 16;
  int64_t head = n, n_vec = 0;              // offsets from a 16-byte boundary differ: every element on the scalar path
  if ((uintptr_t)x0 % 16 == mis && (uintptr_t)noise % 16 == mis) {
    head = (int64_t)((16 - mis) % 16 / 4);
    if (head > n) head = n;
    n_vec = (n - head) / 4;
  }
  const int64_t threads = n_vec + (n - 4 * n_vec);
  ICV_REQUIRE((threads + 255) / 256 < (1ll << 31), "icv_add_noise_f32: %lld elements are too many for one launch", (long long)n);
  hipLaunchKernelGGL(add_noise_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x0, noise, out, n,
                     head, n_vec, sigma, round_bf16);
  return icv_check_launch("icv_add_noise_f32");
}
