// Coarse-to-fine sampling, the stage switch: the coarse stage's x0-prediction resized to the fine latent grid and
// noised to the fine stage's first sigma, in one launch, into the fine noise's own tensor.
//   icv_latent_resize_noise_f32   noise_out[p, Y, X] = (1 - sigma) * up(x0)[p, Y, X] + sigma * noise_out[p, Y, X]
// up = bilinear resize of every plane, half-pixel centres (the arithmetic is stated in include/icvideo.h).  HBM-bound, once per call:
// per output element one read and one write of noise_out and four gathered reads of x0, which is at most as large and stays in
// cache.  noise_out is one contiguous run of planes * h_out * w_out floats, so the 16-byte body is laid over the FLAT run, as in
// add_noise_kernel (v2v.hip): a vector may end one row and begin the next (a ragged width costs no vector), and the up-to-3
// elements before the first 16-byte boundary and after the last one go one by one.  Every element's (plane, Y, X) comes from its
// flat index; a thread divides once and steps X, wrapping into the next row where its vector crosses one.
#include "icv_common.h"

// No fused multiply-add contraction in this file: the result is compared bit for bit against a restatement with one tensor
// operation per rounding, in both rounding modes.
#pragma clang fp contract(off)

struct resize_dims {
  unsigned h_in, w_in, h_out, w_out;
  float scale_y, scale_x;      // h_in / h_out and w_in / w_out, divided in f32 on the host
};

// Source cell and weight of output index `o` along one axis: s = max((o + 0.5) * scale - 0.5, 0), i0 = min(floor(s), n_in - 1),
// i1 = min(i0 + 1, n_in - 1), l = s - i0.
__device__ __forceinline__ void source_of(unsigned o, float scale, unsigned n_in, unsigned& i0, unsigned& i1, float& l) {
  const float s = fmaxf(((float)o + 0.5f) * scale - 0.5f, 0.0f);
  i0 = min((unsigned)s, n_in - 1);          // s >= 0: the conversion truncates = floor
  i1 = min(i0 + 1, n_in - 1);
  l = s - (float)i0;
}

struct row_state {
  const float* top;      // x0 rows y0 and y1 of the element's plane
  const float* bot;
  float ly, wy0;         // ly and 1 - ly
};

__device__ __forceinline__ row_state row_of(const float* x0, unsigned row, const resize_dims& d) {
  const unsigned p = row / d.h_out, Y = row - p * d.h_out;
  unsigned y0, y1;
  row_state r;
  source_of(Y, d.scale_y, d.h_in, y0, y1, r.ly);
  r.wy0 = 1.0f - r.ly;
  const float* plane = x0 + (int64_t)p * d.h_in * d.w_in;
  r.top = plane + (int64_t)y0 * d.w_in;
  r.bot = plane + (int64_t)y1 * d.w_in;
  return r;
}

__device__ __forceinline__ float resize_noise_one(const row_state& r, unsigned X, float z, const resize_dims& d, float one_minus,
                                                  float sigma, int round_bf16) {
  unsigned x0i, x1i;
  float lx;
  source_of(X, d.scale_x, d.w_in, x0i, x1i, lx);
  const float wx0 = 1.0f - lx;
  const float t = wx0 * r.top[x0i] + lx * r.top[x1i];
  const float b = wx0 * r.bot[x0i] + lx * r.bot[x1i];
  const float v = r.wy0 * t + r.ly * b;
  return add_noise_one(v, z, one_minus, sigma, round_bf16);
}

// Threads [0, n_vec): one 16-byte vector each, flat elements [head + 4 idx, head + 4 idx + 4).  Threads [n_vec, n_vec + n - 4 n_vec):
// one element each - first the `head` elements in front of the vector body, then the ones behind it.  n < 2^31 (the dispatcher).
__global__ __launch_bounds__(256) void latent_resize_noise_kernel(const float* x0, float* noise_out, unsigned n, unsigned head,
                                                                  unsigned n_vec, resize_dims d, float sigma, int round_bf16) {
  const unsigned idx = blockIdx.x * 256u + threadIdx.x;
  const float one_minus = 1.0f - sigma;
  if (idx < n_vec) {
    const unsigned i = head + 4 * idx;
    unsigned row = i / d.w_out, X = i - row * d.w_out;
    row_state r = row_of(x0, row, d);
    const f32x4 z = *reinterpret_cast<const f32x4*>(noise_out + i);
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (X == d.w_out) {      // the vector runs on into the next row (i + j < n: that row exists)
        X = 0;
        r = row_of(x0, ++row, d);
      }
      o[j] = resize_noise_one(r, X, z[j], d, one_minus, sigma, round_bf16);
      ++X;
    }
    *reinterpret_cast<f32x4*>(noise_out + i) = o;
    return;
  }
  const unsigned k = idx - n_vec;
  const unsigned i = k < head ? k : 4 * n_vec + k;
  if (i < n) {
    const unsigned row = i / d.w_out;
    const row_state r = row_of(x0, row, d);
    noise_out[i] = resize_noise_one(r, i - row * d.w_out, noise_out[i], d, one_minus, sigma, round_bf16);
  }
}

extern "C" int icv_latent_resize_noise_f32(const float* x0, float* noise_out, int64_t planes, int64_t h_in, int64_t w_in,
                                           int64_t h_out, int64_t w_out, float sigma, int round_bf16, void* stream) {
  ICV_REQUIRE(planes >= 0, "icv_latent_resize_noise_f32: negative plane count %lld", (long long)planes);
  if (planes == 0) return 0;
  ICV_REQUIRE(x0 && noise_out, "icv_latent_resize_noise_f32: null argument");
  ICV_REQUIRE(h_in >= 1 && w_in >= 1, "icv_latent_resize_noise_f32: the input plane must be at least 1 x 1, got %lld x %lld",
              (long long)h_in, (long long)w_in);
  ICV_REQUIRE(h_out >= h_in && w_out >= w_in,
              "icv_latent_resize_noise_f32: the output plane %lld x %lld must be at least the input plane %lld x %lld in both dimensions",
              (long long)h_out, (long long)w_out, (long long)h_in, (long long)w_in);
  ICV_REQUIRE(((uintptr_t)x0 | (uintptr_t)noise_out) % 4 == 0, "icv_latent_resize_noise_f32: x0 and noise_out must be 4-byte aligned");
  // 32-bit element indices in the kernel; h_out, w_out < 2^31 first, so that the products below cannot overflow 64 bits
  const int64_t lim = 1ll << 31;
  ICV_REQUIRE(h_out < lim && w_out < lim && planes < lim && h_out * w_out < lim && planes * (h_out * w_out) < lim,
              "icv_latent_resize_noise_f32: %lld planes of %lld x %lld elements are too many for one launch (2^31 - 1 elements at most)",
              (long long)planes, (long long)h_out, (long long)w_out);
  const int64_t n = planes * h_out * w_out;
  int64_t head = (int64_t)((16 - (uintptr_t)noise_out % 16) % 16 / 4);
  if (head > n) head = n;
  const int64_t n_vec = (n - head) / 4;
  const int64_t threads = n_vec + (n - 4 * n_vec);
  resize_dims d;
  d.h_in = (unsigned)h_in, d.w_in = (unsigned)w_in, d.h_out = (unsigned)h_out, d.w_out = (unsigned)w_out;
  d.scale_y = (float)h_in / (float)h_out;
  d.scale_x = (float)w_in / (float)w_out;
  hipLaunchKernelGGL(latent_resize_noise_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x0,
                     noise_out, (unsigned)n, (unsigned)head, (unsigned)n_vec, d, sigma, round_bf16);
  return icv_check_launch("icv_latent_resize_noise_f32");
}
