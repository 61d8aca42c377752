// Regenerating part of a clip: the known cells of the latent are put back on the noising trajectory of the known
// clip after every step, with the noise the call drew.
//   icv_latent_keep_mask_u8   keep[t, h, w] = 1 iff every mask byte of the cell's stride footprint is 0   (once per call)
//   icv_pin_known_f32         latent[c, j] = (1 - sigma_next) * x0[c, j] + sigma_next * noise[c, j] where keep[j]   (once per step)
// Both are HBM-bound and plain C++.  The pin is shaped for a clip of which a few latent frames are kept: a thread reads the keep
// bytes of its cells first and touches nothing else when none is set.
#include "icv_common.h"

// No fused multiply-add contraction in this file: the pin is add_noise_one (icv_common.h), icv_add_noise_f32's arithmetic, and is
// compared bit for bit against that kernel and against the torch restatement, in both rounding modes.
#pragma clang fp contract(off)

// One thread per latent cell: the 8 x 8 bytes of each of its 1 (t = 0) or 4 frames, OR-ed.  Neighbouring threads read neighbouring
// 8-byte groups of one mask row.  wide: the mask is 8-byte aligned (W is a multiple of 16, so every group then is).
__global__ __launch_bounds__(256) void latent_keep_mask_kernel(const uint8_t* mask, uint8_t* keep, int64_t H, int64_t W,
                                                               int64_t n_cells, int wide) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n_cells) return;
  const int64_t W8 = W / 8, H8 = H / 8;
  const int64_t w = idx % W8, h = (idx / W8) % H8, t = idx / (W8 * H8);
  const int64_t f0 = t == 0 ? 0 : 4 * t - 3, f1 = 4 * t;
  unsigned long long acc = 0;
  for (int64_t f = f0; f <= f1; ++f) {
    const uint8_t* base = mask + (f * H + 8 * h) * W + 8 * w;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const uint8_t* row = base + r * W;
      if (wide) {
        acc |= *reinterpret_cast<const unsigned long long*>(row);
      } else {
#pragma unroll
        for (int b = 0; b < 8; ++b) acc |= row[b];
      }
    }
  }
  keep[idx] = acc == 0 ? 1 : 0;
}

extern "C" int icv_latent_keep_mask_u8(const uint8_t* mask, uint8_t* keep, int64_t N, int64_t H, int64_t W, void* stream) {
  ICV_REQUIRE(N >= 1 && N % 4 == 1, "icv_latent_keep_mask_u8: %lld frames, need 4k + 1", (long long)N);
  ICV_REQUIRE(H >= 0 && W >= 0 && H % 16 == 0 && W % 16 == 0, "icv_latent_keep_mask_u8: height %lld and width %lld must be multiples of 16",
              (long long)H, (long long)W);
  if (H == 0 || W == 0) return 0;
  ICV_REQUIRE(mask && keep, "icv_latent_keep_mask_u8: null argument");
  const int64_t n_cells = ((N - 1) / 4 + 1) * (H / 8) * (W / 8);
  ICV_REQUIRE((n_cells + 255) / 256 < (1ll << 31), "icv_latent_keep_mask_u8: %lld cells are too many for one launch", (long long)n_cells);
  hipLaunchKernelGGL(latent_keep_mask_kernel, dim3((unsigned)((n_cells + 255) / 256)), dim3(256), 0, (hipStream_t)stream, mask, keep, H,
                     W, n_cells, (int)((uintptr_t)mask % 8 == 0));
  return icv_check_launch("icv_latent_keep_mask_u8");
}

// Per channel (blockIdx.y, strided over C), slots [0, n_vec): the four cells [head + 4 s, head + 4 s + 4), one 16-byte vector of
// every tensor, guarded by their four keep bytes (one 32-bit word where keep + head is 4-byte aligned: keep_word).  Slots
// [n_vec, n_vec + cells - 4 n_vec): one cell each - first the `head` cells in front of the vector body, then the ones behind it.
// The keep bytes are read before anything else; a slot with none set returns.  A vector with all four set is stored as a vector,
// a partly kept one element by element: an element whose cell is not kept is never written.
__global__ __launch_bounds__(256) void pin_known_kernel(float* latent, float* x_hat, float* m_new, const float* x0, const float* noise,
                                                        const uint8_t* keep, int64_t C, int64_t cells, int64_t head, int64_t n_vec,
                                                        int keep_word, float sigma_next, float sigma_cur, int round_bf16) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n_vec + (cells - 4 * n_vec)) return;
  const float om_next = 1.0f - sigma_next, om_cur = 1.0f - sigma_cur;
  if (idx < n_vec) {
    const int64_t j = head + 4 * idx;
    unsigned kw;
    if (keep_word) {
      kw = *reinterpret_cast<const unsigned*>(keep + j);
    } else {
      kw = (unsigned)keep[j] | (unsigned)keep[j + 1] << 8 | (unsigned)keep[j + 2] << 16 | (unsigned)keep[j + 3] << 24;
    }
    if (kw == 0) return;
    const bool all = (kw & 0xffu) && (kw & 0xff00u) && (kw & 0xff0000u) && (kw & 0xff000000u);
    for (int64_t c = blockIdx.y; c < C; c += gridDim.y) {
      const int64_t i = c * cells + j;
      const f32x4 x = *reinterpret_cast<const f32x4*>(x0 + i);
      const f32x4 z = *reinterpret_cast<const f32x4*>(noise + i);
      f32x4 o, hcur;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        o[e] = add_noise_one(x[e], z[e], om_next, sigma_next, round_bf16);
        hcur[e] = x_hat ? add_noise_one(x[e], z[e], om_cur, sigma_cur, round_bf16) : 0.f;
      }
      if (all) {
        *reinterpret_cast<f32x4*>(latent + i) = o;
        if (x_hat) *reinterpret_cast<f32x4*>(x_hat + i) = hcur;
        if (m_new) *reinterpret_cast<f32x4*>(m_new + i) = x;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if ((kw >> (8 * e)) & 0xffu) {
            latent[i + e] = o[e];
            if (x_hat) x_hat[i + e] = hcur[e];
            if (m_new) m_new[i + e] = x[e];
          }
        }
      }
    }
    return;
  }
  const int64_t k = idx - n_vec;
  const int64_t j = k < head ? k : 4 * n_vec + k;
  if (keep[j] == 0) return;
  for (int64_t c = blockIdx.y; c < C; c += gridDim.y) {
    const int64_t i = c * cells + j;
    const float x = x0[i], z = noise[i];
    latent[i] = add_noise_one(x, z, om_next, sigma_next, round_bf16);
    if (x_hat) x_hat[i] = add_noise_one(x, z, om_cur, sigma_cur, round_bf16);
    if (m_new) m_new[i] = x;
  }
}

extern "C" int icv_pin_known_f32(float* latent, float* x_hat, float* m_new, const float* x0, const float* noise, const uint8_t* keep,
                                 int64_t C, int64_t cells, float sigma_next, float sigma_cur, int round_bf16, void* stream) {
  ICV_REQUIRE(C >= 0 && cells >= 0, "icv_pin_known_f32: negative size (C %lld, cells %lld)", (long long)C, (long long)cells);
  if (C == 0 || cells == 0) return 0;
  ICV_REQUIRE(latent && x0 && noise && keep, "icv_pin_known_f32: null argument");
  ICV_REQUIRE(((uintptr_t)latent | (uintptr_t)x_hat | (uintptr_t)m_new | (uintptr_t)x0 | (uintptr_t)noise) % 4 == 0,
              "icv_pin_known_f32: latent, x_hat, m_new, x0 and noise must be 4-byte aligned");
  ICV_REQUIRE(cells < (1ll << 40) && C < (1ll << 22), "icv_pin_known_f32: C %lld x cells %lld is too large", (long long)C, (long long)cells);
  // 16-byte vectors where every tensor sits at the same offset from a 16-byte boundary AND a channel is a whole number of
  // vectors (so that the offset is every channel's); otherwise every cell on the scalar path
  const uintptr_t mis = (uintptr_t)latent % 16;
  int64_t head = cells, n_vec = 0;
  if (cells % 4 == 0 && (uintptr_t)x0 % 16 == mis && (uintptr_t)noise % 16 == mis && (!x_hat || (uintptr_t)x_hat % 16 == mis) &&
      (!m_new || (uintptr_t)m_new % 16 == mis)) {
    head = (int64_t)((16 - mis) % 16 / 4);      // < 4 <= cells
    n_vec = (cells - head) / 4;
  }
  const int64_t slots = n_vec + (cells - 4 * n_vec);
  hipLaunchKernelGGL(pin_known_kernel, dim3((unsigned)((slots + 255) / 256), (unsigned)(C < 65535 ? C : 65535)), dim3(256), 0,
                     (hipStream_t)stream, latent, x_hat, m_new, x0, noise, keep, C, cells, head, n_vec,
                     (int)(((uintptr_t)keep + (uintptr_t)head) % 4 == 0), sigma_next, sigma_cur, round_bf16);
  return icv_check_launch("icv_pin_known_f32");
}
