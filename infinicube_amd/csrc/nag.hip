// Normalized Attention Guidance: the token-local pass behind the two text cross-attention launches of a layer.
//   icv_nag_combine_bf16   per row, in f32:  g = p + (scale - 1) (p - n)   (= scale p - (scale - 1) n)
//                                            c = |g|_1 > tau |p|_1 ? tau |p|_1 / |g|_1 : 1
//                                            out = bf16(alpha c g + (1 - alpha) p)
// HBM-bound, the shape of ln_modulate_kernel (elementwise.hip): a row is owned by W waves of a 256-thread block, every lane keeps
// its 16-byte vectors of BOTH inputs packed in VGPRs between the norm pass and the write pass (each input byte is read once, and
// out may be either input), the two L1 norms are reduced across lanes and meet the other waves of the row through 32 bytes of LDS.
#include "icv_common.h"

#define NAG_NV 4      // 16-byte vectors (8 bf16) per lane and input at most: 64 lanes x W = 4 waves x 4 x 8 = 8192 columns

// One width-independent body per W: vector slot i of wave `sub` is vector (i * W + sub) * 64 + lane of the row, live while it is
// below nvec = d / 8 (d % 256 == 0: a half-wave boundary at the finest).  A dead slot holds zeros, adds nothing to either norm and
// is not stored.
template <int W>
__global__ __launch_bounds__(256) void nag_combine_kernel(const bf16_t* zp, int64_t ldp, const bf16_t* zn, int64_t ldn, bf16_t* out,
                                                          int64_t ldo, int64_t rows, int nvec, float sm1, float tau, float alpha) {
  __shared__ float red[8];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  constexpr int RPB = 4 / W;             // rows per block
  const int64_t row_raw = (int64_t)blockIdx.x * RPB + wave / W;
  const bool live = row_raw < rows;      // dead rows still take part in the barrier
  const int64_t row = live ? row_raw : rows - 1;
  const int sub = wave % W;
  const u32x4* pr = reinterpret_cast<const u32x4*>(zp + row * ldp);
  const u32x4* nr = reinterpret_cast<const u32x4*>(zn + row * ldn);
  u32x4 p[NAG_NV], n[NAG_NV];
#pragma unroll
  for (int i = 0; i < NAG_NV; ++i) {
    const int c = (i * W + sub) * 64 + lane;
    const u32x4 zero = {0u, 0u, 0u, 0u};
    p[i] = c < nvec ? pr[c] : zero;
    n[i] = c < nvec ? nr[c] : zero;
  }
  float np = 0.f, ng = 0.f;
#pragma unroll
  for (int i = 0; i < NAG_NV; ++i) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float p0 = bf16lo_to_f32(p[i][e]), p1 = bf16hi_to_f32(p[i][e]);
      const float n0 = bf16lo_to_f32(n[i][e]), n1 = bf16hi_to_f32(n[i][e]);
      np += fabsf(p0) + fabsf(p1);
      ng += fabsf(fmaf(sm1, p0 - n0, p0)) + fabsf(fmaf(sm1, p1 - n1, p1));
    }
  }
  np = wave_sum(np);
  ng = wave_sum(ng);
  if (W > 1) {
    if (lane == 0) { red[wave] = np; red[4 + wave] = ng; }
    __syncthreads();
    const int base = (wave / W) * W;
    np = 0.f; ng = 0.f;
#pragma unroll
    for (int i = 0; i < W; ++i) { np += red[base + i]; ng += red[4 + base + i]; }
  }
  if (!live) return;
  const float lim = tau * np;
  const float ac = alpha * (ng > lim ? lim / ng : 1.0f);      // np == 0: 0 (ng > 0) or alpha (g == 0 everywhere); never a division by 0
  const float om = 1.0f - alpha;
  u32x4* orow = reinterpret_cast<u32x4*>(out + row * ldo);
#pragma unroll
  for (int i = 0; i < NAG_NV; ++i) {
    const int c = (i * W + sub) * 64 + lane;
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float p0 = bf16lo_to_f32(p[i][e]), p1 = bf16hi_to_f32(p[i][e]);
      const float n0 = bf16lo_to_f32(n[i][e]), n1 = bf16hi_to_f32(n[i][e]);
      o[e] = pack_bf16x2(ac * fmaf(sm1, p0 - n0, p0) + om * p0, ac * fmaf(sm1, p1 - n1, p1) + om * p1);
    }
    if (c < nvec) orow[c] = o;
  }
}

extern "C" int icv_nag_combine_bf16(const void* z_pos, int64_t ld_pos, const void* z_neg, int64_t ld_neg, void* out, int64_t ld_out,
                                    int64_t rows, int64_t d, float scale, float tau, float alpha, void* stream) {
  ICV_REQUIRE(z_pos && z_neg && out, "icv_nag_combine_bf16: null argument");
  ICV_REQUIRE(rows > 0 && rows < (1ll << 31), "icv_nag_combine_bf16: rows=%lld must be in [1, 2^31)", (long long)rows);
  ICV_REQUIRE(d > 0 && d % 256 == 0 && d <= 8192, "icv_nag_combine_bf16: d=%lld must be a multiple of 256 and <= 8192", (long long)d);
  ICV_REQUIRE(ld_pos % 8 == 0 && ld_neg % 8 == 0 && ld_out % 8 == 0 && ld_pos >= d && ld_neg >= d && ld_out >= d,
              "icv_nag_combine_bf16: leading dimensions (%lld, %lld, %lld) must be multiples of 8 and >= d=%lld", (long long)ld_pos,
              (long long)ld_neg, (long long)ld_out, (long long)d);
  ICV_REQUIRE(((uintptr_t)z_pos | (uintptr_t)z_neg | (uintptr_t)out) % 16 == 0, "icv_nag_combine_bf16: z_pos, z_neg and out must be 16-byte aligned");
  ICV_REQUIRE((out != z_pos || ld_out == ld_pos) && (out != z_neg || ld_out == ld_neg),
              "icv_nag_combine_bf16: out may be an input only with that input's leading dimension");
  const int nvec = (int)(d / 8);
  const int W = nvec <= 64 * NAG_NV ? 1 : nvec <= 128 * NAG_NV ? 2 : 4;      // the fewest waves whose NAG_NV slots cover the row
  const dim3 grid((unsigned)((rows * W + 3) / 4)), block(256);
  const bf16_t *zp = (const bf16_t*)z_pos, *zn = (const bf16_t*)z_neg;
  bf16_t* o = (bf16_t*)out;
  hipStream_t st = (hipStream_t)stream;
  const float sm1 = scale - 1.0f;
  if (W == 1) hipLaunchKernelGGL(nag_combine_kernel<1>, grid, block, 0, st, zp, ld_pos, zn, ld_neg, o, ld_out, rows, nvec, sm1, tau, alpha);
  else if (W == 2) hipLaunchKernelGGL(nag_combine_kernel<2>, grid, block, 0, st, zp, ld_pos, zn, ld_neg, o, ld_out, rows, nvec, sm1, tau, alpha);
  else hipLaunchKernelGGL(nag_combine_kernel<4>, grid, block, 0, st, zp, ld_pos, zn, ld_neg, o, ld_out, rows, nvec, sm1, tau, alpha);
  return icv_check_launch("icv_nag_combine_bf16");
}
