// Sliding temporal windows: the end of a denoising step when the DiT ran on one temporal window of the latent.
//   icv_unpatchify_cfg_euler_window   latent_next[window frames] += frame_coef[f] * (CFG(hc, hu) * dsigma)
// Overlapping frames are read by two forwards of the SAME step, so the update cannot be in place as in
// icv_unpatchify_cfg_euler (elementwise.hip): the windows of a step all read the step's input latent and accumulate into a copy
// of it, one launch per window on one stream - deterministic, no atomics.
#include "icv_common.h"

// No fused multiply-add contraction in this file: with round_bf16 the kernel is compared bit for bit against a restatement that
// rounds after every tensor operation, and the weighting and the accumulation are two f32 operations there.
#pragma clang fp contract(off)

// One thread per (window-local token, y, c), z = 0, 1 as one float2 - the access pattern of unpatchify_cfg_euler_kernel.
// head-out column = (y*2+z)*C + c.
__global__ __launch_bounds__(256) void unpatchify_cfg_euler_window_kernel(
    float* __restrict__ lat, const float* __restrict__ hc, const float* __restrict__ hu, int64_t ldh, float cfg,
    float dsigma, const float* __restrict__ coef, int64_t frame0, int C, int T, int H8, int W8, int64_t tok0,
    int64_t n_tok, int round_bf16) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n_tok * 2 * C) return;
  const int c = (int)(idx % C);
  const int y = (int)((idx / C) & 1);
  const int64_t r = idx / (2 * C);
  const int64_t tok = tok0 + r;                       // window-local token
  const int Wp = W8 >> 1, Hp = H8 >> 1;
  const int wp = (int)(tok % Wp);
  const int hp = (int)((tok / Wp) % Hp);
  const int f = (int)(tok / ((int64_t)Wp * Hp));      // window-local frame
  const int64_t h0 = r * ldh + (int64_t)(y * 2) * C + c;
  float v0 = hc[h0], v1 = hc[h0 + C];
  const float w = coef[f];
  const int64_t li = (((int64_t)c * T + frame0 + f) * H8 + 2 * hp + y) * W8 + 2 * wp;
  float2* lp = reinterpret_cast<float2*>(lat + li);
  float2 l = *lp;
  if (round_bf16) {
    // the rounding points of unpatchify_cfg_euler_kernel up to v * dsigma; what follows stays f32 (no bf16 pipeline
    // materialises the weighted sum over windows in this order)
    auto rb = [](float x) { return bf16_to_f32((bf16_t)f32_to_bf16_bits(x)); };
    v0 = rb(v0); v1 = rb(v1);
    if (hu) {
      const float u0 = rb(hu[h0]), u1 = rb(hu[h0 + C]);
      v0 = rb(u0 + rb(cfg * rb(v0 - u0)));
      v1 = rb(u1 + rb(cfg * rb(v1 - u1)));
    }
    v0 = rb(v0 * dsigma);
    v1 = rb(v1 * dsigma);
  } else {
    if (hu) {
      const float u0 = hu[h0], u1 = hu[h0 + C];
      v0 = u0 + cfg * (v0 - u0);
      v1 = u1 + cfg * (v1 - u1);
    }
    v0 = v0 * dsigma;
    v1 = v1 * dsigma;
  }
  l.x = l.x + w * v0;
  l.y = l.y + w * v1;
  *lp = l;
}

extern "C" int icv_unpatchify_cfg_euler_window(float* latent_next, const float* hc, const float* hu, int64_t ldh,
                                               float cfg_scale, float dsigma, const float* frame_coef, int64_t frame0,
                                               int64_t C, int64_t T, int64_t H8, int64_t W8, int64_t tok0, int64_t n_tok,
                                               int round_bf16, void* stream) {
  ICV_REQUIRE(latent_next && hc && frame_coef, "icv_unpatchify_cfg_euler_window: null argument");
  ICV_REQUIRE(C > 0 && T > 0 && H8 > 0 && W8 > 0 && H8 % 2 == 0 && W8 % 2 == 0 && n_tok > 0 && ldh >= 4 * C,
              "icv_unpatchify_cfg_euler_window: bad shape");
  ICV_REQUIRE(frame0 >= 0 && frame0 < T && tok0 >= 0 && frame0 * (H8 / 2) * (W8 / 2) + tok0 + n_tok <= T * (H8 / 2) * (W8 / 2),
              "icv_unpatchify_cfg_euler_window: window token range [%lld, %lld) from frame %lld outside the %lld-frame latent",
              (long long)tok0, (long long)(tok0 + n_tok), (long long)frame0, (long long)T);
  const int64_t total = n_tok * 2 * C;
  hipLaunchKernelGGL(unpatchify_cfg_euler_window_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, latent_next, hc, hu, ldh, cfg_scale, dsigma, frame_coef, frame0, (int)C, (int)T,
                     (int)H8, (int)W8, tok0, n_tok, round_bf16);
  return icv_check_launch("icv_unpatchify_cfg_euler_window");
}
