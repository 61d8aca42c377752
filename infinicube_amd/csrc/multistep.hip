// Multistep samplers: the end of a denoising step when the latent update is a linear multistep rule on the
// x0-prediction (UniPC today) instead of the first-order Euler step of icv_unpatchify_cfg_euler (elementwise.hip).
//   icv_unpatchify_cfg_multistep   v = CFG(hc, hu);  m = x - sigma v;  x_c = a . (x_hat, m_prev, m_prev2, m);  x <- c . (x_c, m, m_prev)
// The kernel knows nothing of the solver: the host (videogen/solver.py) hands it the two coefficient vectors of the step.
#include "icv_common.h"

// No fused multiply-add contraction in this file: the sums are evaluated left to right, product by product, as written.
#pragma clang fp contract(off)

struct multistep_coef {
  float sigma;
  float a0, a1, a2, a3;   // x_c = a0 x_hat + a1 m_prev + a2 m_prev2 + a3 m   (corrector != 0; else x_c = x)
  float c0, c1, c2;       // x_next = c0 x_c + c1 m + c2 m_prev
};

// One thread per (local token, y, c), z = 0, 1 as one float2 - the access pattern of unpatchify_cfg_euler_kernel.
// head-out column = (y*2+z)*C + c.  x_hat is read and written by the same thread at the same element; m_new, m_prev and
// m_prev2 are three different buffers.  A buffer whose coefficient is 0 is not read (its pointer may be NULL).
__global__ __launch_bounds__(256) void unpatchify_cfg_multistep_kernel(
    float* __restrict__ lat, float* x_hat, float* __restrict__ m_new, const float* __restrict__ m_prev,
    const float* __restrict__ m_prev2, const float* __restrict__ hc, const float* __restrict__ hu, int64_t ldh, float cfg,
    multistep_coef k, int corrector, int C, int T, int H8, int W8, int64_t tok0, int64_t n_tok, int round_bf16) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n_tok * 2 * C) return;
  const int c = (int)(idx % C);
  const int y = (int)((idx / C) & 1);
  const int64_t r = idx / (2 * C);
  const int64_t tok = tok0 + r;
  const int Wp = W8 >> 1, Hp = H8 >> 1;
  const int wp = (int)(tok % Wp);
  const int hp = (int)((tok / Wp) % Hp);
  const int f = (int)(tok / ((int64_t)Wp * Hp));
  const int64_t h0 = r * ldh + (int64_t)(y * 2) * C + c;
  float v0 = hc[h0], v1 = hc[h0 + C];
  const int64_t li = (((int64_t)c * T + f) * H8 + 2 * hp + y) * W8 + 2 * wp;
  if (round_bf16) {
    // the rounding points of unpatchify_cfg_euler_kernel on the velocity; the solver arithmetic below stays f32
    auto rb = [](float x) { return bf16_to_f32((bf16_t)f32_to_bf16_bits(x)); };
    v0 = rb(v0); v1 = rb(v1);
    if (hu) {
      const float u0 = rb(hu[h0]), u1 = rb(hu[h0 + C]);
      v0 = rb(u0 + rb(cfg * rb(v0 - u0)));
      v1 = rb(u1 + rb(cfg * rb(v1 - u1)));
    }
  } else if (hu) {
    const float u0 = hu[h0], u1 = hu[h0 + C];
    v0 = u0 + cfg * (v0 - u0);
    v1 = u1 + cfg * (v1 - u1);
  }
  const float2 zero = make_float2(0.f, 0.f);
  const float2 x = *reinterpret_cast<const float2*>(lat + li);
  const float2 m = make_float2(x.x - k.sigma * v0, x.y - k.sigma * v1);
  const float2 p1 = (k.a1 != 0.f || k.c2 != 0.f) ? *reinterpret_cast<const float2*>(m_prev + li) : zero;
  float2 xc = x;
  if (corrector) {
    const float2 xh = k.a0 != 0.f ? *reinterpret_cast<const float2*>(x_hat + li) : zero;
    const float2 p2 = k.a2 != 0.f ? *reinterpret_cast<const float2*>(m_prev2 + li) : zero;
    xc.x = k.a0 * xh.x + k.a1 * p1.x + k.a2 * p2.x + k.a3 * m.x;
    xc.y = k.a0 * xh.y + k.a1 * p1.y + k.a2 * p2.y + k.a3 * m.y;
  }
  *reinterpret_cast<float2*>(m_new + li) = m;
  *reinterpret_cast<float2*>(x_hat + li) = xc;
  *reinterpret_cast<float2*>(lat + li) =
      make_float2(k.c0 * xc.x + k.c1 * m.x + k.c2 * p1.x, k.c0 * xc.y + k.c1 * m.y + k.c2 * p1.y);
}

extern "C" int icv_unpatchify_cfg_multistep(float* latent, float* x_hat, float* m_new, const float* m_prev,
                                            const float* m_prev2, const float* hc, const float* hu, int64_t ldh,
                                            float cfg_scale, float sigma, int corrector, float a0, float a1, float a2,
                                            float a3, float c0, float c1, float c2, int64_t C, int64_t T, int64_t H8,
                                            int64_t W8, int64_t tok0, int64_t n_tok, int round_bf16, void* stream) {
  ICV_REQUIRE(latent && x_hat && m_new && hc, "icv_unpatchify_cfg_multistep: null argument");
  ICV_REQUIRE(C > 0 && T > 0 && H8 > 0 && W8 > 0 && H8 % 2 == 0 && W8 % 2 == 0 && n_tok > 0, "icv_unpatchify_cfg_multistep: bad shape");
  ICV_REQUIRE(ldh >= 4 * C, "icv_unpatchify_cfg_multistep: ldh (%lld) is less than the 4 * C = %lld columns of a head row",
              (long long)ldh, (long long)(4 * C));
  ICV_REQUIRE(tok0 >= 0 && tok0 + n_tok <= T * (H8 / 2) * (W8 / 2), "icv_unpatchify_cfg_multistep: token range");
  ICV_REQUIRE(corrector || (a0 == 0.f && a1 == 0.f && a2 == 0.f && a3 == 0.f),
              "icv_unpatchify_cfg_multistep: corrector coefficients given for a step without a corrector");
  ICV_REQUIRE(m_prev || ((!corrector || a1 == 0.f) && c2 == 0.f), "icv_unpatchify_cfg_multistep: m_prev is NULL but its coefficient is not 0");
  ICV_REQUIRE(m_prev2 || !corrector || a2 == 0.f, "icv_unpatchify_cfg_multistep: m_prev2 is NULL but its coefficient is not 0");
  ICV_REQUIRE((((uintptr_t)latent | (uintptr_t)x_hat | (uintptr_t)m_new | (uintptr_t)m_prev | (uintptr_t)m_prev2) & 7) == 0,
              "icv_unpatchify_cfg_multistep: latent, x_hat and the x0-prediction slots must be 8-byte aligned");
  ICV_REQUIRE(m_new != m_prev && m_new != m_prev2 && m_new != latent && m_new != x_hat && x_hat != latent &&
                  (const float*)x_hat != m_prev && (const float*)x_hat != m_prev2 && (const float*)latent != m_prev &&
                  (const float*)latent != m_prev2,
              "icv_unpatchify_cfg_multistep: the written buffers (latent, x_hat, m_new) must differ from each other and from what is read");
  multistep_coef k;
  k.sigma = sigma;
  k.a0 = a0; k.a1 = a1; k.a2 = a2; k.a3 = a3;
  k.c0 = c0; k.c1 = c1; k.c2 = c2;
  const int64_t total = n_tok * 2 * C;
  hipLaunchKernelGGL(unpatchify_cfg_multistep_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, latent, x_hat, m_new, m_prev, m_prev2, hc, hu, ldh, cfg_scale, k, corrector,
                     (int)C, (int)T, (int)H8, (int)W8, tok0, n_tok, round_bf16);
  return icv_check_launch("icv_unpatchify_cfg_multistep");
}
