// Enhance-A-Video: how much a layer's self-attention looks across frames, and the scalar that follows from it.
//   icv_enhance_scores_bf16   per position s and head h, in f32: L[t, t'] = scale <q[(t, s), h], k[(t', s), h]>, A = softmax over
//                             t' of L, the sum over t != t' of A[t, t']; one partial (the sum over h and t) per position -> workspace
//   icv_enhance_apply_bf16    E = max(1, (T + weight) * mean of m), m = the partials / (T (T - 1));  att <- bf16(f32(att) * E)
// The shape of icv_cfg_zero_scale_f32 (guidance.hip): partials at a launch boundary, then EVERY block of the second launch adds them
// in one fixed order, so every block holds the same E.  No atomics, no host read; the same inputs give the same bits.
#include "icv_common.h"

#pragma clang fp contract(off)

#define ENH_THREADS 256
#define ENH_WAVES (ENH_THREADS / 64)
#define ENH_HD 128                       // head width: 8 k-steps of the 32x32x16 MFMA
#define ENH_APPLY_MAX_BLOCKS 2048

// S^T = K Q^T on v_mfma_f32_32x32x16_bf16: A = K [key frame t' x channel], B = Q^T [channel x query frame t].  Lane l (r = l & 31,
// hf = l >> 5) holds A[r][8 hf + j] and B[8 hf + j][r], j = 0..7, of a k-step: for both operands the 16 bytes at channel
// 16 i + 8 hf of row (r, s) in k-step i - one 16-byte global load each, no LDS.  The result has the query frame on the lane
// (column r) and key frame (reg & 3) + 8 (reg >> 2) + 4 hf in register reg: a query's row of logits lives in lanes r and r + 32.
// Frames >= T of the 32-row tile are not loaded (zero fragments): as keys they are masked out of max and sum, as queries dropped.
__global__ __launch_bounds__(ENH_THREADS) void enhance_scores_kernel(const bf16_t* __restrict__ q, int64_t ldq, const bf16_t* __restrict__ k,
                                                                     int64_t ldk, int T, int64_t P, int heads, float c_exp,
                                                                     float* __restrict__ partial) {
  __shared__ float red[ENH_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, hf = lane >> 5;
  const int64_t s = blockIdx.x;
  const bool live = r < T;
  const int64_t row = (int64_t)(live ? r : 0) * P + s;
  const bf16_t* qrow = q + row * ldq + 8 * hf;
  const bf16_t* krow = k + row * ldk + 8 * hf;
  float acc = 0.f;                                   // this wave's heads: sum over t of (off-diagonal mass / total mass)
  for (int h = wave; h < heads; h += ENH_WAVES) {
    bf16x8 a[8], b[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
      a[i] = live ? *reinterpret_cast<const bf16x8*>(krow + h * ENH_HD + 16 * i) : zero;
      b[i] = live ? *reinterpret_cast<const bf16x8*>(qrow + h * ENH_HD + 16 * i) : zero;
    }
    f32x16 st = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 8; ++i) st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[i], st, 0, 0, 0);
    float mx = -INFINITY;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int tk = (g & 3) + 8 * (g >> 2) + 4 * hf;
      if (tk < T) mx = fmaxf(mx, st[g]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));          // T >= 2: key frames 0 (hf 0) and >= 1 exist, and the pair of lanes covers all
    float sum = 0.f, off = 0.f;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int tk = (g & 3) + 8 * (g >> 2) + 4 * hf;
      const float e = tk < T ? __builtin_amdgcn_exp2f((st[g] - mx) * c_exp) : 0.f;
      sum += e;
      off += tk != r ? e : 0.f;
    }
    sum += __shfl_xor(sum, 32, 64);
    off += __shfl_xor(off, 32, 64);
    acc += wave_sum(live && hf == 0 ? off / sum : 0.f);
  }
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[s] = (red[0] + red[1]) + (red[2] + red[3]);
}

// The sum of the P partials, in every block the same way: thread t adds partials t, t + 256, ... in fp64, then a fixed-shape tree.
__device__ __forceinline__ float enhance_factor(const float* __restrict__ partial, int64_t P, float coef, double* tree) {
  const int tid = threadIdx.x;
  double v = 0.0;
  for (int64_t i = tid; i < P; i += ENH_THREADS) v += (double)partial[i];
  tree[tid] = v;
  __syncthreads();
  for (int w = ENH_THREADS / 2; w > 0; w >>= 1) {
    if (tid < w) tree[tid] += tree[tid + w];
    __syncthreads();
  }
  return fmaxf(1.0f, coef * (float)tree[0]);        // coef = (T + weight) / (T (T - 1) P heads)
}

__global__ __launch_bounds__(ENH_THREADS) void enhance_factor_kernel(const float* __restrict__ partial, int64_t P, float coef,
                                                                     float* __restrict__ score_out) {
  __shared__ double tree[ENH_THREADS];
  const float E = enhance_factor(partial, P, coef, tree);
  if (threadIdx.x == 0) score_out[0] = E;
}

__global__ __launch_bounds__(ENH_THREADS) void enhance_apply_kernel(bf16_t* __restrict__ att, int64_t ld, int64_t n_vec, int vec_per_row,
                                                                    const float* __restrict__ partial, int64_t P, float coef,
                                                                    float* __restrict__ score_out) {
  __shared__ double tree[ENH_THREADS];
  const float E = enhance_factor(partial, P, coef, tree);
  if (blockIdx.x == 0 && threadIdx.x == 0) score_out[0] = E;
  if (E == 1.0f) return;                             // x * 1 is x: the plain bits, without the pass over att
  for (int64_t v = (int64_t)blockIdx.x * ENH_THREADS + threadIdx.x; v < n_vec; v += (int64_t)gridDim.x * ENH_THREADS) {
    const int64_t row = v / vec_per_row;
    u32x4* p = reinterpret_cast<u32x4*>(att + row * ld) + (v - row * vec_per_row);
    u32x4 x = *p;
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = pack_bf16x2(bf16lo_to_f32(x[e]) * E, bf16hi_to_f32(x[e]) * E);
    *p = x;
  }
}

static int enhance_check_grid(const char* who, int64_t T, int64_t P, int64_t heads, float weight) {
  ICV_REQUIRE(T >= 2 && T <= 32, "%s: T=%lld latent frames must be in [2, 32] (one 32-frame tile)", who, (long long)T);
  ICV_REQUIRE(heads > 0 && heads < (1 << 16), "%s: heads=%lld must be in [1, 65535]", who, (long long)heads);
  ICV_REQUIRE(P > 0 && P <= ICV_ENHANCE_WORKSPACE_FLOATS, "%s: P=%lld positions per frame must be in [1, %d] (one partial sum each in the workspace)",
              who, (long long)P, ICV_ENHANCE_WORKSPACE_FLOATS);
  ICV_REQUIRE(weight >= 0.f && weight <= 3.0e38f, "%s: weight=%g must be finite and >= 0", who, (double)weight);
  return 0;
}

static float enhance_coef(int64_t T, int64_t P, int64_t heads, float weight) {
  return (float)(((double)T + (double)weight) / ((double)T * (double)(T - 1) * (double)P * (double)heads));
}

extern "C" int icv_enhance_scores_bf16(const void* q, int64_t ldq, const void* k, int64_t ldk, int64_t T, int64_t P, int64_t heads,
                                       float scale, float weight, float* workspace, float* score_out, void* stream) {
  ICV_REQUIRE(q && k && workspace, "icv_enhance_scores_bf16: null argument");
  if (enhance_check_grid("icv_enhance_scores_bf16", T, P, heads, weight)) return 1;
  ICV_REQUIRE(scale > 0.f && scale <= 3.0e38f, "icv_enhance_scores_bf16: scale=%g must be finite and > 0", (double)scale);
  const int64_t d = heads * ENH_HD;
  ICV_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldq >= d && ldk >= d,
              "icv_enhance_scores_bf16: leading dimensions (%lld, %lld) must be multiples of 8 and >= heads * 128 = %lld (head width 128 only)",
              (long long)ldq, (long long)ldk, (long long)d);
  ICV_REQUIRE(((uintptr_t)q | (uintptr_t)k) % 16 == 0, "icv_enhance_scores_bf16: q and k must be 16-byte aligned");
  ICV_REQUIRE(((uintptr_t)workspace | (uintptr_t)score_out) % 4 == 0, "icv_enhance_scores_bf16: workspace and score_out must be 4-byte aligned");
  const hipStream_t st = (hipStream_t)stream;
  const float c_exp = (float)((double)scale * 1.4426950408889634);      // exp(scale x) = 2^(c_exp x)
  hipLaunchKernelGGL(enhance_scores_kernel, dim3((unsigned)P), dim3(ENH_THREADS), 0, st, (const bf16_t*)q, ldq, (const bf16_t*)k, ldk, (int)T, P,
                     (int)heads, c_exp, workspace);
  if (score_out)
    hipLaunchKernelGGL(enhance_factor_kernel, dim3(1), dim3(ENH_THREADS), 0, st, (const float*)workspace, P, enhance_coef(T, P, heads, weight), score_out);
  return icv_check_launch("icv_enhance_scores_bf16");
}

extern "C" int icv_enhance_apply_bf16(void* att, int64_t ld, int64_t rows, int64_t d, const float* workspace, int64_t T, int64_t P,
                                      int64_t heads, float weight, float* score_out, void* stream) {
  ICV_REQUIRE(att && workspace && score_out, "icv_enhance_apply_bf16: null argument");
  if (enhance_check_grid("icv_enhance_apply_bf16", T, P, heads, weight)) return 1;
  ICV_REQUIRE(rows > 0 && rows < (1ll << 31), "icv_enhance_apply_bf16: rows=%lld must be in [1, 2^31)", (long long)rows);
  ICV_REQUIRE(d > 0 && d % 8 == 0 && d < (1ll << 31), "icv_enhance_apply_bf16: d=%lld must be a positive multiple of 8", (long long)d);
  ICV_REQUIRE(ld % 8 == 0 && ld >= d, "icv_enhance_apply_bf16: ld=%lld must be a multiple of 8 and >= d=%lld", (long long)ld, (long long)d);
  ICV_REQUIRE((uintptr_t)att % 16 == 0, "icv_enhance_apply_bf16: att must be 16-byte aligned");
  ICV_REQUIRE(((uintptr_t)workspace | (uintptr_t)score_out) % 4 == 0, "icv_enhance_apply_bf16: workspace and score_out must be 4-byte aligned");
  const int64_t n_vec = rows * (d / 8);
  const int64_t want = (n_vec + ENH_THREADS - 1) / ENH_THREADS;
  const unsigned blocks = (unsigned)(want < ENH_APPLY_MAX_BLOCKS ? want : ENH_APPLY_MAX_BLOCKS);
  hipLaunchKernelGGL(enhance_apply_kernel, dim3(blocks), dim3(ENH_THREADS), 0, (hipStream_t)stream, (bf16_t*)att, ld, n_vec, (int)(d / 8), workspace,
                     P, enhance_coef(T, P, heads, weight), score_out);
  return icv_check_launch("icv_enhance_apply_bf16");
}
