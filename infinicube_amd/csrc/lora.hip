// LoRA merge into a packed projection weight:
//   icv_lora_merge_bf16   W[n, k] <- bf16_rn( f32(W[n, k]) + alpha * sum_j up[n, j] * down_t[k, j] )
// W is a plain row-major bf16 matrix that every consumer of the engine holds by pointer, so the update is in place.  The rank
// sum runs on the 32x32x16 bf16 MFMA in f32; alpha and the addition of W are one f32 fused multiply-add; ONE rounding, at the
// store.  Memory-bound: 4 N K bytes of W traffic against 2 N K R flops.
//
// One wave owns a 64 x 64 tile of W as 2 x 2 MFMA tiles.  D = A B with A = down_t rows (the MFMA's M index = a column of W)
// and B = up rows (the MFMA's N index = a row of W): both are rank-contiguous, so a lane's operand fragment (8 ranks of one
// row) is one 16-byte global load - no LDS.  The accumulator then has the W ROW on the lane (lane & 31) and 16 W COLUMNS in
// its registers.  Which W column an MFMA row stands for is this kernel's choice (it only picks the down_t row the A lane
// loads): MFMA row m = 8g + 4h + i of column-tile t is W column 32h + 16t + 4g + i, so that the 32 accumulator values of a
// lane (h = lane >> 5 is fixed per lane) are 32 CONSECUTIVE columns of one W row: four 16-byte loads and stores per lane
// and row-tile, and the two lanes of a row cover one 128-byte line.
#include "icv_common.h"

#define LORA_TILE 64

__global__ __launch_bounds__(256) void lora_merge_kernel(bf16_t* __restrict__ W, int64_t ldw, const bf16_t* __restrict__ up,
                                                         int64_t ldu, const bf16_t* __restrict__ down_t, int64_t ldd,
                                                         int tiles_k, int64_t n_tiles, int R, float alpha) {
  const int lane = threadIdx.x & 63;
  const int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);      // consecutive waves: neighbouring column tiles of one row tile
  if (tile >= n_tiles) return;
  const int64_t n0 = (tile / tiles_k) * LORA_TILE, k0 = (tile % tiles_k) * LORA_TILE;
  const int r = lane & 31, h = lane >> 5;
  // A operand of column-tile t: MFMA row r = 8g + 4hh + i  ->  W column 32hh + 16t + 4g + i
  const int kcol = 32 * ((r >> 2) & 1) + 4 * (r >> 3) + (r & 3);
  const bf16_t* dp[2] = {down_t + (k0 + kcol) * ldd + 8 * h, down_t + (k0 + kcol + 16) * ldd + 8 * h};
  const bf16_t* upp[2] = {up + (n0 + r) * ldu + 8 * h, up + (n0 + 32 + r) * ldu + 8 * h};
  f32x16 acc[2][2];       // [row tile][column tile]
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[a][t][i] = 0.f;
  for (int j = 0; j < R; j += 16) {
    bf16x8 df[2], uf[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) df[t] = *reinterpret_cast<const bf16x8*>(dp[t] + j);
#pragma unroll
    for (int a = 0; a < 2; ++a) uf[a] = *reinterpret_cast<const bf16x8*>(upp[a] + j);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int t = 0; t < 2; ++t) acc[a][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(df[t], uf[a], acc[a][t], 0, 0, 0);
  }
  // accumulator register 4g + i of column-tile t  ->  W column k0 + 32h + 16t + 4g + i: 16-byte chunk c = 2t + (g >> 1)
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    u32x4* wp = reinterpret_cast<u32x4*>(W + (n0 + 32 * a + r) * ldw + k0 + 32 * h);
    u32x4 w[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) w[c] = wp[c];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int reg = 8 * (c & 1) + 2 * p;
        const float lo = fmaf(alpha, acc[a][c >> 1][reg], bf16lo_to_f32(w[c][p]));
        const float hi = fmaf(alpha, acc[a][c >> 1][reg + 1], bf16hi_to_f32(w[c][p]));
        w[c][p] = pack_bf16x2(lo, hi);
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) wp[c] = w[c];
  }
}

extern "C" int icv_lora_merge_bf16(void* W, int64_t ldw, const void* up, int64_t ldu, const void* down_t, int64_t ldd, int64_t N,
                                   int64_t K, int64_t R, float alpha, void* stream) {
  ICV_REQUIRE(W && up && down_t, "icv_lora_merge_bf16: null argument");
  ICV_REQUIRE(N > 0 && K > 0 && N % LORA_TILE == 0 && K % LORA_TILE == 0,
              "icv_lora_merge_bf16: N = %lld and K = %lld must be positive multiples of 64", (long long)N, (long long)K);
  ICV_REQUIRE(R >= 32 && R <= 512 && R % 32 == 0, "icv_lora_merge_bf16: rank %lld must be a multiple of 32 in [32, 512] (zero-pad smaller ranks)",
              (long long)R);
  ICV_REQUIRE(ldw >= K && ldu >= R && ldd >= R && ldw % 8 == 0 && ldu % 8 == 0 && ldd % 8 == 0,
              "icv_lora_merge_bf16: row strides (%lld, %lld, %lld) must be multiples of 8 elements and cover K = %lld / R = %lld",
              (long long)ldw, (long long)ldu, (long long)ldd, (long long)K, (long long)R);
  ICV_REQUIRE(((uintptr_t)W | (uintptr_t)up | (uintptr_t)down_t) % 16 == 0, "icv_lora_merge_bf16: W, up and down_t must be 16-byte aligned");
  const int64_t n_tiles = (N / LORA_TILE) * (K / LORA_TILE);
  ICV_REQUIRE(K / LORA_TILE < (1ll << 31) && (n_tiles + 3) / 4 < (1ll << 31), "icv_lora_merge_bf16: matrix too large");
  if (alpha == 0.0f) return 0;      // W + 0 * (B A) is W: nothing to read or write
  hipLaunchKernelGGL(lora_merge_kernel, dim3((unsigned)((n_tiles + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (bf16_t*)W, ldw,
                     (const bf16_t*)up, ldu, (const bf16_t*)down_t, ldd, (int)(K / LORA_TILE), n_tiles, (int)R, alpha);
  return icv_check_launch("icv_lora_merge_bf16");
}
