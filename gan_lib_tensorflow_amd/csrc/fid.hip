// The statistics stage of the Frechet Inception Distance (common/fid.py; the FID column and TODO entry of the reference's README):
//   gank_mean_hw_f32     pool_3 of the Inception trunk WITHOUT the 16-bit rounding of gank_pool2d's output: fp32 means over HW;
//   gank_moments_update  the running float64 moments of a feature set: sum[j] += sum_i x[i][j] and, for the 16x16 tiles on and
//                        above the diagonal, gram[j][k] += sum_i x[i][j] x[i][k], on v_mfma_f64_16x16x4_f64.
//
// moments_update.  A 256-thread workgroup owns one 64 x 64 block (bi <= bj) of gram; its four waves own a 32 x 32 quadrant each,
// i.e. 2 x 2 MFMA tiles, so every 16 x 16 tile has exactly one owner.  The rows of x are walked in chunks of 32: the workgroup
// stages x[chunk][64 columns of bi] and x[chunk][64 columns of bj] in LDS once, converted to float64 (exact: the inputs are
// fp32 or 16-bit), rows past n and columns past D as zeros; the next chunk's global loads are in flight while the current one
// is multiplied.  With A[i][k] = x[k0 + k][r0 + i] and B[k][j] = x[k0 + k][c0 + j] the f64 MFMA's operand map (lane l holds
// A[l & 15][l >> 4] and B[l >> 4][l & 15]) makes both operands plain reads of a staged row; the result map is the f64 one,
// col = l & 15, row = (l >> 4) + 4 * reg (NOT the fp32 map).  The sum over i runs in index order inside one accumulator per
// element, there is no split over i and there are no atomics, so two calls on the same data give the same bits.  Tiles
// strictly below the diagonal (possible only in a diagonal workgroup) and tiles past D are neither read nor written.  The
// column sums are taken by the diagonal workgroups from the staged panel, one thread per column, in index order.
#include "f64_tile.h"

namespace {

constexpr int kFidThreads = 256;
constexpr int kFidBlock = 64;      // gram rows / columns per workgroup
constexpr int kFidRows = 32;       // rows of x per staged chunk
constexpr int kFidPitch = 80;      // doubles per staged row: rows k and k + 1 of a 32-lane ds_read_b64 fall on disjoint banks
constexpr int kFidItems = 2 * kFidRows * (kFidBlock / 4) / kFidThreads;     // 4-element staging items per thread and chunk

__device__ __forceinline__ void fid_widen(const f32x4& v, double (&d)[4]) {
#pragma unroll
  for (int e = 0; e < 4; e++) d[e] = (double)v[e];
}
__device__ __forceinline__ void fid_widen(const bf16x4& v, double (&d)[4]) {
#pragma unroll
  for (int e = 0; e < 4; e++) d[e] = (double)bf2f(v[e]);
}

template <typename T, typename T4>
__global__ __launch_bounds__(kFidThreads) void moments_update_kernel(const T* __restrict__ x, int n, int D, double* __restrict__ sum,
                                                                     double* __restrict__ gram) {
  __shared__ __attribute__((aligned(16))) double xs[2][kFidRows][kFidPitch];
  const int nb = (D + kFidBlock - 1) / kFidBlock;
  int bi = 0, rem = blockIdx.x;                       // blockIdx.x enumerates the pairs bi <= bj row by row
  while (rem >= nb - bi) { rem -= nb - bi; bi++; }
  const int bj = bi + rem;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = w >> 1, wc = w & 1;
  const int nt = D >> 4;
  const int tr0 = bi * 4 + wr * 2, tc0 = bj * 4 + wc * 2;      // the wave's first tile row / tile column

  // staging item q of this thread: side (0: the columns of bi, 1: of bj), row r of the chunk, 4 columns from c4
  T4 raw[kFidItems];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int q = 0; q < kFidItems; q++) {
      const int it = tid + q * kFidThreads;
      const int side = it >> 9, r = (it >> 4) & (kFidRows - 1), c4 = (it & 15) * 4;
      const int row = k0 + r, col = (side ? bj : bi) * kFidBlock + c4;
      T4 v = {};
      if (row < n && col < D) v = *reinterpret_cast<const T4*>(x + (size_t)row * D + col);      // D % 16 == 0: col < D covers col + 3
      raw[q] = v;
    }
  };

  f64x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
  double colsum = 0.0;
  const bool sums = bi == bj && tid < kFidBlock;

  fetch(0);
  for (int k0 = 0; k0 < n; k0 += kFidRows) {
#pragma unroll
    for (int q = 0; q < kFidItems; q++) {
      const int it = tid + q * kFidThreads;
      const int side = it >> 9, r = (it >> 4) & (kFidRows - 1), c4 = (it & 15) * 4;
      double d[4];
      fid_widen(raw[q], d);
      f64x2* dst = reinterpret_cast<f64x2*>(&xs[side][r][c4]);
      dst[0] = f64x2{d[0], d[1]};
      dst[1] = f64x2{d[2], d[3]};
    }
    __syncthreads();
    if (k0 + kFidRows < n) fetch(k0 + kFidRows);
#pragma unroll
    for (int kk = 0; kk < kFidRows / 4; kk++) {
      const int k = kk * 4 + (lane >> 4);
      double a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; i++) {
        a[i] = xs[0][k][wr * 32 + i * 16 + (lane & 15)];
        b[i] = xs[1][k][wc * 32 + i * 16 + (lane & 15)];
      }
#pragma unroll
      for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    if (sums) {
      for (int r = 0; r < kFidRows; r++) colsum += xs[0][r][tid];      // rows past n are staged as zeros
    }
    __syncthreads();
  }

#pragma unroll
  for (int i = 0; i < 2; i++) {
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const int tr = tr0 + i, tc = tc0 + j;
      if (tr <= tc && tc < nt) {          // wave-uniform; tr <= tc < nt keeps every access inside gram
#pragma unroll
        for (int r = 0; r < 4; r++) {
          double* g = gram + (size_t)(tr * 16 + (lane >> 4) + 4 * r) * D + tc * 16 + (lane & 15);
          *g += acc[i][j][r];
        }
      }
    }
  }
  if (sums && bi * kFidBlock + tid < D) sum[bi * kFidBlock + tid] += colsum;
}

// one thread per (image, 8 channels): the HW addends in index order, fp32
__global__ __launch_bounds__(256) void mean_hw_f32_kernel(const bf16* __restrict__ x, float* __restrict__ y, long total8, int HW, int C) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= total8) return;
  const int cg = C >> 3;
  const long n = i / cg;
  const int c = (int)(i - n * cg) * 8;
  const bf16* src = x + (size_t)n * HW * C + c;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int p = 0; p < HW; p++) {
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(src + (size_t)p * C);
#pragma unroll
    for (int e = 0; e < 8; e++) acc[e] += bf2f(v[e]);
  }
  float* dst = y + (size_t)n * C + c;
#pragma unroll
  for (int e = 0; e < 8; e++) dst[e] = acc[e] / (float)HW;
}

}  // namespace

extern "C" int gank_mean_hw_f32(const void* x, float* y, int n, int HW, int C, void* stream) {
  GANK_REQUIRE(x && y, "mean_hw_f32: null pointer");
  GANK_REQUIRE(n >= 1 && HW >= 1, "mean_hw_f32: empty input (n=%d HW=%d)", n, HW);
  GANK_REQUIRE(C >= 8 && C % 8 == 0, "mean_hw_f32: C=%d unsupported (need C %% 8 == 0)", C);
  GANK_REQUIRE(((uintptr_t)x & 15) == 0, "mean_hw_f32: x must be 16-byte aligned");
  const long total8 = (long)n * (C / 8);
  GANK_REQUIRE(total8 < (1L << 31), "mean_hw_f32: %ld outputs", total8 * 8);
  hipLaunchKernelGGL(mean_hw_f32_kernel, dim3((unsigned)cdiv(total8, 256)), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, y, total8, HW, C);
  GANK_LAUNCH_OK("mean_hw_f32");
  return 0;
}

extern "C" int gank_moments_update(const void* x, int dtype, int n, int D, double* sum, double* gram, void* stream) {
  GANK_REQUIRE(x && sum && gram, "moments_update: null pointer");
  GANK_REQUIRE(dtype == 0 || dtype == 1, "moments_update: unknown input dtype code %d (0 = the 16-bit activation type, 1 = float32)", dtype);
  GANK_REQUIRE(n >= 1, "moments_update: n = %d, needs at least one row", n);
  GANK_REQUIRE(D >= 16 && D <= 4096 && D % 16 == 0, "moments_update: D = %d unsupported (a multiple of 16 in 16..4096)", D);
  GANK_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)sum & 7) == 0 && ((uintptr_t)gram & 7) == 0, "moments_update: misaligned pointer");
  const int nb = cdiv(D, kFidBlock);
  const dim3 grid((unsigned)(nb * (nb + 1) / 2)), block(kFidThreads);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == 0)
    hipLaunchKernelGGL((moments_update_kernel<bf16, bf16x4>), grid, block, 0, s, (const bf16*)x, n, D, sum, gram);
  else
    hipLaunchKernelGGL((moments_update_kernel<float, f32x4>), grid, block, 0, s, (const float*)x, n, D, sum, gram);
  GANK_LAUNCH_OK("moments_update");
  return 0;
}
