// The statistics stage of the Kernel Inception Distance (common/kid.py; Binkowski et al., "Demystifying MMD GANs": the unbiased
// MMD^2 of the pool_3 features under the polynomial kernel k(a, b) = (gamma <a, b> + coef0)^degree):
//   gank_kid_block_sums  for every subset s and each of the blocks XX, YY, XY the sums of k over 64 x 64 tiles of the m x m
//                        kernel matrix of the subset's rows, one partial per tile, on v_mfma_f64_16x16x4_f64;
//   gank_kid_finish      the tile partials of a (subset, block) added in index order -> out [subsets, 3].
//
// block_sums.  A 256-thread workgroup owns one 64 x 64 tile (bi, bj) of one block of one subset; its four waves own a 32 x 32
// quadrant each, 2 x 2 MFMA tiles.  XX and YY are symmetric, so only their tiles with bi <= bj exist: an off-diagonal tile's sum
// is doubled (by thread 0, here and nowhere else; exact), a diagonal tile is computed whole with its elements i == j left out
// -- together the sum over all i != j, the unbiased estimator's.  XY has all T x T tiles and no element is left out.
// blockIdx.x enumerates, per subset, the tri = T (T + 1) / 2 tiles of XX row by row, then those of YY, then the T * T of XY
// (T = ceil(m / 64)); partial[s][blockIdx.x] is that tile's sum, so a subset's row of `partial` is 2 tri + T * T long and its
// three blocks start at 0, tri and 2 tri.
//
// Dot products.  The contraction runs over the FEATURE axis: A[i][k] = x[ix[s][r0 + i]][k0 + k], B[k][j] = y[iy[s][c0 + j]][k0 + k].
// The workgroup gathers its 64 + 64 rows through the tables (each thread resolves its four row pointers once; positions past
// m re-read position m - 1 and are masked in the epilogue) and hands them to f64_tile_dots (f64_tile.h: the staging in chunks
// of 32 features widened to float64, the f64 MFMA's operand map and the conflict-free LDS pitch are documented there).
//
// Epilogue, float64: t = gamma * dot + coef0, t^degree by repeated multiplication, the masks (row or column >= m; i == j in a
// diagonal tile of XX / YY), then a sum in a fixed order: the lane's 16 elements in register order, then block_sum
// (f64_tile.h: an xor butterfly over the 64 lanes, the four waves through LDS, added in index order); one plain store by
// thread 0.  No atomics, no split of the contraction: two calls on the same data return the same bits.
#include "f64_tile.h"

namespace {

constexpr int kKidThreads = kF64Threads;
constexpr int kKidTile = kF64Tile;         // rows / columns of the kernel matrix per workgroup
constexpr int kKidMaxM = 65536;    // T <= 1024: 2 tri + T * T fits gridDim.x and an int
constexpr int kKidMaxSubsets = 65535;      // gridDim.y

__host__ __device__ inline int kid_tiles(int m) { return (m + kKidTile - 1) / kKidTile; }

__global__ __launch_bounds__(kKidThreads) void kid_block_sums_kernel(const float* __restrict__ x, const float* __restrict__ y, int D,
                                                                     const int* __restrict__ ix, const int* __restrict__ iy, int m,
                                                                     double gamma, double coef0, int degree,
                                                                     double* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) double fs[kF64StageDoubles];
  __shared__ double red[4];
  const int T = kid_tiles(m), tri = T * (T + 1) / 2;
  int t = blockIdx.x, block = 0;                      // block 0: XX, 1: YY, 2: XY
  if (t >= 2 * tri) { block = 2; t -= 2 * tri; }
  else if (t >= tri) { block = 1; t -= tri; }
  int bi, bj;
  if (block < 2) {                                    // the pairs bi <= bj row by row
    bi = 0;
    while (t >= T - bi) { t -= T - bi; bi++; }
    bj = bi + t;
  } else {
    bi = t / T;
    bj = t - bi * T;
  }
  const int s = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = w >> 1, wc = w & 1;

  // staging item q of this thread (f64_tile.h): row (tid >> 3) + 32 q of the 128 staged rows (side 0: the tile's rows, side 1:
  // its columns), 4 features from c4 of the chunk
  const int c4 = (tid & 7) * 4;
  const float* src[kF64Items];
#pragma unroll
  for (int q = 0; q < kF64Items; q++) {
    const int r = (tid >> 3) + 32 * q, side = r >> 6;
    int pos = (side ? bj : bi) * kKidTile + (r & (kKidTile - 1));
    pos = pos < m ? pos : m - 1;
    const bool from_y = side ? block != 0 : block == 1;
    const int row = (from_y ? iy : ix)[(size_t)s * m + pos];
    src[q] = (from_y ? y : x) + (size_t)row * D + c4;
  }
  f64x4 acc[2][2];
  f64_tile_dots(src, D, fs, acc, F64NoStagingHook());

  const bool diagonal = block < 2 && bi == bj;
  double sum = 0.0;
#pragma unroll
  for (int i = 0; i < 2; i++) {
#pragma unroll
    for (int j = 0; j < 2; j++) {
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int gi = bi * kKidTile + wr * 32 + i * 16 + (lane >> 4) + 4 * r;
        const int gj = bj * kKidTile + wc * 32 + j * 16 + (lane & 15);
        const double tv = gamma * acc[i][j][r] + coef0;
        double p = tv;
        if (degree >= 2) p *= tv;
        if (degree >= 3) p *= tv;
        sum += (gi < m && gj < m && !(diagonal && gi == gj)) ? p : 0.0;
      }
    }
  }
  double total = block_sum(sum, red);
  if (tid == 0) {
    if (block < 2 && bi < bj) total *= 2.0;           // the mirror tile (bj, bi) has no workgroup
    partial[(size_t)s * gridDim.x + blockIdx.x] = total;
  }
}

// blockIdx.x = block, blockIdx.y = subset; one wave: lane l adds tiles l, l + 64, .. in index order, then the xor butterfly
__global__ __launch_bounds__(64) void kid_finish_kernel(const double* __restrict__ partial, int m, double* __restrict__ out) {
  const int T = kid_tiles(m), tri = T * (T + 1) / 2;
  const int block = blockIdx.x, s = blockIdx.y, lane = threadIdx.x;
  const int count = block < 2 ? tri : T * T;
  const double* p = partial + (size_t)s * (2 * tri + T * T) + block * tri;
  double v = 0.0;
  for (int t = lane; t < count; t += 64) v += p[t];
  v = wave_sum(v);
  if (lane == 0) out[(size_t)s * 3 + block] = v;
}

}  // namespace

extern "C" int gank_kid_block_sums(const float* x, int nx, const float* y, int ny, int D, const int* ix, const int* iy, int subsets, int m,
                                   double gamma, double coef0, int degree, double* partial, void* stream) {
  GANK_REQUIRE(x && y && ix && iy && partial, "kid_block_sums: null pointer");
  GANK_REQUIRE(D >= 16 && D <= 4096 && D % 16 == 0, "kid_block_sums: D = %d unsupported (a multiple of 16 in 16..4096)", D);
  GANK_REQUIRE(m >= 2, "kid_block_sums: m = %d, the unbiased estimator needs at least 2 rows per side", m);
  GANK_REQUIRE(m <= nx && m <= ny, "kid_block_sums: m = %d exceeds the feature banks (nx = %d, ny = %d)", m, nx, ny);
  GANK_REQUIRE(m <= kKidMaxM, "kid_block_sums: m = %d, at most %d rows per subset", m, kKidMaxM);
  GANK_REQUIRE(subsets >= 1 && subsets <= kKidMaxSubsets, "kid_block_sums: subsets = %d (1..%d)", subsets, kKidMaxSubsets);
  GANK_REQUIRE(degree >= 1 && degree <= 3, "kid_block_sums: degree = %d unsupported (1..3)", degree);
  GANK_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0 && ((uintptr_t)ix & 3) == 0 && ((uintptr_t)iy & 3) == 0 &&
                   ((uintptr_t)partial & 7) == 0,
               "kid_block_sums: misaligned pointer");
  const int T = kid_tiles(m);
  const dim3 grid((unsigned)(T * (T + 1) + T * T), (unsigned)subsets);
  hipLaunchKernelGGL(kid_block_sums_kernel, grid, dim3(kKidThreads), 0, (hipStream_t)stream, x, y, D, ix, iy, m, gamma, coef0, degree, partial);
  GANK_LAUNCH_OK("kid_block_sums");
  return 0;
}

extern "C" int gank_kid_finish(const double* partial, int subsets, int m, double* out, void* stream) {
  GANK_REQUIRE(partial && out, "kid_finish: null pointer");
  GANK_REQUIRE(m >= 2 && m <= kKidMaxM, "kid_finish: m = %d (2..%d)", m, kKidMaxM);
  GANK_REQUIRE(subsets >= 1 && subsets <= kKidMaxSubsets, "kid_finish: subsets = %d (1..%d)", subsets, kKidMaxSubsets);
  GANK_REQUIRE(((uintptr_t)partial & 7) == 0 && ((uintptr_t)out & 7) == 0, "kid_finish: misaligned pointer");
  hipLaunchKernelGGL(kid_finish_kernel, dim3(3, (unsigned)subsets), dim3(64), 0, (hipStream_t)stream, partial, m, out);
  GANK_LAUNCH_OK("kid_finish");
  return 0;
}
