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
// Staging.  The contraction runs over the FEATURE axis: A[i][k] = x[ix[s][r0 + i]][k0 + k], B[k][j] = y[iy[s][c0 + j]][k0 + k].
// The workgroup gathers its 64 + 64 rows through the tables (each thread resolves its four row pointers once; positions past
// m re-read position m - 1 and are masked in the epilogue) and stages them in chunks of 32 features as fs[side][row][k],
// widened to float64 (exact), features past D as zeros; the next chunk's global loads are in flight while the current one is
// multiplied.  The f64 MFMA's operand map is: lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15], four contraction steps per
// instruction, one per value of l >> 4.  Which feature a step stands for is free as long as A and B agree, so a lane reads
// the PAIR of features fs[side][q0 + (l & 15)][8 kg + 2 (l >> 4) + {0, 1}] with one 16-byte LDS read and feeds element 0 to one
// MFMA (features 8 kg + {0, 2, 4, 6}) and element 1 to the next (8 kg + {1, 3, 5, 7}): half the LDS instructions of one read
// per MFMA operand.  The result map is the f64 one, col = l & 15, row = (l >> 4) + 4 * reg (NOT the fp32 map).
//
// The LDS pitch.  A ds_read_b128 is served in four groups of 16 lanes -- {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the
// same + 32 -- and a lane takes the 4 banks (2 e) mod 64 .. + 3 of its first double's index e, so a group is conflict-free
// when its 16 values of (e / 2) mod 16 differ.  Here e / 2 = (l & 15) * pitch / 2 + (l >> 4) + const.  With pitch = 36,
// pitch / 2 = 18 = 2 (mod 16): the first group holds rows {0-3, 12-15} of one l >> 4, residues 2 i = the 8 even ones, and rows
// 4-11 of the next l >> 4, residues 2 i + 1 = the 8 odd ones; the second group the same with the roles swapped: 16 distinct
// residues each.  (The 80 of fid.hip serves 8-byte reads ALONG a staged row, the row fixed per half-wave; here the row varies
// with the lane and 80 / 2 = 8 (mod 16) would put rows i and i + 2 on one bank.)  36 * 8 bytes is a multiple of 16, so the
// 16-byte reads and staging stores are aligned.
//
// Epilogue, float64: t = gamma * dot + coef0, t^degree by repeated multiplication, the masks (row or column >= m; i == j in a
// diagonal tile of XX / YY), then a sum in a fixed order: the lane's 16 elements in register order, an xor butterfly over the
// 64 lanes (32, 16, .., 1), the four waves through LDS and thread 0 adding them in index order; one plain store.  No atomics,
// no split of the contraction: two calls on the same data return the same bits.
#include "gank_common.h"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

constexpr int kKidThreads = 256;
constexpr int kKidTile = 64;       // rows / columns of the kernel matrix per workgroup
constexpr int kKidChunk = 32;      // features per staged chunk
constexpr int kKidPitch = 36;     // doubles per staged row (header: why it is conflict-free)
constexpr int kKidItems = 2 * kKidTile * (kKidChunk / 4) / kKidThreads;     // 4-feature staging items per thread and chunk
constexpr int kKidMaxM = 65536;    // T <= 1024: 2 tri + T * T fits gridDim.x and an int
constexpr int kKidMaxSubsets = 65535;      // gridDim.y

__host__ __device__ inline int kid_tiles(int m) { return (m + kKidTile - 1) / kKidTile; }

__device__ __forceinline__ double kid_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(kKidThreads) void kid_block_sums_kernel(const float* __restrict__ x, const float* __restrict__ y, int D,
                                                                     const int* __restrict__ ix, const int* __restrict__ iy, int m,
                                                                     double gamma, double coef0, int degree,
                                                                     double* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) double fs[2][kKidTile][kKidPitch];
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

  // staging item q of this thread: row (tid >> 3) + 32 q of the 128 staged rows (side 0: the tile's rows, side 1: its columns),
  // 4 features from c4 of the chunk
  const int c4 = (tid & 7) * 4;
  const float* src[kKidItems];
#pragma unroll
  for (int q = 0; q < kKidItems; q++) {
    const int r = (tid >> 3) + 32 * q, side = r >> 6;
    int pos = (side ? bj : bi) * kKidTile + (r & (kKidTile - 1));
    pos = pos < m ? pos : m - 1;
    const bool from_y = side ? block != 0 : block == 1;
    const int row = (from_y ? iy : ix)[(size_t)s * m + pos];
    src[q] = (from_y ? y : x) + (size_t)row * D + c4;
  }
  f32x4 raw[kKidItems];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int q = 0; q < kKidItems; q++) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (k0 + c4 < D) v = *reinterpret_cast<const f32x4*>(src[q] + k0);      // D % 16 == 0: k0 + c4 < D covers k0 + c4 + 3
      raw[q] = v;
    }
  };

  f64x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};

  fetch(0);
  for (int k0 = 0; k0 < D; k0 += kKidChunk) {
#pragma unroll
    for (int q = 0; q < kKidItems; q++) {
      const int r = (tid >> 3) + 32 * q;
      f64x2* dst = reinterpret_cast<f64x2*>(&fs[r >> 6][r & (kKidTile - 1)][c4]);
      dst[0] = f64x2{(double)raw[q][0], (double)raw[q][1]};
      dst[1] = f64x2{(double)raw[q][2], (double)raw[q][3]};
    }
    __syncthreads();
    if (k0 + kKidChunk < D) fetch(k0 + kKidChunk);
#pragma unroll
    for (int kg = 0; kg < kKidChunk / 8; kg++) {
      const int k = kg * 8 + 2 * (lane >> 4);         // this lane's feature pair of the group of 8
      f64x2 a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; i++) {
        a[i] = *reinterpret_cast<const f64x2*>(&fs[0][wr * 32 + i * 16 + (lane & 15)][k]);
        b[i] = *reinterpret_cast<const f64x2*>(&fs[1][wc * 32 + i * 16 + (lane & 15)][k]);
      }
#pragma unroll
      for (int e = 0; e < 2; e++)
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
          for (int j = 0; j < 2; j++) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i][e], b[j][e], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }

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
  sum = kid_wave_sum(sum);
  if (lane == 0) red[w] = sum;
  __syncthreads();
  if (tid == 0) {
    double total = ((red[0] + red[1]) + red[2]) + red[3];
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
  v = kid_wave_sum(v);
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
