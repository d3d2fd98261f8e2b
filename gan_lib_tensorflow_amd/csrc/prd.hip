// The statistics stage of improved precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020) on
// the pool_3 features (common/precision_recall.py).  All four values are functions of the k-th-nearest-neighbour radius of
// every row inside its own set and of membership tests d2(a, b) <= radius2(b) across the sets:
//   gank_prd_knn_partial     per row of a bank and per column segment the k smallest d2 to the OTHER rows of the bank;
//   gank_prd_knn_finish      the segments of a row merged -> radii2 [n], the k-th smallest;
//   gank_prd_counts_partial  per query row and column segment the number of bank rows j with d2_ij <= radii2[j], and min_j d2_ij;
//   gank_prd_counts_finish   an int sum and a min over the segments;
//   gank_prd_scores_partial  per query row and column segment max_j radii2[j] / d2_ij and the smallest radii2[j] among the balls
//                            that hold the row (the realism and rarity scores of common/sample_scores.py), pruned balls left out;
//   gank_prd_scores_finish   a max and a min over the segments.
// d2_ij = (|a_i|^2 + |b_j|^2) - 2 <a_i, b_j> in float64 on float32 features (the widening is exact), clamped at 0.
//
// Decomposition.  A 256-thread workgroup owns a strip of 64 rows (blockIdx.x) and walks the 64-column tiles of one column
// segment (blockIdx.y): the T = ceil(n / 64) column tiles are cut into `segments` contiguous ranges, segment s = tiles
// [T s / segments, T (s + 1) / segments), so that a small n still fills the chip.  The full matrix is computed, also bank
// against itself.  Per tile the dot products are f64_tile_dots (f64_tile.h, shared with kid.hip: the contraction over the
// feature axis on v_mfma_f64_16x16x4_f64, the four waves a 32 x 32 quadrant each; the staging, the LDS pitch and the operand
// map are documented there).  The result map is the f64 one, col = l & 15, row = (l >> 4) + 4 * reg (NOT the fp32 map).  Rows and
// columns past the end re-read the last row and are masked below.
//
// Norms.  Through the staging hook of f64_tile_dots a staging thread squares the 4 features it has just widened and adds them
// to a float64 partial of its row (the products of float32 values are exact); 8 consecutive lanes stage one row, an xor
// butterfly (1, 2, 4) adds their partials after the last chunk.  The order is fixed, so a row's norm is the same bits in whichever workgroup computes it.  The strip's own
// norms are formed during the segment's first tile only.
//
// Epilogue.  The staging buffer is free after the last chunk; the waves store their dot products there as a 64 x 64 tile, pitch
// 68 doubles.  Then the 256 threads act as 64 rows x 4 column classes: thread t owns row t >> 2 and the columns 4 j + (t & 3),
// j = 0..15.  An 8-byte LDS read is served in two groups of 32 lanes = 8 rows x 4 classes, and a double's bank pair is its index
// mod 32: (row * 68 + 4 j + class) mod 32 = (4 row + class + 4 j) mod 32 takes 32 distinct values over the group.  The store is
// served in groups of 16 consecutive lanes = 16 consecutive columns of one row: distinct.
//   radii:  d2 of a column >= n or of the row's own INDEX is +inf; the thread keeps the 8 smallest values it has seen sorted in
//           registers (min / max chain, entered only when the value beats the list's last).  After the last tile the four
//           classes of a row merge by xor shuffles (1, 2) and the first k values go to part[row][segment][0..k), ascending,
//           padded with +inf.  A duplicated row is a neighbour at distance 0: nothing is excluded by value.
//   counts: count += d2 <= radii2[column] (inclusive; the tile's 64 radii sit in LDS, -1 for columns >= n), nearest = min d2;
//           the four classes add / min by xor shuffles -> part_count[row][segment], part_min[row][segment].
//   scores: a column with radii2 < 0 (pruned by the caller, or >= n: the -1 of the counts) is skipped.  Otherwise ratio =
//           max(ratio, d2 == 0 ? +inf : radii2 / d2), one IEEE division (d2 == 0 also covers 0 / 0), from -inf; rare =
//           min(rare, radii2) where d2 <= radii2, from +inf; max / min over the classes by xor shuffles -> part[row][segment],
//           part2[row][segment].  The division runs after the accumulators have gone to LDS, on registers they have freed.
// The k smallest of a set, an integer sum and a max / min do not depend on the order or on the cut into segments; no atomics, no split of
// the contraction: two calls on the same data, with any segment counts, return the same bits.
#include "f64_tile.h"

namespace {

constexpr int kPrdThreads = kF64Threads;
constexpr int kPrdTile = kF64Tile;         // rows per strip / columns per tile
constexpr int kPrdD2Pitch = 68;    // doubles per row of the tile of dot products (header)
constexpr int kPrdMaxK = 8;
constexpr int kPrdMaxRows = 1 << 24;       // ceil(n / 64) fits gridDim.x with room, n * 64 an int
constexpr int kPrdMaxSegments = 65535;     // gridDim.y
static_assert(kPrdTile * kPrdD2Pitch <= kF64StageDoubles, "the tile of dot products lives in the staging buffer");

__host__ __device__ inline int prd_tiles(int n) { return (n + kPrdTile - 1) / kPrdTile; }
__host__ __device__ inline int prd_segment_begin(int T, int segments, int s) { return (int)((long long)T * s / segments); }

// v into the ascending list: the list keeps its 8 smallest
__device__ __forceinline__ void prd_insert(double (&best)[kPrdMaxK], double v) {
#pragma unroll
  for (int s = 0; s < kPrdMaxK; s++) {
    const double lo = fmin(best[s], v);
    v = fmax(best[s], v);
    best[s] = lo;
  }
}

enum PrdMode { kPrdRadii, kPrdCounts, kPrdScores };

// kPrdRadii: a == b (the bank against itself), `part` = the k-lists.  Otherwise a = queries, b = bank; kPrdCounts: `part` = the
// minima, `part_count` the counts; kPrdScores: `part` = the ratios, `part2` = the smallest holding radii.
template <PrdMode kMode>
__global__ __launch_bounds__(kPrdThreads) void prd_strip_kernel(const float* __restrict__ a, int na, const float* __restrict__ b, int nb, int D,
                                                                const double* __restrict__ radii2, int k, int segments,
                                                                double* __restrict__ part, int* __restrict__ part_count,
                                                                double* __restrict__ part2) {
  __shared__ __attribute__((aligned(16))) double buf[kF64StageDoubles];      // fs[side][row][k], then dots[row][col]
  __shared__ double norm[2][kPrdTile];
  __shared__ double rad[kPrdTile];
  const int T = prd_tiles(nb), bi = blockIdx.x, seg = blockIdx.y;
  const int t0 = prd_segment_begin(T, segments, seg), t1 = prd_segment_begin(T, segments, seg + 1);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = w >> 1, wc = w & 1;
  const int c4 = (tid & 7) * 4;                       // staging item q: row (tid >> 3) + 32 q of the 128 staged rows, 4 features from c4
  const int srow = tid >> 2, cls = tid & 3;           // the epilogue's row and column class
  const int grow = bi * kPrdTile + srow;
  constexpr bool kRadii = kMode == kPrdRadii;

  double best[kPrdMaxK];
#pragma unroll
  for (int s = 0; s < kPrdMaxK; s++) best[s] = INFINITY;
  int count = 0;
  double nearest = INFINITY;
  double ratio = -INFINITY, rare = INFINITY;

  for (int bj = t0; bj < t1; bj++) {
    const float* src[kF64Items];
#pragma unroll
    for (int q = 0; q < kF64Items; q++) {
      const int r = (tid >> 3) + 32 * q, side = r >> 6;
      int pos = (side ? bj : bi) * kPrdTile + (r & (kPrdTile - 1));
      const int last = (side ? nb : na) - 1;
      pos = pos < last ? pos : last;
      src[q] = (side ? b : a) + (size_t)pos * D + c4;
    }
    double sq[kF64Items];
#pragma unroll
    for (int q = 0; q < kF64Items; q++) sq[q] = 0.0;
    const bool first = bj == t0;                      // the strip's own norms are formed once
    f64x4 acc[2][2];
    f64_tile_dots(src, D, buf, acc, [&](int q, double d0, double d1, double d2, double d3) {
      const int r = (tid >> 3) + 32 * q;
      if (r >= kPrdTile || first) sq[q] = (((sq[q] + d0 * d0) + d1 * d1) + d2 * d2) + d3 * d3;
    });

    // the staging buffer is free: norms, the tile's radii and the dot products go to LDS
#pragma unroll
    for (int q = 0; q < kF64Items; q++) {
      const int r = (tid >> 3) + 32 * q;
      if (r >= kPrdTile || first) {                   // uniform over the wave: all 8 lanes of a row take part
        double v = sq[q];
        v += __shfl_xor(v, 1, 64);
        v += __shfl_xor(v, 2, 64);
        v += __shfl_xor(v, 4, 64);
        if ((tid & 7) == 0) norm[r >> 6][r & (kPrdTile - 1)] = v;
      }
    }
    if (!kRadii && tid < kPrdTile) {
      const int col = bj * kPrdTile + tid;
      rad[tid] = col < nb ? radii2[col] : -1.0;       // d2 >= 0 and +inf in a masked column: never inside
    }
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < 2; j++)
#pragma unroll
        for (int r = 0; r < 4; r++)
          buf[(wr * 32 + i * 16 + (lane >> 4) + 4 * r) * kPrdD2Pitch + wc * 32 + j * 16 + (lane & 15)] = acc[i][j][r];
    __syncthreads();

    const double na2 = norm[0][srow];
#pragma unroll 4
    for (int j = 0; j < kPrdTile / 4; j++) {
      const int c = 4 * j + cls, col = bj * kPrdTile + c;
      const double d2 = fmax((na2 + norm[1][c]) - 2.0 * buf[srow * kPrdD2Pitch + c], 0.0);
      if (kRadii) {
        const double v = (col < nb && col != grow) ? d2 : INFINITY;       // self-exclusion by index
        if (v < best[kPrdMaxK - 1]) prd_insert(best, v);
      } else if (kMode == kPrdCounts) {
        const double v = col < nb ? d2 : INFINITY;
        count += v <= rad[c] ? 1 : 0;
        nearest = fmin(nearest, v);
      } else {
        const double r2 = rad[c];
        if (r2 >= 0.0) {                                // not pruned, and col < nb
          ratio = fmax(ratio, d2 == 0.0 ? (double)INFINITY : r2 / d2);
          if (d2 <= r2) rare = fmin(rare, r2);
        }
      }
    }
    __syncthreads();                                  // the next tile stages over the dot products
  }

  // the four column classes of a row are four neighbouring lanes
  if (kRadii) {
#pragma unroll
    for (int o = 1; o <= 2; o <<= 1) {
      double other[kPrdMaxK];
#pragma unroll
      for (int s = 0; s < kPrdMaxK; s++) other[s] = __shfl_xor(best[s], o, 64);
#pragma unroll
      for (int s = 0; s < kPrdMaxK; s++) prd_insert(best, other[s]);
    }
    if (cls == 0 && grow < na) {
      double* dst = part + ((size_t)grow * segments + seg) * k;
#pragma unroll
      for (int s = 0; s < kPrdMaxK; s++)
        if (s < k) dst[s] = best[s];
    }
  } else if (kMode == kPrdCounts) {
#pragma unroll
    for (int o = 1; o <= 2; o <<= 1) {
      count += __shfl_xor(count, o, 64);
      nearest = fmin(nearest, __shfl_xor(nearest, o, 64));
    }
    if (cls == 0 && grow < na) {
      part_count[(size_t)grow * segments + seg] = count;
      part[(size_t)grow * segments + seg] = nearest;
    }
  } else {
#pragma unroll
    for (int o = 1; o <= 2; o <<= 1) {
      ratio = fmax(ratio, __shfl_xor(ratio, o, 64));
      rare = fmin(rare, __shfl_xor(rare, o, 64));
    }
    if (cls == 0 && grow < na) {
      part[(size_t)grow * segments + seg] = ratio;
      part2[(size_t)grow * segments + seg] = rare;
    }
  }
}

// one thread per row: the k-th smallest of its segments * k values
__global__ __launch_bounds__(kPrdThreads) void prd_knn_finish_kernel(const double* __restrict__ part, int n, int k, int segments,
                                                                     double* __restrict__ radii2) {
  const int i = blockIdx.x * kPrdThreads + threadIdx.x;
  if (i >= n) return;
  double best[kPrdMaxK];
#pragma unroll
  for (int s = 0; s < kPrdMaxK; s++) best[s] = INFINITY;
  const double* p = part + (size_t)i * segments * k;
  for (int e = 0; e < segments * k; e++) {
    const double v = p[e];
    if (v < best[kPrdMaxK - 1]) prd_insert(best, v);
  }
  double out = best[0];
#pragma unroll
  for (int s = 1; s < kPrdMaxK; s++)
    if (s == k - 1) out = best[s];
  radii2[i] = out;
}

__global__ __launch_bounds__(kPrdThreads) void prd_counts_finish_kernel(const int* __restrict__ part_count, const double* __restrict__ part_min,
                                                                        int nq, int segments, int* __restrict__ count,
                                                                        double* __restrict__ nearest2) {
  const int i = blockIdx.x * kPrdThreads + threadIdx.x;
  if (i >= nq) return;
  int c = 0;
  double m = INFINITY;
  for (int s = 0; s < segments; s++) {
    c += part_count[(size_t)i * segments + s];
    m = fmin(m, part_min[(size_t)i * segments + s]);
  }
  count[i] = c;
  nearest2[i] = m;
}

__global__ __launch_bounds__(kPrdThreads) void prd_scores_finish_kernel(const double* __restrict__ part_ratio2, const double* __restrict__ part_rare2,
                                                                        int nq, int segments, double* __restrict__ ratio2,
                                                                        double* __restrict__ rare2) {
  const int i = blockIdx.x * kPrdThreads + threadIdx.x;
  if (i >= nq) return;
  double hi = -INFINITY, lo = INFINITY;
  for (int s = 0; s < segments; s++) {
    hi = fmax(hi, part_ratio2[(size_t)i * segments + s]);
    lo = fmin(lo, part_rare2[(size_t)i * segments + s]);
  }
  ratio2[i] = hi;
  rare2[i] = lo;
}

int prd_check_shape(const char* what, int D, int segments, int columns) {
  GANK_REQUIRE(D >= 16 && D <= 4096 && D % 16 == 0, "%s: D = %d unsupported (a multiple of 16 in 16..4096)", what, D);
  GANK_REQUIRE(segments >= 1 && segments <= kPrdMaxSegments && segments <= prd_tiles(columns),
               "%s: segments = %d (1..%d, at most the %d column tiles of %d rows)", what, segments, kPrdMaxSegments, prd_tiles(columns), columns);
  return 0;
}

}  // namespace

extern "C" int gank_prd_knn_partial(const float* x, int n, int D, int k, int segments, double* part, void* stream) {
  GANK_REQUIRE(x && part, "prd_knn_partial: null pointer");
  GANK_REQUIRE(k >= 1 && k <= kPrdMaxK, "prd_knn_partial: k = %d unsupported (1..%d)", k, kPrdMaxK);
  GANK_REQUIRE(n >= k + 1, "prd_knn_partial: n = %d, the k = %d nearest other rows need at least %d rows", n, k, k + 1);
  GANK_REQUIRE(n <= kPrdMaxRows, "prd_knn_partial: n = %d, at most %d rows", n, kPrdMaxRows);
  if (prd_check_shape("prd_knn_partial", D, segments, n)) return 1;
  GANK_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)part & 7) == 0, "prd_knn_partial: misaligned pointer");
  const dim3 grid((unsigned)prd_tiles(n), (unsigned)segments);
  hipLaunchKernelGGL(prd_strip_kernel<kPrdRadii>, grid, dim3(kPrdThreads), 0, (hipStream_t)stream, x, n, x, n, D, (const double*)nullptr, k, segments,
                     part, (int*)nullptr, (double*)nullptr);
  GANK_LAUNCH_OK("prd_knn_partial");
  return 0;
}

extern "C" int gank_prd_knn_finish(const double* part, int n, int k, int segments, double* radii2, void* stream) {
  GANK_REQUIRE(part && radii2, "prd_knn_finish: null pointer");
  GANK_REQUIRE(k >= 1 && k <= kPrdMaxK, "prd_knn_finish: k = %d unsupported (1..%d)", k, kPrdMaxK);
  GANK_REQUIRE(n >= k + 1 && n <= kPrdMaxRows, "prd_knn_finish: n = %d (%d..%d)", n, k + 1, kPrdMaxRows);
  GANK_REQUIRE(segments >= 1 && segments <= kPrdMaxSegments, "prd_knn_finish: segments = %d (1..%d)", segments, kPrdMaxSegments);
  GANK_REQUIRE(((uintptr_t)part & 7) == 0 && ((uintptr_t)radii2 & 7) == 0, "prd_knn_finish: misaligned pointer");
  hipLaunchKernelGGL(prd_knn_finish_kernel, dim3((unsigned)cdiv(n, kPrdThreads)), dim3(kPrdThreads), 0, (hipStream_t)stream, part, n, k, segments,
                     radii2);
  GANK_LAUNCH_OK("prd_knn_finish");
  return 0;
}

extern "C" int gank_prd_counts_partial(const float* q, int nq, const float* r, int nr, int D, const double* radii2, int segments, int* part_count,
                                       double* part_min, void* stream) {
  GANK_REQUIRE(q && r && radii2 && part_count && part_min, "prd_counts_partial: null pointer");
  GANK_REQUIRE(nq >= 1 && nq <= kPrdMaxRows && nr >= 1 && nr <= kPrdMaxRows, "prd_counts_partial: nq = %d, nr = %d (1..%d)", nq, nr, kPrdMaxRows);
  if (prd_check_shape("prd_counts_partial", D, segments, nr)) return 1;
  GANK_REQUIRE(((uintptr_t)q & 15) == 0 && ((uintptr_t)r & 15) == 0 && ((uintptr_t)radii2 & 7) == 0 && ((uintptr_t)part_count & 3) == 0 &&
                   ((uintptr_t)part_min & 7) == 0,
               "prd_counts_partial: misaligned pointer");
  const dim3 grid((unsigned)prd_tiles(nq), (unsigned)segments);
  hipLaunchKernelGGL(prd_strip_kernel<kPrdCounts>, grid, dim3(kPrdThreads), 0, (hipStream_t)stream, q, nq, r, nr, D, radii2, 0, segments, part_min,
                     part_count, (double*)nullptr);
  GANK_LAUNCH_OK("prd_counts_partial");
  return 0;
}

extern "C" int gank_prd_counts_finish(const int* part_count, const double* part_min, int nq, int segments, int* count, double* nearest2,
                                      void* stream) {
  GANK_REQUIRE(part_count && part_min && count && nearest2, "prd_counts_finish: null pointer");
  GANK_REQUIRE(nq >= 1 && nq <= kPrdMaxRows, "prd_counts_finish: nq = %d (1..%d)", nq, kPrdMaxRows);
  GANK_REQUIRE(segments >= 1 && segments <= kPrdMaxSegments, "prd_counts_finish: segments = %d (1..%d)", segments, kPrdMaxSegments);
  GANK_REQUIRE(((uintptr_t)part_count & 3) == 0 && ((uintptr_t)part_min & 7) == 0 && ((uintptr_t)count & 3) == 0 && ((uintptr_t)nearest2 & 7) == 0,
               "prd_counts_finish: misaligned pointer");
  hipLaunchKernelGGL(prd_counts_finish_kernel, dim3((unsigned)cdiv(nq, kPrdThreads)), dim3(kPrdThreads), 0, (hipStream_t)stream, part_count,
                     part_min, nq, segments, count, nearest2);
  GANK_LAUNCH_OK("prd_counts_finish");
  return 0;
}

extern "C" int gank_prd_scores_partial(const float* q, int nq, const float* r, int nr, int D, const double* radii2, int segments,
                                       double* part_ratio2, double* part_rare2, void* stream) {
  GANK_REQUIRE(q && r && radii2 && part_ratio2 && part_rare2, "prd_scores_partial: null pointer");
  GANK_REQUIRE(nq >= 1 && nq <= kPrdMaxRows && nr >= 1 && nr <= kPrdMaxRows, "prd_scores_partial: nq = %d, nr = %d (1..%d)", nq, nr, kPrdMaxRows);
  if (prd_check_shape("prd_scores_partial", D, segments, nr)) return 1;
  GANK_REQUIRE(((uintptr_t)q & 15) == 0 && ((uintptr_t)r & 15) == 0 && ((uintptr_t)radii2 & 7) == 0 && ((uintptr_t)part_ratio2 & 7) == 0 &&
                   ((uintptr_t)part_rare2 & 7) == 0,
               "prd_scores_partial: misaligned pointer");
  const dim3 grid((unsigned)prd_tiles(nq), (unsigned)segments);
  hipLaunchKernelGGL(prd_strip_kernel<kPrdScores>, grid, dim3(kPrdThreads), 0, (hipStream_t)stream, q, nq, r, nr, D, radii2, 0, segments,
                     part_ratio2, (int*)nullptr, part_rare2);
  GANK_LAUNCH_OK("prd_scores_partial");
  return 0;
}

extern "C" int gank_prd_scores_finish(const double* part_ratio2, const double* part_rare2, int nq, int segments, double* ratio2, double* rare2,
                                      void* stream) {
  GANK_REQUIRE(part_ratio2 && part_rare2 && ratio2 && rare2, "prd_scores_finish: null pointer");
  GANK_REQUIRE(nq >= 1 && nq <= kPrdMaxRows, "prd_scores_finish: nq = %d (1..%d)", nq, kPrdMaxRows);
  GANK_REQUIRE(segments >= 1 && segments <= kPrdMaxSegments, "prd_scores_finish: segments = %d (1..%d)", segments, kPrdMaxSegments);
  GANK_REQUIRE(((uintptr_t)part_ratio2 & 7) == 0 && ((uintptr_t)part_rare2 & 7) == 0 && ((uintptr_t)ratio2 & 7) == 0 && ((uintptr_t)rare2 & 7) == 0,
               "prd_scores_finish: misaligned pointer");
  hipLaunchKernelGGL(prd_scores_finish_kernel, dim3((unsigned)cdiv(nq, kPrdThreads)), dim3(kPrdThreads), 0, (hipStream_t)stream, part_ratio2,
                     part_rare2, nq, segments, ratio2, rare2);
  GANK_LAUNCH_OK("prd_scores_finish");
  return 0;
}
