// NDB / JSD (Richardson & Weiss, "On GANs and GMMs", NeurIPS 2018, section 2; common/ndb.py): k-means of the training images in
// pixel space, Lloyd's iteration on the device.
//   gank_ndb_pixel_features  uint8 images [n, P] -> float32 features [n, Dp]: the chosen pixels, zero columns up to Dp % 16 == 0;
//   gank_ndb_assign          per row the nearest centroid (ties to the lowest index) and its d2, per strip of 64 rows the sum
//                            of the d2 and the number of rows whose label changed;
//   gank_ndb_group_rows      the stable counting sort of the row indices by label: count, offset, perm;
//   gank_ndb_centroids       per cluster and feature the float64 sum of its rows in perm order, / count, rounded to float32.
//
// assign.  d2_ik = (|x_i|^2 + |c_k|^2) - 2 <x_i, c_k> in float64 on float32 features, clamped at 0, formed exactly as prd.hip
// forms it: a 256-thread workgroup owns a strip of 64 rows (blockIdx.x) and walks the ceil(K / 64) centroid tiles through
// f64_tile_dots (f64_tile.h); the norms come through the staging hook (8 lanes a row, an xor butterfly 1, 2, 4; the strip's own
// norms during the first tile only); rows >= n and columns >= K re-read the last row and are masked below.  There are no column
// segments: at the sizes this metric runs (N >= 10 000 training rows) there are >= 157 strips, more than half the chip's compute
// units before a second centroid tile is even needed, and a segment count would only add a merge pass.
// Epilogue, as in prd.hip: the staging buffer is free after the last chunk, the waves store their dot products there as a 64 x 64
// tile of pitch 68 doubles, and the 256 threads act as 64 rows x 4 column classes, thread t row t >> 2 and the columns
// 4 j + (t & 3).  The 8-byte reads are served in two groups of 32 lanes = 8 rows x 4 classes on bank pairs
// (4 row + class + 4 j) mod 32: 32 distinct values; the stores in groups of 16 consecutive columns of one row: distinct.
// A thread keeps (min d2, argmin); the merge with every further column, across the four classes (xor shuffles 1, 2) and so
// across tiles is the LEXICOGRAPHIC minimum of (d2, index): associative and commutative, so the order of merging cannot matter
// and a tie goes to the lowest centroid index (numpy.argmin's rule).  d2 of a valid column is finite (fmax(NaN, 0) = 0), a
// masked column never enters, so a label is always in [0, K).
// part_inertia[strip] = block_sum (f64_tile.h) of the strip's d2, one value per row in the row's class-0 lane, 0 elsewhere and
// for rows >= n; part_changed[strip] = the number of rows < n with label != prev (0 when prev is null).
//
// group_rows.  A unit is 2048 consecutive rows, owned by one wave (a 64-thread workgroup).  (1) the unit's histogram in LDS ->
// ws[label][unit]; (2) per label an exclusive scan of ws[label][.] over the units in place, count[label] = its total; then an
// exclusive scan of count -> offset; (3) the unit walks its rows again, 64 at a time in row order: a row's slot is
// offset[label] + ws[label][unit] + the rows of that label met earlier in the unit.  Inside a group of 64 the lanes of one label
// find each other by ten ballots on the label's bits; a lane's rank is the number of lower lanes of its label, and the lowest
// lane of a label adds the group's count to the unit's running number.  Integer sums only, every slot has one owner:
// perm == argsort(label, stable), no atomics.  A label is clamped into [0, K) for memory safety only.
//
// centroids.  The grid is (cluster, group of 256 features); a workgroup is one wave, a lane owns 4 consecutive features and
// reads a row's 16 bytes of them: one float64 accumulator per (cluster, feature), the rows added in perm order (8 row loads in
// flight, added in order), then / count and one rounding to float32.  No split of a cluster's rows: the result does not depend
// on the grid.  count == 0: nothing is written, the centroid keeps its bytes.  perm, count and offset are device memory the host
// cannot see: they are clamped into the arrays for memory safety only.
#include <climits>

#include "f64_tile.h"

namespace {

constexpr int kNdbThreads = kF64Threads;
constexpr int kNdbTile = kF64Tile;
constexpr int kNdbD2Pitch = 68;            // doubles per row of the tile of dot products (header)
constexpr int kNdbMaxRows = 1 << 24;
constexpr int kNdbMaxK = 1024;
constexpr int kNdbMaxPixels = 1 << 30;
constexpr int kNdbUnit = 2048;             // rows per unit of group_rows
constexpr int kNdbWave = 64;
constexpr int kNdbCentFeatures = 4 * kNdbWave;     // features per workgroup of centroids
constexpr int kNdbCentDepth = 8;           // row loads in flight per lane
static_assert(kNdbTile * kNdbD2Pitch <= kF64StageDoubles, "the tile of dot products lives in the staging buffer");

__host__ __device__ inline int ndb_tiles(int n) { return (n + kNdbTile - 1) / kNdbTile; }
__host__ __device__ inline int ndb_units(int n) { return (n + kNdbUnit - 1) / kNdbUnit; }

// (best, besti) = the lexicographic minimum of itself and (v, i)
__device__ __forceinline__ void ndb_take(double& best, int& besti, double v, int i) {
  if (v < best || (v == best && i < besti)) {
    best = v;
    besti = i;
  }
}

__global__ __launch_bounds__(kNdbThreads) void ndb_pixel_features_kernel(const unsigned char* __restrict__ img, int P,
                                                                         const int* __restrict__ dims, int Dsel, int Dp,
                                                                         float* __restrict__ out) {
  const unsigned char* row = img + (size_t)blockIdx.x * P;
  float* dst = out + (size_t)blockIdx.x * Dp;
  for (int j = threadIdx.x; j < Dp; j += kNdbThreads) {
    float v = 0.f;
    if (j < Dsel) {
      int p = dims ? dims[j] : j;
      p = p < 0 ? 0 : (p < P ? p : P - 1);             // memory safety only: the wrapper checks the table before upload
      v = (float)row[p];
    }
    dst[j] = v;
  }
}

__global__ __launch_bounds__(kNdbThreads) void ndb_assign_kernel(const float* __restrict__ x, int n, const float* __restrict__ c, int K, int D,
                                                                 const int* __restrict__ prev, int* __restrict__ label,
                                                                 double* __restrict__ d2out, double* __restrict__ part_inertia,
                                                                 int* __restrict__ part_changed) {
  __shared__ __attribute__((aligned(16))) double buf[kF64StageDoubles];      // fs[side][row][k], then dots[row][col]
  __shared__ double norm[2][kNdbTile];
  __shared__ double red[4];
  __shared__ int redi[4];
  const int T = ndb_tiles(K), bi = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = w >> 1, wc = w & 1;
  const int c4 = (tid & 7) * 4;                       // staging item q: row (tid >> 3) + 32 q of the 128 staged rows, 4 features from c4
  const int srow = tid >> 2, cls = tid & 3;           // the epilogue's row and column class
  const int grow = bi * kNdbTile + srow;

  double best = INFINITY;
  int besti = INT_MAX;

  for (int bj = 0; bj < T; bj++) {
    const float* src[kF64Items];
#pragma unroll
    for (int q = 0; q < kF64Items; q++) {
      const int r = (tid >> 3) + 32 * q, side = r >> 6;
      int pos = (side ? bj : bi) * kNdbTile + (r & (kNdbTile - 1));
      const int last = (side ? K : n) - 1;
      pos = pos < last ? pos : last;
      src[q] = (side ? c : x) + (size_t)pos * D + c4;
    }
    double sq[kF64Items];
#pragma unroll
    for (int q = 0; q < kF64Items; q++) sq[q] = 0.0;
    const bool first = bj == 0;                       // the strip's own norms are formed once
    f64x4 acc[2][2];
    f64_tile_dots(src, D, buf, acc, [&](int q, double d0, double d1, double d2, double d3) {
      const int r = (tid >> 3) + 32 * q;
      if (r >= kNdbTile || first) sq[q] = (((sq[q] + d0 * d0) + d1 * d1) + d2 * d2) + d3 * d3;
    });

    // the staging buffer is free: norms and the dot products go to LDS
#pragma unroll
    for (int q = 0; q < kF64Items; q++) {
      const int r = (tid >> 3) + 32 * q;
      if (r >= kNdbTile || first) {                   // uniform over the wave: all 8 lanes of a row take part
        double v = sq[q];
        v += __shfl_xor(v, 1, 64);
        v += __shfl_xor(v, 2, 64);
        v += __shfl_xor(v, 4, 64);
        if ((tid & 7) == 0) norm[r >> 6][r & (kNdbTile - 1)] = v;
      }
    }
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < 2; j++)
#pragma unroll
        for (int r = 0; r < 4; r++)
          buf[(wr * 32 + i * 16 + (lane >> 4) + 4 * r) * kNdbD2Pitch + wc * 32 + j * 16 + (lane & 15)] = acc[i][j][r];
    __syncthreads();

    const double nx2 = norm[0][srow];
#pragma unroll 4
    for (int j = 0; j < kNdbTile / 4; j++) {
      const int cc = 4 * j + cls, col = bj * kNdbTile + cc;
      const double d2 = fmax((nx2 + norm[1][cc]) - 2.0 * buf[srow * kNdbD2Pitch + cc], 0.0);
      if (col < K) ndb_take(best, besti, d2, col);
    }
    __syncthreads();                                  // the next tile stages over the dot products
  }

  // the four column classes of a row are four neighbouring lanes
#pragma unroll
  for (int o = 1; o <= 2; o <<= 1) {
    const double v = __shfl_xor(best, o, 64);
    const int i = __shfl_xor(besti, o, 64);
    ndb_take(best, besti, v, i);
  }
  const bool owner = cls == 0 && grow < n;
  if (owner) {
    label[grow] = besti;
    d2out[grow] = best;
  }
  const double inertia = block_sum(owner ? best : 0.0, red);
  const bool moved = owner && prev != nullptr && prev[grow] != besti;
  const int in_wave = __popcll(__ballot(moved));
  if (lane == 0) redi[w] = in_wave;
  __syncthreads();
  if (tid == 0) {
    part_inertia[bi] = inertia;
    part_changed[bi] = ((redi[0] + redi[1]) + redi[2]) + redi[3];
  }
}

// the lanes of the wave that hold the same label as this one, among the `valid` lanes (K <= 1024: ten bits)
__device__ __forceinline__ unsigned long long ndb_peers(int lab, bool valid) {
  unsigned long long peers = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 10; b++) {
    const bool bit = (lab >> b) & 1;
    const unsigned long long set = __ballot(bit);
    peers &= bit ? set : ~set;
  }
  return peers;
}

__device__ __forceinline__ int ndb_label(const int* __restrict__ label, int r, int K) {
  const int lab = label[r];
  return lab < 0 ? 0 : (lab < K ? lab : K - 1);
}

// kScatter = false: ws[label][unit] = the unit's number of rows of the label.  kScatter = true: ws holds the unit's first slot
// inside the label's range (the scan below), perm is written.
template <bool kScatter>
__global__ __launch_bounds__(kNdbWave) void ndb_group_unit_kernel(const int* __restrict__ label, int n, int K, int units, int* __restrict__ ws,
                                                                  const int* __restrict__ offset, int* __restrict__ perm) {
  __shared__ int run[kNdbMaxK];
  const int u = blockIdx.x, lane = threadIdx.x;
  for (int k = lane; k < K; k += kNdbWave) run[k] = kScatter ? offset[k] + ws[(size_t)k * units + u] : 0;
  __syncthreads();
  const int begin = u * kNdbUnit, end = min(n, begin + kNdbUnit);
  for (int r0 = begin; r0 < end; r0 += kNdbWave) {      // uniform over the wave
    const int r = r0 + lane;
    const bool valid = r < end;
    const int lab = valid ? ndb_label(label, r, K) : 0;
    const unsigned long long peers = ndb_peers(lab, valid);
    const int rank = __popcll(peers & ((1ull << lane) - 1ull));
    int base = 0;
    if (valid) base = run[lab];
    __syncthreads();                                    // every lane has read the running numbers
    if (valid) {
      if (kScatter) {
        const int slot = base + rank;
        if ((unsigned)slot < (unsigned)n) perm[slot] = r;       // always true for labels that did not change between the passes
      }
      if (rank == 0) run[lab] = base + __popcll(peers);         // one lane per label
    }
    __syncthreads();
  }
  if (!kScatter)
    for (int k = lane; k < K; k += kNdbWave) ws[(size_t)k * units + u] = run[k];
}

// exclusive scan of m ints by one 256-thread workgroup, in place; returns the total in every thread.  A thread owns a
// contiguous piece; the 256 piece sums are scanned in LDS (integers: any order gives the same result).
__device__ __forceinline__ int ndb_block_scan(int* v, int m, int* sums) {
  const int tid = threadIdx.x, per = (m + kNdbThreads - 1) / kNdbThreads;
  const int b = min(m, tid * per), e = min(m, b + per);
  int s = 0;
  for (int i = b; i < e; i++) s += v[i];
  sums[tid] = s;
  __syncthreads();
  for (int o = 1; o < kNdbThreads; o <<= 1) {
    const int add = tid >= o ? sums[tid - o] : 0;
    __syncthreads();
    sums[tid] += add;
    __syncthreads();
  }
  const int total = sums[kNdbThreads - 1];
  int at = sums[tid] - s;
  for (int i = b; i < e; i++) {
    const int c = v[i];
    v[i] = at;
    at += c;
  }
  __syncthreads();
  return total;
}

__global__ __launch_bounds__(kNdbThreads) void ndb_group_scan_units_kernel(int* __restrict__ ws, int units, int* __restrict__ count) {
  __shared__ int sums[kNdbThreads];
  const int total = ndb_block_scan(ws + (size_t)blockIdx.x * units, units, sums);
  if (threadIdx.x == 0) count[blockIdx.x] = total;
}

__global__ __launch_bounds__(kNdbThreads) void ndb_group_scan_labels_kernel(const int* __restrict__ count, int K, int* __restrict__ offset) {
  __shared__ int sums[kNdbThreads];
  for (int k = threadIdx.x; k < K; k += kNdbThreads) offset[k] = count[k];
  __syncthreads();
  ndb_block_scan(offset, K, sums);
}

__global__ __launch_bounds__(kNdbWave) void ndb_centroids_kernel(const float* __restrict__ x, int n, int D, const int* __restrict__ perm,
                                                                 const int* __restrict__ count, const int* __restrict__ offset,
                                                                 float* __restrict__ c) {
  const int k = blockIdx.x, j = blockIdx.y * kNdbCentFeatures + threadIdx.x * 4;
  int off = offset[k], cnt = count[k];
  off = off < 0 ? 0 : (off < n ? off : n);              // memory safety only (header)
  cnt = cnt < 0 ? 0 : (cnt < n - off ? cnt : n - off);
  if (cnt == 0 || j >= D) return;                       // D % 16 == 0: j < D covers j + 3
  const int* rows = perm + off;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  auto fetch = [&](int i) {
    int r = rows[i];
    r = r < 0 ? 0 : (r < n ? r : n - 1);
    return *reinterpret_cast<const f32x4*>(x + (size_t)r * D + j);
  };
  int i = 0;
  for (; i + kNdbCentDepth <= cnt; i += kNdbCentDepth) {
    f32x4 v[kNdbCentDepth];
#pragma unroll
    for (int e = 0; e < kNdbCentDepth; e++) v[e] = fetch(i + e);
#pragma unroll
    for (int e = 0; e < kNdbCentDepth; e++) {
      s0 += (double)v[e][0];
      s1 += (double)v[e][1];
      s2 += (double)v[e][2];
      s3 += (double)v[e][3];
    }
  }
  for (; i < cnt; i++) {
    const f32x4 v = fetch(i);
    s0 += (double)v[0];
    s1 += (double)v[1];
    s2 += (double)v[2];
    s3 += (double)v[3];
  }
  const double m = (double)cnt;
  *reinterpret_cast<f32x4*>(c + (size_t)k * D + j) = f32x4{(float)(s0 / m), (float)(s1 / m), (float)(s2 / m), (float)(s3 / m)};
}

int ndb_check_features(const char* what, int n, int K, int D) {
  GANK_REQUIRE(D >= 16 && D <= 4096 && D % 16 == 0, "%s: D = %d unsupported (a multiple of 16 in 16..4096)", what, D);
  GANK_REQUIRE(K >= 1 && K <= kNdbMaxK, "%s: K = %d unsupported (1..%d)", what, K, kNdbMaxK);
  GANK_REQUIRE(n >= 1 && n <= kNdbMaxRows, "%s: n = %d (1..%d)", what, n, kNdbMaxRows);
  return 0;
}

}  // namespace

extern "C" int gank_ndb_pixel_features(const unsigned char* img, int n, int P, const int* dims, int Dsel, float* out, void* stream) {
  GANK_REQUIRE(img && out, "ndb_pixel_features: null pointer");
  GANK_REQUIRE(n >= 1 && n <= kNdbMaxRows, "ndb_pixel_features: n = %d (1..%d)", n, kNdbMaxRows);
  GANK_REQUIRE(P >= 1 && P <= kNdbMaxPixels, "ndb_pixel_features: P = %d (1..%d)", P, kNdbMaxPixels);
  GANK_REQUIRE(Dsel >= 1 && Dsel <= 4096 && Dsel <= P, "ndb_pixel_features: Dsel = %d (1..4096, at most the %d pixels)", Dsel, P);
  GANK_REQUIRE(((uintptr_t)out & 15) == 0 && ((uintptr_t)dims & 3) == 0, "ndb_pixel_features: misaligned pointer");
  hipLaunchKernelGGL(ndb_pixel_features_kernel, dim3((unsigned)n), dim3(kNdbThreads), 0, (hipStream_t)stream, img, P, dims, Dsel,
                     roundup(Dsel, 16), out);
  GANK_LAUNCH_OK("ndb_pixel_features");
  return 0;
}

extern "C" int gank_ndb_assign(const float* x, int n, const float* c, int K, int D, const int* prev, int* label, double* d2,
                               double* part_inertia, int* part_changed, void* stream) {
  GANK_REQUIRE(x && c && label && d2 && part_inertia && part_changed, "ndb_assign: null pointer");
  if (ndb_check_features("ndb_assign", n, K, D)) return 1;
  GANK_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)c & 15) == 0 && ((uintptr_t)prev & 3) == 0 && ((uintptr_t)label & 3) == 0 &&
                   ((uintptr_t)d2 & 7) == 0 && ((uintptr_t)part_inertia & 7) == 0 && ((uintptr_t)part_changed & 3) == 0,
               "ndb_assign: misaligned pointer");
  hipLaunchKernelGGL(ndb_assign_kernel, dim3((unsigned)ndb_tiles(n)), dim3(kNdbThreads), 0, (hipStream_t)stream, x, n, c, K, D, prev, label, d2,
                     part_inertia, part_changed);
  GANK_LAUNCH_OK("ndb_assign");
  return 0;
}

extern "C" long gank_ndb_group_ws_elems(int n, int K) {
  if (n < 1 || n > kNdbMaxRows || K < 1 || K > kNdbMaxK) return 0;
  return (long)K * ndb_units(n);
}

extern "C" int gank_ndb_group_rows(const int* label, int n, int K, int* count, int* offset, int* perm, int* ws, void* stream) {
  GANK_REQUIRE(label && count && offset && perm && ws, "ndb_group_rows: null pointer");
  GANK_REQUIRE(K >= 1 && K <= kNdbMaxK, "ndb_group_rows: K = %d unsupported (1..%d)", K, kNdbMaxK);
  GANK_REQUIRE(n >= 1 && n <= kNdbMaxRows, "ndb_group_rows: n = %d (1..%d)", n, kNdbMaxRows);
  GANK_REQUIRE((((uintptr_t)label | (uintptr_t)count | (uintptr_t)offset | (uintptr_t)perm | (uintptr_t)ws) & 3) == 0,
               "ndb_group_rows: misaligned pointer");
  const int units = ndb_units(n);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ndb_group_unit_kernel<false>, dim3((unsigned)units), dim3(kNdbWave), 0, s, label, n, K, units, ws, (const int*)nullptr,
                     (int*)nullptr);
  hipLaunchKernelGGL(ndb_group_scan_units_kernel, dim3((unsigned)K), dim3(kNdbThreads), 0, s, ws, units, count);
  hipLaunchKernelGGL(ndb_group_scan_labels_kernel, dim3(1), dim3(kNdbThreads), 0, s, (const int*)count, K, offset);
  hipLaunchKernelGGL(ndb_group_unit_kernel<true>, dim3((unsigned)units), dim3(kNdbWave), 0, s, label, n, K, units, ws, (const int*)offset, perm);
  GANK_LAUNCH_OK("ndb_group_rows");
  return 0;
}

extern "C" int gank_ndb_centroids(const float* x, int n, int D, const int* perm, const int* count, const int* offset, int K, float* c,
                                  void* stream) {
  GANK_REQUIRE(x && perm && count && offset && c, "ndb_centroids: null pointer");
  if (ndb_check_features("ndb_centroids", n, K, D)) return 1;
  GANK_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)c & 15) == 0 && (((uintptr_t)perm | (uintptr_t)count | (uintptr_t)offset) & 3) == 0,
               "ndb_centroids: misaligned pointer");
  hipLaunchKernelGGL(ndb_centroids_kernel, dim3((unsigned)K, (unsigned)cdiv(D, kNdbCentFeatures)), dim3(kNdbWave), 0, (hipStream_t)stream, x, n, D,
                     perm, count, offset, c);
  GANK_LAUNCH_OK("ndb_centroids");
  return 0;
}
