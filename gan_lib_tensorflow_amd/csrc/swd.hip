// The sliced Wasserstein distance on Laplacian-pyramid patches (Karras et al., "Progressive Growing of GANs", section 5;
// common/swd.py).  Everything is float64, nothing is atomic, every output element has one owner and one plain store:
//   gank_swd_pyr_down      5 x 5 binomial window, mirror boundary, even rows and columns kept;
//   gank_swd_laplacian     fine -= pyr_up(coarse): the window times 4 on the zero-stuffed grid, mirror taken on that grid;
//   gank_swd_patch_stats   per channel sum (x - shift) and sum (x - shift)^2 over all patches, gathered through centre tables;
//   gank_swd_project       key[d][r] = sum_k (patch_r[k] - mean_c) / std_c * dirs[k][d], patches gathered straight from the level;
//   gank_swd_sort_rows     every row of keys ascending;
//   gank_swd_sorted_l1     per direction and workgroup sum_r |a[d][r] - b[d][r]|.
//
// Stencils.  One thread per output element, the 25 taps in row-major order.  The window entries k / 256 (k / 64 for pyr_up) are
// powers of two times small integers: on uint8 input every product and partial sum is exact, so the order does not matter.
//
// Statistics.  One thread per patch and channel walks the nhood x nhood elements in (y, x) order; the 256 threads of a
// workgroup are added by a fixed LDS tree; a second launch adds the workgroup partials (thread t the partials t, t + 256, ..,
// then the same tree).  The caller runs it twice: shift = 0 gives the mean, shift = mean gives sum (x - mean)^2 without the
// cancellation of sum x^2 - n mean^2 (the coarsest level has a mean of about 127).
//
// Projection.  A 256-thread workgroup owns 128 patches x 64 directions; the contraction axis K = C * nhood^2 is walked in
// chunks of 16 (the tail masked with zeros: K = 147 is no multiple of anything useful).  Per chunk the normalised patch values
// go to LDS as P[k][row] -- thread t always stages row t & 127, so its patch origin is computed once -- and the directions as
// D[k][dir].  Thread (tr = t & 15, td = t >> 4) accumulates rows tr + 16 i (i < 8) x directions 4 td + j (j < 4) with explicit
// fma: 16 consecutive lanes read 16 consecutive doubles of P (no bank conflict), the four 16-lane groups of a wave read four
// addresses of D (broadcast).  The vector FMA rate equals the f64 MFMA rate on this chip, so the MFMA would buy operand
// bandwidth only; the sort below dominates the metric, and the plain form has no padding to get wrong.  Keys are stored
// key[d][row]: 16 lanes write 128 consecutive bytes.
//
// Sort.  Least-significant-digit radix sort on the order-preserving transform of the key's bits (negative: all bits flipped,
// else the sign bit set), 8 passes of 8 bits, ping-pong between `keys` and `tmp`, so the result is back in `keys`.  The unit
// of work is a wave and its 2048 consecutive keys, so a row never has to fit one workgroup's LDS.  Per pass three launches:
//   count    every wave counts the digits of its keys -> hist[row][unit][256];
//   scan     one workgroup per row, thread t = digit t: exclusive prefix over (digit, unit) in digit-major order, in place;
//   scatter  every wave walks its keys in order, 64 at a time: the lanes with equal digits find each other with 8 ballots, a
//            key's slot is base[digit] + (equal-digit lanes below it), the group's highest lane advances base[digit].
// The order (unit, round, lane) is the order of the input, so every pass is stable, which LSD needs, and nothing depends on
// timing: same bits every call.  No atomics: a digit's counter in LDS is advanced by exactly one lane per round.
// Traffic: a pass reads the keys twice and writes them once, 24 bytes a key, 192 bytes a key for the sort, plus the histograms
// (1 KiB per 2048 keys, written once and read twice: under 1 % ).  A merge sort of 2048-key blocks needs log2(M / 2048) = 9 merge
// passes of 16 bytes at M = 2^20 plus the block sort, about the same traffic but with data-dependent merge-path searches; the
// radix form has fixed work per key, and its scattered 8-byte stores fall into at most 256 open runs per wave.
// Contract: finite keys of either sign, subnormals included.  NaN sorts by its bit pattern (after +inf when positive) and -0.0
// sorts before +0.0: both are the caller's error, the metric never produces them from finite images.
#include "gank_common.h"

namespace {

constexpr int kSwdThreads = 256;
constexpr int kSwdMaxC = 16;
constexpr int kSwdMaxNhood = 15;
constexpr int kSwdMaxSide = 4096;
constexpr int kSwdMaxRows = 1 << 24;           // patches a side and level (M): rows of a sort
constexpr int kSwdMaxDirs = 65535;             // gridDim.y
constexpr int kSortUnit = 2048;                // keys per wave
constexpr int kSortWaves = kSwdThreads / 64;   // units per workgroup
constexpr int kProjRows = 128, kProjDirs = 64, kProjChunk = 16;
constexpr int kL1PerBlock = 4096;              // keys per workgroup of gank_swd_sorted_l1

__device__ __forceinline__ int swd_mirror(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

__device__ __forceinline__ double swd_tap(int t) { return t == 0 || t == 4 ? 1.0 : (t == 2 ? 6.0 : 4.0); }

// fixed tree over the 256 threads of a workgroup; every thread returns the sum
__device__ __forceinline__ double swd_block_sum(double v, double* red) {
  const int t = threadIdx.x;
  __syncthreads();
  red[t] = v;
  __syncthreads();
#pragma unroll
  for (int o = kSwdThreads / 2; o > 0; o >>= 1) {
    if (t < o) red[t] = red[t] + red[t + o];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(kSwdThreads) void swd_pyr_down_kernel(const double* __restrict__ x, int H, int W, int C, double* __restrict__ y,
                                                                   size_t total) {
  const size_t e = (size_t)blockIdx.x * kSwdThreads + threadIdx.x;
  if (e >= total) return;
  const int h2 = H / 2, w2 = W / 2;
  const int c = (int)(e % C);
  size_t p = e / C;
  const int ox = (int)(p % w2);
  p /= w2;
  const int oy = (int)(p % h2);
  const size_t n = p / h2;
  const double* img = x + n * (size_t)H * W * C + c;
  double acc = 0.0;
#pragma unroll
  for (int a = 0; a < 5; a++) {
    const int iy = swd_mirror(2 * oy + a - 2, H);
#pragma unroll
    for (int b = 0; b < 5; b++) {
      const int ix = swd_mirror(2 * ox + b - 2, W);
      acc += (swd_tap(a) * swd_tap(b) / 256.0) * img[((size_t)iy * W + ix) * C];
    }
  }
  y[e] = acc;
}

// H, W: the fine size; coarse is [N, H/2, W/2, C]
__global__ __launch_bounds__(kSwdThreads) void swd_laplacian_kernel(double* __restrict__ fine, const double* __restrict__ coarse, int H, int W,
                                                                    int C, size_t total) {
  const size_t e = (size_t)blockIdx.x * kSwdThreads + threadIdx.x;
  if (e >= total) return;
  const int h2 = H / 2, w2 = W / 2;
  const int c = (int)(e % C);
  size_t p = e / C;
  const int ox = (int)(p % W);
  p /= W;
  const int oy = (int)(p % H);
  const size_t n = p / H;
  const double* img = coarse + n * (size_t)h2 * w2 * C + c;
  double acc = 0.0;
#pragma unroll
  for (int a = 0; a < 5; a++) {
    const int iy = swd_mirror(oy + a - 2, H);
#pragma unroll
    for (int b = 0; b < 5; b++) {
      const int ix = swd_mirror(ox + b - 2, W);
      if (((iy | ix) & 1) == 0) acc += (swd_tap(a) * swd_tap(b) / 64.0) * img[((size_t)(iy >> 1) * w2 + (ix >> 1)) * C];
    }
  }
  fine[e] = fine[e] - acc;
}

// part[block][c][2]; grid = ceil(M / 256)
__global__ __launch_bounds__(kSwdThreads) void swd_patch_stats_kernel(const double* __restrict__ level, int H, int W, int C,
                                                                      const int* __restrict__ cx, const int* __restrict__ cy, int M, int nhood,
                                                                      int per_image, const double* __restrict__ shift, double* __restrict__ part) {
  __shared__ double red[kSwdThreads];
  const int r = blockIdx.x * kSwdThreads + threadIdx.x;
  const bool live = r < M;
  const int h = nhood / 2;
  const double* org = level;
  if (live) org += (((size_t)(r / per_image) * H + (cy[r] - h)) * W + (cx[r] - h)) * C;
  for (int c = 0; c < C; c++) {
    const double sh = shift ? shift[c] : 0.0;
    double s1 = 0.0, s2 = 0.0;
    if (live)
      for (int dy = 0; dy < nhood; dy++)
        for (int dx = 0; dx < nhood; dx++) {
          const double v = org[((size_t)dy * W + dx) * C + c] - sh;
          s1 += v;
          s2 += v * v;
        }
    s1 = swd_block_sum(s1, red);
    s2 = swd_block_sum(s2, red);
    if (threadIdx.x == 0) {
      part[((size_t)blockIdx.x * C + c) * 2 + 0] = s1;
      part[((size_t)blockIdx.x * C + c) * 2 + 1] = s2;
    }
  }
}

// out[c][2]: block b = entry (c, which) adds its `parts` partials
__global__ __launch_bounds__(kSwdThreads) void swd_patch_stats_finish_kernel(const double* __restrict__ part, int parts, int entries,
                                                                             double* __restrict__ out) {
  __shared__ double red[kSwdThreads];
  double s = 0.0;
  for (int p = threadIdx.x; p < parts; p += kSwdThreads) s += part[(size_t)p * entries + blockIdx.x];
  s = swd_block_sum(s, red);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}

__global__ __launch_bounds__(kSwdThreads) void swd_project_kernel(const double* __restrict__ level, int H, int W, int C,
                                                                  const int* __restrict__ cx, const int* __restrict__ cy, int M, int nhood,
                                                                  int per_image, const double* __restrict__ mean_std,
                                                                  const double* __restrict__ dirs, int ndirs, double* __restrict__ keys) {
  __shared__ double P[kProjChunk][kProjRows];
  __shared__ __attribute__((aligned(16))) double D[kProjChunk][kProjDirs];
  __shared__ double ms[2 * kSwdMaxC];
  const int tid = threadIdx.x, tr = tid & 15, td = tid >> 4;
  const int row0 = blockIdx.x * kProjRows, dir0 = blockIdx.y * kProjDirs;
  const int K = C * nhood * nhood, n2 = nhood * nhood, h = nhood / 2;
  if (tid < 2 * C) ms[tid] = mean_std[tid];
  const int srow = row0 + (tid & (kProjRows - 1));          // the patch this thread stages
  const bool live = srow < M;
  const double* org = level;
  if (live) org += (((size_t)(srow / per_image) * H + (cy[srow] - h)) * W + (cx[srow] - h)) * C;
  double acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = 0.0;
  __syncthreads();

  for (int k0 = 0; k0 < K; k0 += kProjChunk) {
#pragma unroll
    for (int i = 0; i < kProjChunk * kProjRows / kSwdThreads; i++) {
      const int kk = (tid >> 7) + 2 * i, k = k0 + kk;
      double v = 0.0;
      if (live && k < K) {
        const int c = k / n2, rem = k - c * n2, dy = rem / nhood, dx = rem - dy * nhood;
        v = (org[((size_t)dy * W + dx) * C + c] - ms[c]) / ms[C + c];
      }
      P[kk][tid & (kProjRows - 1)] = v;
    }
#pragma unroll
    for (int i = 0; i < kProjChunk * kProjDirs / kSwdThreads; i++) {
      const int kk = (tid >> 6) + 4 * i, k = k0 + kk, d = dir0 + (tid & (kProjDirs - 1));
      D[kk][tid & (kProjDirs - 1)] = (k < K && d < ndirs) ? dirs[(size_t)k * ndirs + d] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kProjChunk; kk++) {
      double p[8], q[4];
#pragma unroll
      for (int i = 0; i < 8; i++) p[i] = P[kk][tr + 16 * i];
#pragma unroll
      for (int j = 0; j < 4; j++) q[j] = D[kk][4 * td + j];
#pragma unroll
      for (int i = 0; i < 8; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = __builtin_fma(p[i], q[j], acc[i][j]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int d = dir0 + 4 * td + j;
    if (d >= ndirs) continue;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int r = row0 + tr + 16 * i;
      if (r < M) keys[(size_t)d * M + r] = acc[i][j];
    }
  }
}

// ---- sort
__device__ __forceinline__ unsigned swd_digit(double v, int shift) {
  unsigned long long u = (unsigned long long)__double_as_longlong(v);
  u ^= (u >> 63) ? ~0ull : 0x8000000000000000ull;
  return (unsigned)(u >> shift) & 255u;
}

// the lanes of the wave that are `valid` and hold the same digit as this lane
__device__ __forceinline__ unsigned long long swd_match(unsigned digit, bool valid) {
  unsigned long long m = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 8; b++) {
    const bool bit = (digit >> b) & 1u;
    const unsigned long long bal = __ballot(bit);
    m &= bit ? bal : ~bal;
  }
  return m;
}

__host__ __device__ inline int swd_sort_units(int M) { return (M + kSortUnit - 1) / kSortUnit; }

// COUNT: hist[row][unit][digit] = the unit's digit counts.  SCATTER: hist holds the exclusive prefix; dst gets the keys.
// grid (ceil(units / 4), dirs): a wave that has no unit writes nothing but takes part in every barrier.
template <bool kScatter>
__global__ __launch_bounds__(kSwdThreads) void swd_sort_pass_kernel(const double* __restrict__ src, double* __restrict__ dst, int M, int units,
                                                                    int shift, unsigned* __restrict__ hist) {
  __shared__ unsigned counter[kSortWaves][256];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int unit = blockIdx.x * kSortWaves + w, row = blockIdx.y;
  const bool has_unit = unit < units;
  unsigned* h = hist + ((size_t)row * units + (has_unit ? unit : 0)) * 256;
#pragma unroll
  for (int q = 0; q < 4; q++) counter[w][lane + 64 * q] = kScatter ? h[lane + 64 * q] : 0u;
  __syncthreads();
  const double* s = src + (size_t)row * M;
  double* d = dst + (size_t)row * M;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int round = 0; round < kSortUnit / 64; round++) {
    const long long idx = (long long)unit * kSortUnit + round * 64 + lane;
    const bool valid = has_unit && idx < M;
    const double v = valid ? s[idx] : 0.0;
    const unsigned digit = swd_digit(v, shift);
    const unsigned long long m = swd_match(digit, valid);
    const int rank = __popcll(m & below), count = __popcll(m);
    const unsigned base = counter[w][digit];
    __syncthreads();                                   // every lane has read its base before any counter moves
    if (valid) {
      if (kScatter) d[base + rank] = v;
      if (rank == count - 1) counter[w][digit] = base + count;       // one lane per digit and round
    }
    __syncthreads();
  }
  if (!kScatter && has_unit) {
#pragma unroll
    for (int q = 0; q < 4; q++) h[lane + 64 * q] = counter[w][lane + 64 * q];
  }
}

// one workgroup per row, thread t = digit t: hist[row][unit][digit] -> its exclusive prefix in (digit, unit) order
__global__ __launch_bounds__(256) void swd_sort_scan_kernel(unsigned* __restrict__ hist, int units) {
  __shared__ unsigned total[256];
  const int t = threadIdx.x;
  unsigned* h = hist + (size_t)blockIdx.x * units * 256;
  unsigned run = 0;
  for (int u = 0; u < units; u++) {
    const unsigned c = h[(size_t)u * 256 + t];
    h[(size_t)u * 256 + t] = run;
    run += c;
  }
  total[t] = run;
  __syncthreads();
  unsigned base = 0;
  for (int dgt = 0; dgt < t; dgt++) base += total[dgt];
  for (int u = 0; u < units; u++) h[(size_t)u * 256 + t] += base;
}

// part[d][block]; grid (ceil(M / 4096), dirs)
__global__ __launch_bounds__(kSwdThreads) void swd_sorted_l1_kernel(const double* __restrict__ a, const double* __restrict__ b, int M, int parts,
                                                                    double* __restrict__ part) {
  __shared__ double red[kSwdThreads];
  const size_t rowoff = (size_t)blockIdx.y * M;
  double s = 0.0;
#pragma unroll 4
  for (int i = 0; i < kL1PerBlock / kSwdThreads; i++) {
    const long long r = (long long)blockIdx.x * kL1PerBlock + i * kSwdThreads + threadIdx.x;
    if (r < M) s += fabs(a[rowoff + r] - b[rowoff + r]);
  }
  s = swd_block_sum(s, red);
  if (threadIdx.x == 0) part[(size_t)blockIdx.y * parts + blockIdx.x] = s;
}

int swd_check_level(const char* what, int N, int H, int W, int C) {
  GANK_REQUIRE(N >= 1 && H >= 1 && W >= 1 && H <= kSwdMaxSide && W <= kSwdMaxSide, "%s: images [%d, %d, %d, %d] unsupported (sides 1..%d)", what, N,
               H, W, C, kSwdMaxSide);
  GANK_REQUIRE(C >= 1 && C <= kSwdMaxC, "%s: C = %d unsupported (1..%d)", what, C, kSwdMaxC);
  GANK_REQUIRE((double)N * H * W * C < 68719476736.0, "%s: [%d, %d, %d, %d] has too many elements (2^36)", what, N, H, W, C);
  return 0;
}

int swd_check_patches(const char* what, int N, int H, int W, int M, int nhood, int per_image) {
  GANK_REQUIRE(nhood >= 1 && nhood <= kSwdMaxNhood && (nhood & 1), "%s: nhood_size = %d unsupported (odd, 1..%d)", what, nhood, kSwdMaxNhood);
  GANK_REQUIRE(nhood <= H && nhood <= W, "%s: a %d x %d patch does not fit a %d x %d level", what, nhood, nhood, H, W);
  GANK_REQUIRE(M >= 1 && M <= kSwdMaxRows, "%s: M = %d patches (1..%d)", what, M, kSwdMaxRows);
  GANK_REQUIRE(per_image >= 1 && (long long)per_image * N >= M, "%s: %d patches at %d per image need more than %d images", what, M, per_image, N);
  return 0;
}

}  // namespace

extern "C" int gank_swd_pyr_down(const double* x, int N, int H, int W, int C, double* y, void* stream) {
  GANK_REQUIRE(x && y, "swd_pyr_down: null pointer");
  if (swd_check_level("swd_pyr_down", N, H, W, C)) return 1;
  GANK_REQUIRE(H >= 4 && W >= 4 && H % 2 == 0 && W % 2 == 0, "swd_pyr_down: a %d x %d image cannot be halved (even sides >= 4)", H, W);
  const size_t total = (size_t)N * (H / 2) * (W / 2) * C;
  hipLaunchKernelGGL(swd_pyr_down_kernel, dim3((unsigned)((total + kSwdThreads - 1) / kSwdThreads)), dim3(kSwdThreads), 0, (hipStream_t)stream, x,
                     H, W, C, y, total);
  GANK_LAUNCH_OK("swd_pyr_down");
  return 0;
}

extern "C" int gank_swd_laplacian(double* fine, const double* coarse, int N, int H, int W, int C, void* stream) {
  GANK_REQUIRE(fine && coarse, "swd_laplacian: null pointer");
  if (swd_check_level("swd_laplacian", N, H, W, C)) return 1;
  GANK_REQUIRE(H >= 4 && W >= 4 && H % 2 == 0 && W % 2 == 0, "swd_laplacian: a %d x %d level has no half-size level (even sides >= 4)", H, W);
  const size_t total = (size_t)N * H * W * C;
  hipLaunchKernelGGL(swd_laplacian_kernel, dim3((unsigned)((total + kSwdThreads - 1) / kSwdThreads)), dim3(kSwdThreads), 0, (hipStream_t)stream,
                     fine, coarse, H, W, C, total);
  GANK_LAUNCH_OK("swd_laplacian");
  return 0;
}

extern "C" int gank_swd_patch_stats_parts(int M) { return M >= 1 ? cdiv(M, kSwdThreads) : 0; }

extern "C" int gank_swd_patch_stats(const double* level, int N, int H, int W, int C, const int* cx, const int* cy, int M, int nhood,
                                    int per_image, const double* shift, double* part, double* out, void* stream) {
  GANK_REQUIRE(level && cx && cy && part && out, "swd_patch_stats: null pointer");
  if (swd_check_level("swd_patch_stats", N, H, W, C) || swd_check_patches("swd_patch_stats", N, H, W, M, nhood, per_image)) return 1;
  const int parts = cdiv(M, kSwdThreads);
  hipLaunchKernelGGL(swd_patch_stats_kernel, dim3((unsigned)parts), dim3(kSwdThreads), 0, (hipStream_t)stream, level, H, W, C, cx, cy, M, nhood,
                     per_image, shift, part);
  GANK_LAUNCH_OK("swd_patch_stats");
  hipLaunchKernelGGL(swd_patch_stats_finish_kernel, dim3((unsigned)(2 * C)), dim3(kSwdThreads), 0, (hipStream_t)stream, (const double*)part, parts,
                     2 * C, out);
  GANK_LAUNCH_OK("swd_patch_stats_finish");
  return 0;
}

extern "C" int gank_swd_project(const double* level, int N, int H, int W, int C, const int* cx, const int* cy, int M, int nhood, int per_image,
                                const double* mean_std, const double* dirs, int ndirs, double* keys, void* stream) {
  GANK_REQUIRE(level && cx && cy && mean_std && dirs && keys, "swd_project: null pointer");
  if (swd_check_level("swd_project", N, H, W, C) || swd_check_patches("swd_project", N, H, W, M, nhood, per_image)) return 1;
  GANK_REQUIRE(ndirs >= 1 && ndirs <= kSwdMaxDirs, "swd_project: %d directions (1..%d)", ndirs, kSwdMaxDirs);
  const dim3 grid((unsigned)cdiv(M, kProjRows), (unsigned)cdiv(ndirs, kProjDirs));
  hipLaunchKernelGGL(swd_project_kernel, grid, dim3(kSwdThreads), 0, (hipStream_t)stream, level, H, W, C, cx, cy, M, nhood, per_image, mean_std,
                     dirs, ndirs, keys);
  GANK_LAUNCH_OK("swd_project");
  return 0;
}

extern "C" int gank_swd_sort_max_rows(void) { return kSwdMaxRows; }

extern "C" long gank_swd_sort_ws_elems(int dirs, int M) {
  if (dirs < 1 || M < 1) return 0;
  return (long)dirs * swd_sort_units(M) * 256;
}

extern "C" int gank_swd_sort_rows(double* keys, double* tmp, int dirs, int M, unsigned* hist, void* stream) {
  GANK_REQUIRE(keys && tmp && hist, "swd_sort_rows: null pointer");
  GANK_REQUIRE(M >= 1 && M <= kSwdMaxRows, "swd_sort_rows: M = %d keys a row unsupported (1..%d)", M, kSwdMaxRows);
  GANK_REQUIRE(dirs >= 1 && dirs <= kSwdMaxDirs, "swd_sort_rows: %d rows (1..%d)", dirs, kSwdMaxDirs);
  GANK_REQUIRE(keys != tmp, "swd_sort_rows: keys and tmp are the same buffer");
  const int units = swd_sort_units(M);
  const dim3 grid((unsigned)cdiv(units, kSortWaves), (unsigned)dirs);
  double *src = keys, *dst = tmp;
  for (int pass = 0; pass < 8; pass++) {
    hipLaunchKernelGGL(swd_sort_pass_kernel<false>, grid, dim3(kSwdThreads), 0, (hipStream_t)stream, (const double*)src, dst, M, units, 8 * pass,
                       hist);
    hipLaunchKernelGGL(swd_sort_scan_kernel, dim3((unsigned)dirs), dim3(256), 0, (hipStream_t)stream, hist, units);
    hipLaunchKernelGGL(swd_sort_pass_kernel<true>, grid, dim3(kSwdThreads), 0, (hipStream_t)stream, (const double*)src, dst, M, units, 8 * pass,
                       hist);
    GANK_LAUNCH_OK("swd_sort_rows");
    double* t = src;
    src = dst;
    dst = t;
  }
  return 0;      // 8 passes: the sorted rows are back in `keys`
}

extern "C" int gank_swd_sorted_l1_parts(int M) { return M >= 1 ? cdiv(M, kL1PerBlock) : 0; }

extern "C" int gank_swd_sorted_l1(const double* a, const double* b, int dirs, int M, double* part, void* stream) {
  GANK_REQUIRE(a && b && part, "swd_sorted_l1: null pointer");
  GANK_REQUIRE(M >= 1 && M <= kSwdMaxRows, "swd_sorted_l1: M = %d keys a row unsupported (1..%d)", M, kSwdMaxRows);
  GANK_REQUIRE(dirs >= 1 && dirs <= kSwdMaxDirs, "swd_sorted_l1: %d rows (1..%d)", dirs, kSwdMaxDirs);
  const int parts = cdiv(M, kL1PerBlock);
  hipLaunchKernelGGL(swd_sorted_l1_kernel, dim3((unsigned)parts, (unsigned)dirs), dim3(kSwdThreads), 0, (hipStream_t)stream, a, b, M, parts, part);
  GANK_LAUNCH_OK("swd_sorted_l1");
  return 0;
}
