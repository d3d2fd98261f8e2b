// The statistics stage of the Inception score (common/inception/inception_score.py: InceptionScore; the one filled column of the
// reference README's "Quantitative evaluation" table, inception_score.py:49-66 of the reference):
//   gank_inception_score_update  a batch of float32 logits is added to the running float64 state of the splits it falls in.
//
// For one split of n_s rows, with lse_x = logsumexp(l_x) and p_xy = exp(l_xy - lse_x),
//   mean_x KL(p_x || m) = (1/n_s) sum_x sum_y p_xy (l_xy - lse_x)  -  sum_y m_y log m_y,     m_y = (1/n_s) sum_x p_xy,
// so a split needs 1000 class sums and one scalar, state[j][0..999] and state[j][1000], and no probability is kept.
//
// Two launches per call.
//   row pass     one 256-thread workgroup per row: the row maximum (float32, exact), S = sum_y exp(l_y - max) and
//                lse = max + log S in float64, then E = sum_y p_y (l_y - lse) with p_y = exp(l_y - lse); scratch[r] = (lse, E).
//                A thread adds its columns in index order, the 64 lanes of a wave meet in an xor butterfly (every lane ends
//                with the same bits: a + b == b + a), the four waves are added in index order.  What a row gives depends on
//                that row alone, not on the call it came in.
//   column pass  one thread per (split touched by the call, column): it loads state[j][y], adds p_y = exp(l_y - lse) of the
//                call's rows of split j IN ASCENDING ROW ORDER, one addition per row onto the running value, and stores it;
//                column 1000 adds the rows' E the same way.  Every state element has one owner and receives its rows in
//                global row order, so the same rows fed in calls of any sizes leave the same bits: state after a call is
//                (..((state + t_0) + t_1).. + t_k), whichever call t_i arrived in.  No atomics, no partial sums per call.
// The parallelism is over columns x splits (a wave per 64 columns), not over rows: 100 x 1000 float64 exp per call.
#include "f64_tile.h"

namespace {

constexpr int kIsClasses = 1000;               // the first 1000 of the frozen graph's 1008 logits (inception_score.py:55)
constexpr int kIsState = kIsClasses + 1;       // + the scalar sum_x sum_y p (l - lse)
constexpr int kIsRowThreads = kF64Threads;     // block_sum (f64_tile.h) is the sum over 256 threads
constexpr int kIsColThreads = 64;

__global__ __launch_bounds__(kIsRowThreads) void is_row_kernel(const float* __restrict__ logits, int ld, double* __restrict__ scratch) {
  __shared__ double red[4];
  __shared__ float redm[4];
  const int r = blockIdx.x, tid = threadIdx.x;
  const float* row = logits + (size_t)r * ld;
  float m = -INFINITY;
  for (int y = tid; y < kIsClasses; y += kIsRowThreads) m = fmaxf(m, row[y]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((tid & 63) == 0) redm[tid >> 6] = m;
  __syncthreads();
  const double mx = (double)fmaxf(fmaxf(redm[0], redm[1]), fmaxf(redm[2], redm[3]));
  double s = 0.0;
  for (int y = tid; y < kIsClasses; y += kIsRowThreads) s += exp((double)row[y] - mx);
  const double lse = mx + log(block_sum(s, red));
  double e = 0.0;
  for (int y = tid; y < kIsClasses; y += kIsRowThreads) {
    const double d = (double)row[y] - lse;
    e += exp(d) * d;              // exp underflows to 0 long before d reaches -inf: 0 * finite, never 0 * -inf
  }
  e = block_sum(e, red);
  if (tid == 0) {
    scratch[2 * (size_t)r] = lse;
    scratch[2 * (size_t)r + 1] = e;
  }
}

// blockIdx.y = split j0 + blockIdx.y; thread = column y of [0, 1001)
__global__ __launch_bounds__(kIsColThreads) void is_col_kernel(const float* __restrict__ logits, int n_rows, int ld, long long row0,
                                                               long long n_total, int splits, int j0, const double* __restrict__ scratch,
                                                               double* __restrict__ state) {
  const int y = blockIdx.x * kIsColThreads + threadIdx.x;
  if (y >= kIsState) return;
  const int j = j0 + blockIdx.y;
  const long long lo = (long long)j * n_total / splits, hi = (long long)(j + 1) * n_total / splits;      // preds2score's slice
  const int r0 = (int)((lo > row0 ? lo : row0) - row0);
  const long long end = row0 + n_rows;
  const int r1 = (int)((hi < end ? hi : end) - row0);
  double* dst = state + (size_t)j * kIsState + y;
  double acc = *dst;
  if (y < kIsClasses) {
    for (int r = r0; r < r1; r++) acc += exp((double)logits[(size_t)r * ld + y] - scratch[2 * (size_t)r]);
  } else {
    for (int r = r0; r < r1; r++) acc += scratch[2 * (size_t)r + 1];
  }
  *dst = acc;
}

// the split a global row belongs to: j with j * n / s <= row < (j + 1) * n / s
int is_split_of(long long row, long long n_total, int splits) {
  long long j = row * splits / n_total;         // n_total * splits <= 2^62 (checked by the caller): no product overflows
  while (j + 1 < splits && (j + 1) * n_total / splits <= row) j++;
  while (j > 0 && j * n_total / splits > row) j--;
  return (int)j;
}

}  // namespace

extern "C" int gank_inception_score_update(const float* logits, int n_rows, int ld, long long row0, long long n_total, int splits,
                                           double* state, double* scratch, void* stream) {
  GANK_REQUIRE(logits && state && scratch, "inception_score_update: null pointer");
  GANK_REQUIRE(n_rows >= 1, "inception_score_update: n_rows = %d, needs at least one row", n_rows);
  GANK_REQUIRE(ld >= kIsClasses, "inception_score_update: ld = %d, a row holds at least %d logits", ld, kIsClasses);
  GANK_REQUIRE(splits >= 1, "inception_score_update: splits = %d, needs at least one", splits);
  GANK_REQUIRE((long long)splits <= n_total, "inception_score_update: splits = %d exceeds n_total = %lld (an empty split has no score)", splits,
               n_total);
  GANK_REQUIRE(row0 >= 0, "inception_score_update: row0 = %lld is negative", row0);
  GANK_REQUIRE(row0 <= n_total - n_rows, "inception_score_update: rows %lld..%lld exceed n_total = %lld", row0, row0 + n_rows - 1, n_total);
  GANK_REQUIRE(n_total <= (1LL << 62) / splits, "inception_score_update: n_total = %lld x splits = %d overflows the slice bounds", n_total, splits);
  GANK_REQUIRE(((uintptr_t)logits & 3) == 0 && ((uintptr_t)state & 7) == 0 && ((uintptr_t)scratch & 7) == 0,
               "inception_score_update: misaligned pointer");
  const int j0 = is_split_of(row0, n_total, splits), j1 = is_split_of(row0 + n_rows - 1, n_total, splits);
  GANK_REQUIRE(j1 - j0 < 65535, "inception_score_update: one call touches %d splits (at most 65535)", j1 - j0 + 1);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(is_row_kernel, dim3((unsigned)n_rows), dim3(kIsRowThreads), 0, s, logits, ld, scratch);
  GANK_LAUNCH_OK("inception_score_update (row pass)");
  hipLaunchKernelGGL(is_col_kernel, dim3((unsigned)cdiv(kIsState, kIsColThreads), (unsigned)(j1 - j0 + 1)), dim3(kIsColThreads), 0, s, logits,
                     n_rows, ld, row0, n_total, splits, j0, (const double*)scratch, state);
  GANK_LAUNCH_OK("inception_score_update (column pass)");
  return 0;
}
