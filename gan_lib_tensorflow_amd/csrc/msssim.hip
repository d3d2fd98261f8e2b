// One pyramid level of MS-SSIM (common/msssim.py:50-123 per level, :181-183 between levels) for a whole batch of image
// pairs in ONE launch: Gaussian-windowed moments (separable VALID blur of x, y, x^2, y^2, xy), the ssim and cs maps, their
// per-image sums, and the 2x2-mean-pooled pair that feeds the next level.  No MFMA: the kernel is LDS- and VALU-bound.
//
// A workgroup of 256 threads serves `G` image slots (G = 2^glog, T = 256 / G threads per slot):
//   - large images (regime A): G = 1 and the slot is one 16 x 32-pixel tile of output positions of one image, for one chunk
//     of at most 4 channels; grid = images x tiles;
//   - small images (regime B: H, W <= 32 and C <= 4): the slot is a WHOLE image and a workgroup takes up to 64 images,
//     so the 4x4 / 2x2 / 1x1 levels of a 25 000-pair batch are a few hundred workgroups and not 25 000 near-empty ones.
// Per slot: (1) both images' tile with its size-1 halo goes into LDS once, as fp32 with the constant `offset` (max_val / 2)
// subtracted -- the variances and the covariance are shift invariant, and E[x^2] - mu^2 cancels far less around 0 than around
// 250; the offset goes back onto mu only; (2) the horizontal pass writes five LDS planes; (3) the vertical pass reads them in
// strips of 4 output rows per thread, forms ssim and cs in registers and accumulates them per thread; (4) the 2x2 means are
// written from the staged tile (the last row / column is replicated when H / W is odd: scipy's 'reflect' on a 2-tap window);
// (5) the slot's T threads reduce with cross-lane butterflies, waves through LDS, and ONE thread stores the slot's two fp32
// partial sums.  Nothing else goes back to memory: no blurred map is materialised, and there are no atomics -- the order of
// every addition is fixed, so two calls give the same bits.  The per-image sum over tiles is the caller's (float64, fixed order).
#include "gank_common.h"

namespace {

constexpr int kMsThreads = 256;
constexpr int kMsMaxSize = 11;
constexpr int kMsTileH = 16, kMsTileW = 32, kMsChunk = 4;   // regime A tile (output positions; both even: 2x2 pooling windows never straddle two tiles)
constexpr int kMsSmall = 32;                                 // regime B: whole images up to kMsSmall x kMsSmall x kMsChunk
constexpr int kMsRed = 16;                                   // floats of reduction scratch in front of the slots
constexpr int kMsRows = 4;                                   // output rows per thread of the vertical pass

struct MsPlan {
  int th, tw;                  // tile extent in output positions
  int tiles_y, tiles_x, nchunk, cc;
  int glog;                    // log2(image slots per workgroup)
  int rows_max, pitch_in, pitch_h, slot_floats;
  int tiles() const { return tiles_y * tiles_x * nchunk; }
  size_t lds_bytes() const { return sizeof(float) * ((size_t)kMsRed + ((size_t)slot_floats << glog)); }
};

struct MsParams {
  const void* a;
  const void* b;
  float* pool_a;
  float* pool_b;
  float* part;
  int N, H, W, C, size, dtype;
  MsPlan plan;
  float c1, c2, offset;
  float taps[kMsMaxSize];
};

bool ms_plan(int H, int W, int C, int size, MsPlan* p) {
  if (size < 1 || size > kMsMaxSize || C < 1 || H < size || W < size) return false;
  const int Ho = H - size + 1, Wo = W - size + 1;
  const bool small = H <= kMsSmall && W <= kMsSmall && C <= kMsChunk;
  p->th = small ? Ho : kMsTileH;
  p->tw = small ? Wo : kMsTileW;
  p->tiles_y = cdiv(Ho, p->th);
  p->tiles_x = cdiv(Wo, p->tw);
  p->cc = C < kMsChunk ? C : kMsChunk;
  p->nchunk = cdiv(C, p->cc);
  p->rows_max = (p->th + size - 1 < H) ? p->th + size - 1 : H;
  const int cols_max = (p->tw + size - 1 < W) ? p->tw + size - 1 : W;
  p->pitch_in = cols_max * p->cc;
  p->pitch_h = (p->tw < Wo ? p->tw : Wo) * p->cc;
  p->slot_floats = 2 * p->rows_max * p->pitch_in + 5 * p->rows_max * p->pitch_h;
  p->glog = 0;
  if (small)
    while (p->glog < 6 && ((size_t)p->slot_floats << (p->glog + 1)) * sizeof(float) <= 60 * 1024) p->glog++;
  return true;
}

// n / d for n * d < 2^32 with m = ceil(2^32 / d) (d >= 2; d == 1 is passed through)
__device__ __forceinline__ unsigned ms_magic(unsigned d) { return d > 1 ? 0xFFFFFFFFu / d + 1u : 0u; }
__device__ __forceinline__ unsigned ms_div(unsigned n, unsigned d, unsigned m) { return d > 1 ? __umulhi(n, m) : n; }

template <int SIZE>      // SIZE = 11: the full window, unrolled; 0: the window size of the launch (small levels, other filter sizes)
__global__ __launch_bounds__(kMsThreads) void msssim_level_kernel(const MsParams p) {
  extern __shared__ __attribute__((aligned(16))) float ms_lds[];
  const MsPlan& pl = p.plan;
  const int size = SIZE ? SIZE : p.size;
  const int tid = threadIdx.x;
  const int T = kMsThreads >> pl.glog;          // threads per image slot
  const int g = tid >> (8 - pl.glog), lt = tid & (T - 1);
  const int tiles = pl.tiles_y * pl.tiles_x * pl.nchunk;
  const int bimg = blockIdx.x / tiles, tile = blockIdx.x - bimg * tiles;
  const int img = (bimg << pl.glog) + g;
  const bool live = img < p.N;                  // the last workgroup of regime B may hold empty slots: they only meet the barriers
  const int t2 = tile / pl.nchunk, chunk = tile - t2 * pl.nchunk;
  const int ty = t2 / pl.tiles_x, tx = t2 - ty * pl.tiles_x;
  const int c0 = chunk * pl.cc, ccn = (p.C - c0 < pl.cc) ? p.C - c0 : pl.cc;
  const int H = p.H, W = p.W, C = p.C;
  const int Ho = H - size + 1, Wo = W - size + 1;
  const int oy0 = ty * pl.th, ox0 = tx * pl.tw;
  const int oh = (Ho - oy0 < pl.th) ? Ho - oy0 : pl.th, ow = (Wo - ox0 < pl.tw) ? Wo - ox0 : pl.tw;
  const int rows = oh + size - 1, cols = ow + size - 1;     // staged pixels: the last tile of an axis reaches row H-1 / column W-1
  const int we = cols * ccn, owe = ow * ccn;                // staged / output elements per row
  float* s1 = ms_lds + kMsRed + (size_t)g * pl.slot_floats;
  float* s2 = s1 + pl.rows_max * pl.pitch_in;
  float* hp = s2 + pl.rows_max * pl.pitch_in;               // five planes [rows][pitch_h]
  const int plane = pl.rows_max * pl.pitch_h;
  float k[kMsMaxSize];
#pragma unroll
  for (int t = 0; t < kMsMaxSize; t++) k[t] = p.taps[t];

  // (1) stage
  if (live) {
    const unsigned m_we = ms_magic(we), m_cc = ms_magic(ccn);
    const size_t img_off = (size_t)img * H * W * C;
    for (int item = lt; item < rows * we; item += T) {
      const int r = ms_div(item, we, m_we), e = item - r * we;
      size_t src;
      if (ccn == C) {
        src = img_off + ((size_t)(oy0 + r) * W + ox0) * C + e;
      } else {
        const int px = ms_div(e, ccn, m_cc), c = e - px * ccn;
        src = img_off + ((size_t)(oy0 + r) * W + ox0 + px) * C + c0 + c;
      }
      float x, y;
      if (p.dtype == 0) {
        x = (float)((const uint8_t*)p.a)[src];
        y = (float)((const uint8_t*)p.b)[src];
      } else {
        x = ((const float*)p.a)[src];
        y = ((const float*)p.b)[src];
      }
      s1[r * pl.pitch_in + e] = x - p.offset;
      s2[r * pl.pitch_in + e] = y - p.offset;
    }
  }
  __syncthreads();

  // (2) horizontal pass: five moments per staged row and output column
  if (live) {
    const unsigned m_owe = ms_magic(owe);
    for (int item = lt; item < rows * owe; item += T) {
      const int r = ms_div(item, owe, m_owe), e = item - r * owe;
      const float* x1 = s1 + r * pl.pitch_in + e;
      const float* x2 = s2 + r * pl.pitch_in + e;
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
#pragma unroll
      for (int t = 0; t < kMsMaxSize; t++) {
        if (t < size) {
          const float x = x1[t * ccn], y = x2[t * ccn];
          a0 = fmaf(k[t], x, a0);
          a1 = fmaf(k[t], y, a1);
          a2 = fmaf(k[t], x * x, a2);
          a3 = fmaf(k[t], y * y, a3);
          a4 = fmaf(k[t], x * y, a4);
        }
      }
      float* o = hp + r * pl.pitch_h + e;
      o[0] = a0;
      o[plane] = a1;
      o[2 * plane] = a2;
      o[3 * plane] = a3;
      o[4 * plane] = a4;
    }

    // (4) the next level's pair, from the staged tile: out[i][j] = mean(x[2i..2i+1][2j..2j+1]), indices clamped to the image.
    // The tile owns the pooled pixels whose top-left input pixel lies in its th x tw block (the last tile: to the image's edge).
    if (p.pool_a) {
      const int Hp = (H + 1) / 2, Wp = (W + 1) / 2;
      const int i0 = oy0 / 2, i1 = (ty == pl.tiles_y - 1) ? Hp : (oy0 + pl.th) / 2;
      const int j0 = ox0 / 2, j1 = (tx == pl.tiles_x - 1) ? Wp : (ox0 + pl.tw) / 2;
      const int rowe = (j1 - j0) * ccn;
      const unsigned m_rowe = ms_magic(rowe), m_cc = ms_magic(ccn);
      const int per = (i1 - i0) * rowe;
      for (int item = lt; item < 2 * per; item += T) {
        const int which = item >= per, it = item - which * per;
        const int ii = ms_div(it, rowe, m_rowe), e = it - ii * rowe;
        const int jj = ms_div(e, ccn, m_cc), c = e - jj * ccn;
        const int i = i0 + ii, j = j0 + jj;
        const int ra = 2 * i - oy0, rb = ((2 * i + 1 < H) ? 2 * i + 1 : H - 1) - oy0;
        const int ca = 2 * j - ox0, cb = ((2 * j + 1 < W) ? 2 * j + 1 : W - 1) - ox0;
        const float* s = which ? s2 : s1;
        const float v = 0.25f * ((s[ra * pl.pitch_in + ca * ccn + c] + s[ra * pl.pitch_in + cb * ccn + c]) +
                                 (s[rb * pl.pitch_in + ca * ccn + c] + s[rb * pl.pitch_in + cb * ccn + c])) + p.offset;
        (which ? p.pool_b : p.pool_a)[(((size_t)img * Hp + i) * Wp + j) * C + c0 + c] = v;
      }
    }
  }
  __syncthreads();

  // (3) vertical pass in strips of kMsRows output rows, ssim and cs per output element, per-thread sums
  float sum_ssim = 0.f, sum_cs = 0.f;
  if (live) {
    const unsigned m_owe = ms_magic(owe);
    const int strips = (oh + kMsRows - 1) / kMsRows;
    for (int item = lt; item < strips * owe; item += T) {
      const int sb = ms_div(item, owe, m_owe), e = item - sb * owe;
      const int r0 = sb * kMsRows;
      float acc[kMsRows][5];
#pragma unroll
      for (int q = 0; q < kMsRows; q++)
#pragma unroll
        for (int m = 0; m < 5; m++) acc[q][m] = 0.f;
      const float* col = hp + r0 * pl.pitch_h + e;
#pragma unroll
      for (int j = 0; j < kMsMaxSize + kMsRows - 1; j++) {
        if (j < size + kMsRows - 1 && r0 + j < rows) {
          float v[5];
#pragma unroll
          for (int m = 0; m < 5; m++) v[m] = col[m * plane + j * pl.pitch_h];
#pragma unroll
          for (int q = 0; q < kMsRows; q++) {
            const int t = j - q;
            if (t >= 0 && t < kMsMaxSize && t < size) {
#pragma unroll
              for (int m = 0; m < 5; m++) acc[q][m] = fmaf(k[t], v[m], acc[q][m]);
            }
          }
        }
      }
#pragma unroll
      for (int q = 0; q < kMsRows; q++) {
        if (r0 + q < oh) {
          const float m1 = acc[q][0], m2 = acc[q][1];
          const float s11 = acc[q][2] - m1 * m1, s22 = acc[q][3] - m2 * m2, s12 = acc[q][4] - m1 * m2;
          const float mu1 = m1 + p.offset, mu2 = m2 + p.offset;
          const float v1 = 2.0f * s12 + p.c2, v2 = s11 + s22 + p.c2;
          sum_cs += v1 / v2;
          sum_ssim += ((2.0f * (mu1 * mu2) + p.c1) * v1) / ((mu1 * mu1 + mu2 * mu2 + p.c1) * v2);
        }
      }
    }
  }

  // (5) reduce over the slot's T threads: butterflies inside the wave, waves through LDS, one store per slot
  const int span = T < 64 ? T : 64;
  for (int o = span >> 1; o > 0; o >>= 1) {
    sum_ssim += __shfl_xor(sum_ssim, o, 64);
    sum_cs += __shfl_xor(sum_cs, o, 64);
  }
  if (T > 64) {                                   // glog < 2: one or two slots of 4 or 2 waves
    const int w = tid >> 6;
    if ((tid & 63) == 0) { ms_lds[2 * w] = sum_ssim; ms_lds[2 * w + 1] = sum_cs; }
    __syncthreads();
    if (lt == 0) {
      const int nw = T >> 6, w0 = g * nw;
      sum_ssim = 0.f; sum_cs = 0.f;
      for (int i = 0; i < nw; i++) { sum_ssim += ms_lds[2 * (w0 + i)]; sum_cs += ms_lds[2 * (w0 + i) + 1]; }
    }
  }
  if (live && lt == 0) {
    float* out = p.part + ((size_t)img * tiles + tile) * 2;
    out[0] = sum_ssim;
    out[1] = sum_cs;
  }
}

}  // namespace

extern "C" int gank_msssim_level_parts(int H, int W, int C, int size) {
  MsPlan pl;
  if (!ms_plan(H, W, C, size, &pl)) {
    gank_set_error("msssim_level_parts: unsupported H=%d W=%d C=%d size=%d (1 <= size <= %d, C >= 1, H and W >= size)", H, W, C, size, kMsMaxSize);
    return 0;
  }
  return pl.tiles();
}

extern "C" int gank_msssim_level(const void* img1, const void* img2, int dtype, int N, int H, int W, int C, int size, const float* taps,
                                 float c1, float c2, float offset, float* part, float* pool1, float* pool2, void* stream) {
  GANK_REQUIRE(img1 && img2 && taps && part, "msssim_level: null pointer");
  GANK_REQUIRE((pool1 != nullptr) == (pool2 != nullptr), "msssim_level: pool1 and pool2 go together (both or neither)");
  GANK_REQUIRE(dtype == 0 || dtype == 1, "msssim_level: unknown input dtype code %d (0 = uint8, 1 = float32)", dtype);
  GANK_REQUIRE(size >= 1 && size <= kMsMaxSize, "msssim_level: window size %d outside 1..%d", size, kMsMaxSize);
  GANK_REQUIRE(C >= 1, "msssim_level: C = %d, needs at least one channel", C);
  GANK_REQUIRE(N >= 1 && H >= 1 && W >= 1, "msssim_level: empty batch or image (N=%d H=%d W=%d)", N, H, W);
  GANK_REQUIRE(H >= size && W >= size, "msssim_level: image %d x %d smaller than the window %d (VALID blur)", H, W, size);
  GANK_REQUIRE((long)N * H * W * C < (1L << 40), "msssim_level: batch too large");
  MsParams p;
  GANK_REQUIRE(ms_plan(H, W, C, size, &p.plan), "msssim_level: unsupported shape");
  p.a = img1; p.b = img2; p.pool_a = pool1; p.pool_b = pool2; p.part = part;
  p.N = N; p.H = H; p.W = W; p.C = C; p.size = size; p.dtype = dtype;
  p.c1 = c1; p.c2 = c2; p.offset = offset;
  for (int t = 0; t < kMsMaxSize; t++) p.taps[t] = t < size ? taps[t] : 0.f;
  const size_t lds = p.plan.lds_bytes();
  GANK_REQUIRE(lds <= 160 * 1024, "msssim_level: tile needs %zu bytes of LDS", lds);
  const long groups = (long)cdiv(N, 1 << p.plan.glog) * p.plan.tiles();
  GANK_REQUIRE(groups < (1L << 31), "msssim_level: %ld workgroups", groups);
  hipStream_t s = (hipStream_t)stream;
  if (size == kMsMaxSize) {
    GANK_MAX_DYNAMIC_LDS(msssim_level_kernel<kMsMaxSize>, 160 * 1024, "msssim_level");
    hipLaunchKernelGGL(msssim_level_kernel<kMsMaxSize>, dim3((unsigned)groups), dim3(kMsThreads), lds, s, p);
  } else {
    GANK_MAX_DYNAMIC_LDS(msssim_level_kernel<0>, 160 * 1024, "msssim_level");
    hipLaunchKernelGGL(msssim_level_kernel<0>, dim3((unsigned)groups), dim3(kMsThreads), lds, s, p);
  }
  GANK_LAUNCH_OK("msssim_level");
  return 0;
}
