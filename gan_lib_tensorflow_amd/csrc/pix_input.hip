// The Pix2Pix input pipeline (Pix2Pix/train.py:135-271, 355-431, 601-660 of the reference) on the device.
//
// pix_load_examples_kernel: the whole of load_examples for a batch in ONE launch -- uint8 -> [0,1], the split into panels,
// preprocess (or rgb_to_lab + preprocess_lab, per SOURCE pixel: the Lab map is not linear, so it comes before the resize),
// the horizontal flip, tf.image.resize_images(ResizeMethod.AREA) to [scale_h, scale_w] and the crop, for input AND target with
// the same (flip, offset_y, offset_x) of the image.  Memory-bound gather: no MFMA.
//
// A workgroup of 256 threads owns R x 32 output pixels of one image (R in {8,4,2,1}: the largest whose footprint fits LDS):
//   (1) the source rows and, per panel, the source columns its outputs overlap are read as DWORDS of the raw uint8 rows
//       (coalesced: consecutive lanes, consecutive words; a row start need not be 4-byte aligned, so the words of a row start
//       at its address rounded down and the residue is remembered) and land in LDS unchanged;
//   (2) one thread per staged pixel turns its 3 bytes per panel into fp32 in the reference's order -- x * (1/255), then
//       x * 2 - 1, or the Lab map -- and stores them channel-interleaved (panel-major) at the pixel's FLIPPED position, so that
//       what follows never sees the flip;
//   (3) one thread per output pixel forms the AREA sums of all Ca + Cb channels from LDS;
//   (4) the R row segments of both outputs leave LDS as 16-byte stores (element stores when a segment is not 16-byte aligned).
// AREA: output y of `out` rows over `in` rows covers [y*in/out, (y+1)*in/out); source row i weighs the length of its overlap
// with that span and the sum is divided by in/out.  The spans are held as INTEGERS in units of 1/out (a = y*in, b = a + in,
// row i = [i*out, (i+1)*out)): the overlap is an exact integer, the weight overlap / in is one fp32 division, weights of a span
// add up to 1 and no index ever leaves the image.  in == out gives weight 1.0 on one pixel: placement is exact.
#include "gank_common.h"

namespace {

constexpr int kPixThreads = 256;
constexpr int kPixTX = 32;                  // output columns per workgroup (32 * C * 2 bytes is a multiple of 16 for every C)
constexpr int kPixMaxC = 9;                 // staged channels: pair 3 + 3, multiple_A 6 + 3, Lab 1 + 2
constexpr int kPixLds = 64 * 1024;
constexpr int kPixMaxDim = 16384;           // (scaled coordinate) * (source extent) stays below 2^31

struct PixPlan {
  int R, rows_max, npx_max, rawpitch;       // rawpitch: words per staged (row, panel)
  int raw_words, st_floats, out_words;
  size_t lds_bytes() const { return 4 * ((size_t)raw_words + st_floats + out_words); }
};

struct PixParams {
  const uint8_t* raw;
  const int* table;
  void* dst_a;                              // receives the first Ca staged channels, dst_b the next Cb
  void* dst_b;
  long long raw_bytes;
  int N, H, Wraw, Wp, P, lab, Ca, Cb, scale_h, scale_w, crop, esz;
  PixPlan plan;
};

bool pix_plan(int H, int Wp, int P, int CT, int scale_h, int scale_w, PixPlan* p) {
  p->npx_max = (int)(((long)kPixTX * Wp + scale_w - 1) / scale_w) + 1;
  p->rawpitch = (p->npx_max * 3 + 3) / 4 + 1;
  for (int R = 8; R >= 1; R >>= 1) {
    p->R = R;
    p->rows_max = (int)(((long)R * H + scale_h - 1) / scale_h) + 1;
    const long raw = (long)p->rows_max * P * p->rawpitch, st = (long)p->rows_max * p->npx_max * CT;
    p->raw_words = (int)((raw + 3) / 4 * 4);          // every region starts 16-byte aligned
    p->st_floats = (int)((st + 3) / 4 * 4);
    p->out_words = R * kPixTX * CT;
    if (4 * (raw + st + 8 + p->out_words) <= kPixLds) return true;
  }
  return false;
}

// ---- colour maps (train.py:178-262), fp32, constants / masks / clip as the reference has them ------------------------------
__device__ __forceinline__ void pix_rgb_to_lab(float r, float g, float b, float& L, float& A, float& B) {
  float c[3] = {r, g, b};
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const float lin = c[i] <= 0.04045f ? 1.f : 0.f, ex = c[i] > 0.04045f ? 1.f : 0.f;
    c[i] = (c[i] / 12.92f * lin) + powf((c[i] + 0.055f) / 1.055f, 2.4f) * ex;
  }
  float t[3] = {c[0] * 0.412453f + c[1] * 0.357580f + c[2] * 0.180423f,
                c[0] * 0.212671f + c[1] * 0.715160f + c[2] * 0.072169f,
                c[0] * 0.019334f + c[1] * 0.119193f + c[2] * 0.950227f};
  t[0] *= (float)(1.0 / 0.950456);
  t[2] *= (float)(1.0 / 1.088754);
  constexpr double eps = 6.0 / 29.0;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const float lin = t[i] <= (float)(eps * eps * eps) ? 1.f : 0.f, ex = t[i] > (float)(eps * eps * eps) ? 1.f : 0.f;
    t[i] = (t[i] / (float)(3.0 * eps * eps) + (float)(4.0 / 29.0)) * lin + cbrtf(t[i]) * ex;
  }
  L = t[1] * 116.f + -16.f;
  A = t[0] * 500.f + t[1] * -500.f;
  B = t[1] * 200.f + t[2] * -200.f;
}

__device__ __forceinline__ void pix_lab_to_rgb(float L, float A, float B, float& r, float& g, float& b) {
  const float l16 = L + 16.f;
  float f[3] = {l16 * (float)(1.0 / 116.0) + A * (float)(1.0 / 500.0), l16 * (float)(1.0 / 116.0),
                l16 * (float)(1.0 / 116.0) + B * (float)(-1.0 / 200.0)};
  constexpr double eps = 6.0 / 29.0;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const float lin = f[i] <= (float)eps ? 1.f : 0.f, ex = f[i] > (float)eps ? 1.f : 0.f;
    f[i] = ((float)(3.0 * eps * eps) * (f[i] - (float)(4.0 / 29.0))) * lin + (f[i] * f[i] * f[i]) * ex;
  }
  f[0] *= 0.950456f;
  f[2] *= 1.088754f;
  float c[3] = {f[0] * 3.2404542f + f[1] * -1.5371385f + f[2] * -0.4985314f,
                f[0] * -0.9692660f + f[1] * 1.8760108f + f[2] * 0.0415560f,
                f[0] * 0.0556434f + f[1] * -0.2040259f + f[2] * 1.0572252f};
#pragma unroll
  for (int i = 0; i < 3; i++) {
    c[i] = fminf(fmaxf(c[i], 0.f), 1.f);
    const float lin = c[i] <= 0.0031308f ? 1.f : 0.f, ex = c[i] > 0.0031308f ? 1.f : 0.f;
    c[i] = (c[i] * 12.92f * lin) + ((powf(c[i], (float)(1.0 / 2.4)) * 1.055f) - 0.055f) * ex;
  }
  r = c[0]; g = c[1]; b = c[2];
}

// deprocess + convert_image_dtype(uint8, saturate=True) (train.py:141-144, 633): scale by max + 0.5, saturate, truncate
__device__ __forceinline__ uint8_t pix_to_u8(float x01) {
  return (uint8_t)(int)fminf(fmaxf(x01 * 255.5f, 0.f), 255.f);
}

__device__ __forceinline__ int pix_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// (4): `nr` row segments of seg_bytes from LDS (pitch lds_pitch bytes) to global rows `g_pitch` bytes apart
__device__ __forceinline__ void pix_store_rows(const unsigned char* lds, int lds_pitch, unsigned char* g, size_t g_pitch, int nr,
                                               int seg_bytes, int esz) {
  const bool vec = (seg_bytes & 15) == 0 && (g_pitch & 15) == 0 && ((uintptr_t)g & 15) == 0;
  if (vec) {
    const int per = seg_bytes >> 4;
    for (int item = threadIdx.x; item < nr * per; item += kPixThreads) {
      const int yy = item / per, q = item - yy * per;
      *(u32x4*)(g + yy * g_pitch + 16 * q) = *(const u32x4*)(lds + yy * lds_pitch + 16 * q);
    }
  } else if (esz == 2) {
    const int per = seg_bytes >> 1;
    for (int item = threadIdx.x; item < nr * per; item += kPixThreads) {
      const int yy = item / per, q = item - yy * per;
      *(unsigned short*)(g + yy * g_pitch + 2 * q) = *(const unsigned short*)(lds + yy * lds_pitch + 2 * q);
    }
  } else {
    const int per = seg_bytes >> 2;
    for (int item = threadIdx.x; item < nr * per; item += kPixThreads) {
      const int yy = item / per, q = item - yy * per;
      *(unsigned*)(g + yy * g_pitch + 4 * q) = *(const unsigned*)(lds + yy * lds_pitch + 4 * q);
    }
  }
}

__global__ __launch_bounds__(kPixThreads) void pix_load_examples_kernel(const PixParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned pix_lds[];
  const PixPlan& pl = p.plan;
  unsigned* rawl = pix_lds;
  float* st = (float*)(pix_lds + pl.raw_words);
  unsigned char* outl = (unsigned char*)(pix_lds + pl.raw_words + pl.st_floats);
  const int tid = threadIdx.x;
  const int n = blockIdx.z, CT = p.Ca + p.Cb, P = p.P;
  const int Y0 = blockIdx.y * pl.R, X0 = blockIdx.x * kPixTX;
  const int nr = min(pl.R, p.crop - Y0), nc = min(kPixTX, p.crop - X0);
  // the table is device memory, so the host cannot refuse a bad row of it: the values are clamped into their ranges here
  const int flip = p.table[3 * n] != 0;
  const int oy = pix_clamp(p.table[3 * n + 1], 0, p.scale_h - p.crop), ox = pix_clamp(p.table[3 * n + 2], 0, p.scale_w - p.crop);
  const int sy0 = Y0 + oy, sx0 = X0 + ox;                                   // in the scaled (and flipped) image
  const int r0 = (sy0 * p.H) / p.scale_h, r1 = ((sy0 + nr) * p.H + p.scale_h - 1) / p.scale_h;
  const int j0 = (sx0 * p.Wp) / p.scale_w, j1 = ((sx0 + nc) * p.Wp + p.scale_w - 1) / p.scale_w;
  const int nrows = r1 - r0, npx = j1 - j0;                                 // <= rows_max, npx_max; r1 <= H, j1 <= Wp
  const int c0 = flip ? p.Wp - j1 : j0;                                     // first source column of a panel

  // (1) raw words
  for (int item = tid; item < nrows * P * pl.rawpitch; item += kPixThreads) {
    const int rp = item / pl.rawpitch, w = item - rp * pl.rawpitch;
    const int row = rp / P, pan = rp - row * P;
    const long long bs = (((long long)n * p.H + r0 + row) * p.Wraw + pan * p.Wp + c0) * 3, be = bs + npx * 3;
    const long long gb = ((bs >> 2) + w) * 4;
    unsigned v = 0;
    if (gb < be) {
      if (gb + 4 <= p.raw_bytes) {
        v = *(const unsigned*)(p.raw + gb);
      } else {                                                              // the last word of the buffer, when its size is not a multiple of 4
        for (int q = 0; q < 4; q++)
          if (gb + q < p.raw_bytes) v |= (unsigned)p.raw[gb + q] << (8 * q);
      }
    }
    rawl[item] = v;
  }
  __syncthreads();

  // (2) bytes -> fp32, flipped into place
  {
    const unsigned char* rawb = (const unsigned char*)rawl;
    for (int item = tid; item < nrows * npx; item += kPixThreads) {
      const int row = item / npx, k = item - row * npx;
      float* o = st + ((size_t)row * npx + (flip ? npx - 1 - k : k)) * CT;
      for (int pan = 0; pan < P; pan++) {
        const long long bs = (((long long)n * p.H + r0 + row) * p.Wraw + pan * p.Wp + c0) * 3;
        const unsigned char* b = rawb + (size_t)(row * P + pan) * pl.rawpitch * 4 + (int)(bs & 3) + 3 * k;
        const float x0 = (float)b[0] * (1.0f / 255.0f), x1 = (float)b[1] * (1.0f / 255.0f), x2 = (float)b[2] * (1.0f / 255.0f);
        if (p.lab) {
          float L, A, B;
          pix_rgb_to_lab(x0, x1, x2, L, A, B);
          o[0] = L / 50.f - 1.f;
          o[1] = A / 110.f;
          o[2] = B / 110.f;
        } else {
          o[3 * pan] = x0 * 2.f - 1.f;
          o[3 * pan + 1] = x1 * 2.f - 1.f;
          o[3 * pan + 2] = x2 * 2.f - 1.f;
        }
      }
    }
  }
  __syncthreads();

  // (3) AREA sums
  const int pitch_a = kPixTX * p.Ca * p.esz, pitch_b = kPixTX * p.Cb * p.esz;
  unsigned char* out_a = outl;
  unsigned char* out_b = outl + pl.R * pitch_a;
  {
    const int yy = tid / kPixTX, xx = tid - yy * kPixTX;
    if (yy < nr && xx < nc) {
      float acc[kPixMaxC];
#pragma unroll
      for (int c = 0; c < kPixMaxC; c++) acc[c] = 0.f;
      const int ay = (sy0 + yy) * p.H, by = ay + p.H, ax = (sx0 + xx) * p.Wp, bx = ax + p.Wp;
      const int i1 = (by + p.scale_h - 1) / p.scale_h, jj1 = (bx + p.scale_w - 1) / p.scale_w;
      const float fh = (float)p.H, fw = (float)p.Wp;
      for (int i = ay / p.scale_h; i < i1; i++) {
        const float wy = (float)(min(by, (i + 1) * p.scale_h) - max(ay, i * p.scale_h)) / fh;
        const float* srow = st + (size_t)(i - r0) * npx * CT;
        for (int j = ax / p.scale_w; j < jj1; j++) {
          const float w = wy * ((float)(min(bx, (j + 1) * p.scale_w) - max(ax, j * p.scale_w)) / fw);
          const float* s = srow + (j - j0) * CT;
#pragma unroll
          for (int c = 0; c < kPixMaxC; c++)
            if (c < CT) acc[c] += w * s[c];
        }
      }
#pragma unroll
      for (int c = 0; c < kPixMaxC; c++) {
        if (c < CT) {
          const bool in_a = c < p.Ca;
          unsigned char* o = in_a ? out_a + yy * pitch_a + (xx * p.Ca + c) * p.esz : out_b + yy * pitch_b + (xx * p.Cb + c - p.Ca) * p.esz;
          if (p.esz == 2) *(bf16*)o = f2bf(acc[c]);
          else *(float*)o = acc[c];
        }
      }
    }
  }
  __syncthreads();

  // (4) stores
  const size_t pix0 = ((size_t)n * p.crop + Y0) * p.crop + X0;
  pix_store_rows(out_a, pitch_a, (unsigned char*)p.dst_a + pix0 * p.Ca * p.esz, (size_t)p.crop * p.Ca * p.esz, nr, nc * p.Ca * p.esz, p.esz);
  pix_store_rows(out_b, pitch_b, (unsigned char*)p.dst_b + pix0 * p.Cb * p.esz, (size_t)p.crop * p.Cb * p.esz, nr, nc * p.Cb * p.esz, p.esz);
}

// ---- elementwise --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pix_rgb_to_lab_kernel(const float* __restrict__ x, float* __restrict__ y, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float L, A, B;
  pix_rgb_to_lab(x[3 * i], x[3 * i + 1], x[3 * i + 2], L, A, B);
  y[3 * i] = L; y[3 * i + 1] = A; y[3 * i + 2] = B;
}

__global__ __launch_bounds__(256) void pix_lab_to_rgb_kernel(const float* __restrict__ x, float* __restrict__ y, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float r, g, b;
  pix_lab_to_rgb(x[3 * i], x[3 * i + 1], x[3 * i + 2], r, g, b);
  y[3 * i] = r; y[3 * i + 1] = g; y[3 * i + 2] = b;
}

template <typename T>
__device__ __forceinline__ float pix_ld(const void* p, long i) { return (float)((const T*)p)[i]; }

// One thread per 4 consecutive output bytes (one dword store; the tail and an unaligned `out` by bytes).  FULL: the window
// is every channel, so the 4 inputs are consecutive too (one 8- or 16-byte load).
template <typename T, bool FULL>
__global__ __launch_bounds__(256) void pix_convert_u8_kernel(const T* __restrict__ x, uint8_t* __restrict__ out, long total, int C, int c0, int Cw,
                                                             int out_aligned, int deprocess) {
  const long e0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (e0 >= total) return;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  const int cnt = total - e0 < 4 ? (int)(total - e0) : 4;
  if (FULL && cnt == 4 && (((uintptr_t)x) & (4 * sizeof(T) - 1)) == 0) {
    struct alignas(4 * sizeof(T)) Q { T a[4]; };
    const Q q = *(const Q*)(x + e0);
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = (float)q.a[k];
  } else {
    for (int k = 0; k < cnt; k++) {
      const long e = e0 + k, px = e / Cw;
      v[k] = (float)x[px * C + c0 + (int)(e - px * Cw)];
    }
  }
  unsigned word = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) word |= (unsigned)pix_to_u8(deprocess ? (v[k] + 1.f) / 2.f : v[k]) << (8 * k);
  if (cnt == 4 && out_aligned) {
    *(unsigned*)(out + e0) = word;
  } else {
    for (int k = 0; k < cnt; k++) out[e0 + k] = (uint8_t)(word >> (8 * k));
  }
}

// augment (train.py:265-271) + convert: brightness [P,1], ab [P,2] -> deprocess_lab -> lab_to_rgb -> uint8 [P,3]
template <typename T>
__global__ __launch_bounds__(256) void pix_augment_u8_kernel(const T* __restrict__ ab, const T* __restrict__ brightness, uint8_t* __restrict__ out, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float L = ((float)brightness[i] + 1.f) / 2.f * 100.f, A = (float)ab[2 * i] * 110.f, B = (float)ab[2 * i + 1] * 110.f;
  float r, g, b;
  pix_lab_to_rgb(L, A, B, r, g, b);
  out[3 * i] = pix_to_u8(r);
  out[3 * i + 1] = pix_to_u8(g);
  out[3 * i + 2] = pix_to_u8(b);
}

}  // namespace

extern "C" int gank_pix2pix_load_examples(const void* raw, int N, int H, int Wraw, int mode, int direction, int scale_h, int scale_w,
                                          int crop, const int* table, void* inputs, void* targets, int out_dtype, void* stream) {
  GANK_REQUIRE(raw && table && inputs && targets, "pix2pix_load_examples: null pointer");
  GANK_REQUIRE(mode >= 0 && mode <= 2, "pix2pix_load_examples: unknown mode %d (0 = pair, 1 = multiple_A, 2 = lab_colorization)", mode);
  GANK_REQUIRE(direction == 0 || direction == 1, "pix2pix_load_examples: unknown direction %d (0 = AtoB, 1 = BtoA)", direction);
  GANK_REQUIRE(out_dtype == 0 || out_dtype == 1, "pix2pix_load_examples: unknown out_dtype %d (0 = 16-bit activation type, 1 = float32)", out_dtype);
  GANK_REQUIRE(N >= 1 && H >= 1 && Wraw >= 1 && crop >= 1, "pix2pix_load_examples: empty batch or image (N=%d H=%d Wraw=%d crop=%d)", N, H, Wraw, crop);
  const int P = mode == 0 ? 2 : (mode == 1 ? 3 : 1);
  GANK_REQUIRE(Wraw % P == 0, "pix2pix_load_examples: raw width %d is not divisible by %d (mode %d splits it into %d panels)", Wraw, P, mode, P);
  GANK_REQUIRE(scale_h >= crop && scale_w >= crop, "pix2pix_load_examples: scale size cannot be less than crop size (scale %d x %d, crop %d)",
               scale_h, scale_w, crop);
  GANK_REQUIRE(H <= kPixMaxDim && Wraw <= kPixMaxDim && scale_h <= kPixMaxDim && scale_w <= kPixMaxDim && N <= 65535,
               "pix2pix_load_examples: sizes above %d (or more than 65535 images)", kPixMaxDim);
  GANK_REQUIRE(((uintptr_t)raw & 3) == 0, "pix2pix_load_examples: raw must be 4-byte aligned");
  PixParams p;
  p.raw = (const uint8_t*)raw; p.table = table;
  p.N = N; p.H = H; p.Wraw = Wraw; p.Wp = Wraw / P; p.P = P; p.lab = mode == 2;
  p.Ca = mode == 0 ? 3 : (mode == 1 ? 6 : 1);
  p.Cb = mode == 2 ? 2 : 3;
  p.dst_a = direction == 0 ? inputs : targets;
  p.dst_b = direction == 0 ? targets : inputs;
  p.raw_bytes = (long long)N * H * Wraw * 3;
  p.scale_h = scale_h; p.scale_w = scale_w; p.crop = crop; p.esz = out_dtype == 0 ? 2 : 4;
  GANK_REQUIRE(pix_plan(H, p.Wp, P, p.Ca + p.Cb, scale_h, scale_w, &p.plan),
               "pix2pix_load_examples: a %d x %d panel to %d x %d needs more than %d bytes of LDS per output row", H, p.Wp, scale_h, scale_w, kPixLds);
  const dim3 grid(cdiv(crop, kPixTX), cdiv(crop, p.plan.R), N);
  GANK_REQUIRE(grid.y <= 65535, "pix2pix_load_examples: crop %d too large", crop);
  hipLaunchKernelGGL(pix_load_examples_kernel, grid, dim3(kPixThreads), p.plan.lds_bytes(), (hipStream_t)stream, p);
  GANK_LAUNCH_OK("pix2pix_load_examples");
  return 0;
}

extern "C" int gank_rgb_to_lab(const float* srgb, float* lab, long pixels, void* stream) {
  GANK_REQUIRE(srgb && lab, "rgb_to_lab: null pointer");
  GANK_REQUIRE(pixels >= 1 && pixels < (1L << 37), "rgb_to_lab: %ld pixels", pixels);
  hipLaunchKernelGGL(pix_rgb_to_lab_kernel, dim3((unsigned)cdiv(pixels, 256)), dim3(256), 0, (hipStream_t)stream, srgb, lab, pixels);
  GANK_LAUNCH_OK("rgb_to_lab");
  return 0;
}

extern "C" int gank_lab_to_rgb(const float* lab, float* srgb, long pixels, void* stream) {
  GANK_REQUIRE(lab && srgb, "lab_to_rgb: null pointer");
  GANK_REQUIRE(pixels >= 1 && pixels < (1L << 37), "lab_to_rgb: %ld pixels", pixels);
  hipLaunchKernelGGL(pix_lab_to_rgb_kernel, dim3((unsigned)cdiv(pixels, 256)), dim3(256), 0, (hipStream_t)stream, lab, srgb, pixels);
  GANK_LAUNCH_OK("lab_to_rgb");
  return 0;
}

extern "C" int gank_pix2pix_convert_u8(const void* x, const void* brightness, int in_dtype, long pixels, int C, int c0, int Cw, int deprocess,
                                       void* out_u8, void* stream) {
  uint8_t* out = (uint8_t*)out_u8;
  GANK_REQUIRE(x && out, "pix2pix_convert_u8: null pointer");
  GANK_REQUIRE(in_dtype == 0 || in_dtype == 1, "pix2pix_convert_u8: unknown in_dtype %d (0 = 16-bit activation type, 1 = float32)", in_dtype);
  GANK_REQUIRE(pixels >= 1 && pixels < (1L << 37), "pix2pix_convert_u8: %ld pixels", pixels);
  hipStream_t s = (hipStream_t)stream;
  if (brightness) {
    GANK_REQUIRE(C == 2 && c0 == 0 && Cw == 3, "pix2pix_convert_u8: with a brightness operand x is the 2-channel ab tensor and the output has 3 channels "
                 "(C=%d c0=%d Cw=%d)", C, c0, Cw);
    const dim3 grid((unsigned)cdiv(pixels, 256));
    if (in_dtype == 0) hipLaunchKernelGGL(pix_augment_u8_kernel<bf16>, grid, dim3(256), 0, s, (const bf16*)x, (const bf16*)brightness, out, pixels);
    else hipLaunchKernelGGL(pix_augment_u8_kernel<float>, grid, dim3(256), 0, s, (const float*)x, (const float*)brightness, out, pixels);
  } else {
    GANK_REQUIRE(C >= 1 && Cw >= 1 && c0 >= 0 && c0 + Cw <= C, "pix2pix_convert_u8: channel window [%d, %d) outside the %d channels", c0, c0 + Cw, C);
    const long total = pixels * Cw;
    const dim3 grid((unsigned)cdiv(cdiv(total, 4), 256));
    const int al = ((uintptr_t)out & 3) == 0;
    const bool full = Cw == C;
    if (in_dtype == 0) {
      if (full) hipLaunchKernelGGL((pix_convert_u8_kernel<bf16, true>), grid, dim3(256), 0, s, (const bf16*)x, out, total, C, c0, Cw, al, deprocess);
      else hipLaunchKernelGGL((pix_convert_u8_kernel<bf16, false>), grid, dim3(256), 0, s, (const bf16*)x, out, total, C, c0, Cw, al, deprocess);
    } else {
      if (full) hipLaunchKernelGGL((pix_convert_u8_kernel<float, true>), grid, dim3(256), 0, s, (const float*)x, out, total, C, c0, Cw, al, deprocess);
      else hipLaunchKernelGGL((pix_convert_u8_kernel<float, false>), grid, dim3(256), 0, s, (const float*)x, out, total, C, c0, Cw, al, deprocess);
    }
  }
  GANK_LAUNCH_OK("pix2pix_convert_u8");
  return 0;
}
