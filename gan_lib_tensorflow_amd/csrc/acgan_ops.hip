// Kernels only the ACGAN configuration needs (BASELINE.json config 3; ACGAN/train.py:89-121, ACGAN/model.py:49-90):
//   * the second derivative of train-mode batch normalisation (the WGAN-GP term differentiates the critic's INPUT
//     gradient with respect to the critic's weights, ACGAN/train.py:99-107: every op of the critic is differentiated
//     twice; conv / dense / pooling / leaky-relu compose from their own first-order kernels, batch norm does not);
//   * the moving-statistics update of tf.contrib.layers.batch_norm (common/ops/normalization.py:8-24) as one launch;
//   * the gradient-penalty reduction, the real/fake interpolation, spatial mean and its adjoint, uniform random numbers;
//   * the penalties beside WGAN-GP on the same double backward (one-sided, squared norm, any target) and DRAGAN's perturbed point.
// All HBM / latency bound; 16 bytes per lane where the shape allows.
#include "gank_common.h"

// ---------------------------------------------------------------------------------------------------------------
// batch norm, second order.  First backward (per channel, M = N*HW rows, xh = (x - mu) * s, s = invstd):
//     dx = gamma * s * (dy - mean(dy) - xh * mean(dy * xh))
// Given a = dL/d(dx), this returns  gI = dL/dx,  ggO = dL/d(dy)  and accumulates  gG = dL/dgamma  (the terms of
// upstream gradients with respect to dgamma / dbeta do not occur: the penalty only uses the input gradient).
// With  A0 = sum a, A1 = sum a*(x-mu), G0 = sum dy, G1 = sum dy*(x-mu), AG = sum a*dy :
//     ggO = gamma*s/M * (M*a - A0 - (x-mu)*s^2*A1)
//     gI  = gamma * [ (x-mu)*s^3/M * (A0*G0/M - AG + 3*s^2*G1*A1/M) + A1*s^3/M * (G0/M - dy) + G1*s^3/M * (A0/M - a) ]
//     gG  = s * (AG - A0*G0/M - s^2*A1*G1/M)
// a and dy are not centred: with a mean of order one over 2^18 rows, AG and A0*G0/M agree in their leading five digits,
// and a float running sum of a thousand block partials (atomics, arrival order) alone spent most of the 2e-3 allowed on
// gG.  So a thread's few rows are summed in float, everything above that (row lanes, blocks) in double, and the two
// differences that cancel -- AG - A0*G0/M, and x - mean(x) for a and dy -- are formed in double before they become float.
// ---------------------------------------------------------------------------------------------------------------
__global__ void bn2_zero_kernel(double* __restrict__ p, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 0.0;
}

__global__ __launch_bounds__(256) void bn2_sums_kernel(const bf16* __restrict__ a, const bf16* __restrict__ dy, const bf16* __restrict__ x,
                                                       const float* __restrict__ stats, double* __restrict__ ws, long rows, int C, long rows_per_block) {
  // thread = (8-channel group, row lane); ws [5][C] double (atomics: a few hundred blocks x C adds)
  const int cg = C >> 3, RL = 256 / cg;
  const int g = threadIdx.x % cg, rl = threadIdx.x / cg;
  const long r0 = blockIdx.x * rows_per_block;
  long r1 = r0 + rows_per_block;
  if (r1 > rows) r1 = rows;
  float mu[8], s[5][8];
#pragma unroll
  for (int e = 0; e < 8; e++) {
    mu[e] = stats[g * 8 + e];
#pragma unroll
    for (int k = 0; k < 5; k++) s[k][e] = 0.f;
  }
  if (rl < RL)
    for (long r = r0 + rl; r < r1; r += RL) {
      const bf16x8 va = *reinterpret_cast<const bf16x8*>(a + r * C + g * 8);
      const bf16x8 vg = *reinterpret_cast<const bf16x8*>(dy + r * C + g * 8);
      const bf16x8 vx = *reinterpret_cast<const bf16x8*>(x + r * C + g * 8);
#pragma unroll
      for (int e = 0; e < 8; e++) {
        const float fa = bf2f(va[e]), fg = bf2f(vg[e]), d = bf2f(vx[e]) - mu[e];
        s[0][e] += fa; s[1][e] += fa * d; s[2][e] += fg; s[3][e] += fg * d; s[4][e] += fa * fg;
      }
    }
  __shared__ float red[256 * 8];
  for (int k = 0; k < 5; k++) {
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 8; e++) red[threadIdx.x * 8 + e] = s[k][e];
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
      double t = 0.0;
      for (int l = 0; l < RL; l++) t += (double)red[(l * cg + (c >> 3)) * 8 + (c & 7)];
      atomicAdd(ws + k * C + c, t);
    }
  }
}

__global__ __launch_bounds__(256) void bn2_apply_kernel(const bf16* __restrict__ a, const bf16* __restrict__ dy, const bf16* __restrict__ x,
                                                        const float* __restrict__ gamma, const float* __restrict__ stats, const double* __restrict__ ws,
                                                        bf16* __restrict__ gI, bf16* __restrict__ ggO, float* __restrict__ gG, long rows, int C) {
  const long n8 = rows * (C >> 3);
  const float M = (float)rows;
  const double invM = 1.0 / (double)rows;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    const int c0 = (int)(i % (C >> 3)) * 8;
    const bf16x8 va = *reinterpret_cast<const bf16x8*>(a + i * 8);
    const bf16x8 vg = *reinterpret_cast<const bf16x8*>(dy + i * 8);
    const bf16x8 vx = *reinterpret_cast<const bf16x8*>(x + i * 8);
    bf16x8 oI, oO;
#pragma unroll
    for (int e = 0; e < 8; e++) {
      const int c = c0 + e;
      const float mu = stats[c], s = stats[C + c], gm = gamma[c];
      const double A0 = ws[c], G0 = ws[2 * C + c];
      const float A1 = (float)ws[C + c], G1 = (float)ws[3 * C + c];
      const float cov = (float)(ws[4 * C + c] - A0 * G0 * invM);                          // AG - A0*G0/M
      const float fa = bf2f(va[e]), fg = bf2f(vg[e]), d = bf2f(vx[e]) - mu;
      const float ca = (float)((double)fa - A0 * invM), cg = (float)((double)fg - G0 * invM);   // a - mean(a), dy - mean(dy)
      const float s2 = s * s, s3 = s2 * s;
      oO[e] = f2bf(gm * s * (ca - d * s2 * A1 / M));
      const float all_sub = 3.f * s2 * G1 * A1 / M - cov;
      oI[e] = f2bf(gm * (d * s3 / M * all_sub - A1 * s3 / M * cg - G1 * s3 / M * ca));
    }
    *reinterpret_cast<bf16x8*>(gI + i * 8) = oI;
    *reinterpret_cast<bf16x8*>(ggO + i * 8) = oO;
  }
  if (gG && blockIdx.x == 0)
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
      const float s = stats[C + c];
      gG[c] += s * ((float)(ws[4 * C + c] - ws[c] * ws[2 * C + c] * invM) - s * s * (float)ws[C + c] * (float)ws[3 * C + c] / M);
    }
}

extern "C" int gank_bn_bwd_bwd(const void* ggI, const void* dy, const void* x, const float* gamma, const float* stats, void* gI, void* ggO,
                               float* gG, float* ws, long rows, int C, void* stream) {
  GANK_REQUIRE(ggI && dy && x && gamma && stats && gI && ggO && ws && rows > 0, "bn_bwd_bwd: null pointer");
  GANK_REQUIRE(C % 8 == 0 && C <= 2048 && 256 % (C / 8) == 0, "bn_bwd_bwd: unsupported channel count %d", C);
  hipStream_t s = (hipStream_t)stream;
  GANK_REQUIRE(((size_t)ws & 7) == 0, "bn_bwd_bwd: ws must be 8-byte aligned (it holds 5*C doubles)");
  double* wsd = reinterpret_cast<double*>(ws);
  hipLaunchKernelGGL(bn2_zero_kernel, dim3((5 * C + 255) / 256), dim3(256), 0, s, wsd, 5 * C);
  long blocks = (rows + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  const long rpb = (rows + blocks - 1) / blocks;
  hipLaunchKernelGGL(bn2_sums_kernel, dim3((unsigned)((rows + rpb - 1) / rpb)), dim3(256), 0, s, (const bf16*)ggI, (const bf16*)dy, (const bf16*)x, stats,
                     wsd, rows, C, rpb);
  long ab = (rows * (C / 8) + 255) / 256;
  if (ab > 2048) ab = 2048;
  hipLaunchKernelGGL(bn2_apply_kernel, dim3((unsigned)ab), dim3(256), 0, s, (const bf16*)ggI, (const bf16*)dy, (const bf16*)x, gamma, stats, wsd,
                     (bf16*)gI, (bf16*)ggO, gG, rows, C);
  GANK_LAUNCH_OK("bn_bwd_bwd");
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// tf.contrib.layers.batch_norm moving statistics (decay, zero_debias_moving_mean=True; normalization.py:10-22), one
// launch per call for all towers:  for each tower g in order:
//   moving_variance <- decay*mv + (1-decay) * var_g * n/(n-1);  biased <- decay*biased + (1-decay)*mean_g;
//   local_step += 1;  moving_mean <- biased / (1 - decay^local_step)
// stats [groups][2][C] = (mean, invstd) as the forward kernels leave them; var = 1/invstd^2 - eps.
// ---------------------------------------------------------------------------------------------------------------
__global__ void bn_moving_kernel(const float* __restrict__ stats, float* __restrict__ mm, float* __restrict__ mv, float* __restrict__ biased,
                                 float* __restrict__ step, int C, int groups, float decay, float eps, float unbias) {
  // ONE block: every thread reads local_step before thread 0 rewrites it (barrier in between, no early exit)
  const int c = threadIdx.x;
  float st = step[0];
  if (c < C) {
    float b = biased[c], v = mv[c], m = mm[c];
    for (int g = 0; g < groups; g++) {
      const float mean = stats[(g * 2) * C + c], is = stats[(g * 2 + 1) * C + c];
      v = decay * v + (1.f - decay) * (1.f / (is * is) - eps) * unbias;
      b = decay * b + (1.f - decay) * mean;
      st += 1.f;
      m = b / (1.f - powf(decay, st));
    }
    mm[c] = m; mv[c] = v; biased[c] = b;
  }
  __syncthreads();
  if (c == 0) step[0] = step[0] + (float)groups;
}

extern "C" int gank_bn_moving_update(const float* stats, float* moving_mean, float* moving_var, float* biased, float* local_step, int C,
                                     int groups, long count, float decay, float eps, void* stream) {
  GANK_REQUIRE(stats && moving_mean && moving_var && biased && local_step && C > 0 && groups > 0 && count > 0, "bn_moving_update: bad arguments");
  GANK_REQUIRE(C <= 1024, "bn_moving_update: one block handles all channels (C = %d > 1024)", C);   // one block: step[0] is read before it is written
  const float unbias = count > 1 ? (float)count / (float)(count - 1) : 1.f;
  hipLaunchKernelGGL(bn_moving_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, stats, moving_mean, moving_var, biased, local_step, C, groups,
                     decay, eps, unbias);
  GANK_LAUNCH_OK("bn_moving_update");
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// gradient penalty  lambda * mean_n (sqrt(sum_d g[n,d]^2 + 1e-10) - 1)^2   (ACGAN/train.py:104-106; misc.py WGAN-GP)
// and its derivative with respect to g; one block per sample, then one block sums the per-sample terms.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gp_rows_kernel(const bf16* __restrict__ g, float* __restrict__ pen, float* __restrict__ dg, int N, long D, float lambda) {
  __shared__ float red[16];
  const long n = blockIdx.x;
  float acc = 0.f;
  for (long i = threadIdx.x; i < D; i += blockDim.x) { const float v = bf2f(g[n * D + i]); acc += v * v; }
  const float tot = block_sum(acc, red);
  const float slope = sqrtf(tot + 1e-10f);
  if (threadIdx.x == 0) pen[n] = lambda * (slope - 1.f) * (slope - 1.f) / (float)N;
  const float k = lambda * 2.f * (slope - 1.f) / (slope * (float)N);
  for (long i = threadIdx.x; i < D; i += blockDim.x) dg[n * D + i] = k * bf2f(g[n * D + i]);
}
__global__ __launch_bounds__(256) void sum_small_kernel(const float* __restrict__ v, float* __restrict__ out, int n) {
  __shared__ float red[16];
  float acc = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) acc += v[i];
  const float tot = block_sum(acc, red);
  if (threadIdx.x == 0) out[0] = tot;
}
extern "C" int gank_gp_loss(const void* grad, float* loss, void* dgrad, float* ws, int N, long D, float lambda, void* stream) {
  GANK_REQUIRE(grad && loss && dgrad && ws && N > 0 && D > 0, "gp_loss: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(gp_rows_kernel, dim3(N), dim3(256), 0, s, (const bf16*)grad, ws, (float*)dgrad, N, D, lambda);
  hipLaunchKernelGGL(sum_small_kernel, dim3(1), dim3(256), 0, s, ws, loss, N);
  GANK_LAUNCH_OK("gp_loss");
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// The gradient penalties beside WGAN-GP (the family misc.py:337-352 leaves to the call site).  With
// s_n = sqrt(sum_d g[n,d]^2 + 1e-10):
//   kind 0  two-sided   lambda * mean_n (s_n - target)^2            (Gulrajani et al. 2017; DRAGAN, Kodali et al. 2017)
//   kind 1  one-sided   lambda * mean_n max(0, s_n - target)^2      (WGAN-LP, Petzka et al. 2018): a row at or below the target
//                       contributes exactly 0 and has dgrad exactly 0
//   kind 2  squared     lambda * mean_n sum_d g[n,d]^2              (R1 / R2, Mescheder et al. 2018): no square root, no epsilon,
//                       dgrad = 2 lambda / N * g, so a zero gradient has derivative 0 and not 0/0
// One block per row.  A row of D % 8 == 0, D <= 4096 elements (the trainer's 3072: 384 vectors of 8 on 256 threads) is read once
// into registers, 16 bytes per lane, and dgrad is written from them; any other row takes the looped path, which reads it twice.
// fp32 accumulation in a fixed order (thread-serial, xor butterfly, wave order), no atomics; sum_small_kernel takes the mean.
// ---------------------------------------------------------------------------------------------------------------
#define GPEN_VEC 2                      // 8-element vectors a thread holds on the resident path: rows up to 256 * 8 * GPEN_VEC

__device__ __forceinline__ float gpen_row_term(float tot, float lambda, float target, int kind, int N, float* pen) {
  // -> k with dgrad = k * g; *pen = this row's share of the loss
  if (kind == 2) {
    *pen = lambda * tot / (float)N;
    return 2.f * lambda / (float)N;
  }
  const float slope = sqrtf(tot + 1e-10f);
  const float e = slope - target;
  if (kind == 1 && !(e > 0.f)) {
    *pen = 0.f;
    return 0.f;
  }
  *pen = lambda * e * e / (float)N;
  return lambda * 2.f * e / (slope * (float)N);
}

template <bool RESIDENT>
__global__ __launch_bounds__(256) void grad_penalty_rows_kernel(const bf16* __restrict__ g, float* __restrict__ pen, float* __restrict__ dg, int N, long D,
                                                                float lambda, float target, int kind) {
  __shared__ float red[16];
  const bf16* row = g + (long)blockIdx.x * D;
  float* drow = dg + (long)blockIdx.x * D;
  float acc = 0.f, p = 0.f;
  if (RESIDENT) {                       // D % 8 == 0, D <= 2048 * GPEN_VEC, both rows 16-byte aligned (checked by the caller)
    const int nvec = (int)(D >> 3);
    bf16x8 v[GPEN_VEC];
#pragma unroll
    for (int j = 0; j < GPEN_VEC; j++) {
      const int iv = j * 256 + threadIdx.x;
      if (iv < nvec) {
        v[j] = *reinterpret_cast<const bf16x8*>(row + (long)iv * 8);
#pragma unroll
        for (int e = 0; e < 8; e++) { const float f = bf2f(v[j][e]); acc += f * f; }
      }
    }
    const float k = gpen_row_term(block_sum(acc, red), lambda, target, kind, N, &p);
#pragma unroll
    for (int j = 0; j < GPEN_VEC; j++) {
      const int iv = j * 256 + threadIdx.x;
      if (iv < nvec) {
        f32x4 lo, hi;
#pragma unroll
        for (int e = 0; e < 4; e++) { lo[e] = k * bf2f(v[j][e]); hi[e] = k * bf2f(v[j][4 + e]); }
        *reinterpret_cast<f32x4*>(drow + (long)iv * 8) = lo;
        *reinterpret_cast<f32x4*>(drow + (long)iv * 8 + 4) = hi;
      }
    }
  } else {
    for (long i = threadIdx.x; i < D; i += 256) { const float f = bf2f(row[i]); acc += f * f; }
    const float k = gpen_row_term(block_sum(acc, red), lambda, target, kind, N, &p);
    for (long i = threadIdx.x; i < D; i += 256) drow[i] = k * bf2f(row[i]);
  }
  if (threadIdx.x == 0) pen[blockIdx.x] = p;
}

extern "C" int gank_grad_penalty(const void* grad, float* loss, void* dgrad, float* ws, int N, long D, float lambda, float target, int kind,
                                 void* stream) {
  GANK_REQUIRE(grad && loss && dgrad && ws && N > 0 && D > 0, "grad_penalty: bad arguments");
  GANK_REQUIRE(kind >= 0 && kind <= 2, "grad_penalty: kind %d (0 two-sided, 1 one-sided, 2 squared norm)", kind);
  hipStream_t s = (hipStream_t)stream;
  const bool resident = D % 8 == 0 && D <= 2048L * GPEN_VEC && ((size_t)grad & 15) == 0 && ((size_t)dgrad & 15) == 0;
  if (resident)
    hipLaunchKernelGGL(grad_penalty_rows_kernel<true>, dim3(N), dim3(256), 0, s, (const bf16*)grad, ws, (float*)dgrad, N, D, lambda, target, kind);
  else
    hipLaunchKernelGGL(grad_penalty_rows_kernel<false>, dim3(N), dim3(256), 0, s, (const bf16*)grad, ws, (float*)dgrad, N, D, lambda, target, kind);
  hipLaunchKernelGGL(sum_small_kernel, dim3(1), dim3(256), 0, s, ws, loss, N);
  GANK_LAUNCH_OK("grad_penalty");
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// DRAGAN's penalised point (Kodali et al. 2017): out = real + 0.5 * sigma * u, sigma = the population standard deviation of
// ALL elements of real (x.std() of the original), u in [0, 1) one per element.  sigma never leaves the device:
//   1. block b sums (x - x0) and (x - x0)^2 over its DRAGAN_CHUNK elements in fp32 (x0 = real[0]: the variance does not see
//      the shift, a constant image sums exact zeros, and an image that is nearly constant no longer cancels in E[x^2] - E[x]^2)
//      -> ws[2b], ws[2b + 1]; thread-serial, xor butterfly, wave order: fixed;
//   2. one block adds the partials in double in a fixed order, forms the variance in double -> ws[2 * parts] = sigma;
//   3. out = bf16(real + 0.5 * sigma * u), one rounding; where the perturbation is zero `real` passes through to the bit.
// ---------------------------------------------------------------------------------------------------------------
#define DRAGAN_CHUNK 4096               // elements per fp32 partial: 256 threads x 2 vectors of 8

__global__ __launch_bounds__(256) void dragan_partials_kernel(const bf16* __restrict__ x, float* __restrict__ ws, long total) {
  __shared__ float red[16];
  const float x0 = bf2f(x[0]);
  const long c0 = (long)blockIdx.x * DRAGAN_CHUNK;
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int j = 0; j < DRAGAN_CHUNK / 2048; j++) {
    const long i = c0 + (long)(j * 256 + threadIdx.x) * 8;
    if (i + 8 <= total) {
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(x + i);
#pragma unroll
      for (int e = 0; e < 8; e++) { const float d = bf2f(v[e]) - x0; s1 += d; s2 += d * d; }
    } else {
      for (long q = i; q < total; q++) { const float d = bf2f(x[q]) - x0; s1 += d; s2 += d * d; }
    }
  }
  s1 = block_sum(s1, red);
  s2 = block_sum(s2, red);
  if (threadIdx.x == 0) { ws[2 * (long)blockIdx.x] = s1; ws[2 * (long)blockIdx.x + 1] = s2; }
}

__global__ __launch_bounds__(256) void dragan_sigma_kernel(float* __restrict__ ws, long parts, long total) {
  __shared__ double r1[256], r2[256];
  double a = 0.0, b = 0.0;
  for (long i = threadIdx.x; i < parts; i += 256) { a += (double)ws[2 * i]; b += (double)ws[2 * i + 1]; }
  r1[threadIdx.x] = a;
  r2[threadIdx.x] = b;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t1 = 0.0, t2 = 0.0;
    for (int i = 0; i < 256; i++) { t1 += r1[i]; t2 += r2[i]; }
    const double m = t1 / (double)total;
    const double var = t2 / (double)total - m * m;
    ws[2 * parts] = var > 0.0 ? (float)sqrt(var) : 0.f;
  }
}

__global__ void dragan_apply_kernel(const bf16* __restrict__ x, const float* __restrict__ u, const float* __restrict__ sigma, bf16* __restrict__ out,
                                    long total) {
  const float hs = 0.5f * sigma[0];
  const long nvec = total >> 3;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < nvec; i += (long)gridDim.x * blockDim.x) {
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(x + i * 8);
    const f32x4 ua = *reinterpret_cast<const f32x4*>(u + i * 8), ub = *reinterpret_cast<const f32x4*>(u + i * 8 + 4);
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; e++) {
      const float d = hs * (e < 4 ? ua[e] : ub[e - 4]);
      o[e] = d == 0.f ? v[e] : f2bf(bf2f(v[e]) + d);
    }
    *reinterpret_cast<bf16x8*>(out + i * 8) = o;
  }
  if (blockIdx.x == 0)
    for (long i = nvec * 8 + threadIdx.x; i < total; i += blockDim.x) {
      const float d = hs * u[i];
      out[i] = d == 0.f ? x[i] : f2bf(bf2f(x[i]) + d);
    }
}

extern "C" int gank_dragan_perturb(const void* real, const float* u, void* out, float* ws, long total, void* stream) {
  GANK_REQUIRE(real && u && out && ws && total > 0, "dragan_perturb: bad arguments");
  GANK_REQUIRE(((size_t)real & 15) == 0 && ((size_t)u & 15) == 0 && ((size_t)out & 15) == 0, "dragan_perturb: real, u and out must be 16-byte aligned");
  const long parts = (total + DRAGAN_CHUNK - 1) / DRAGAN_CHUNK;
  GANK_REQUIRE(parts <= 0x7fffffffL, "dragan_perturb: %ld elements are more than one grid of partials holds", total);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(dragan_partials_kernel, dim3((unsigned)parts), dim3(256), 0, s, (const bf16*)real, ws, total);
  hipLaunchKernelGGL(dragan_sigma_kernel, dim3(1), dim3(256), 0, s, ws, parts, total);
  long blocks = ((total >> 3) + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(dragan_apply_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const bf16*)real, u, ws + 2 * parts, (bf16*)out, total);
  GANK_LAUNCH_OK("dragan_perturb");
  return 0;
}

// interpolates = real + alpha[n] * (fake - real)     (ACGAN/train.py:99-101)
__global__ void lerp_rows_kernel(const bf16* __restrict__ real, const bf16* __restrict__ fake, const float* __restrict__ alpha, bf16* __restrict__ out,
                                 long D, long total) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const float a = alpha[i / D], r = bf2f(real[i]);
    out[i] = f2bf(r + a * (bf2f(fake[i]) - r));
  }
}
extern "C" int gank_lerp_rows(const void* real, const void* fake, const float* alpha, void* out, int N, long D, void* stream) {
  GANK_REQUIRE(real && fake && alpha && out && N > 0 && D > 0, "lerp_rows: bad arguments");
  const long total = (long)N * D;
  long blocks = (total + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(lerp_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const bf16*)real, (const bf16*)fake, alpha,
                     (bf16*)out, D, total);
  GANK_LAUNCH_OK("lerp_rows");
  return 0;
}

// y[n,c] = scale * sum_hw x[n,hw,c]  and its adjoint  y[n,hw,c] = scale * g[n,c]     (tf.reduce_mean(axis=[1,2]), model.py:72)
__global__ void sum_hw_kernel(const bf16* __restrict__ x, bf16* __restrict__ y, int HW, int C, float scale, long total) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long n = i / C;
    const int c = (int)(i - n * C);
    float acc = 0.f;
    for (int p = 0; p < HW; p++) acc += bf2f(x[(n * HW + p) * C + c]);
    y[i] = f2bf(acc * scale);
  }
}
__global__ void bcast_hw_kernel(const bf16* __restrict__ g, bf16* __restrict__ y, int HW, int C, float scale, long total) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long n = i / ((long)HW * C);
    const int c = (int)(i % C);
    y[i] = f2bf(bf2f(g[n * C + c]) * scale);
  }
}
extern "C" int gank_sum_hw(const void* x, void* y, int N, int HW, int C, float scale, void* stream) {
  GANK_REQUIRE(x && y && N > 0 && HW > 0 && C > 0, "sum_hw: bad arguments");
  const long total = (long)N * C;
  hipLaunchKernelGGL(sum_hw_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, (bf16*)y, HW, C, scale, total);
  GANK_LAUNCH_OK("sum_hw");
  return 0;
}
extern "C" int gank_bcast_hw(const void* g, void* y, int N, int HW, int C, float scale, void* stream) {
  GANK_REQUIRE(g && y && N > 0 && HW > 0 && C > 0, "bcast_hw: bad arguments");
  const long total = (long)N * HW * C;
  long blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(bcast_hw_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const bf16*)g, (bf16*)y, HW, C, scale, total);
  GANK_LAUNCH_OK("bcast_hw");
  return 0;
}
