// Projection discriminator head (Miyato & Koyama, cGANs with Projection Discriminator):
//   logit[n] = <x[n], w> + b + <x[n], E[y_n]> = sum_k x[n][k] * (w[k] + E[y_n][k]) + b
// on the pooled critic features x [M,K] (bf16), the normalised D.Output weight w [K] and the normalised label table E [V,K]
// (fp32).  Three entry points share ONE kernel, so the logits and dx of the fused launch are the bits of the unfused ones:
//   gank_proj_head_fwd            logits
//   gank_proj_head_bwd            dx and the accumulated w / b / E gradients from an arbitrary upstream dl
//   gank_proj_head_hinge_scaled   logits + hinge loss + its derivative + the four gradients (gank_critic_head_hinge_scaled's
//                                 conventions)
// A latency-bound head (M a few hundred, K = 128, V = 10): one workgroup of 16 wave64 waves, every sum in a fixed order
// through registers and LDS, no float atomics -- two runs give the same bits.
#include "gank_common.h"

#define PH_FWD 1      // logits
#define PH_HINGE 2    // hinge loss of the logits and its derivative (needs PH_FWD)
#define PH_BWD 4      // dx, w_grad, b_grad, e_grad

#define PH_MAX_M 1024
#define PH_MAX_K 1024
#define PH_MAX_V 256

// the coefficient of x[n][k] in the logit: ONE fp32 addition (a label outside [0, V) reads a zero row, as gank_embedding_fwd)
__device__ __forceinline__ float proj_coef(const float* __restrict__ s_w, const float* __restrict__ e_row, int k) {
  return s_w[k] + (e_row ? e_row[k] : 0.f);
}

static size_t proj_head_lds_floats(int M, int K, int V) {
  // dl[M] | label[M] | list[M] | w[K] | red[32] | off[V+1], cnt[V] (rounded to 4) | part[8][K]
  return (size_t)3 * M + K + 32 + (size_t)((2 * V + 1 + 3) & ~3) + (size_t)8 * K;
}

__global__ __launch_bounds__(1024) void proj_head_kernel(const bf16* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                        const float* __restrict__ E, const int* __restrict__ labels, bf16* __restrict__ logits,
                                                        const bf16* __restrict__ dl_in, float* __restrict__ loss, bf16* __restrict__ dx,
                                                        float* __restrict__ w_grad, float* __restrict__ b_grad, float* __restrict__ e_grad, int M,
                                                        int K, int V, int n_real, int mode, float loss_scale, int what) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* s_dl = sm;                                   // [M] d loss / d logit, as the 16-bit value it is handed on as
  int* s_lab = reinterpret_cast<int*>(sm + M);        // [M] label, -1 where it is outside [0, V)
  int* s_list = s_lab + M;                            // [M] the rows sorted by label, increasing row index inside a label
  float* s_w = sm + 3 * (size_t)M;                    // [K]
  float* red = s_w + K;                               // [32]
  int* s_off = reinterpret_cast<int*>(red + 32);      // [V + 1] first list entry of a label
  int* s_cnt = s_off + V + 1;                         // [V]
  float* part = red + 32 + ((2 * V + 1 + 3) & ~3);    // [8][K]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nw = blockDim.x >> 6;
  for (int k = tid; k < K; k += blockDim.x) s_w[k] = w[k];
  for (int m = tid; m < M; m += blockDim.x) {
    const int r = labels[m];
    s_lab[m] = (r >= 0 && r < V) ? r : -1;
    if (!(what & PH_FWD)) s_dl[m] = bf2f(dl_in[m]);
  }
  __syncthreads();
  if (what & PH_FWD) {
    const float bias = b ? b[0] : 0.f;
    const int n_fake = M - n_real;
    float acc = 0.f;
    // one wave per row, 8 rows in flight.  Association of a logit (include/gank.h): lane l sums its products
    // x[m][k] * (w[k] + E[y][k]) for k = l, l + 64, ... in increasing k; the 64 lane sums meet in the xor butterfly of wave_sum
    // (offsets 32, 16, .., 1); the bias is added last; one rounding to 16 bits.
    for (int mb = wv; mb < M; mb += 8 * nw) {
      float tt[8];
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const int m = mb + u * nw;
        float t = 0.f;
        if (m < M) {
          const int y = s_lab[m];
          const float* e_row = y >= 0 ? E + (long)y * K : nullptr;
          for (int k = lane; k < K; k += 64) t += bf2f(x[(long)m * K + k]) * proj_coef(s_w, e_row, k);
        }
        tt[u] = t;
      }
#pragma unroll
      for (int u = 0; u < 8; u++) tt[u] = wave_sum(tt[u]);
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const int m = mb + u * nw;
        if (lane == 0 && m < M) {
          const bf16 lg = f2bf(tt[u] + bias);
          logits[m] = lg;
          if (what & PH_HINGE) {          // the arithmetic of critic_head_hinge_kernel (loss_opt.hip)
            const float v = bf2f(lg);
            float d, l;
            if (mode == 1) { l = -v / (float)M; d = -1.f / (float)M; }
            else if (m < n_real) { const float q = 1.f - v; l = fmaxf(q, 0.f) / (float)n_real; d = q > 0.f ? -1.f / (float)n_real : 0.f; }
            else { const float q = 1.f + v; l = fmaxf(q, 0.f) / (float)n_fake; d = q > 0.f ? 1.f / (float)n_fake : 0.f; }
            s_dl[m] = bf2f(f2bf(d * loss_scale));
            acc += l;
          }
        }
      }
    }
    if (what & PH_HINGE) {
      if (lane != 0) acc = 0.f;
      acc = wave_sum(acc);
      if (lane == 0) red[wv] = acc;
      __syncthreads();
      if (tid == 0) {
        float t = 0.f;
        for (int i = 0; i < nw; i++) t += red[i];
        loss[0] = t;
      }
    }
  }
  if (!(what & PH_BWD)) return;
  __syncthreads();                                    // s_dl is complete
  // d logit / d x = dl[m] * (w[k] + E[y_m][k]): the coefficient of the forward pass, one product, one rounding
  if (dx)
    for (long i = tid; i < (long)M * K; i += blockDim.x) {
      const int m = (int)(i / K), k = (int)(i - (long)m * K);
      const int y = s_lab[m];
      dx[i] = f2bf(s_dl[m] * proj_coef(s_w, y >= 0 ? E + (long)y * K : nullptr, k));
    }
  // w_grad[k] += sum_m x[m][k] dl[m]: the rows in 8 slices per column, each summed in increasing m, the 8 partial sums added
  // in slice order (critic_head_hinge_kernel's scheme)
  if (w_grad) {
    const int nsl = 8, per = (M + nsl - 1) / nsl;
    for (int i = tid; i < nsl * K; i += blockDim.x) {
      const int sl = i / K, k = i - sl * K;
      const int m0 = sl * per, m1 = min(M, m0 + per);
      float t = 0.f;
      for (int m = m0; m < m1; m++) t += bf2f(x[(long)m * K + k]) * s_dl[m];
      part[i] = t;
    }
    __syncthreads();
    for (int k = tid; k < K; k += blockDim.x) {
      float t = 0.f;
#pragma unroll
      for (int sl = 0; sl < 8; sl++) t += part[sl * K + k];
      w_grad[k] += t;
    }
  }
  // b_grad += sum_m dl[m]: lane l of the first wave sums m = l, l + 64, ..; xor butterfly
  if (b_grad && tid < 64) {
    float t = 0.f;
    for (int m = tid; m < M; m += 64) t += s_dl[m];
    t = wave_sum(t);
    if (tid == 0) b_grad[0] += t;
  }
  // e_grad[v][k] += sum_{m: y_m = v} x[m][k] dl[m] in increasing m.  The rows of a label come from a stable counting sort:
  // a wave per label counts its rows by ballots over 64-row groups, one thread turns the counts into offsets, the same
  // ballots place the rows.  A label that no row carries owns no list entries: its row of e_grad is neither read nor written.
  if (e_grad) {
    for (int v = wv; v < V; v += nw) {
      int cnt = 0;
      for (int m0 = 0; m0 < M; m0 += 64) {
        const int m = m0 + lane;
        cnt += __popcll(__ballot(m < M && s_lab[m] == v));
      }
      if (lane == 0) s_cnt[v] = cnt;
    }
    __syncthreads();
    if (tid == 0) {
      int o = 0;
      for (int v = 0; v < V; v++) { s_off[v] = o; o += s_cnt[v]; }
      s_off[V] = o;
    }
    __syncthreads();
    for (int v = wv; v < V; v += nw) {
      int pos = s_off[v];
      for (int m0 = 0; m0 < M; m0 += 64) {
        const int m = m0 + lane;
        const bool hit = m < M && s_lab[m] == v;
        const unsigned long long mask = __ballot(hit);
        if (hit) s_list[pos + __popcll(mask & ((1ull << lane) - 1ull))] = m;
        pos += __popcll(mask);
      }
    }
    __syncthreads();
    for (long i = tid; i < (long)V * K; i += blockDim.x) {
      const int v = (int)(i / K), k = (int)(i - (long)v * K);
      const int j0 = s_off[v], j1 = s_off[v + 1];
      if (j1 > j0) {
        float t = 0.f;
        for (int j = j0; j < j1; j++) {
          const int m = s_list[j];
          t += bf2f(x[(long)m * K + k]) * s_dl[m];
        }
        e_grad[i] += t;
      }
    }
  }
}

static int proj_head_launch(const char* name, const void* x, const float* w, const float* b, const float* E, const int32_t* labels, void* logits,
                            const void* dl, float* loss, void* dx, float* w_grad, float* b_grad, float* e_grad, int M, int K, int V, int n_real,
                            int mode, float loss_scale, int what, void* stream) {
  GANK_REQUIRE(x && w && E && labels, "%s: null pointer (x, w, E and labels are required)", name);
  GANK_REQUIRE(M >= 1 && M <= PH_MAX_M && K >= 1 && K <= PH_MAX_K && V >= 1 && V <= PH_MAX_V,
               "%s: unsupported shape M = %d, K = %d, V = %d (1..%d, 1..%d, 1..%d)", name, M, K, V, PH_MAX_M, PH_MAX_K, PH_MAX_V);
  const size_t lds = proj_head_lds_floats(M, K, V) * sizeof(float);      // <= 52 KB at the largest supported shape
  hipLaunchKernelGGL(proj_head_kernel, dim3(1), dim3(1024), lds, (hipStream_t)stream, (const bf16*)x, w, b, E, labels, (bf16*)logits, (const bf16*)dl,
                     loss, (bf16*)dx, w_grad, b_grad, e_grad, M, K, V, n_real, mode, loss_scale, what);
  GANK_LAUNCH_OK(name);
  return 0;
}

extern "C" int gank_proj_head_fwd(const void* x, const float* w, const float* b, const float* E, const int32_t* labels, void* logits, int M, int K,
                                  int V, void* stream) {
  GANK_REQUIRE(logits, "proj_head_fwd: null pointer (logits)");
  return proj_head_launch("proj_head_fwd", x, w, b, E, labels, logits, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, M, K, V, 0, 1, 1.f, PH_FWD,
                          stream);
}

extern "C" int gank_proj_head_bwd(const void* dl, const void* x, const float* w, const float* E, const int32_t* labels, void* dx, float* w_grad,
                                  float* b_grad, float* e_grad, int M, int K, int V, void* stream) {
  GANK_REQUIRE(dl, "proj_head_bwd: null pointer (dl)");
  return proj_head_launch("proj_head_bwd", x, w, nullptr, E, labels, nullptr, dl, nullptr, dx, w_grad, b_grad, e_grad, M, K, V, 0, 1, 1.f, PH_BWD, stream);
}

extern "C" int gank_proj_head_hinge_scaled(const void* x, const float* w, const float* b, const float* E, const int32_t* labels, void* logits,
                                           float* loss, void* dx, float* w_grad, float* b_grad, float* e_grad, int M, int K, int V, int n_real,
                                           int mode, float loss_scale, void* stream) {
  GANK_REQUIRE(logits && loss, "proj_head_hinge: null pointer (logits and loss are required)");
  GANK_REQUIRE(mode == 0 || mode == 1, "proj_head_hinge: mode %d (0: critic loss, 1: generator loss)", mode);
  GANK_REQUIRE(mode == 1 || (n_real > 0 && n_real < M), "proj_head_hinge: n_real must split the batch");
  GANK_REQUIRE(loss_scale > 0.f, "proj_head_hinge: loss_scale must be positive");
  return proj_head_launch("proj_head_hinge", x, w, b, E, labels, logits, nullptr, loss, dx, w_grad, b_grad, e_grad, M, K, V, n_real, mode, loss_scale,
                          PH_FWD | PH_HINGE | PH_BWD, stream);
}
