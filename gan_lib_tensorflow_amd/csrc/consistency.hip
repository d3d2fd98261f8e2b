// Consistency regularisation of the critic (Zhang et al. 2020, "Consistency Regularization for GANs", section 3.1, eq. 5-7; Zhao et al.
// 2020, "Improved Consistency Regularization for GANs", section 3.1, eq. 1-2):
//     L_cr  = w_real * mean_i || D(x_i)    - D(T(x_i))    ||^2
//     L_bcr = L_cr + w_fake * mean_i || D(G(z_i)) - D(T(G(z_i))) ||^2
// T is the augmentation of CR-GAN's CIFAR-10 experiments (section 4.1 there): a random horizontal flip and a random shift by whole
// pixels.  Three entry points: the draw of T's parameters from the library's Philox stream, the gather that applies them, and the
// squared difference of two sets of logits with both derivatives.
#include "gank_common.h"
#include "feed.h"

// ---------------------------------------------------------------------------------------------------------------
// gank_cr_draw.  Row i of the table takes Philox call i of the draw at the stream's offset (counter i: one call a row) and uses three
// of its four words:
//     flip = word 0 >> 31                       the top bit
//     dx   = mulhi(word 1, 2 s + 1) - s         floor(word * (2 s + 1) / 2^32) - s, in [-s, s]
//     dy   = mulhi(word 2, 2 s + 1) - s
// (word 3 is not used).  The multiply-high map sends either floor or ceil(2^32 / (2 s + 1)) words to each value: the probabilities of
// two values differ by at most 2^-32, a relative bias below (2 s + 1) * 2^-32.  One block: every thread has read {seed, offset} before
// the barrier behind which thread 0 rewrites the offset (+ 1, as every other draw), so a captured graph draws afresh on each replay.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cr_draw_kernel(int* __restrict__ table, long n, int s, unsigned long long* state) {
  const unsigned long long seed = state[0], off = state[1];
  const unsigned m = 2u * (unsigned)s + 1u;
  for (long i = threadIdx.x; i < n; i += 256) {
    const u4 r = philox4x32_10((unsigned long long)i, off, seed);
    table[3 * i] = (int)(r.x >> 31);
    table[3 * i + 1] = (int)__umulhi(r.y, m) - s;
    table[3 * i + 2] = (int)__umulhi(r.z, m) - s;
  }
  __syncthreads();
  if (threadIdx.x == 0) state[1] = off + 1;
}

extern "C" int gank_cr_draw(int32_t* table, long n, int shift, uint64_t* rng_state, void* stream) {
  GANK_REQUIRE(table && rng_state && n > 0, "cr_draw: bad arguments");
  GANK_REQUIRE(shift >= 0 && shift <= 32767, "cr_draw: shift %d (0 .. 32767 pixels)", shift);
  hipLaunchKernelGGL(cr_draw_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, table, n, shift, (unsigned long long*)rng_state);
  GANK_LAUNCH_OK("cr_draw");
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// gank_cr_augment.  out[b, y, x, :] = in[b, R(y - dy, H), R(xf - dx, W), :], xf = W - 1 - x where the image is flipped, R the
// reflection that does not repeat the edge (np.pad(mode='reflect'): R(i, n) = -i below 0 and 2 (n - 1) - i from n on; defined for
// shifts below n).  A pure gather of 16-bit elements: the values are never converted, so the result is exact in either element type.
//
// Lanes and bytes.  A pixel is 2 C bytes (6 at C = 3), a flipped row reverses the pixels and keeps the channels in order, and a
// reflected edge turns the direction round in the middle of a row: no load wider than one pixel survives every table, and 6 bytes is
// no load width, so loads are one 16-bit element a lane and instruction.  The reflection is worked out once per block for every row
// (srow: the source row's offset) and every column (scol: the offset in that row of each of the W C output elements) into LDS, and an
// output element is two table reads and one load away.  Consecutive lanes take consecutive pieces of the OUTPUT, so the stores are
// contiguous and, outside a reflected edge, so are the addresses of a load instruction (ascending, or descending by pixels when
// flipped): a CIFAR row is 192 bytes, three cache lines that the eight loads of a lane's piece share.  Where the row length allows
// (W C a multiple of 8 and `out` 16-byte aligned) a lane gathers 8 elements and stores them as 16 bytes, 1 KiB a wave instruction
// instead of 128 bytes; any other shape takes one element a lane.  393 KB at the trainer's batch of 64: bound by the launch.
// ---------------------------------------------------------------------------------------------------------------
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));

template <int V>
__global__ __launch_bounds__(256) void cr_augment_kernel(const unsigned short* __restrict__ x, const int* __restrict__ table,
                                                         unsigned short* __restrict__ out, int H, int W, int C, int smax) {
  extern __shared__ int cr_lds[];
  int* srow = cr_lds;                   // [H]      source row of output row y, times the row length
  int* scol = cr_lds + H;               // [W * C]  source element (within its row) of output element x * C + c
  const int b = blockIdx.x, rowlen = W * C;
  const bool flip = table[3 * b] != 0;
  // (a table entry beyond the caller's largest shift is clamped to it: no table can point outside the image)
  const int dx = min(max(table[3 * b + 1], -smax), smax), dy = min(max(table[3 * b + 2], -smax), smax);
  for (int y = threadIdx.x; y < H; y += 256) {
    int sy = y - dy;
    sy = sy < 0 ? -sy : (sy >= H ? 2 * (H - 1) - sy : sy);
    srow[y] = sy * rowlen;
  }
  for (int xo = threadIdx.x; xo < W; xo += 256) {
    int sx = (flip ? W - 1 - xo : xo) - dx;
    sx = sx < 0 ? -sx : (sx >= W ? 2 * (W - 1) - sx : sx);
    for (int c = 0; c < C; c++) scol[xo * C + c] = sx * C + c;
  }
  __syncthreads();
  const long img = (long)b * H * rowlen;
  const int per_row = rowlen / V, pieces = H * per_row;
  for (int p = blockIdx.y * 256 + threadIdx.x; p < pieces; p += gridDim.y * 256) {
    const int y = p / per_row, r = (p - y * per_row) * V;
    const unsigned short* src = x + img + srow[y];
    unsigned short* dst = out + img + y * rowlen + r;
    if (V == 8) {
      u16x8 o;
#pragma unroll
      for (int e = 0; e < 8; e++) o[e] = src[scol[r + e]];
      *reinterpret_cast<u16x8*>(dst) = o;
    } else {
      *dst = src[scol[r]];
    }
  }
}

extern "C" int gank_cr_augment(const void* x, const int32_t* table, void* out, int B, int H, int W, int C, int max_shift, void* stream) {
  GANK_REQUIRE(x && table && out && B > 0 && H > 0 && W > 0 && C > 0, "cr_augment: bad arguments");
  GANK_REQUIRE(x != out, "cr_augment: out must not be the input (a gather)");
  GANK_REQUIRE(max_shift >= 0 && max_shift < (H < W ? H : W),
               "cr_augment: shift %d on %d x %d images: the reflection is defined for shifts below min(H, W)", max_shift, H, W);
  GANK_REQUIRE((long)H * W * C < 0x7fffffffL && (long)H + (long)W * C <= 16384,
               "cr_augment: %d x %d x %d images are more than the row and column tables hold (H + W C <= 16384)", H, W, C);
  const int rowlen = W * C;
  const bool wide = rowlen % 8 == 0 && ((size_t)out & 15) == 0;
  const long pieces = (long)H * (wide ? rowlen / 8 : rowlen);
  long gy = (pieces + 255) / 256;
  if (gy > 1024) gy = 1024;
  const size_t lds = (size_t)(H + rowlen) * sizeof(int);
  hipStream_t s = (hipStream_t)stream;
  if (wide)
    hipLaunchKernelGGL(cr_augment_kernel<8>, dim3(B, (unsigned)gy), dim3(256), lds, s, (const unsigned short*)x, table, (unsigned short*)out, H, W, C, max_shift);
  else
    hipLaunchKernelGGL(cr_augment_kernel<1>, dim3(B, (unsigned)gy), dim3(256), lds, s, (const unsigned short*)x, table, (unsigned short*)out, H, W, C, max_shift);
  GANK_LAUNCH_OK("cr_augment");
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// gank_consistency_loss.  loss = w / B * sum_i sum_c (a - b)^2, da = 2 w / B * (a - b), db = -da, over n = B C elements, in one launch
// of one block (the logits of a batch: 64, or 640 with the class head).  fp32 in a fixed order, no atomics: thread t adds the squares
// of elements t, t + 256, ... in that order, the 64 lanes of a wave add by the xor butterfly, the four waves are added in order; so
// two runs agree to the bit.  Roundings between the exact value and `loss`: 3 a term (the difference, squared, and the square), at
// most ceil(n / 256) - 1 + 6 + 3 in the sums, 2 in w / B and the product with it -- ceil(n / 256) + 13 in all, every term >= 0.  A
// derivative has 3 (the difference, w / B, the product; the doubling is exact) and is an exact zero where a == b; db is da with the
// sign bit turned.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void consistency_loss_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ loss,
                                                               float* __restrict__ da, float* __restrict__ db, long n, int B, float w) {
  __shared__ float red[16];
  const float wb = w / (float)B, k = 2.f * wb;
  float acc = 0.f;
  for (long i = threadIdx.x; i < n; i += 256) {
    const float d = a[i] - b[i];
    acc += d * d;
    const float g = k * d;
    da[i] = g;
    db[i] = -g;
  }
  const float tot = block_sum(acc, red);
  if (threadIdx.x == 0) loss[0] = wb * tot;
}

extern "C" int gank_consistency_loss(const float* a, const float* b, float* loss, float* da, float* db, int B, int C, float w, void* stream) {
  GANK_REQUIRE(a && b && loss && da && db && B > 0 && C > 0, "consistency_loss: bad arguments");
  hipLaunchKernelGGL(consistency_loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a, b, loss, da, db, (long)B * C, B, w);
  GANK_LAUNCH_OK("consistency_loss");
  return 0;
}
