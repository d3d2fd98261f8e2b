// What the float64 metric kernels share (fid.hip: the vector types only; inception_score.hip: the sums; kid.hip and prd.hip:
// the sums and the 64 x 64 tile of dot products over the FEATURE axis on v_mfma_f64_16x16x4_f64).
//
// The tile of dot products.  f64_tile_dots contracts 64 rows against 64 rows (the tile's rows and its columns), float32
// features [*, D]: acc = <row i, row j> for the 64 x 64 pairs, the four waves of a 256-thread workgroup a 32 x 32 quadrant
// each, 2 x 2 MFMA tiles.  The caller resolves the rows: each thread hands in its four row pointers (a gather through tables
// in kid.hip, clamped positions in prd.hip); everything between them and the accumulators is here.
//
// Staging.  A[i][k] = rows[i][k0 + k], B[k][j] = columns[j][k0 + k].  The workgroup stages its 64 + 64 rows in chunks of 32
// features as fs[side][row][k], widened to float64 (exact), features past D as zeros; the next chunk's global loads are in
// flight while the current one is multiplied.  The f64 MFMA's operand map is: lane l holds A[l & 15][l >> 4] and
// B[l >> 4][l & 15], four contraction steps per instruction, one per value of l >> 4.  Which feature a step stands for is
// free as long as A and B agree, so a lane reads the PAIR of features fs[side][q0 + (l & 15)][8 kg + 2 (l >> 4) + {0, 1}] with
// one 16-byte LDS read and feeds element 0 to one MFMA (features 8 kg + {0, 2, 4, 6}) and element 1 to the next
// (8 kg + {1, 3, 5, 7}): half the LDS instructions of one read per MFMA operand.  The result map is the f64 one, col = l & 15,
// row = (l >> 4) + 4 * reg (NOT the fp32 map).
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
// No atomics and no split of the contraction: an element's products are added in one accumulator in a fixed feature order.
#pragma once
#include "gank_common.h"

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

constexpr int kF64Threads = 256;   // the workgroup of f64_tile_dots and of the float64 block_sum
constexpr int kF64Tile = 64;       // rows / columns per tile
constexpr int kF64Chunk = 32;      // features per staged chunk
constexpr int kF64Pitch = 36;      // doubles per staged row (above: why it is conflict-free)
constexpr int kF64Items = 2 * kF64Tile * (kF64Chunk / 4) / kF64Threads;     // 4-feature staging items per thread and chunk
constexpr int kF64StageDoubles = 2 * kF64Tile * kF64Pitch;                   // the staging buffer fs[2][64][36]

#ifdef __HIPCC__
// the xor butterfly of gank_common.h's wave_sum in float64: every lane ends with the same bits (a + b == b + a)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Sum over the 256 threads of a workgroup, the same bits in every thread: the butterfly, then the four waves through LDS,
// added in index order.  `red` holds 4 doubles.  (swd.hip's swd_block_sum is not this one: it is an LDS halving tree over
// the 256 values, another order of additions and so other bits.)
__device__ __forceinline__ double block_sum(double v, double* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// the staging hook of a kernel that wants nothing beside the dot products
struct F64NoStagingHook {
  __device__ __forceinline__ void operator()(int, double, double, double, double) const {}
};

// The 64 x 64 tile of dot products (header).  Staging item q of a thread is row (tid >> 3) + 32 q of the 128 staged rows (the
// tile's 64 rows, then its 64 columns), 4 features from c4 = (tid & 7) * 4 of the chunk: src[q] points at feature c4 of that
// row, 16-byte aligned, D % 16 == 0.  fs: kF64StageDoubles doubles of LDS, 16-byte aligned, free on entry (the caller's barrier)
// and free again on return (the last chunk's barrier).  staged(q, d0, d1, d2, d3) sees the four widened values of every item
// as it is staged, chunks in feature order.  -> acc, the wave's quadrant: acc[i][j][reg] is row wr * 32 + i * 16 + (l >> 4) +
// 4 * reg against column wc * 32 + j * 16 + (l & 15), with wr = wave >> 1, wc = wave & 1.
template <typename Staged>
__device__ __forceinline__ void f64_tile_dots(const float* const (&src)[kF64Items], int D, double* fs, f64x4 (&acc)[2][2],
                                              Staged staged) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = w >> 1, wc = w & 1;
  const int c4 = (tid & 7) * 4;
  f32x4 raw[kF64Items];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int q = 0; q < kF64Items; q++) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (k0 + c4 < D) v = *reinterpret_cast<const f32x4*>(src[q] + k0);      // D % 16 == 0: k0 + c4 < D covers k0 + c4 + 3
      raw[q] = v;
    }
  };
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};

  fetch(0);
  for (int k0 = 0; k0 < D; k0 += kF64Chunk) {
#pragma unroll
    for (int q = 0; q < kF64Items; q++) {
      const int r = (tid >> 3) + 32 * q;
      const double d0 = raw[q][0], d1 = raw[q][1], d2 = raw[q][2], d3 = raw[q][3];
      f64x2* dst = reinterpret_cast<f64x2*>(&fs[r * kF64Pitch + c4]);
      dst[0] = f64x2{d0, d1};
      dst[1] = f64x2{d2, d3};
      staged(q, d0, d1, d2, d3);
    }
    __syncthreads();
    if (k0 + kF64Chunk < D) fetch(k0 + kF64Chunk);
#pragma unroll
    for (int kg = 0; kg < kF64Chunk / 8; kg++) {
      const int k = kg * 8 + 2 * (lane >> 4);           // this lane's feature pair of the group of 8
      f64x2 a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; i++) {
        a[i] = *reinterpret_cast<const f64x2*>(&fs[(wr * 32 + i * 16 + (lane & 15)) * kF64Pitch + k]);
        b[i] = *reinterpret_cast<const f64x2*>(&fs[(kF64Tile + wc * 32 + i * 16 + (lane & 15)) * kF64Pitch + k]);
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
}
#endif
