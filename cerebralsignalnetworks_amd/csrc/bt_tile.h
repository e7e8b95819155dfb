// bt_tile: the float64 contraction tile of the fused losses (barlow_loss.hip, contrastive_loss.hip) -- the pattern of
// l2_tile.h with float64 operands: a 64 x 64 output tile per 256-thread workgroup, 4 x 4 results per thread, the summed
// dimension staged through LDS in slices of 32 as [k][row] float64 -- already normalised -- so the inner loop is 16 fma on
// registers.  One chain per result in ascending k, never split: the bits do not depend on the grid.  Rows, columns and
// summed indices that do not exist are staged as zeros (fma(0, 0, acc) = acc).
#pragma once
#include "csn_common.h"

namespace csn {
namespace bt {

typedef __attribute__((ext_vector_type(2))) double f64x2;

constexpr int TR = 64, TC = 64, KS = 32;
constexpr int LDK = 72;       // doubles per k-row of a staged slice: 16-byte aligned rows, a k step moves 16 banks
constexpr int TILE_LDS_DOUBLES = 2 * KS * LDK;      // 36864 bytes

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Every thread of the 256 calls it.  as / bs: [KS][LDK] doubles of LDS each.  load_a(k, r) / load_b(k, r): the operand
// element of summed index k (0 <= k < a multiple of 32 that covers K) and local row / column r (0 .. 63), 0.0 where either
// does not exist.  A_KMAJOR / B_KMAJOR: consecutive k of one r are consecutive in memory (the staging threads then run
// along k); otherwise consecutive r of one k are.  acc[i][j] belongs to tile row tq * 4 + i and tile column tg * 4 + j.
template <bool A_KMAJOR, bool B_KMAJOR, class LoadA, class LoadB>
__device__ __forceinline__ void bt_tile(double (&acc)[4][4], double* as, double* bs, int tid, int K, LoadA load_a, LoadB load_b) {
  const int tq = tid >> 4, tg = tid & 15;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;

  // staging maps, 8 elements per thread and operand: (k, r) of element j
  auto ak = [&](int j) { return A_KMAJOR ? (tid & 7) + 8 * (j & 3) : (tid >> 6) + 4 * j; };
  auto ar = [&](int j) { return A_KMAJOR ? (tid >> 3) + 32 * (j >> 2) : (tid & 63); };
  auto bk = [&](int j) { return B_KMAJOR ? (tid & 7) + 8 * (j & 3) : (tid >> 6) + 4 * j; };
  auto br = [&](int j) { return B_KMAJOR ? (tid >> 3) + 32 * (j >> 2) : (tid & 63); };

  double pa[8], pb[8];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      pa[j] = load_a(k0 + ak(j), ar(j));
      pb[j] = load_b(k0 + bk(j), br(j));
    }
  };
  fetch(0);
  for (int k0 = 0; k0 < K; k0 += KS) {
    __syncthreads();          // the previous slice's reads are done
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      as[ak(j) * LDK + ar(j)] = pa[j];
      bs[bk(j) * LDK + br(j)] = pb[j];
    }
    __syncthreads();
    if (k0 + KS < K) fetch(k0 + KS);
#pragma unroll 4
    for (int k = 0; k < KS; ++k) {
      const f64x2 a0 = *reinterpret_cast<const f64x2*>(as + k * LDK + tq * 4);
      const f64x2 a1 = *reinterpret_cast<const f64x2*>(as + k * LDK + tq * 4 + 2);
      const f64x2 b0 = *reinterpret_cast<const f64x2*>(bs + k * LDK + tg * 4);
      const f64x2 b1 = *reinterpret_cast<const f64x2*>(bs + k * LDK + tg * 4 + 2);
      const double av[4] = {a0[0], a0[1], a1[0], a1[1]};
      const double bv[4] = {b0[0], b0[1], b1[0], b1[1]};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fma(av[i], bv[j], acc[i][j]);
    }
  }
}

}  // namespace bt
}  // namespace csn
