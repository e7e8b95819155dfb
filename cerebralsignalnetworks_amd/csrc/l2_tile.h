// The distance-tile body shared by csn_l2_topk_tiled (retrieval_tiled.hip) and csn_chan_l2_dist (channel_l2.hip):
// 64 x 64 squared-L2 distances of 64 query rows and 64 gallery rows, 16 x 16 threads, 4 x 4 pairs per thread.
//   Operand rows go through LDS in 32-wide slices of the summed dimension as float32, transposed ([d][row], row stride 68
//   words so that the staging writes and the 16-byte reads are conflict free); each element is converted to float64 once
//   per thread that reads it; the inner loop is sub + fma on registers.  One chain per pair in ascending d, never split:
//   acc = 0.0; for d: df = (double)q[d] - (double)g[d]; acc = fma(df, df, acc).  Elements beyond D, or of rows that do
//   not exist, are staged as zeros by the caller's loaders (fma(0, 0, acc) = acc: they leave the chain's bits alone).
#pragma once
#include "csn_common.h"

namespace csn {
namespace tk {

constexpr int TQ = 64, TG = 64, DS = 32;
constexpr int LDP = 68;       // words per d-row of a staged operand slice: 16-byte aligned, bank = (4c + r) mod 32 on the writes
static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
constexpr int TILE_LDS_BYTES = 2 * DS * LDP * (int)sizeof(float);      // both operand slices: 17408

// Every thread of the 256 calls it.  qs / gs: [DS][LDP] floats of LDS each.  load_q(r, c) / load_g(r, c): element c
// (0 <= c < a multiple of 32 that covers D) of local row r (0 .. 63), 0.0f where the row or the element does not exist.
// The first statement of every slice is a barrier, so LDS the caller still reads on entry is safe; on return other waves
// may still be reading the last slice.
template <class LoadQ, class LoadG>
__device__ __forceinline__ void l2_tile_distances(double (&acc)[4][4], float* qs, float* gs, int tid, int D, LoadQ load_q,
                                                  LoadG load_g) {
  const int tq = tid >> 4, tg = tid & 15;
  // staging map: 8 elements per thread and operand; a 32-lane half writes 8 consecutive d of 4 consecutive rows
  const int sc = tid & 7, sr = tid >> 3;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;

  float qr[8], gr[8];
  auto fetch = [&](int d0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = d0 + sc + 8 * (j & 3);
      const int r = sr + 32 * (j >> 2);
      qr[j] = load_q(r, c);
      gr[j] = load_g(r, c);
    }
  };
  fetch(0);
  for (int d0 = 0; d0 < D; d0 += DS) {
    __syncthreads();          // the previous slice's reads, or the caller's reads of this LDS, are done
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int o = (sc + 8 * (j & 3)) * LDP + sr + 32 * (j >> 2);
      qs[o] = qr[j];
      gs[o] = gr[j];
    }
    __syncthreads();
    if (d0 + DS < D) fetch(d0 + DS);
#pragma unroll 4
    for (int c = 0; c < DS; ++c) {
      const f32x4 qf = *reinterpret_cast<const f32x4*>(qs + c * LDP + tq * 4);
      const f32x4 gf = *reinterpret_cast<const f32x4*>(gs + c * LDP + tg * 4);
      double qd[4], gd[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        qd[i] = (double)qf[i];
        gd[i] = (double)gf[i];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const double df = qd[i] - gd[j];
          acc[i][j] = fma(df, df, acc[i][j]);
        }
    }
  }
}

}  // namespace tk
}  // namespace csn
