// Inter-layer dropout of the stacked LSTM (include/csn_hip.h: csn_lstm_plan_set_dropout): the
// counter-based generator that defines the mask, shared by the kernels of lstm_dropout.hip and the host function
// csn_lstm_dropout_keep, and the launchers lstm.hip calls.
#pragma once
#include "csn_common.h"

namespace csn {

struct Philox4 { uint32_t w[4]; };

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): ten rounds, the key bumped by the
// Weyl constants between them
__host__ __device__ inline Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// What a plan's dropout setting comes to for the kernels.  Element e (64-bit: ((l T + t) B + b) H + u, l the interface
// between layers l and l + 1, T B H the plan's) is kept iff word (e & 3) of
// philox(counter = (lo32(e >> 2), hi32(e >> 2), subsequence, 0), key = (lo32(seed), hi32(seed))) is >= thr.
struct DropoutCfg {
  uint32_t k0, k1, subsequence;
  uint64_t thr;      // floor(float32(p) 2^32); 2^32 at p = 1: no 32-bit word reaches it, nothing is kept
  float scale;       // 1.0f / (1.0f - p), float32 arithmetic (inf at p = 1, where it multiplies nothing)
};
__host__ __device__ inline Philox4 dropout_words(const DropoutCfg& c, uint64_t quad) {
  return philox4x32_10((uint32_t)quad, (uint32_t)(quad >> 32), c.subsequence, 0u, c.k0, c.k1);
}
static inline DropoutCfg dropout_cfg(float p, uint64_t seed, uint32_t subsequence) {
  DropoutCfg c;
  c.k0 = (uint32_t)seed;
  c.k1 = (uint32_t)(seed >> 32);
  c.subsequence = subsequence;
  c.thr = (uint64_t)((double)p * 4294967296.0);      // exact: a float32 times a power of two, then floor
  c.scale = 1.0f / (1.0f - p);
  return c;
}

// h_drop[i] = keep(e0 + i) ? (T)(float(h[i]) * scale) : 0 for i in [0, n): a time-major slab of whole steps, so n % 32 == 0
// and e0 % 4 == 0 (H % 32 == 0); h and h_drop 16-B aligned
int launch_lstm_dropout_fwd(const void* h, void* h_drop, int64_t n, uint64_t e0, int dtype, const DropoutCfg& cfg, hipStream_t st);
// dx[i] = keep(e0 + i) ? dx[i] * scale : 0 in place (float32), same slab form
int launch_lstm_dropout_bwd(float* dx, int64_t n, uint64_t e0, const DropoutCfg& cfg, hipStream_t st);

// Output dropout (csn_lstm_plan_set_output_dropout): the mask on the caller's [B, Tn, .] tensor, applied by the layout
// passes themselves (lstm_boundary.hip: y_out and dy_in).  Element (b, t, h) has the index
// first + (b Tn + t) index_pitch + h; first % 4 == 0, index_pitch % 4 == 0 and H % 32 == 0 put every four consecutive h on
// one Philox call.
struct OutDropCfg {
  DropoutCfg cfg;
  uint64_t first;
  int64_t index_pitch;
};

}  // namespace csn
