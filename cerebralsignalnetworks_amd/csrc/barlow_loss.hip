// K7b: the Barlow-Twins loss (EEG-BarlowNetworks/net.py:33-42), value and both gradients in float64.
// Two entry points because the reference all-reduces c between them; the formulas are in include/csn_hip.h.
//   csn_barlow_corr   bt_stats_kernel    column mean and 1/sqrt(var + eps) of z1 and of z2 (two passes), running statistics
//                     bt_tile_kernel<0>  c = inv_batch z1n^T z2n            (summed over B)
//   csn_barlow_grad   bt_ck_kernel       one pass over c: loss terms, k1 (whole rows), partial column sums of k2
//                     bt_finish_kernel   k2 and the loss from the partial sums
//                     bt_tile_kernel<1>  dz1 (blockIdx.z 0, summed over D) and dz2 (blockIdx.z 1, summed over D)
// The three contractions share bt_tile (bt_tile.h), the pattern of l2_tile.h with float64 operands: a 64 x 64 output tile per 256-thread
// workgroup, 4 x 4 results per thread, the summed dimension staged through LDS in slices of 32 as [k][row] float64 -- already
// normalised (z - mean) rstd, or already G -- so the inner loop is 16 fma on registers.  One chain per result in ascending k,
// never split: the bits do not depend on the grid.  Rows, columns and summed indices that do not exist are staged as zeros
// (fma(0, 0, acc) = acc).  No atomics, no waits between workgroups; every loop is bounded by B or D.
#include <math.h>

#include "bt_tile.h"

namespace csn {
namespace bt {

constexpr int CK_ROWS = 16;   // rows of c per workgroup of bt_ck_kernel: 4 waves x 4 rows
constexpr int ST_GROUPS = 16; // row groups (waves) per workgroup of bt_stats_kernel

// saved: mean1[D], rstd1[D], mean2[D], rstd2[D]
struct Saved {
  const double *mean1, *rstd1, *mean2, *rstd2;
  __host__ __device__ Saved(const void* p, int D)
      : mean1((const double*)p), rstd1((const double*)p + D), mean2((const double*)p + 2 * (int64_t)D),
        rstd2((const double*)p + 3 * (int64_t)D) {}
};

// Column statistics of z1 and then of z2: 64 columns per workgroup, wave g adds rows g, g + 16, ... in ascending order and
// the 16 partial sums are added in ascending g -- an order that depends on B only.
__global__ void __launch_bounds__(64 * ST_GROUPS) bt_stats_kernel(const float* __restrict__ z1, const float* __restrict__ z2,
                                                                  int B, int D, double eps, double* __restrict__ saved,
                                                                  float* __restrict__ running_mean,
                                                                  float* __restrict__ running_var, double momentum) {
  __shared__ double red[ST_GROUPS][64];
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + lane;
  const bool live = col < D;
  for (int which = 0; which < 2; ++which) {
    const float* z = which == 0 ? z1 : z2;
    double s = 0.0;
    if (live)
      for (int b = g; b < B; b += ST_GROUPS) s += (double)z[(int64_t)b * D + col];
    red[g][lane] = s;
    __syncthreads();
    double mean = 0.0;
#pragma unroll
    for (int i = 0; i < ST_GROUPS; ++i) mean += red[i][lane];
    mean /= (double)B;
    __syncthreads();
    double q = 0.0;
    if (live)
      for (int b = g; b < B; b += ST_GROUPS) {
        const double d = (double)z[(int64_t)b * D + col] - mean;
        q = fma(d, d, q);
      }
    red[g][lane] = q;
    __syncthreads();
    if (g == 0 && live) {
      double var = 0.0;
#pragma unroll
      for (int i = 0; i < ST_GROUPS; ++i) var += red[i][lane];
      var /= (double)B;
      saved[(int64_t)(2 * which) * D + col] = mean;
      saved[(int64_t)(2 * which + 1) * D + col] = 1.0 / sqrt(var + eps);
      if (running_mean != nullptr) {      // the one buffer pair, for z1 and then for z2: the same thread does both
        running_mean[col] = (float)((1.0 - momentum) * (double)running_mean[col] + momentum * mean);
        running_var[col] = (float)((1.0 - momentum) * (double)running_var[col] + momentum * var * (double)B / (double)(B - 1));
      }
    }
    __syncthreads();
  }
}

struct TileArgs {
  const float* z1;
  const float* z2;
  int B, D;
  const void* saved;
  double inv_batch;
  // WHAT 0 (c)
  double* c_out;
  // WHAT 1 (dz1 / dz2)
  const double* c;
  const double* k1;
  const double* k2;
  double lambd, grad_scale;
  float* dz_a;        // blockIdx.z 0 writes it; with one gradient wanted it is that one and side0 names it
  float* dz_b;        // blockIdx.z 1: always dz2
  int side0;          // which gradient dz_a is: 0 = dz1, 1 = dz2
};

__device__ __forceinline__ double bt_zn(const float* z, const double* mean, const double* rstd, int B, int D, int b, int col) {
  return (b < B && col < D) ? ((double)z[(int64_t)b * D + col] - mean[col]) * rstd[col] : 0.0;
}
__device__ __forceinline__ double bt_g(const double* c, int D, int i, int j, double lambd) {
  if (i >= D || j >= D) return 0.0;
  const double v = c[(int64_t)i * D + j];
  return i == j ? 2.0 * (v - 1.0) : 2.0 * lambd * v;
}

// WHAT 0: c[i,j] = inv_batch sum_b z1n[b,i] z2n[b,j]; grid (cdiv(D,64), cdiv(D,64)): blockIdx.y the 64 i, blockIdx.x the 64 j.
// WHAT 1: grid (cdiv(D,64), cdiv(B,64), 1 or 2): blockIdx.y the 64 rows b, blockIdx.x the 64 columns of the output.
template <int WHAT>
__global__ void __launch_bounds__(256) bt_tile_kernel(const TileArgs a) {
  __shared__ __attribute__((aligned(16))) double lds[TILE_LDS_DOUBLES];
  double* as = lds;
  double* bs = lds + KS * LDK;
  const int tid = threadIdx.x, tq = tid >> 4, tg = tid & 15;
  const int B = a.B, D = a.D;
  const Saved sv(a.saved, D);
  const int r0 = blockIdx.y * TR, c0 = blockIdx.x * TC;
  double acc[4][4];
  if constexpr (WHAT == 0) {
    bt_tile<false, false>(acc, as, bs, tid, B,
                          [&](int k, int r) { return bt_zn(a.z1, sv.mean1, sv.rstd1, B, D, k, r0 + r); },
                          [&](int k, int r) { return bt_zn(a.z2, sv.mean2, sv.rstd2, B, D, k, c0 + r); });
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = r0 + tq * 4 + i, col = c0 + tg * 4 + j;
        if (row < D && col < D) a.c_out[(int64_t)row * D + col] = a.inv_batch * acc[i][j];
      }
  } else {
    const int side = blockIdx.z == 0 ? a.side0 : 1;
    float* out = blockIdx.z == 0 ? a.dz_a : a.dz_b;
    if (side == 0) {      // dz1[b,i]: sum_j z2n[b,j] G[i,j]
      bt_tile<true, true>(acc, as, bs, tid, D,
                          [&](int k, int r) { return bt_zn(a.z2, sv.mean2, sv.rstd2, B, D, r0 + r, k); },
                          [&](int k, int r) { return bt_g(a.c, D, c0 + r, k, a.lambd); });
    } else {              // dz2[b,j]: sum_i z1n[b,i] G[i,j]
      bt_tile<true, false>(acc, as, bs, tid, D,
                           [&](int k, int r) { return bt_zn(a.z1, sv.mean1, sv.rstd1, B, D, r0 + r, k); },
                           [&](int k, int r) { return bt_g(a.c, D, k, c0 + r, a.lambd); });
    }
    const float* z = side == 0 ? a.z1 : a.z2;
    const double* mean = side == 0 ? sv.mean1 : sv.mean2;
    const double* rstd = side == 0 ? sv.rstd1 : sv.rstd2;
    const double* kk = side == 0 ? a.k1 : a.k2;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = r0 + tq * 4 + i, col = c0 + tg * 4 + j;
        if (row < B && col < D) {
          const double zn = bt_zn(z, mean, rstd, B, D, row, col);
          out[(int64_t)row * D + col] = (float)(a.grad_scale * rstd[col] * (a.inv_batch * acc[i][j] - zn * kk[col]));
        }
      }
  }
}

// One pass over c (summed over ranks) and c_local: 16 rows per workgroup, 4 per wave, lane l the columns l, l + 64, ...
//   k1[i] = sum_j G[i,j] c_local[i,j] / B       a wave holds whole rows: finished here (butterfly of wave_sum)
//   k2part[blk][j] = sum over the workgroup's 16 rows of G[i,j] c_local[i,j]        ((w0 + w1) + w2) + w3 over the waves
//   onoff[blk], onoff[nblk + blk] = the workgroup's sum of (c_ii - 1)^2 and of c_ij^2 (i != j)
__global__ void __launch_bounds__(256) bt_ck_kernel(const double* __restrict__ c, const double* __restrict__ c_local, int D,
                                                    double lambd, double inv_B, double* __restrict__ k1,
                                                    double* __restrict__ k2part, double* __restrict__ onoff, int nblk) {
  __shared__ double colp[4][64];
  __shared__ double oo[2][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i0 = blockIdx.x * CK_ROWS + wave * 4;
  double krow[4] = {0.0, 0.0, 0.0, 0.0}, on = 0.0, off = 0.0;
  for (int j0 = 0; j0 < D; j0 += 64) {
    const int j = j0 + lane;
    double col = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + r;
      if (i < D && j < D) {
        const double cv = c[(int64_t)i * D + j], cl = c_local[(int64_t)i * D + j];
        double g;
        if (i == j) {
          const double d = cv - 1.0;
          g = 2.0 * d;
          on = fma(d, d, on);
        } else {
          g = 2.0 * lambd * cv;
          off = fma(cv, cv, off);
        }
        const double p = g * cl;
        krow[r] += p;
        col += p;
      }
    }
    colp[wave][lane] = col;
    __syncthreads();
    if (wave == 0 && j < D) k2part[(int64_t)blockIdx.x * D + j] = ((colp[0][lane] + colp[1][lane]) + colp[2][lane]) + colp[3][lane];
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const double s = wave_sum(krow[r]);
    if (lane == 0 && i0 + r < D) k1[i0 + r] = s * inv_B;
  }
  on = wave_sum(on);
  off = wave_sum(off);
  if (lane == 0) {
    oo[0][wave] = on;
    oo[1][wave] = off;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    onoff[blockIdx.x] = ((oo[0][0] + oo[0][1]) + oo[0][2]) + oo[0][3];
    onoff[nblk + blockIdx.x] = ((oo[1][0] + oo[1][1]) + oo[1][2]) + oo[1][3];
  }
}

// k2[j] = sum_blk k2part[blk][j] / B in ascending blk; workgroup 0's first wave: loss = fl32(sum on + lambd sum off), lane l
// the workgroups l, l + 64, ... ascending, then the butterfly.  Both orders depend on D only.
__global__ void __launch_bounds__(256) bt_finish_kernel(const double* __restrict__ k2part, const double* __restrict__ onoff,
                                                        int D, int nblk, double lambd, double inv_B, double* __restrict__ k2,
                                                        float* __restrict__ loss) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < D) {
    double s = 0.0;
    for (int blk = 0; blk < nblk; ++blk) s += k2part[(int64_t)blk * D + j];
    k2[j] = s * inv_B;
  }
  if (blockIdx.x == 0 && threadIdx.x < 64) {
    double on = 0.0, off = 0.0;
    for (int blk = threadIdx.x; blk < nblk; blk += 64) {
      on += onoff[blk];
      off += onoff[nblk + blk];
    }
    on = wave_sum(on);
    off = wave_sum(off);
    if (threadIdx.x == 0) loss[0] = (float)(on + lambd * off);
  }
}

static inline int ck_blocks(int D) { return (D + CK_ROWS - 1) / CK_ROWS; }
static inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

}  // namespace bt
}  // namespace csn

using namespace csn;

extern "C" size_t csn_barlow_saved_bytes(int D) { return D > 0 ? (size_t)D * 4 * sizeof(double) : 0; }

// k1[D], k2[D], onoff[2 nblk], k2part[nblk][D]
extern "C" size_t csn_barlow_scratch_bytes(int B, int D) {
  if (B <= 0 || D <= 0) return 0;
  const size_t nblk = (size_t)bt::ck_blocks(D);
  return (2 * (size_t)D + 2 * nblk + nblk * (size_t)D) * sizeof(double);
}

extern "C" int csn_barlow_corr(const float* z1, const float* z2, int B, int D, double eps, double inv_batch, double* c,
                               void* saved, float* running_mean, float* running_var, double momentum, csnStream_t stream) {
  CSN_REQUIRE(z1 && z2 && c && saved, "csn_barlow_corr: null pointer");
  CSN_REQUIRE(B >= 2 && D >= 1, "csn_barlow_corr: bad shape B=%d D=%d (batch statistics need two rows)", B, D);
  CSN_REQUIRE(isfinite(eps) && eps > 0.0, "csn_barlow_corr: eps must be finite and positive, got %g", eps);
  CSN_REQUIRE(isfinite(inv_batch) && inv_batch > 0.0, "csn_barlow_corr: inv_batch must be finite and positive, got %g", inv_batch);
  CSN_REQUIRE(momentum >= 0.0 && momentum <= 1.0, "csn_barlow_corr: momentum %g outside [0, 1]", momentum);
  CSN_REQUIRE((running_mean == nullptr) == (running_var == nullptr),
              "csn_barlow_corr: running_mean and running_var go together (both NULL or both set)");
  CSN_REQUIRE(bt::aligned8(c) && bt::aligned8(saved), "csn_barlow_corr: c and saved must be 8-byte aligned");
  hipStream_t st = as_stream(stream);
  const unsigned nd = (unsigned)((D + 63) / 64);
  bt::bt_stats_kernel<<<nd, 64 * bt::ST_GROUPS, 0, st>>>(z1, z2, B, D, eps, (double*)saved, running_mean, running_var, momentum);
  CSN_LAUNCH_CHECK();
  bt::TileArgs a{};
  a.z1 = z1; a.z2 = z2; a.B = B; a.D = D; a.saved = saved; a.inv_batch = inv_batch; a.c_out = c;
  bt::bt_tile_kernel<0><<<dim3(nd, nd), 256, 0, st>>>(a);
  CSN_LAUNCH_CHECK();
  return CSN_OK;
}

extern "C" int csn_barlow_grad(const float* z1, const float* z2, int B, int D, const double* c, const double* c_local,
                               const void* saved, double inv_batch, double lambd, float grad_scale, float* loss, float* dz1,
                               float* dz2, void* scratch, csnStream_t stream) {
  CSN_REQUIRE(z1 && z2 && c && c_local && saved && loss && scratch, "csn_barlow_grad: null pointer");
  CSN_REQUIRE(B >= 2 && D >= 1, "csn_barlow_grad: bad shape B=%d D=%d (batch statistics need two rows)", B, D);
  CSN_REQUIRE(isfinite(inv_batch) && inv_batch > 0.0, "csn_barlow_grad: inv_batch must be finite and positive, got %g", inv_batch);
  CSN_REQUIRE(isfinite(lambd), "csn_barlow_grad: lambd must be finite, got %g", lambd);
  CSN_REQUIRE(bt::aligned8(c) && bt::aligned8(c_local) && bt::aligned8(saved) && bt::aligned8(scratch),
              "csn_barlow_grad: c, c_local, saved and scratch must be 8-byte aligned");
  hipStream_t st = as_stream(stream);
  const int nblk = bt::ck_blocks(D);
  double* k1 = (double*)scratch;
  double* k2 = k1 + D;
  double* onoff = k2 + D;
  double* k2part = onoff + 2 * (size_t)nblk;
  const double inv_B = 1.0 / (double)B;
  bt::bt_ck_kernel<<<(unsigned)nblk, 256, 0, st>>>(c, c_local, D, lambd, inv_B, k1, k2part, onoff, nblk);
  CSN_LAUNCH_CHECK();
  bt::bt_finish_kernel<<<(unsigned)((D + 255) / 256), 256, 0, st>>>(k2part, onoff, D, nblk, lambd, inv_B, k2, loss);
  CSN_LAUNCH_CHECK();
  if (dz1 != nullptr || dz2 != nullptr) {
    bt::TileArgs a{};
    a.z1 = z1; a.z2 = z2; a.B = B; a.D = D; a.saved = saved; a.inv_batch = inv_batch;
    a.c = c; a.k1 = k1; a.k2 = k2; a.lambd = lambd; a.grad_scale = (double)grad_scale;
    a.side0 = dz1 != nullptr ? 0 : 1;
    a.dz_a = dz1 != nullptr ? dz1 : dz2;
    a.dz_b = dz2;
    const unsigned nz = (dz1 != nullptr && dz2 != nullptr) ? 2u : 1u;
    bt::bt_tile_kernel<1><<<dim3((unsigned)((D + 63) / 64), (unsigned)((B + 63) / 64), nz), 256, 0, st>>>(a);
    CSN_LAUNCH_CHECK();
  }
  return CSN_OK;
}
