// K7c: the symmetric in-batch contrastive (InfoNCE) loss over the global batch of all ranks, value and gradient in float64
// (DESIGN.md section 24).  Two entry points because the second gradient term needs lB of rows other ranks own; the formulas are in
// include/csn_hip.h.
//   csn_contrastive_lse    cl_norm_kernel      |s_j|, 1 / max(|s_j|, eps), 1 / max(|t_j|, eps) of all N rows, a wave per row
//                          cl_logit_kernel<0>  per (row tile, key tile, direction): the tile's (max, sum exp) of every row
//                          cl_lse_finish       merges the key tiles in ascending order: lA, lB, p and the loss partial
//   csn_contrastive_grad   cl_norm_kernel
//                          cl_logit_kernel<1>  W[i,j] = w_a PA_ij + w_b PB_ji for local i and all j (one logit serves both);
//                                              with dscale_part the row sums of PA d and (direction 1) of PB d per key tile
//                          cl_ds_kernel        sum_j W[i,j] t^_j over a split of 256 keys (blockIdx.z), float64 partials
//                          cl_ds_finish        splits in ascending order, - (w_a + w_b) t^_i, through the normalisation, ds
//                          cl_dscale_finish    (with dscale_part) the row sums in ascending tile order, then over the rows
// The contractions are bt_tile (bt_tile.h): operands staged already normalised, one fma chain per result in ascending order.
// Every log-sum-exp subtracts its maximum.  A key that is left out is never put through exp: its term is the constant 0.
// No atomics, no waits between workgroups; every loop is bounded by B, N or D.  What a row's outputs go through depends on
// its place in a tile only by WHICH thread computes them, never in which order: lA, lB, p and ds of a row depend on (N, D)
// and the data alone.
#include <math.h>

#include "bt_tile.h"

namespace csn {
namespace cl {

using bt::bt_tile;
using bt::wave_sum;
using bt::KS;
using bt::LDK;
using bt::TILE_LDS_DOUBLES;

constexpr double EPS = 1e-12;       // F.normalize
constexpr int SPLIT = 256;          // keys per split of the ds contraction: the split depends on N only
constexpr int FIN = 256;            // threads of the single-workgroup finish kernels

static inline int key_tiles(int N) { return (N + 63) / 64; }
static inline int splits(int N) { return (N + SPLIT - 1) / SPLIT; }

// scratch, in doubles: rn_s[N] rn_t[N] nrm_s[N] | tiles[4 KT B] | diag[B] | W[B N] | part[S B D]
struct Scratch {
  double *rn_s, *rn_t, *nrm_s, *tiles, *diag, *W, *part;
  __host__ Scratch(void* p, int B, int N, int D) {
    double* d = (double*)p;
    rn_s = d; rn_t = d + N; nrm_s = d + 2 * (size_t)N;
    tiles = d + 3 * (size_t)N;
    diag = tiles + 4 * (size_t)key_tiles(N) * B;
    W = diag + B;
    part = W + (size_t)B * N;
  }
  static size_t doubles(int B, int N, int D) {
    return 3 * (size_t)N + 4 * (size_t)key_tiles(N) * B + (size_t)B + (size_t)B * N + (size_t)splits(N) * B * D;
  }
};

// Rows 0 .. N-1: s, rows N .. 2N-1: t.  Lane l adds the squares of elements l, l + 64, ... in ascending order, then the
// butterfly: an order that depends on D only.  A NaN norm stays NaN (torch's clamp_min propagates it).
__global__ void __launch_bounds__(256) cl_norm_kernel(const float* __restrict__ s, const float* __restrict__ t, int N, int D,
                                                      double* __restrict__ rn_s, double* __restrict__ rn_t,
                                                      double* __restrict__ nrm_s) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= 2 * N) return;
  const float* x = row < N ? s + (int64_t)row * D : t + (int64_t)(row - N) * D;
  double q = 0.0;
  for (int d = lane; d < D; d += 64) {
    const double v = (double)x[d];
    q = fma(v, v, q);
  }
  const double nrm = sqrt(wave_sum(q));
  if (lane == 0) {
    const double rn = 1.0 / (nrm < EPS ? EPS : nrm);
    if (row < N) {
      rn_s[row] = rn;
      nrm_s[row] = nrm;
    } else {
      rn_t[row - N] = rn;
    }
  }
}

struct LogitArgs {
  const float* s;
  const float* t;
  const int* group;           // NULL: nothing is left out
  int N, D, row0, B;
  double scale, w_a, w_b;
  const double *rn_s, *rn_t;
  // WHAT 0 (lse): (max, sum exp) of every row per key tile, [dir][kt][B][2]; p of the local rows
  double* tiles;
  double* p_out;
  // WHAT 1 (grad)
  const double* lse_a;        // [B]
  const double* lse_b;        // [N]
  double* W;                  // [B,N]
  double* rowsum;             // NULL, or [dir][kt][B]
  double* diag;               // with rowsum: s^_i . t^_i of the local rows
};

// The four partners of a tile row are the 16 lanes that share tid >> 4.
__device__ __forceinline__ double row_max(double v) {
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ double row_sum(double v) {
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// grid (key tiles, row tiles, directions).  Direction 0: queries s^ of the local rows against keys t^ of all rows;
// direction 1: queries t^ of the local rows against keys s^ of all rows.
template <int WHAT>
__global__ void __launch_bounds__(256) cl_logit_kernel(const LogitArgs a) {
  __shared__ __attribute__((aligned(16))) double lds[TILE_LDS_DOUBLES];
  double* as = lds;
  double* bs = lds + KS * LDK;
  const int tid = threadIdx.x, tq = tid >> 4, tg = tid & 15;
  const int N = a.N, D = a.D, B = a.B;
  const int dir = blockIdx.z, kt = blockIdx.x;
  const int r0 = blockIdx.y * 64, c0 = kt * 64;
  const float* q = dir == 0 ? a.s : a.t;
  const float* k = dir == 0 ? a.t : a.s;
  const double* rn_q = dir == 0 ? a.rn_s : a.rn_t;
  const double* rn_k = dir == 0 ? a.rn_t : a.rn_s;
  double acc[4][4];
  bt_tile<true, true>(acc, as, bs, tid, D,
                      [&](int d, int r) {
                        const int row = a.row0 + r0 + r;
                        return (r0 + r < B && d < D) ? (double)q[(int64_t)row * D + d] * rn_q[row] : 0.0;
                      },
                      [&](int d, int r) {
                        const int col = c0 + r;
                        return (col < N && d < D) ? (double)k[(int64_t)col * D + d] * rn_k[col] : 0.0;
                      });
  int gcol[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = c0 + tg * 4 + j;
    gcol[j] = (a.group != nullptr && col < N) ? a.group[col] : 0;
  }
  const int nkt = gridDim.x;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = r0 + tq * 4 + i;             // local row; every lane goes through the shuffles
    const int row = a.row0 + r;                // global row
    const bool live = r < B;
    const int grow = (a.group != nullptr && live) ? a.group[row] : 0;
    bool allowed[4];
    double z[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = c0 + tg * 4 + j;
      allowed[j] = live && col < N && (a.group == nullptr || col == row || gcol[j] != grow);
      z[j] = a.scale * acc[i][j];
    }
    if constexpr (WHAT == 0) {
      double m = -INFINITY;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (allowed[j]) m = fmax(m, z[j]);
      m = row_max(m);
      double e = 0.0;
#pragma unroll
      for (int j = 0; j < 4; ++j) e += allowed[j] ? exp(z[j] - m) : 0.0;
      e = row_sum(e);
      if (live && tg == 0) {
        double* out = a.tiles + (((size_t)dir * nkt + kt) * B + r) * 2;
        out[0] = m;
        out[1] = e;
      }
      if (dir == 0 && live)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (c0 + tg * 4 + j == row) a.p_out[r] = z[j];
    } else {
      if (dir == 0) {
        const double la = live ? a.lse_a[r] : 0.0;
        double ps = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int col = c0 + tg * 4 + j;
          double w = 0.0;
          if (allowed[j]) {
            const double pa = exp(z[j] - la);
            w = a.w_a * pa + a.w_b * exp(z[j] - a.lse_b[col]);
            ps = fma(pa, acc[i][j], ps);
          }
          if (live && col < N) a.W[(size_t)r * N + col] = w;
          if (a.rowsum != nullptr && live && col == row) a.diag[r] = acc[i][j];
        }
        if (a.rowsum != nullptr) {
          ps = row_sum(ps);
          if (live && tg == 0) a.rowsum[(size_t)kt * B + r] = ps;
        }
      } else {                                  // only launched with rowsum
        const double lb = live ? a.lse_b[row] : 0.0;
        double ps = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (allowed[j]) ps = fma(exp(z[j] - lb), acc[i][j], ps);
        ps = row_sum(ps);
        if (live && tg == 0) a.rowsum[((size_t)nkt + kt) * B + r] = ps;
      }
    }
  }
}

// The sum of v over the workgroup in a fixed tree; every thread calls it.
__device__ __forceinline__ double block_sum(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int off = FIN / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  return red[0];
}

// One workgroup.  Thread x owns the rows x, x + 256, ...: per direction the maximum of the tiles' maxima, then
// sum_kt e_kt exp(m_kt - M) in ascending kt (an order fixed by N), l = M + log(sum).  The loss terms are added per thread in
// ascending row order and then in the tree of block_sum: an order that depends on B only.
__global__ void __launch_bounds__(FIN) cl_lse_finish(const double* __restrict__ tiles, int nkt, int B, double w_a, double w_b,
                                                      double inv_N, double* __restrict__ rows_out,
                                                      double* __restrict__ loss_part) {
  __shared__ double red[FIN];
  double total = 0.0;
  for (int r = threadIdx.x; r < B; r += FIN) {
    double l[2];
    for (int dir = 0; dir < 2; ++dir) {
      const double* tl = tiles + ((size_t)dir * nkt * B + r) * 2;
      double M = -INFINITY;
      for (int kt = 0; kt < nkt; ++kt) M = fmax(M, tl[(size_t)kt * B * 2]);
      double S = 0.0;
      for (int kt = 0; kt < nkt; ++kt) {
        const double m = tl[(size_t)kt * B * 2], e = tl[(size_t)kt * B * 2 + 1];
        if (m != -INFINITY || e != 0.0) S = fma(e, exp(m - M), S);      // a tile with every key left out adds nothing
      }
      l[dir] = M + log(S);
      rows_out[(size_t)dir * B + r] = l[dir];
    }
    const double p = rows_out[(size_t)2 * B + r];
    total += w_a * (l[0] - p) + w_b * (l[1] - p);
  }
  total = block_sum(total, red);
  if (threadIdx.x == 0) loss_part[0] = total * inv_N;
}

struct DsArgs {
  const float* s;
  const float* t;
  int N, D, row0, B;
  const double *rn_s, *rn_t, *nrm_s;
  const double* W;
  double* part;               // [S][B][D]
  double coef;                // logit_scale / N
  double wsum;                // w_a + w_b
  double grad_scale;
  float* ds;
};

// part[z][i][d] = sum over the keys j of split z of W[i,j] t^_j[d]; grid (cdiv(D,64), cdiv(B,64), splits).
__global__ void __launch_bounds__(256) cl_ds_kernel(const DsArgs a) {
  __shared__ __attribute__((aligned(16))) double lds[TILE_LDS_DOUBLES];
  double* as = lds;
  double* bs = lds + KS * LDK;
  const int tid = threadIdx.x, tq = tid >> 4, tg = tid & 15;
  const int N = a.N, D = a.D, B = a.B;
  const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
  const int k_lo = blockIdx.z * SPLIT;
  const int klen = min(SPLIT, N - k_lo);
  double acc[4][4];
  bt_tile<true, false>(acc, as, bs, tid, klen,
                       [&](int k, int r) { return (r0 + r < B && k < klen) ? a.W[(size_t)(r0 + r) * N + k_lo + k] : 0.0; },
                       [&](int k, int r) {
                         const int j = k_lo + k, d = c0 + r;
                         return (k < klen && d < D) ? (double)a.t[(int64_t)j * D + d] * a.rn_t[j] : 0.0;
                       });
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = r0 + tq * 4 + i, d = c0 + tg * 4 + j;
      if (r < B && d < D) a.part[((size_t)blockIdx.z * B + r) * D + d] = acc[i][j];
    }
}

// A wave per local row.  g[d] = coef (sum_z part[z][i][d] - wsum t^_i[d]) with the splits in ascending order and the
// product rounded on its own (a row with every other key left out then gives exactly 0); through the normalisation:
//   ds[d] = fl32( grad_scale (g[d] - s^[d] (s^ . g)) / max(|s|, eps) ),  the projection only where |s| > eps.
__global__ void __launch_bounds__(256) cl_ds_finish(const DsArgs a, int nsplit) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= a.B) return;
  const int D = a.D, row = a.row0 + r;
  const double rs = a.rn_s[row], rt = a.rn_t[row];
  auto g_of = [&](int d) {
    double v = a.part[(size_t)r * D + d];
    for (int z = 1; z < nsplit; ++z) v += a.part[((size_t)z * a.B + r) * D + d];
    return a.coef * (v - __dmul_rn(a.wsum, (double)a.t[(int64_t)row * D + d] * rt));
  };
  double dot = 0.0;
  if (a.nrm_s[row] > EPS) {
    for (int d = lane; d < D; d += 64) dot = fma((double)a.s[(int64_t)row * D + d] * rs, g_of(d), dot);
    dot = wave_sum(dot);
  }
  for (int d = lane; d < D; d += 64) {
    const double sh = (double)a.s[(int64_t)row * D + d] * rs;
    a.ds[(size_t)r * D + d] = (float)(a.grad_scale * ((g_of(d) - __dmul_rn(sh, dot)) * rs));
  }
}

// One workgroup: per local row the tiles' sums in ascending order, the terms added as in cl_lse_finish.
__global__ void __launch_bounds__(FIN) cl_dscale_finish(const double* __restrict__ rowsum, const double* __restrict__ diag,
                                                         int nkt, int B, double w_a, double w_b, double inv_N,
                                                         double* __restrict__ dscale_part) {
  __shared__ double red[FIN];
  double total = 0.0;
  for (int r = threadIdx.x; r < B; r += FIN) {
    double sa = 0.0, sb = 0.0;
    for (int kt = 0; kt < nkt; ++kt) {
      sa += rowsum[(size_t)kt * B + r];
      sb += rowsum[((size_t)nkt + kt) * B + r];
    }
    total += w_a * (sa - diag[r]) + w_b * (sb - diag[r]);
  }
  total = block_sum(total, red);
  if (threadIdx.x == 0) dscale_part[0] = total * inv_N;
}

static inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }
static inline bool shape_ok(int B, int N, int D) { return B > 0 && N > 0 && D > 0 && B <= N; }

}  // namespace cl
}  // namespace csn

using namespace csn;

extern "C" size_t csn_contrastive_scratch_bytes(int B, int N, int D) {
  return cl::shape_ok(B, N, D) ? cl::Scratch::doubles(B, N, D) * sizeof(double) : 0;
}

#define CL_REQUIRE_COMMON(who)                                                                                              \
  CSN_REQUIRE(N > 0 && D > 0 && B > 0 && row0 >= 0 && (int64_t)row0 + B <= N,                                               \
              who ": bad shape N=%d D=%d row0=%d B=%d (the local rows are row0 .. row0+B-1 of the N global rows)", N, D,    \
              row0, B);                                                                                                     \
  CSN_REQUIRE(isfinite(logit_scale) && logit_scale > 0.0, who ": logit_scale must be finite and positive, got %g",          \
              logit_scale);                                                                                                 \
  CSN_REQUIRE(isfinite(w_a) && isfinite(w_b), who ": the weights must be finite, got %g and %g", w_a, w_b)

extern "C" int csn_contrastive_lse(const float* s_all, const float* t_all, const int* group_all, int N, int D, int row0, int B,
                                   double logit_scale, double w_a, double w_b, double* rows_out, double* loss_part,
                                   void* scratch, csnStream_t stream) {
  CSN_REQUIRE(s_all && t_all && rows_out && loss_part && scratch, "csn_contrastive_lse: null pointer");
  CL_REQUIRE_COMMON("csn_contrastive_lse");
  CSN_REQUIRE(cl::aligned8(rows_out) && cl::aligned8(loss_part) && cl::aligned8(scratch),
              "csn_contrastive_lse: rows_out, loss_part and scratch must be 8-byte aligned");
  hipStream_t st = as_stream(stream);
  const cl::Scratch sc(scratch, B, N, D);
  const int nkt = cl::key_tiles(N);
  cl::cl_norm_kernel<<<(unsigned)((2 * (int64_t)N + 3) / 4), 256, 0, st>>>(s_all, t_all, N, D, sc.rn_s, sc.rn_t, sc.nrm_s);
  CSN_LAUNCH_CHECK();
  cl::LogitArgs a{};
  a.s = s_all; a.t = t_all; a.group = group_all; a.N = N; a.D = D; a.row0 = row0; a.B = B;
  a.scale = logit_scale; a.w_a = w_a; a.w_b = w_b; a.rn_s = sc.rn_s; a.rn_t = sc.rn_t;
  a.tiles = sc.tiles; a.p_out = rows_out + 2 * (size_t)B;
  cl::cl_logit_kernel<0><<<dim3((unsigned)nkt, (unsigned)((B + 63) / 64), 2), 256, 0, st>>>(a);
  CSN_LAUNCH_CHECK();
  cl::cl_lse_finish<<<1, cl::FIN, 0, st>>>(sc.tiles, nkt, B, w_a, w_b, 1.0 / (double)N, rows_out, loss_part);
  CSN_LAUNCH_CHECK();
  return CSN_OK;
}

extern "C" int csn_contrastive_grad(const float* s_all, const float* t_all, const int* group_all, int N, int D, int row0,
                                    int B, double logit_scale, const double* lse_a_local, const double* lse_b_all, double w_a,
                                    double w_b, double grad_scale, float* ds, double* dscale_part, void* scratch,
                                    csnStream_t stream) {
  CSN_REQUIRE(s_all && t_all && lse_a_local && lse_b_all && ds && scratch, "csn_contrastive_grad: null pointer");
  CL_REQUIRE_COMMON("csn_contrastive_grad");
  CSN_REQUIRE(cl::aligned8(lse_a_local) && cl::aligned8(lse_b_all) && cl::aligned8(dscale_part) && cl::aligned8(scratch),
              "csn_contrastive_grad: lse_a_local, lse_b_all, dscale_part and scratch must be 8-byte aligned");
  hipStream_t st = as_stream(stream);
  const cl::Scratch sc(scratch, B, N, D);
  const int nkt = cl::key_tiles(N), nsplit = cl::splits(N);
  const unsigned row_tiles = (unsigned)((B + 63) / 64);
  cl::cl_norm_kernel<<<(unsigned)((2 * (int64_t)N + 3) / 4), 256, 0, st>>>(s_all, t_all, N, D, sc.rn_s, sc.rn_t, sc.nrm_s);
  CSN_LAUNCH_CHECK();
  cl::LogitArgs a{};
  a.s = s_all; a.t = t_all; a.group = group_all; a.N = N; a.D = D; a.row0 = row0; a.B = B;
  a.scale = logit_scale; a.w_a = w_a; a.w_b = w_b; a.rn_s = sc.rn_s; a.rn_t = sc.rn_t;
  a.lse_a = lse_a_local; a.lse_b = lse_b_all; a.W = sc.W;
  a.rowsum = dscale_part != nullptr ? sc.tiles : nullptr;
  a.diag = sc.diag;
  cl::cl_logit_kernel<1><<<dim3((unsigned)nkt, row_tiles, dscale_part != nullptr ? 2u : 1u), 256, 0, st>>>(a);
  CSN_LAUNCH_CHECK();
  cl::DsArgs d{};
  d.s = s_all; d.t = t_all; d.N = N; d.D = D; d.row0 = row0; d.B = B;
  d.rn_s = sc.rn_s; d.rn_t = sc.rn_t; d.nrm_s = sc.nrm_s; d.W = sc.W; d.part = sc.part;
  d.coef = logit_scale / (double)N; d.wsum = w_a + w_b; d.grad_scale = grad_scale; d.ds = ds;
  cl::cl_ds_kernel<<<dim3((unsigned)((D + 63) / 64), row_tiles, (unsigned)nsplit), 256, 0, st>>>(d);
  CSN_LAUNCH_CHECK();
  cl::cl_ds_finish<<<(unsigned)((B + 3) / 4), 256, 0, st>>>(d, nsplit);
  CSN_LAUNCH_CHECK();
  if (dscale_part != nullptr) {
    cl::cl_dscale_finish<<<1, cl::FIN, 0, st>>>(sc.tiles, sc.diag, nkt, B, w_a, w_b, 1.0 / (double)N, dscale_part);
    CSN_LAUNCH_CHECK();
  }
  return CSN_OK;
}
