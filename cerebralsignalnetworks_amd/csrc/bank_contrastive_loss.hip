// K7d: the contrastive (InfoNCE) loss of student rows against a fixed BANK of teacher rows -- every image of the dataset a
// negative at every step -- value and gradient in float64.  The formulas are in include/csn_hip.h.
//   csn_bank_norms        bc_norm_kernel     1 / max(|t_m|, eps) of the M bank rows, a wave per row; once per bank
//   csn_bank_contrastive  bc_norm_kernel     |s_i| and 1 / max(|s_i|, eps) of the B student rows
//                         bc_logit_kernel    Z[i,m] = s^_i . t^_m, a 64 x 64 tile per workgroup (bt_tile), or
//                         bc_logit_small     the same bits on 16 x 16 tiles where the 64 x 64 grid would leave the chip idle
//                         bc_row_kernel      a workgroup per query: the maximum, the sum of exp, l and p; with a gradient the
//                                            row of Z becomes the row of P in place, and sum_m P_im s^_i . t^_m
//                         bc_sum_finish      the loss partial (and dscale_part) over the B rows
//                         bc_ds_kernel       sum_m P[i,m] t^_m over a split of the keys (blockIdx.z), float64 partials
//                         bc_ds_finish       splits in ascending order, - t^_pos, through the normalisation, ds
// The logit kernels only contract: one fma chain per logit in ascending d, whatever the tile, so the tile shape is free to
// follow B.  Everything that sums over keys runs per row in an order fixed by M alone: thread x of the row's workgroup adds
// keys x, x + 256, ... in ascending order, then the tree of block_sum; the ds contraction is split into splits(M) runs of
// split_width(M) keys, each one fma chain, merged in ascending order.  So l, p and ds of a row depend on (M, D), the scalars
// and the data alone, not on B or on the row's place in the batch.
// Every log-sum-exp subtracts its maximum.  A key that is left out is never put through exp: its weight is the constant 0,
// and the ds contraction stages a non-finite t^ as 0 -- a query that may see such a key has a NaN l and with it a NaN weight
// for every key, so its ds row is NaN whatever is staged, and a query that leaves the key out gets exactly nothing from it.
// No atomics, no waits between workgroups; every loop is bounded by B, M or D.
#include <math.h>

#include "bt_tile.h"

namespace csn {
namespace bc {

using bt::bt_tile;
using bt::wave_sum;
using bt::KS;
using bt::LDK;
using bt::TILE_LDS_DOUBLES;

constexpr double EPS = 1e-12;       // F.normalize
constexpr int WG = 256;             // threads of the row and finish kernels
constexpr int ST = 16, SLD = 17;    // the small logit tile: 16 x 16 results, staged [k][row] with rows of 17 doubles
constexpr int FILL = 128;           // 64 x 64 logit tiles below which the 16 x 16 tiles are launched instead

// keys per split of the ds contraction and their number: functions of M alone.  64 keys up to M = 4096, then as many
// (a multiple of the staging slice) as keep the splits at 64 or fewer.
static inline int split_width(int M) {
  const int w = 32 * ((M + 2047) / 2048);
  return w < 64 ? 64 : w;
}
static inline int splits(int M) { return (M + split_width(M) - 1) / split_width(M); }

// scratch, in doubles: rn_s[B] nrm_s[B] term[B] dsc[B] | Z[B M] | part[S B D]
struct Scratch {
  double *rn_s, *nrm_s, *term, *dsc, *Z, *part;
  __host__ Scratch(void* p, int B, int M, int D) {
    double* d = (double*)p;
    rn_s = d; nrm_s = d + B; term = d + 2 * (size_t)B; dsc = d + 3 * (size_t)B;
    Z = d + 4 * (size_t)B;
    part = Z + (size_t)B * M;
  }
  static size_t doubles(int B, int M, int D) { return 4 * (size_t)B + (size_t)B * M + (size_t)splits(M) * B * D; }
};

// Lane l adds the squares of elements l, l + 64, ... in ascending order, then the butterfly: an order that depends on D
// only.  A NaN norm stays NaN (torch's clamp_min propagates it).  nrm may be NULL.
__global__ void __launch_bounds__(256) bc_norm_kernel(const float* __restrict__ x, int R, int D, double* __restrict__ rn,
                                                      double* __restrict__ nrm) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const float* xr = x + (int64_t)row * D;
  double q = 0.0;
  for (int d = lane; d < D; d += 64) {
    const double v = (double)xr[d];
    q = fma(v, v, q);
  }
  const double n = sqrt(wave_sum(q));
  if (lane == 0) {
    rn[row] = 1.0 / (n < EPS ? EPS : n);
    if (nrm != nullptr) nrm[row] = n;
  }
}

struct LogitArgs {
  const float* s;
  const float* bank;
  int B, M, D;
  const double *rn_s, *rn_b;
  double* Z;                  // [B,M]
};

// grid (key tiles, row tiles), 64 x 64 logits per workgroup.
__global__ void __launch_bounds__(256) bc_logit_kernel(const LogitArgs a) {
  __shared__ __attribute__((aligned(16))) double lds[TILE_LDS_DOUBLES];
  double* as = lds;
  double* bs = lds + KS * LDK;
  const int tid = threadIdx.x, tq = tid >> 4, tg = tid & 15;
  const int B = a.B, M = a.M, D = a.D;
  const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
  double acc[4][4];
  bt_tile<true, true>(acc, as, bs, tid, D,
                      [&](int d, int r) {
                        const int row = r0 + r;
                        return (row < B && d < D) ? (double)a.s[(int64_t)row * D + d] * a.rn_s[row] : 0.0;
                      },
                      [&](int d, int r) {
                        const int col = c0 + r;
                        return (col < M && d < D) ? (double)a.bank[(int64_t)col * D + d] * a.rn_b[col] : 0.0;
                      });
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = r0 + tq * 4 + i, col = c0 + tg * 4 + j;
      if (r < B && col < M) a.Z[(size_t)r * M + col] = acc[i][j];
    }
}

// grid (key tiles, row tiles), 16 x 16 logits per workgroup, one per thread: the chain of bt_tile -- from 0.0, ascending d in
// slices of 32 with zeros behind D -- so the bits are those of bc_logit_kernel.
__global__ void __launch_bounds__(256) bc_logit_small(const LogitArgs a) {
  __shared__ double as[KS * SLD];
  __shared__ double bs[KS * SLD];
  const int tid = threadIdx.x, tr = tid >> 4, tc = tid & 15;
  const int B = a.B, M = a.M, D = a.D;
  const int r0 = blockIdx.y * ST, c0 = blockIdx.x * ST;
  double acc = 0.0;
  for (int d0 = 0; d0 < D; d0 += KS) {
    __syncthreads();          // the previous slice's reads are done
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int e = tid + 256 * j, k = e & (KS - 1), r = e >> 5, d = d0 + k;
      const int row = r0 + r, col = c0 + r;
      as[k * SLD + r] = (row < B && d < D) ? (double)a.s[(int64_t)row * D + d] * a.rn_s[row] : 0.0;
      bs[k * SLD + r] = (col < M && d < D) ? (double)a.bank[(int64_t)col * D + d] * a.rn_b[col] : 0.0;
    }
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < KS; ++k) acc = fma(as[k * SLD + tr], bs[k * SLD + tc], acc);
  }
  const int r = r0 + tr, col = c0 + tc;
  if (r < B && col < M) a.Z[(size_t)r * M + col] = acc;
}

// The sum / maximum of v over the workgroup in a fixed tree; every thread calls them.
__device__ __forceinline__ double block_sum(double v, double* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int off = WG / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  return red[0];
}
__device__ __forceinline__ double block_max(double v, double* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int off = WG / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + off]);
    __syncthreads();
  }
  return red[0];
}

struct RowArgs {
  double* Z;                  // [B,M]: the dot products in, with want_w the weights P out
  const int* group;           // NULL: nothing is left out
  const int* pos;
  int B, M;
  double scale;
  int want_w;
  double* rows_out;           // [2][B]: l, p
  double* term;               // [B]: l - p
  double* dsc;                // [B]: sum_m P_im d_im - d_i,pos
};

// A workgroup per query i.  The logit is the product scale * d rounded on its own, so the positive's logit minus the
// maximum is exactly 0 where the positive is the only key: l = p bit for bit, P = 1 on it.  A pos outside [0, M) makes l, p
// and every weight NaN and indexes nothing.
__global__ void __launch_bounds__(WG) bc_row_kernel(const RowArgs a) {
  __shared__ double red[WG];
  const int tid = threadIdx.x, i = blockIdx.x, M = a.M;
  double* zr = a.Z + (size_t)i * M;
  const int pi = a.pos[i];
  const bool valid = pi >= 0 && pi < M;
  const bool masked = a.group != nullptr && valid;
  const int gpos = masked ? a.group[pi] : 0;
  const double d_pos = valid ? zr[pi] : NAN;
  auto allowed = [&](int m) { return !masked || m == pi || a.group[m] != gpos; };
  double mx = -INFINITY;
  for (int m = tid; m < M; m += WG)
    if (allowed(m)) mx = fmax(mx, __dmul_rn(a.scale, zr[m]));
  mx = block_max(mx, red);
  double e = 0.0;
  for (int m = tid; m < M; m += WG)
    if (allowed(m)) e += exp(__dmul_rn(a.scale, zr[m]) - mx);
  e = block_sum(e, red);
  const double l = valid ? mx + log(e) : NAN;
  const double p = __dmul_rn(a.scale, d_pos);
  double ps = 0.0;
  if (a.want_w) {             // (every thread read d_pos before the reductions' barriers)
    for (int m = tid; m < M; m += WG) {
      const double d = zr[m];
      double w = 0.0;
      if (allowed(m)) {
        w = exp(__dmul_rn(a.scale, d) - l);
        ps = fma(w, d, ps);
      }
      zr[m] = w;
    }
    ps = block_sum(ps, red);
  }
  if (tid == 0) {
    a.rows_out[i] = l;
    a.rows_out[(size_t)a.B + i] = p;
    a.term[i] = l - p;
    a.dsc[i] = ps - d_pos;
  }
}

// One workgroup.  The rows' terms are added per thread in ascending row order and then in the tree of block_sum: an order
// that depends on B only.
__global__ void __launch_bounds__(WG) bc_sum_finish(const double* __restrict__ term, const double* __restrict__ dsc, int B,
                                                     double inv_rows, double* __restrict__ loss_part,
                                                     double* __restrict__ dscale_part) {
  __shared__ double red[WG];
  double t = 0.0, s = 0.0;
  for (int r = threadIdx.x; r < B; r += WG) {
    t += term[r];
    if (dscale_part != nullptr) s += dsc[r];
  }
  t = block_sum(t, red);
  if (threadIdx.x == 0) loss_part[0] = t * inv_rows;
  if (dscale_part != nullptr) {
    s = block_sum(s, red);
    if (threadIdx.x == 0) dscale_part[0] = s * inv_rows;
  }
}

struct DsArgs {
  const float* s;
  const float* bank;
  const int* pos;
  int B, M, D, width;         // width: keys per split
  const double *rn_s, *nrm_s, *rn_b;
  const double* W;            // [B,M]
  double* part;               // [S][B][D]
  double coef;                // logit_scale * inv_rows
  double grad_scale;
  float* ds;
};

// part[z][i][d] = sum over the keys m of split z of P[i,m] t^_m[d]; grid (cdiv(D,64), cdiv(B,64), splits).
__global__ void __launch_bounds__(256) bc_ds_kernel(const DsArgs a) {
  __shared__ __attribute__((aligned(16))) double lds[TILE_LDS_DOUBLES];
  double* as = lds;
  double* bs = lds + KS * LDK;
  const int tid = threadIdx.x, tq = tid >> 4, tg = tid & 15;
  const int B = a.B, M = a.M, D = a.D;
  const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
  const int k_lo = blockIdx.z * a.width;
  const int klen = min(a.width, M - k_lo);
  double acc[4][4];
  bt_tile<true, false>(acc, as, bs, tid, klen,
                       [&](int k, int r) { return (r0 + r < B && k < klen) ? a.W[(size_t)(r0 + r) * M + k_lo + k] : 0.0; },
                       [&](int k, int r) {
                         const int m = k_lo + k, d = c0 + r;
                         if (k >= klen || d >= D) return 0.0;
                         const double v = (double)a.bank[(int64_t)m * D + d] * a.rn_b[m];
                         return isfinite(v) ? v : 0.0;
                       });
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = r0 + tq * 4 + i, d = c0 + tg * 4 + j;
      if (r < B && d < D) a.part[((size_t)blockIdx.z * B + r) * D + d] = acc[i][j];
    }
}

// A wave per row.  g[d] = coef (sum_z part[z][i][d] - t^_pos[d]) with the splits in ascending order and t^_pos the product
// rounded on its own, as the contraction staged it (a row whose only key is its positive then gives exactly 0); through
// the normalisation:  ds[d] = fl32( grad_scale (g[d] - s^[d] (s^ . g)) / max(|s|, eps) ),  the projection only where
// |s| > eps.  A pos outside [0, M): a NaN row, nothing indexed.
__global__ void __launch_bounds__(256) bc_ds_finish(const DsArgs a, int nsplit) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= a.B) return;
  const int D = a.D, pi = a.pos[r];
  float* out = a.ds + (size_t)r * D;
  if (pi < 0 || pi >= a.M) {
    for (int d = lane; d < D; d += 64) out[d] = NAN;
    return;
  }
  const double rs = a.rn_s[r], rb = a.rn_b[pi];
  const float* sr = a.s + (int64_t)r * D;
  const float* tp = a.bank + (int64_t)pi * D;
  auto g_of = [&](int d) {
    double v = a.part[(size_t)r * D + d];
    for (int z = 1; z < nsplit; ++z) v += a.part[((size_t)z * a.B + r) * D + d];
    return a.coef * (v - __dmul_rn((double)tp[d], rb));
  };
  double dot = 0.0;
  if (a.nrm_s[r] > EPS) {
    for (int d = lane; d < D; d += 64) dot = fma((double)sr[d] * rs, g_of(d), dot);
    dot = wave_sum(dot);
  }
  for (int d = lane; d < D; d += 64) {
    const double sh = (double)sr[d] * rs;
    out[d] = (float)(a.grad_scale * ((g_of(d) - __dmul_rn(sh, dot)) * rs));
  }
}

static inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }
constexpr int MAX_B = 65535 * ST;  // the row tiles are blockIdx.y
static inline bool shape_ok(int B, int M, int D) { return B > 0 && B <= MAX_B && M > 0 && D > 0; }

}  // namespace bc
}  // namespace csn

using namespace csn;

extern "C" int csn_bank_norms(const float* bank, int M, int D, double* inv_norm, csnStream_t stream) {
  CSN_REQUIRE(bank && inv_norm, "csn_bank_norms: null pointer");
  CSN_REQUIRE(M > 0 && D > 0, "csn_bank_norms: bad shape M=%d D=%d", M, D);
  CSN_REQUIRE(bc::aligned8(inv_norm), "csn_bank_norms: inv_norm must be 8-byte aligned");
  bc::bc_norm_kernel<<<(unsigned)(((int64_t)M + 3) / 4), 256, 0, as_stream(stream)>>>(bank, M, D, inv_norm, nullptr);
  CSN_LAUNCH_CHECK();
  return CSN_OK;
}

extern "C" size_t csn_bank_contrastive_scratch_bytes(int B, int M, int D) {
  return bc::shape_ok(B, M, D) ? bc::Scratch::doubles(B, M, D) * sizeof(double) : 0;
}

extern "C" int csn_bank_contrastive(const float* s, int B, int D, const float* bank, const double* bank_inv_norm,
                                    const int32_t* bank_group, int M, const int32_t* pos, double logit_scale, double inv_rows,
                                    double grad_scale, double* rows_out, double* loss_part, float* ds, double* dscale_part,
                                    void* scratch, csnStream_t stream) {
  CSN_REQUIRE(s && bank && bank_inv_norm && pos && rows_out && loss_part && scratch, "csn_bank_contrastive: null pointer");
  CSN_REQUIRE(bc::shape_ok(B, M, D), "csn_bank_contrastive: bad shape B=%d M=%d D=%d (B at most %d)", B, M, D, bc::MAX_B);
  CSN_REQUIRE(isfinite(logit_scale) && logit_scale > 0.0, "csn_bank_contrastive: logit_scale must be finite and positive, got %g",
              logit_scale);
  CSN_REQUIRE(isfinite(inv_rows) && isfinite(grad_scale), "csn_bank_contrastive: inv_rows and grad_scale must be finite, got %g and %g",
              inv_rows, grad_scale);
  CSN_REQUIRE(bc::aligned8(bank_inv_norm) && bc::aligned8(rows_out) && bc::aligned8(loss_part) && bc::aligned8(dscale_part) &&
                  bc::aligned8(scratch),
              "csn_bank_contrastive: bank_inv_norm, rows_out, loss_part, dscale_part and scratch must be 8-byte aligned");
  hipStream_t st = as_stream(stream);
  const bc::Scratch sc(scratch, B, M, D);
  bc::bc_norm_kernel<<<(unsigned)((B + 3) / 4), 256, 0, st>>>(s, B, D, sc.rn_s, sc.nrm_s);
  CSN_LAUNCH_CHECK();
  bc::LogitArgs a{};
  a.s = s; a.bank = bank; a.B = B; a.M = M; a.D = D; a.rn_s = sc.rn_s; a.rn_b = bank_inv_norm; a.Z = sc.Z;
  // CSN_BANK_TILE = 16 / 64 (diagnostic): the logit tile whatever the shape; the bits are the same
  const char* forced = getenv("CSN_BANK_TILE");
  const int64_t wide_tiles = (int64_t)((B + 63) / 64) * ((M + 63) / 64);
  const bool small = forced != nullptr ? atoi(forced) == 16 : wide_tiles < bc::FILL;
  if (small)
    bc::bc_logit_small<<<dim3((unsigned)((M + bc::ST - 1) / bc::ST), (unsigned)((B + bc::ST - 1) / bc::ST)), 256, 0, st>>>(a);
  else
    bc::bc_logit_kernel<<<dim3((unsigned)((M + 63) / 64), (unsigned)((B + 63) / 64)), 256, 0, st>>>(a);
  CSN_LAUNCH_CHECK();
  bc::RowArgs r{};
  r.Z = sc.Z; r.group = bank_group; r.pos = pos; r.B = B; r.M = M; r.scale = logit_scale;
  r.want_w = (ds != nullptr || dscale_part != nullptr) ? 1 : 0;
  r.rows_out = rows_out; r.term = sc.term; r.dsc = sc.dsc;
  bc::bc_row_kernel<<<(unsigned)B, bc::WG, 0, st>>>(r);
  CSN_LAUNCH_CHECK();
  bc::bc_sum_finish<<<1, bc::WG, 0, st>>>(sc.term, sc.dsc, B, inv_rows, loss_part, dscale_part);
  CSN_LAUNCH_CHECK();
  if (ds == nullptr) return CSN_OK;
  const int nsplit = bc::splits(M);
  bc::DsArgs d{};
  d.s = s; d.bank = bank; d.pos = pos; d.B = B; d.M = M; d.D = D; d.width = bc::split_width(M);
  d.rn_s = sc.rn_s; d.nrm_s = sc.nrm_s; d.rn_b = bank_inv_norm; d.W = sc.Z; d.part = sc.part;
  d.coef = logit_scale * inv_rows; d.grad_scale = grad_scale; d.ds = ds;
  bc::bc_ds_kernel<<<dim3((unsigned)((D + 63) / 64), (unsigned)((B + 63) / 64), (unsigned)nsplit), 256, 0, st>>>(d);
  CSN_LAUNCH_CHECK();
  bc::bc_ds_finish<<<(unsigned)((B + 3) / 4), 256, 0, st>>>(d, nsplit);
  CSN_LAUNCH_CHECK();
  return CSN_OK;
}
