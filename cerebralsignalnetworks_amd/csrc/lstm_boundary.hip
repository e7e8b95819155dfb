// The API boundary of the stacked LSTM: the batch-first <-> time-major layout passes around the recurrence and the per-row
// helpers of variable-length batches (lstm_boundary.h; DESIGN.md sections 10, 16, 23, 26 and 28).  All of it is bandwidth-bound
// element movement; the only arithmetic is the float32 multiply of output dropout, the adding stores, the pooled
// readout: its reduction over time and the one float32 add (and, for the mean, one division) of its gradient, and the
// attention readout: float64 scores, softmax and weighted sums over the saved steps, three float32 operations of its gradient.
#include "lstm_boundary.h"

namespace csn {

// one thread and trip of a layout pass: four consecutive h under output dropout (one Philox call, 16-byte accesses of the
// float32 side, 8-byte loads of bf16), else one element
template <typename T> struct Quad;
template <> struct Quad<bf16_t> { typedef bf16x4 type; };
template <> struct Quad<float> { typedef f32x4 type; };

// element (row, h .. h + 3) of the caller's tensor under the mask: kept and scaled, or a selected zero
template <typename V>
__device__ __forceinline__ f32x4 drop_quad(const V v, const OutDropCfg& od, int64_t row, int64_t h) {
  const Philox4 w = dropout_words(od.cfg, (od.first + (uint64_t)row * (uint64_t)od.index_pitch + (uint64_t)h) >> 2);
  f32x4 out;
#pragma unroll
  for (int j = 0; j < 4; ++j) out[j] = (uint64_t)w.w[j] >= od.cfg.thr ? (float)v[j] * od.cfg.scale : 0.f;
  return out;
}

// y_all[b][t][h] (f32, batch-first, pitched) <- h_all[slot(t)][b][h] (dtype, time-major); zeros from a row's length on
template <typename T, bool DROP>
__global__ void __launch_bounds__(256) y_out(const T* __restrict__ h_all, float* __restrict__ y, RowMap m, OutDropCfg od) {
  constexpr int W = DROP ? 4 : 1;
  const int64_t hw = m.H / W, total = (int64_t)m.B * m.Tn * hw;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t h = (i % hw) * W, r = i / hw, t = r % m.Tn, b = r / m.Tn;
    const RowSteps row(m.len, b, m.Tn, m.rev);
    const T* src = h_all + (row.slot(t) * m.B + b) * (int64_t)m.H + h;       // (read under valid(t) only: later steps never ran)
    float* dst = y + r * m.pitch + h;
    if constexpr (DROP) {
      typedef typename Quad<T>::type V;
      f32x4 out = {0.f, 0.f, 0.f, 0.f};
      if (row.valid(t)) out = drop_quad(*reinterpret_cast<const V*>(src), od, r, h);
      *reinterpret_cast<f32x4*>(dst) = out;
    } else {
      *dst = row.valid(t) ? to_f32(*src) : 0.f;
    }
  }
}

// dy_tm[s][b][h] (dense, time-major), s < Te  <-  dy_all[b][t][h] (batch-first, pitched, or null); zeros from a row's length on.
// POOL (csn_lstm_plan_set_readout): the gradient of the pooled y_last joins every valid step in the same store -- one float32
// add behind the (masked) dy_all element, or the term itself where dy is null: dy_last / n under MEAN, dy_last at the caller
// time argmax[b][h] and +0 elsewhere under MAX; under kPoolAttention (csn_lstm_plan_set_attention) the term of a32[b][t],
// w32[b][t], q[h] and dy_last[b][h] below
template <int POOL>
__device__ __forceinline__ float pool_term(const PoolIn& pl, const RowSteps& row, int64_t b, int64_t t, int64_t h, int H, int64_t brow) {
  const float g = pl.dy_last[b * H + h];
  // kPoolAttention (csn_lstm_plan_set_attention): fl32(fl32(a32 dy_last) + fl32(w32 q)), three roundings, never contracted
  if constexpr (POOL == kPoolAttention) return __fadd_rn(__fmul_rn(pl.a32[brow], g), __fmul_rn(pl.w32[brow], pl.q[h]));
  else if constexpr (POOL == CSN_READOUT_MEAN) return g / (float)row.n;
  else return pl.argmax[b * H + h] == (int)t ? g : 0.f;
}
template <bool DROP, int POOL>
__global__ void __launch_bounds__(256) dy_in(const float* __restrict__ dy, float* __restrict__ dy_tm, RowMap m, OutDropCfg od, PoolIn pl) {
  constexpr int W = DROP ? 4 : 1;
  const int64_t hw = m.H / W, total = (int64_t)m.B * m.Te * hw;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t h = (i % hw) * W, r = i / hw, b = r % m.B, s = r / m.B;
    const RowSteps row(m.len, b, m.Tn, m.rev);
    const bool in = dy != nullptr && row.valid(s);
    const int64_t t = row.flip(s), brow = b * m.Tn + t;
    const float* src = dy + brow * m.pitch + h;
    float* dst = dy_tm + i * W;
    if constexpr (DROP) {
      f32x4 out = {0.f, 0.f, 0.f, 0.f};
      if (in) out = drop_quad(*reinterpret_cast<const f32x4*>(src), od, brow, h);
      if constexpr (POOL != CSN_READOUT_LAST) {
        if (row.valid(s)) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float g = pool_term<POOL>(pl, row, b, t, h + j, m.H, brow);
            out[j] = in ? out[j] + g : g;
          }
        }
      }
      *reinterpret_cast<f32x4*>(dst) = out;
    } else {
      float out = in ? *src : 0.f;
      if constexpr (POOL != CSN_READOUT_LAST) {
        if (row.valid(s)) {
          const float g = pool_term<POOL>(pl, row, b, t, h, m.H, brow);
          out = in ? out + g : g;
        }
      }
      *dst = out;
    }
  }
}

// ---- the pooled readout (csn_lstm_plan_set_readout).  A workgroup owns row b and a strip of kPoolLanes
// 16-byte pieces of h; its 256 threads are kPoolLanes lanes along h times kPoolSplit parts of the row's n steps: part k
// takes the caller times t = k, k + kPoolSplit, ... in rising order, the parts are combined through LDS in the order
// k = 0, 1, ... by one thread per column -- a fixed split, so a call gives the same bits every time.
//   MEAN    float64 partial sums, one rounding of sum / n to float32
//   MAX     the value at the first caller time that attains the maximum; a NaN beats every number, the first NaN wins
//   ARGMAX  that caller time as int32 (-1 for an empty row): what dy_in<., MAX> reads, recomputed by the backward
// Empty rows give zeros.
constexpr int kPoolLanes = 8, kPoolSplit = 256 / kPoolLanes;
constexpr int kPoolArgmax = 3;
// does (v, t) come before (bv, bt) as the row's maximum?  (bt < 0: nothing yet)
__device__ __forceinline__ bool pool_before(float v, int t, float bv, int bt) {
  if (bt < 0) return true;
  const bool vn = v != v, bn = bv != bv;
  if (vn != bn) return vn;
  if (!vn && v != bv) return v > bv;
  return t < bt;
}
template <typename T, int MODE>
__global__ void __launch_bounds__(256) pool_readout(const T* __restrict__ h_all, void* __restrict__ out, RowMap m) {
  constexpr int VEC = 16 / (int)sizeof(T), COLS = kPoolLanes * VEC;
  typedef T Piece __attribute__((ext_vector_type(VEC)));
  __shared__ double lds[kPoolSplit * COLS];      // MEAN: [part][col] sums; else [part][col] float values, then int times
  const int lane = threadIdx.x % kPoolLanes, k = threadIdx.x / kPoolLanes;
  const int64_t b = blockIdx.y, h0 = (int64_t)blockIdx.x * COLS + lane * VEC;
  const RowSteps row(m.len, b, m.Tn, m.rev);
  const int n = (int)row.n;
  const bool live = h0 < m.H;      // (H % 32 == 0: a piece lies inside the row or outside it)
  double sum[VEC];
  float best[VEC];
  int at[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    sum[j] = 0.0;
    best[j] = 0.f;
    at[j] = -1;
  }
  for (int t = k; live && t < n; t += kPoolSplit) {
    const Piece v = *reinterpret_cast<const Piece*>(h_all + (row.slot(t) * m.B + b) * (int64_t)m.H + h0);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const float f = to_f32((T)v[j]);
      if constexpr (MODE == CSN_READOUT_MEAN) {
        sum[j] += (double)f;
      } else if (pool_before(f, t, best[j], at[j])) {
        best[j] = f;
        at[j] = t;
      }
    }
  }
  float* lds_v = reinterpret_cast<float*>(lds);
  int* lds_t = reinterpret_cast<int*>(lds_v + kPoolSplit * COLS);
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    const int c = k * COLS + lane * VEC + j;
    if constexpr (MODE == CSN_READOUT_MEAN) {
      lds[c] = sum[j];
    } else {
      lds_v[c] = best[j];
      lds_t[c] = at[j];
    }
  }
  __syncthreads();
  const int c = threadIdx.x;
  const int64_t h = (int64_t)blockIdx.x * COLS + c;
  if (c >= COLS || h >= m.H) return;
  if constexpr (MODE == CSN_READOUT_MEAN) {
    double s = 0.0;
    for (int p = 0; p < kPoolSplit; ++p) s += lds[p * COLS + c];
    static_cast<float*>(out)[b * m.H + h] = n > 0 ? (float)(s / (double)n) : 0.f;
  } else {
    float bv = 0.f;
    int bt = -1;
    for (int p = 0; p < kPoolSplit; ++p) {
      const float v = lds_v[p * COLS + c];
      const int t = lds_t[p * COLS + c];
      if (t >= 0 && pool_before(v, t, bv, bt)) {
        bv = v;
        bt = t;
      }
    }
    if constexpr (MODE == CSN_READOUT_MAX) static_cast<float*>(out)[b * m.H + h] = bv;
    else static_cast<int*>(out)[b * m.H + h] = bt;
  }
}

// ---- the attention readout (csn_lstm_plan_set_attention): y_last[b] = sum over t < n of a[b][t] v[b][t],
// a = softmax over t < n of scale <v[b][t], q>.  Everything between the loads and the one rounding per result is float64,
// every split of a sum is fixed by the shapes, so a call gives the same bits every time.
//
// Scores.  A group of LG lanes (the power of two that covers the row's 16-byte pieces, 64 at the most: 4 lanes at H 32 in
// bf16, so a wave takes 16 (b, t) rows there) owns one (b, t): lane i takes the pieces i, i + LG, ... in rising order into
// a float64 partial, the partials meet in an xor butterfly (offsets LG / 2 ... 1; IEEE addition commutes, so every lane
// holds the same bits).  BWD: g = <dy_last[b], v> from the same load.  Rows from a row's length on are not read or written.
// The trip count is the workgroup's, not the lane's: every lane of a wave reaches every shuffle.
template <typename T, int LG, bool BWD>
__global__ void __launch_bounds__(256) attn_scores(const T* __restrict__ h_all, const float* __restrict__ q, const float* __restrict__ dy_last,
                                                   double scale, double* __restrict__ z, double* __restrict__ g, RowMap m) {
  constexpr int VEC = 16 / (int)sizeof(T), ROWS = 256 / LG;
  typedef T Piece __attribute__((ext_vector_type(VEC)));
  const int lane = threadIdx.x % LG, pieces = m.H / VEC;
  const int64_t total = (int64_t)m.B * m.Tn, stride = (int64_t)gridDim.x * ROWS;
  for (int64_t r0 = (int64_t)blockIdx.x * ROWS; r0 < total; r0 += stride) {
    const int64_t r = r0 + threadIdx.x / LG, b = r / m.Tn, t = r % m.Tn;
    bool on = r < total;
    double sz = 0.0, sg = 0.0;
    if (on) {
      const RowSteps row(m.len, b, m.Tn, m.rev);
      on = row.valid(t);
      if (on) {
        const T* src = h_all + (row.slot(t) * m.B + b) * (int64_t)m.H;
        for (int p = lane; p < pieces; p += LG) {
          const Piece v = *reinterpret_cast<const Piece*>(src + p * VEC);
#pragma unroll
          for (int j = 0; j < VEC; ++j) {
            const double f = (double)to_f32((T)v[j]);
            sz += f * (double)q[p * VEC + j];
            if constexpr (BWD) sg += (double)dy_last[b * m.H + p * VEC + j] * f;
          }
        }
      }
    }
#pragma unroll
    for (int o = LG / 2; o > 0; o >>= 1) {
      sz += __shfl_xor(sz, o, LG);
      if constexpr (BWD) sg += __shfl_xor(sg, o, LG);
    }
    if (on && lane == 0) {
      z[r] = scale * sz;
      if constexpr (BWD) g[r] = sg;
    }
  }
}

// the 256 partials of a workgroup, one per thread, summed (or maximised) by the fixed LDS tree 128, 64, ... 1
template <bool MAX>
__device__ __forceinline__ double attn_tree(double* lds, double v) {
  const int k = threadIdx.x;
  __syncthreads();      // (the previous tree's result has been read)
  lds[k] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (k < o) lds[k] = MAX ? fmax(lds[k], lds[k + o]) : lds[k] + lds[k + o];
    __syncthreads();
  }
  return lds[0];
}
// Rows.  One workgroup per b over the [Tn] scalars of its row; thread k owns t = k, k + 256, ... in every pass, so the
// in-place z -> exp(z - max) -> a needs no ordering beyond the trees.  a32 (and BWD: w32) are zero from n on; n = 0: all zero.
template <bool BWD>
__global__ void __launch_bounds__(256) attn_rows(double* __restrict__ a64, const double* __restrict__ g64, double scale, float* __restrict__ a32,
                                                 float* __restrict__ w32, RowMap m) {
  __shared__ double lds[256];
  const int64_t b = blockIdx.x;
  const RowSteps row(m.len, b, m.Tn, m.rev);
  const int n = (int)row.n, k = threadIdx.x;
  double* a = a64 + b * m.Tn;
  const double* g = g64 + b * m.Tn;
  float* ao = a32 + b * m.Tn;
  for (int t = n + k; t < m.Tn; t += 256) {
    ao[t] = 0.f;
    if constexpr (BWD) w32[b * m.Tn + t] = 0.f;
  }
  if (n == 0) return;      // (the whole workgroup)
  double mx = -__builtin_huge_val();
  for (int t = k; t < n; t += 256) mx = fmax(mx, a[t]);
  mx = attn_tree<true>(lds, mx);
  double part = 0.0;
  for (int t = k; t < n; t += 256) {
    const double e = exp(a[t] - mx);
    a[t] = e;
    part += e;
  }
  const double sum = attn_tree<false>(lds, part);
  part = 0.0;
  for (int t = k; t < n; t += 256) {
    const double w = a[t] / sum;
    a[t] = w;
    ao[t] = (float)w;
    if constexpr (BWD) part += w * g[t];
  }
  if constexpr (BWD) {
    const double s = attn_tree<false>(lds, part);
    for (int t = k; t < n; t += 256) w32[b * m.Tn + t] = (float)(scale * a[t] * (g[t] - s));
  }
}

// Weighted sums over steps, with the pooled readout's decomposition (kPoolLanes pieces of h times kPoolSplit parts, the parts
// combined through LDS in the order k = 0, 1, ...):
//   DQ = false  y[b][h] = fl32(sum over t < n of a64[b][t] v[b][t][h]): workgroup (strip, b), part k takes t = k, k + kPoolSplit, ...
//   DQ = true   part[p][h] = sum over the (b, t < n) of slice p of w32[b][t] v[b][t][h], float64: workgroup (strip, p) takes the
//               flattened rows r = b Tn + t = p kPoolSplit + k, + gridDim.y kPoolSplit, ...
template <typename T, bool DQ>
__global__ void __launch_bounds__(256) attn_wsum(const T* __restrict__ h_all, const void* __restrict__ wgt, void* __restrict__ out, RowMap m) {
  constexpr int VEC = 16 / (int)sizeof(T), COLS = kPoolLanes * VEC;
  typedef T Piece __attribute__((ext_vector_type(VEC)));
  __shared__ double lds[kPoolSplit * COLS];
  const int lane = threadIdx.x % kPoolLanes, k = threadIdx.x / kPoolLanes;
  const int64_t h0 = (int64_t)blockIdx.x * COLS + lane * VEC;
  const bool live = h0 < m.H;
  double sum[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) sum[j] = 0.0;
  const int64_t total = DQ ? (int64_t)m.B * m.Tn : RowSteps(m.len, blockIdx.y, m.Tn, m.rev).n, step = DQ ? (int64_t)gridDim.y * kPoolSplit : kPoolSplit;
  for (int64_t r = (DQ ? (int64_t)blockIdx.y * kPoolSplit : 0) + k; live && r < total; r += step) {
    const int64_t b = DQ ? r / m.Tn : blockIdx.y, t = DQ ? r % m.Tn : r;
    const RowSteps row(m.len, b, m.Tn, m.rev);
    if (!row.valid(t)) continue;
    const double w = DQ ? (double)static_cast<const float*>(wgt)[b * m.Tn + t] : static_cast<const double*>(wgt)[b * m.Tn + t];
    const Piece v = *reinterpret_cast<const Piece*>(h_all + (row.slot(t) * m.B + b) * (int64_t)m.H + h0);
#pragma unroll
    for (int j = 0; j < VEC; ++j) sum[j] += w * (double)to_f32((T)v[j]);
  }
#pragma unroll
  for (int j = 0; j < VEC; ++j) lds[k * COLS + lane * VEC + j] = sum[j];
  __syncthreads();
  const int c = threadIdx.x;
  const int64_t h = (int64_t)blockIdx.x * COLS + c;
  if (c >= COLS || h >= m.H) return;
  double s = 0.0;
  for (int p = 0; p < kPoolSplit; ++p) s += lds[p * COLS + c];
  if constexpr (DQ) static_cast<double*>(out)[(int64_t)blockIdx.y * m.H + h] = s;
  else static_cast<float*>(out)[(int64_t)blockIdx.y * m.H + h] = (float)s;
}
// dq[h] = fl32(sum over the parts, in their order), or fl32(dq[h] + that)
__global__ void __launch_bounds__(256) attn_dq_sum(const double* __restrict__ part, int parts, float* __restrict__ dq, int H, int add) {
  const int h = blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= H) return;
  double s = 0.0;
  for (int p = 0; p < parts; ++p) s += part[(int64_t)p * H + h];
  dq[h] = add ? __fadd_rn(dq[h], (float)s) : (float)s;
}

// dx[b][t][i] (batch-first, dense) = or += dx_tm[s][b][i] (time-major); the padding is zeroed, or with add left as it is
__global__ void __launch_bounds__(256) dx_out(const float* __restrict__ dx_tm, float* __restrict__ dx, RowMap m) {
  const int64_t total = (int64_t)m.B * m.Tn * m.H;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t h = i % m.H, r = i / m.H, t = r % m.Tn, b = r / m.Tn;
    const RowSteps row(m.len, b, m.Tn, m.rev);
    if (row.valid(t)) {
      const float v = dx_tm[(row.flip(t) * m.B + b) * (int64_t)m.H + h];
      dx[i] = m.add ? dx[i] + v : v;
    } else if (!m.add) {
      dx[i] = 0.f;
    }
  }
}

// ---- the per-row helpers (len == nullptr: every row has T steps) ----
template <typename T>
__global__ void gather_state_kernel(const T* __restrict__ all, const int* __restrict__ len, int Tn, float* __restrict__ out, int B, int H) {
  const int64_t total = (int64_t)B * H;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t n = len != nullptr ? len[i / H] : Tn;
    out[i] = to_f32(all[n * B * H + i]);
  }
}

__global__ void add_at_end_kernel(const float* __restrict__ src, float* __restrict__ dst_tm, const int* __restrict__ len, int Tn, int t_lo, int t_hi, int B, int H) {
  const int64_t total = (int64_t)B * H;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int t = (len != nullptr ? len[i / H] : Tn) - 1;
    if (t >= t_lo && t <= t_hi) dst_tm[(int64_t)t * B * H + i] += src[i];
  }
}

__global__ void add_rows_len0_kernel(const float* __restrict__ src, float* __restrict__ dst, const int* __restrict__ len, int B, int H) {
  const int64_t total = (int64_t)B * H;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride)
    if (len[i / H] == 0) dst[i] += src[i];
}

template <typename T>
__global__ void mask_tm_kernel(T* __restrict__ buf, const int* __restrict__ len, int B, int Tn, int W) {
  const int64_t total = (int64_t)B * Tn * W;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t r = i / W, b = r % B, t = r / B;
    if (t >= len[b]) buf[i] = from_f32<T>(0.f);
  }
}
// one 16-byte piece per thread and trip
__global__ void mask_x_blk_kernel(bf16_t* __restrict__ x_blk, const int* __restrict__ len, int B, int64_t Bpad, int Tn, int I) {
  const int64_t per_t = Bpad * I / 8, kblocks = I >> 5;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t ci = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; ci < per_t * Tn; ci += stride) {
    const int64_t t = ci / per_t, c = ci % per_t, blk = c >> 6, lane = c & 63;
    const int64_t r = (blk / kblocks) * 16 + (lane & 15);
    if (r < B && t >= len[r]) *reinterpret_cast<uint4*>(x_blk + ci * 8) = make_uint4(0u, 0u, 0u, 0u);
  }
}

// ---- launchers ----
// blocks of 256 threads over n items; the masked passes (a Philox call per item) spread over twice as many blocks
static inline unsigned grid_for(int64_t n, int64_t cap = 2048) {
  const int64_t g = (n + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}
static const int64_t kDropBlocks = 4096;

static int check_out_drop(const char* fn, const void* caller, const RowMap& m, const OutDropCfg& od) {
  CSN_REQUIRE(m.H % 32 == 0 && m.pitch % 4 == 0 && m.pitch >= m.H, "%s: H = %d, pitch = %lld: groups of four h are not aligned", fn, m.H,
              (long long)m.pitch);
  CSN_REQUIRE(od.first % 4 == 0 && od.index_pitch % 4 == 0 && od.index_pitch >= m.H, "%s: first = %llu, index_pitch = %lld split a Philox call", fn,
              (unsigned long long)od.first, (long long)od.index_pitch);
  CSN_REQUIRE((reinterpret_cast<uintptr_t>(caller) & 15) == 0, "%s: the caller's tensor must be 16-B aligned", fn);
  return CSN_OK;
}

template <typename T>
static void launch_y_out_t(const void* h_all, float* y, const RowMap& m, const OutDropCfg* od, hipStream_t st) {
  const int64_t n = (int64_t)m.B * m.Tn * m.H;
  if (od) y_out<T, true><<<grid_for(n >> 2, kDropBlocks), 256, 0, st>>>((const T*)h_all, y, m, *od);
  else y_out<T, false><<<grid_for(n), 256, 0, st>>>((const T*)h_all, y, m, OutDropCfg{});
}
int launch_y_out(const void* h_all, int dtype, float* y, const RowMap& m, const OutDropCfg* od, hipStream_t st) {
  if (od)
    if (int rc = check_out_drop("lstm y_out", y, m, *od)) return rc;
  if (dtype == CSN_BF16) launch_y_out_t<bf16_t>(h_all, y, m, od, st);
  else launch_y_out_t<float>(h_all, y, m, od, st);
  CSN_LAUNCH_CHECK();
  return CSN_OK;
}

template <int POOL>
static void launch_dy_in_t(const float* dy, float* dy_tm, const RowMap& m, const OutDropCfg* od, const PoolIn& pl, hipStream_t st) {
  const int64_t n = (int64_t)m.B * m.Te * m.H;
  if (od) dy_in<true, POOL><<<grid_for(n >> 2, kDropBlocks), 256, 0, st>>>(dy, dy_tm, m, *od, pl);
  else dy_in<false, POOL><<<grid_for(n), 256, 0, st>>>(dy, dy_tm, m, OutDropCfg{}, pl);
}
int launch_dy_in(const float* dy, float* dy_tm, const RowMap& m, const OutDropCfg* od, const PoolIn* pool, hipStream_t st) {
  if (od)
    if (int rc = check_out_drop("lstm dy_in", dy, m, *od)) return rc;
  if (pool == nullptr || pool->mode == CSN_READOUT_LAST) {
    launch_dy_in_t<CSN_READOUT_LAST>(dy, dy_tm, m, od, PoolIn{}, st);
  } else if (pool->mode == kPoolAttention) {
    CSN_REQUIRE(pool->dy_last && pool->a32 && pool->w32 && pool->q, "lstm dy_in: attention term without its inputs");
    launch_dy_in_t<kPoolAttention>(dy, dy_tm, m, od, *pool, st);
  } else {
    CSN_REQUIRE(pool->dy_last != nullptr && (pool->mode == CSN_READOUT_MEAN || pool->argmax != nullptr), "lstm dy_in: pooled term without its inputs");
    if (pool->mode == CSN_READOUT_MEAN) launch_dy_in_t<CSN_READOUT_MEAN>(dy, dy_tm, m, od, *pool, st);
    else launch_dy_in_t<CSN_READOUT_MAX>(dy, dy_tm, m, od, *pool, st);
  }
  CSN_LAUNCH_CHECK();
  return CSN_OK;
}

template <typename T>
static void launch_pool_t(const void* h_all, int mode, void* out, const RowMap& m, hipStream_t st) {
  constexpr int cols = kPoolLanes * (16 / (int)sizeof(T));
  const dim3 grid((unsigned)((m.H + cols - 1) / cols), (unsigned)m.B);
  if (mode == CSN_READOUT_MEAN) pool_readout<T, CSN_READOUT_MEAN><<<grid, 256, 0, st>>>((const T*)h_all, out, m);
  else if (mode == CSN_READOUT_MAX) pool_readout<T, CSN_READOUT_MAX><<<grid, 256, 0, st>>>((const T*)h_all, out, m);
  else pool_readout<T, kPoolArgmax><<<grid, 256, 0, st>>>((const T*)h_all, out, m);
}
static int launch_pool(const void* h_all, int dtype, int mode, void* out, const RowMap& m, hipStream_t st) {
  CSN_REQUIRE(m.B <= 65535, "lstm pooled readout: B = %d rows exceed the grid", m.B);
  if (dtype == CSN_BF16) launch_pool_t<bf16_t>(h_all, mode, out, m, st);
  else launch_pool_t<float>(h_all, mode, out, m, st);
  CSN_LAUNCH_CHECK();
  return CSN_OK;
}
int launch_pool_readout(const void* h_all, int dtype, int mode, float* y, const RowMap& m, hipStream_t st) {
  CSN_REQUIRE(mode == CSN_READOUT_MEAN || mode == CSN_READOUT_MAX, "lstm pooled readout: mode %d", mode);
  return launch_pool(h_all, dtype, mode, y, m, st);
}
int launch_pool_argmax(const void* h_all, int dtype, int* argmax, const RowMap& m, hipStream_t st) {
  return launch_pool(h_all, dtype, kPoolArgmax, argmax, m, st);
}

// ---- the attention readout's launches
template <typename T, int LG, bool BWD>
static void launch_attn_scores_g(const void* h_all, const AttnArgs& A, const float* dy_last, const RowMap& m, hipStream_t st) {
  const int64_t rows = (int64_t)m.B * m.Tn;
  attn_scores<T, LG, BWD><<<grid_for(rows * LG, 4096), 256, 0, st>>>((const T*)h_all, A.q, dy_last, (double)A.scale, A.a64, A.g64, m);
}
template <typename T, bool BWD>
static void launch_attn_scores_t(const void* h_all, const AttnArgs& A, const float* dy_last, const RowMap& m, hipStream_t st) {
  const int pieces = m.H * (int)sizeof(T) / 16;      // the smallest group that covers them, a wave at the most
  if (pieces <= 4) launch_attn_scores_g<T, 4, BWD>(h_all, A, dy_last, m, st);
  else if (pieces <= 8) launch_attn_scores_g<T, 8, BWD>(h_all, A, dy_last, m, st);
  else if (pieces <= 16) launch_attn_scores_g<T, 16, BWD>(h_all, A, dy_last, m, st);
  else if (pieces <= 32) launch_attn_scores_g<T, 32, BWD>(h_all, A, dy_last, m, st);
  else launch_attn_scores_g<T, 64, BWD>(h_all, A, dy_last, m, st);
}
static int check_attn(const char* fn, const AttnArgs& A, const RowMap& m, bool bwd) {
  CSN_REQUIRE(A.q && A.a64 && A.a32 && (!bwd || (A.g64 && A.w32)), "%s: attention readout without its buffers", fn);
  CSN_REQUIRE(m.H % 32 == 0 && m.B >= 1 && m.B <= 65535 && m.Tn >= 1, "%s: B = %d, T = %d, H = %d", fn, m.B, m.Tn, m.H);
  return CSN_OK;
}
int launch_attn_forward(const void* h_all, int dtype, const AttnArgs& A, float* y, const RowMap& m, hipStream_t st) {
  if (int rc = check_attn("lstm attention forward", A, m, false)) return rc;
  if (dtype == CSN_BF16) launch_attn_scores_t<bf16_t, false>(h_all, A, nullptr, m, st);
  else launch_attn_scores_t<float, false>(h_all, A, nullptr, m, st);
  CSN_LAUNCH_CHECK();
  attn_rows<false><<<(unsigned)m.B, 256, 0, st>>>(A.a64, A.a64, (double)A.scale, A.a32, nullptr, m);
  CSN_LAUNCH_CHECK();
  if (dtype == CSN_BF16) {
    const dim3 grid((unsigned)((m.H + kPoolLanes * 8 - 1) / (kPoolLanes * 8)), (unsigned)m.B);
    attn_wsum<bf16_t, false><<<grid, 256, 0, st>>>((const bf16_t*)h_all, A.a64, y, m);
  } else {
    const dim3 grid((unsigned)((m.H + kPoolLanes * 4 - 1) / (kPoolLanes * 4)), (unsigned)m.B);
    attn_wsum<float, false><<<grid, 256, 0, st>>>((const float*)h_all, A.a64, y, m);
  }
  CSN_LAUNCH_CHECK();
  return CSN_OK;
}
int launch_attn_backward(const void* h_all, int dtype, const AttnArgs& A, const float* dy_last, float* dq, int accumulate, const RowMap& m,
                         hipStream_t st) {
  if (int rc = check_attn("lstm attention backward", A, m, true)) return rc;
  CSN_REQUIRE(dy_last != nullptr && (dq == nullptr || A.dq_part != nullptr), "lstm attention backward: null pointer");
  if (dtype == CSN_BF16) launch_attn_scores_t<bf16_t, true>(h_all, A, dy_last, m, st);
  else launch_attn_scores_t<float, true>(h_all, A, dy_last, m, st);
  CSN_LAUNCH_CHECK();
  attn_rows<true><<<(unsigned)m.B, 256, 0, st>>>(A.a64, A.g64, (double)A.scale, A.a32, A.w32, m);
  CSN_LAUNCH_CHECK();
  if (dq == nullptr) return CSN_OK;
  // (each thread of a slice takes eight rows or more, kAttnDqParts slices at the most: fixed by the shapes)
  const int64_t want = ((int64_t)m.B * m.Tn + kPoolSplit * 8 - 1) / (kPoolSplit * 8);
  const unsigned parts = (unsigned)(want < 1 ? 1 : (want > kAttnDqParts ? kAttnDqParts : want));
  if (dtype == CSN_BF16) {
    const dim3 grid((unsigned)((m.H + kPoolLanes * 8 - 1) / (kPoolLanes * 8)), parts);
    attn_wsum<bf16_t, true><<<grid, 256, 0, st>>>((const bf16_t*)h_all, A.w32, A.dq_part, m);
  } else {
    const dim3 grid((unsigned)((m.H + kPoolLanes * 4 - 1) / (kPoolLanes * 4)), parts);
    attn_wsum<float, true><<<grid, 256, 0, st>>>((const float*)h_all, A.w32, A.dq_part, m);
  }
  CSN_LAUNCH_CHECK();
  attn_dq_sum<<<(unsigned)((m.H + 255) / 256), 256, 0, st>>>(A.dq_part, (int)parts, dq, m.H, accumulate);
  CSN_LAUNCH_CHECK();
  return CSN_OK;
}

int launch_dx_out(const float* dx_tm, float* dx, const RowMap& m, hipStream_t st) {
  dx_out<<<grid_for((int64_t)m.B * m.Tn * m.H), 256, 0, st>>>(dx_tm, dx, m);
  CSN_LAUNCH_CHECK();
  return CSN_OK;
}

int launch_gather_state(const void* all, int dtype, const int* len, int T, float* out, int B, int H, hipStream_t st) {
  const unsigned grid = grid_for((int64_t)B * H);
  if (dtype == CSN_BF16) gather_state_kernel<bf16_t><<<grid, 256, 0, st>>>((const bf16_t*)all, len, T, out, B, H);
  else gather_state_kernel<float><<<grid, 256, 0, st>>>((const float*)all, len, T, out, B, H);
  CSN_LAUNCH_CHECK();
  return CSN_OK;
}

int launch_add_at_end(const float* src, float* dst_tm, const int* len, int T, int t_lo, int t_hi, int B, int H, hipStream_t st) {
  if (len == nullptr && (T - 1 < t_lo || T - 1 > t_hi)) return CSN_OK;
  add_at_end_kernel<<<grid_for((int64_t)B * H), 256, 0, st>>>(src, dst_tm, len, T, t_lo, t_hi, B, H);
  CSN_LAUNCH_CHECK();
  return CSN_OK;
}

int launch_add_rows_len0(const float* src, float* dst, const int* len, int B, int H, hipStream_t st) {
  add_rows_len0_kernel<<<grid_for((int64_t)B * H), 256, 0, st>>>(src, dst, len, B, H);
  CSN_LAUNCH_CHECK();
  return CSN_OK;
}

int launch_mask_tm(void* buf, int dtype, const int* len, int B, int Tn, int W, hipStream_t st) {
  const unsigned grid = grid_for((int64_t)Tn * B * W);
  if (dtype == CSN_BF16) mask_tm_kernel<bf16_t><<<grid, 256, 0, st>>>((bf16_t*)buf, len, B, Tn, W);
  else mask_tm_kernel<float><<<grid, 256, 0, st>>>((float*)buf, len, B, Tn, W);
  CSN_LAUNCH_CHECK();
  return CSN_OK;
}

int launch_mask_x_blk(bf16_t* x_blk, const int* len, int B, int64_t Bpad, int Tn, int I, hipStream_t st) {
  mask_x_blk_kernel<<<grid_for((int64_t)Tn * Bpad * I / 8), 256, 0, st>>>(x_blk, len, B, Bpad, Tn, I);
  CSN_LAUNCH_CHECK();
  return CSN_OK;
}

}  // namespace csn
