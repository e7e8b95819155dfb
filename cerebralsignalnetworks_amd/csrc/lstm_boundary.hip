// The API boundary of the stacked LSTM: the batch-first <-> time-major layout passes around the recurrence and the per-row
// helpers of variable-length batches (lstm_boundary.h; DESIGN.md sections 10, 16 and 23).  All of it is bandwidth-bound
// element movement; the only arithmetic is the float32 multiply of output dropout and the adding stores.
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

// dy_tm[s][b][h] (dense, time-major), s < Te  <-  dy_all[b][t][h] (batch-first, pitched, or null); zeros from a row's length on
template <bool DROP>
__global__ void __launch_bounds__(256) dy_in(const float* __restrict__ dy, float* __restrict__ dy_tm, RowMap m, OutDropCfg od) {
  constexpr int W = DROP ? 4 : 1;
  const int64_t hw = m.H / W, total = (int64_t)m.B * m.Te * hw;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t h = (i % hw) * W, r = i / hw, b = r % m.B, s = r / m.B;
    const RowSteps row(m.len, b, m.Tn, m.rev);
    const bool in = dy != nullptr && row.valid(s);
    const int64_t brow = b * m.Tn + row.flip(s);
    const float* src = dy + brow * m.pitch + h;
    float* dst = dy_tm + i * W;
    if constexpr (DROP) {
      f32x4 out = {0.f, 0.f, 0.f, 0.f};
      if (in) out = drop_quad(*reinterpret_cast<const f32x4*>(src), od, brow, h);
      *reinterpret_cast<f32x4*>(dst) = out;
    } else {
      *dst = in ? *src : 0.f;
    }
  }
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

int launch_dy_in(const float* dy, float* dy_tm, const RowMap& m, const OutDropCfg* od, hipStream_t st) {
  const int64_t n = (int64_t)m.B * m.Te * m.H;
  if (od) {
    if (int rc = check_out_drop("lstm dy_in", dy, m, *od)) return rc;
    dy_in<true><<<grid_for(n >> 2, kDropBlocks), 256, 0, st>>>(dy, dy_tm, m, *od);
  } else {
    dy_in<false><<<grid_for(n), 256, 0, st>>>(dy, dy_tm, m, OutDropCfg{});
  }
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
