// Inter-layer dropout of the stacked LSTM (nn.LSTM(dropout=p); include/csn_hip.h: csn_lstm_plan_set_dropout, DESIGN.md
// section 15): two element-wise kernels over a time-major slab of whole steps, and the host definition of the mask.
//
//   forward : h_drop[l] = mask * h_all[l] / (1 - p), what layer l + 1's input projection and dW_ih read
//   backward: dx of layer l + 1 (= dgates W_ih, the dy of layer l) *= mask / (1 - p), in place, before dh_n[l] joins it
//
// Both are bandwidth-bound: 16-byte accesses, one Philox4x32-10 call per four consecutive units (the four words of a
// call are four consecutive elements, and H % 32 == 0 keeps every slab aligned on them).  A dropped element is a
// SELECTED zero, never a product: what was there (NaN, Inf) does not get through.
#include "lstm_dropout.h"

namespace csn {

// one thread and trip: 8 consecutive bf16 (two Philox calls) or 4 consecutive float32 (one)
template <typename T> struct DropVec;
template <> struct DropVec<bf16_t> { typedef bf16x8 type; static constexpr int N = 8; };
template <> struct DropVec<float> { typedef f32x4 type; static constexpr int N = 4; };

template <typename T>
__global__ void __launch_bounds__(256) lstm_dropout_fwd_kernel(const T* __restrict__ h, T* __restrict__ out, int64_t nvec, uint64_t e0, DropoutCfg cfg) {
  typedef typename DropVec<T>::type V;
  constexpr int N = DropVec<T>::N;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
    const V v = reinterpret_cast<const V*>(h)[i];
    const uint64_t quad = (e0 + (uint64_t)i * N) >> 2;
    V r;
#pragma unroll
    for (int q = 0; q < N / 4; ++q) {
      const Philox4 w = dropout_words(cfg, quad + q);
#pragma unroll
      for (int j = 0; j < 4; ++j) r[4 * q + j] = (uint64_t)w.w[j] >= cfg.thr ? from_f32<T>(to_f32((T)v[4 * q + j]) * cfg.scale) : from_f32<T>(0.f);
    }
    reinterpret_cast<V*>(out)[i] = r;
  }
}

__global__ void __launch_bounds__(256) lstm_dropout_bwd_kernel(float* __restrict__ dx, int64_t nvec, uint64_t e0, DropoutCfg cfg) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
    const f32x4 v = reinterpret_cast<const f32x4*>(dx)[i];
    const Philox4 w = dropout_words(cfg, (e0 >> 2) + (uint64_t)i);
    f32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = (uint64_t)w.w[j] >= cfg.thr ? v[j] * cfg.scale : 0.f;
    reinterpret_cast<f32x4*>(dx)[i] = r;
  }
}

static inline unsigned drop_grid(int64_t nvec) {
  const int64_t g = (nvec + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

static int check_slab(const void* a, const void* b, int64_t n, uint64_t e0) {
  CSN_REQUIRE(n > 0 && n % 32 == 0 && e0 % 4 == 0, "lstm dropout: slab of %lld elements from element %llu is not whole steps of H %% 32 == 0 units",
              (long long)n, (unsigned long long)e0);
  CSN_REQUIRE(((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0, "lstm dropout: slab must be 16-B aligned");
  return CSN_OK;
}

int launch_lstm_dropout_fwd(const void* h, void* h_drop, int64_t n, uint64_t e0, int dtype, const DropoutCfg& cfg, hipStream_t st) {
  if (int rc = check_slab(h, h_drop, n, e0)) return rc;
  if (dtype == CSN_BF16) {
    lstm_dropout_fwd_kernel<bf16_t><<<drop_grid(n / 8), 256, 0, st>>>((const bf16_t*)h, (bf16_t*)h_drop, n / 8, e0, cfg);
  } else {
    lstm_dropout_fwd_kernel<float><<<drop_grid(n / 4), 256, 0, st>>>((const float*)h, (float*)h_drop, n / 4, e0, cfg);
  }
  CSN_LAUNCH_CHECK();
  return CSN_OK;
}

int launch_lstm_dropout_bwd(float* dx, int64_t n, uint64_t e0, const DropoutCfg& cfg, hipStream_t st) {
  if (int rc = check_slab(dx, dx, n, e0)) return rc;
  lstm_dropout_bwd_kernel<<<drop_grid(n / 4), 256, 0, st>>>(dx, n / 4, e0, cfg);
  CSN_LAUNCH_CHECK();
  return CSN_OK;
}

}  // namespace csn

using namespace csn;

extern "C" int csn_lstm_dropout_keep(uint64_t seed, uint32_t subsequence, float p, int64_t first, int64_t n, uint8_t* keep_host) {
  CSN_REQUIRE(p >= 0.f && p <= 1.f, "csn_lstm_dropout_keep: p = %g outside [0, 1]", (double)p);
  CSN_REQUIRE(first >= 0 && n >= 0, "csn_lstm_dropout_keep: negative first / n");
  CSN_REQUIRE(keep_host != nullptr || n == 0, "csn_lstm_dropout_keep: null output");
  const DropoutCfg cfg = dropout_cfg(p, seed, subsequence);
  uint64_t quad = ~(uint64_t)0;
  Philox4 w{};
  for (int64_t i = 0; i < n; ++i) {
    const uint64_t e = (uint64_t)first + (uint64_t)i;
    if ((e >> 2) != quad || i == 0) {
      quad = e >> 2;
      w = dropout_words(cfg, quad);
    }
    keep_host[i] = (uint64_t)w.w[e & 3] >= cfg.thr ? 1 : 0;
  }
  return CSN_OK;
}
