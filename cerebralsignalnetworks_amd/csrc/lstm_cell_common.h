// Helpers shared by the LSTM cell kernels: 4-wide vector load/store in either storage type.
#pragma once
#include "csn_common.h"

// Streaming (touched-once) epilogue traffic -- xproj, saved gates, c, row-major h / dgates --
// is marked non-temporal so it does not displace the re-read operands (W, h) from L2 and leaves
// fewer dirty lines for the end-of-kernel write-back.
#ifndef CSN_NT
#define CSN_NT 1
#endif
template <typename V> __device__ __forceinline__ V nt_load(const V* p) {
#if CSN_NT
  return __builtin_nontemporal_load(p);
#else
  return *p;
#endif
}
template <typename V> __device__ __forceinline__ void nt_store(V* p, const V& v) {
#if CSN_NT
  __builtin_nontemporal_store(v, p);
#else
  *p = v;
#endif
}
// float4 (a HIP struct type) goes through the equivalent clang vector type
__device__ __forceinline__ float4 nt_load(const float4* p) {
  const csn::f32x4 v = nt_load(reinterpret_cast<const csn::f32x4*>(p));
  return make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void nt_store(float4* p, const float4& v) {
  nt_store(reinterpret_cast<csn::f32x4*>(p), (csn::f32x4){v.x, v.y, v.z, v.w});
}

namespace csn {

template <typename T> struct Vec4;
template <> struct Vec4<float> {
  static __device__ __forceinline__ void store(float* p, const float (&v)[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  }
  static __device__ __forceinline__ void load(const float* p, float (&v)[4]) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  }
};
template <> struct Vec4<bf16_t> {
  static __device__ __forceinline__ void store(bf16_t* p, const float (&v)[4]) {
    bf16x4 o = {(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
    *reinterpret_cast<bf16x4*>(p) = o;
  }
  static __device__ __forceinline__ void load(const bf16_t* p, float (&v)[4]) {
    const bf16x4 q = *reinterpret_cast<const bf16x4*>(p);
    v[0] = (float)q[0]; v[1] = (float)q[1]; v[2] = (float)q[2]; v[3] = (float)q[3];
  }
};


// MFMA operand fragments of the generic cell kernels (lstm_cell.hip) and of the CU-resident recurrence
// (lstm_resident.hip), k-contiguous per lane: W as the A operand, h / dgates as the B operand.
template <typename T> struct Frag;
template <> struct Frag<bf16_t> {
  typedef bf16x8 type;
  static constexpr int kStep = 32;  // k covered by one fragment load (8 per lane x 4 lane groups)
  static constexpr int kLane = 8;   // k per lane
  static __device__ __forceinline__ type load(const bf16_t* row_ptr, int k0, int lane) {
    return *reinterpret_cast<const bf16x8*>(row_ptr + k0 + 8 * (lane >> 4));
  }
  static __device__ __forceinline__ type zero() { return (bf16x8){0, 0, 0, 0, 0, 0, 0, 0}; }
  static __device__ __forceinline__ f32x4 mma(const type& a, const type& b, f32x4 acc) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
  }
};
template <> struct Frag<float> {
  typedef f32x4 type;
  static constexpr int kStep = 16;  // 4 per lane x 4 lane groups
  static constexpr int kLane = 4;
  static __device__ __forceinline__ type load(const float* row_ptr, int k0, int lane) {
    return *reinterpret_cast<const f32x4*>(row_ptr + k0 + 4 * (lane >> 4));
  }
  static __device__ __forceinline__ type zero() { return (f32x4){0.f, 0.f, 0.f, 0.f}; }
  static __device__ __forceinline__ f32x4 mma(const type& a, const type& b, f32x4 acc) {
    // MFMA jj contracts k = k0 + 4*(lane>>4) + jj over the 4 lane groups; A and B use the same map.
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[jj], b[jj], acc, 0, 0, 0);
    return acc;
  }
};

// The per-element cell math of those kernels, four consecutive units of one batch row per lane.  ONE definition for the
// per-step cells and the resident recurrence: the two give the same bits because they evaluate the same expressions.
// forward: pre[gate][r] = pre-activations (i, f, g, o), cp = c_{t-1}
__device__ __forceinline__ void cell_fwd_point(const float (&pre)[4][4], const float (&cp)[4], float (&gi)[4], float (&gf)[4],
                                               float (&gg)[4], float (&go)[4], float (&cn)[4], float (&hn)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    gi[r] = sigmoid_f32(pre[0][r]);
    gf[r] = sigmoid_f32(pre[1][r]);
    gg[r] = tanh_f32(pre[2][r]);
    go[r] = sigmoid_f32(pre[3][r]);
    cn[r] = gf[r] * cp[r] + gi[r] * gg[r];
    hn[r] = go[r] * tanh_f32(cn[r]);
  }
}
// backward: dh = gradient w.r.t. h_t, cc = c_t, cp = c_{t-1}, dcn = the carried dc; the pre-activation gradients and the new carry
__device__ __forceinline__ void cell_bwd_point(const float (&dh)[4], const float (&gi)[4], const float (&gf)[4], const float (&gg)[4],
                                               const float (&go)[4], const float (&cc)[4], const float (&cp)[4], const float (&dcn)[4],
                                               float (&dai)[4], float (&daf)[4], float (&dag)[4], float (&dao)[4], float (&dcarry)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float tc = tanh_f32(cc[r]);
    const float d_o = dh[r] * tc;
    const float dc = dh[r] * go[r] * (1.0f - tc * tc) + dcn[r];
    dai[r] = dc * gg[r] * gi[r] * (1.0f - gi[r]);
    daf[r] = dc * cp[r] * gf[r] * (1.0f - gf[r]);
    dag[r] = dc * gi[r] * (1.0f - gg[r] * gg[r]);
    dao[r] = d_o * go[r] * (1.0f - go[r]);
    dcarry[r] = dc * gf[r];
  }
}
// a cell at t >= lengths[row]: zero gate gradients, the carried dc passes as it came
__device__ __forceinline__ void cell_bwd_dead(const float (&dcn)[4], float (&dai)[4], float (&daf)[4], float (&dag)[4],
                                              float (&dao)[4], float (&dcarry)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    dai[r] = daf[r] = dag[r] = dao[r] = 0.f;
    dcarry[r] = dcn[r];
  }
}

// Fast activations for the bf16 path: v_exp_f32 + v_rcp_f32 (about 1 ulp each), far inside the
// 8 significant bits the bf16 operands keep.  The f32 parity path uses expf / tanhf instead.
__device__ __forceinline__ float fast_sigmoid(float x) {
  return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x));
}
__device__ __forceinline__ float fast_tanh(float x) {
  // 1 - 2 / (1 + e^{2x}); saturates correctly for large |x| (exp2 -> inf or 0)
  return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(2.8853900817779268f * x));
}

// "Fragment-major" (blocked) bf16 layout of a [R, K] matrix, K % 32 == 0, rows padded to 16:
// 16-row x 32-k blocks of 1 KB, block (rb, kb) at ((rb * K/32) + kb) * 512 elements; inside a
// block the 16-byte chunk of (row r, k-octet q) sits at lane position r + 16 q -- exactly the
// operand fragment of v_mfma_f32_16x16x32_bf16 -- so one wave-wide 16-B-per-lane load of a
// fragment is ONE contiguous 1 KB read (8 full cache lines instead of 16 half-used ones).
__host__ __device__ __forceinline__ int64_t blk_offset(int64_t r, int64_t k, int64_t K) {
  return (((r >> 4) * (K >> 5)) + (k >> 5)) * 512 + (((r & 15) + 16 * ((k & 31) >> 3)) << 3) + (k & 7);
}

}  // namespace csn
