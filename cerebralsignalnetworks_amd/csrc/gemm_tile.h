// What the bf16 GEMM kernels of gemm_nt.hip, gemm_tn.hip and gemm_beside.h share: the XCD-aware block order, the
// LDS-DMA and fragment-read primitives, the swizzled LDS images and the store epilogues (one per operand layout).
#pragma once
#include "csn_common.h"

namespace csn {

// XCD-aware block order (cdna_hip_programming.md T1): hardware deals consecutive workgroups round-robin
// over the 8 XCDs (each with a private L2), so tiles that share an operand panel would land on 8
// different L2s and the panel would cross the fabric 8 times (measured with FETCH_SIZE: 12x the
// algorithmic bytes on the NT GEMM, 4.5x on the TN GEMM).  This bijection hands every XCD one
// contiguous range of the logical tile order instead.  Speed only -- any placement is correct.
__device__ __forceinline__ unsigned xcd_remap(unsigned bid, unsigned nwg) {
  const unsigned q = nwg >> 3, r = nwg & 7, xcd = bid & 7, slot = bid >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
}

// NT, LDS image of one operand tile: 128 rows x 64 k (bf16) = 128-byte rows, eight 16-byte chunks
// per row.  Chunk ch of row r is stored at chunk (ch ^ ((r >> 1) & 7)): with that XOR the 16
// lanes of every ds_read_b128 lane group ({0-3,12-15,20-27}, ...) hit 16 distinct 16-byte
// slots of the 256-byte bank row when lane l reads row (l & 15), chunk kk*4 + (l >> 4).
__device__ __forceinline__ int nt_lds_off(int row, int chunk) {  // byte offset inside a tile
  return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4);
}

// NT, LDS image of the stages of 32 contraction columns (gemm_nt_w4_kernel, the wide body of gemm_beside.h): 64-byte
// rows, four 16-byte chunks per row, chunk ch of row r at position ch ^ nt64_sw(r)
__device__ __forceinline__ int nt64_sw(int row) {
  const int g = (row >> 2) & 3;
  return (((g ^ (g >> 1)) & 1) << 1) | (g >> 1);
}

// TN, LDS image of one operand tile: 32 k-rows x 128 columns (bf16) = 256-byte rows, eight
// 16-column blocks per row.  Block cb of k-row r is stored at block (cb ^ s(r)),
// s(r) = (r & 3) | (((r >> 3) & 1) << 2), so the 8 k-rows that the lower (or upper) 32 lanes of
// a ds_read_b64_tr_b16 address fall into 8 distinct 32-byte bank windows.
__device__ __forceinline__ int tn_lds_off(int krow, int col) {  // byte offset; col in elements
  const int s = (krow & 3) | (((krow >> 3) & 1) << 2);
  return krow * 256 + ((((col >> 4) ^ s) << 4) + (col & 15)) * 2;
}
// TN, stage image of the 256-wide tiles: 32 k-rows x 256 columns (512-byte rows, 16 blocks of 16 columns), block cb of
// k-row r at block (cb ^ s(r)) with the s(r) of tn_lds_off, so the 8 k-rows a half-wave of ds_read_b64_tr_b16 touches
// fall into 8 distinct 32-byte bank windows.
__device__ __forceinline__ int tn256_lds_off(int krow, int col) {  // byte offset; col in elements
  const int sw = (krow & 3) | (((krow >> 3) & 1) << 2);
  return krow * 512 + ((((col >> 4) ^ sw) << 4) + (col & 15)) * 2;
}

// =====================================================================================
// LDS-DMA variants (global_load_lds, 16 B per lane): no VGPR staging and no ds_write pass -- the tile goes
// HBM/L2 -> LDS directly, two LDS buffers, ONE barrier per 64-deep k-step, the next tile's loads in flight
// under the MFMAs of the current one.  An LDS-DMA wave-instruction writes 1 KB lane-linearly (LDS address =
// wave-uniform base + 16 * lane), so the XOR swizzles of the images above are applied on the SOURCE side:
// lane i fetches the global chunk whose swizzled position is i (the read side is unchanged).
// Preconditions (checked by the launchers, otherwise the register-staged kernels run): K % 64 == 0, so no
// partial k-tile exists (LDS-DMA cannot zero-fill); rows beyond M / N are clamped to the last valid row and
// their results discarded by the epilogue.
// =====================================================================================
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* gbl_ptr_t;

__device__ __forceinline__ void glds16(const void* g, void* l) {
  __builtin_amdgcn_global_load_lds((gbl_ptr_t)g, (lds_ptr_t)l, 16, 0, 0);
}

// Source of this lane's 16 bytes of 1 KB LDS-DMA piece `piece` (8 rows x 8 chunks) of the 128-byte-row NT image, at
// k = 0: lane -> row r = 8 piece + (lane >> 3), LDS chunk position c = lane & 7 <- global chunk c ^ ((r >> 1) & 7).
// P[rows, K] row-major, the tile starts at row r0; CLAMP: rows beyond the operand read its last row instead.
template <bool CLAMP>
__device__ __forceinline__ const bf16_t* nt_dma_src(const bf16_t* P, int64_t r0, int64_t rows, int64_t K, int piece, int lane) {
  const int row = piece * 8 + (lane >> 3);
  const int ch = (lane & 7) ^ ((row >> 1) & 7);
  int64_t r = r0 + row;
  if (CLAMP) r = r < rows ? r : rows - 1;
  return P + r * K + ch * 8;
}

// Fragment reads in inline asm: for an LDS read it can see, the compiler waits vmcnt(0) while ANY LDS-DMA is outstanding
// (see gemm_tn_256_kernel)
__device__ __forceinline__ bf16x8 lds_read_b128(unsigned addr) {
  bf16x8 v;
  asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(addr) : "memory");
  return v;
}

// =====================================================================================
// Store epilogues.  Accumulator layout of every kernel here (operands swapped, D[row = n][col = m]): of a 16 x 16
// fragment whose first row is mb and first column nb, lane l holds row mb + (l & 15), columns nb + 4 (l >> 4) .. + 3.
// =====================================================================================
// NT: C[idx .. idx + 3] = convert(v (+ old C)); v already carries the bias
template <typename OutT>
__device__ __forceinline__ void nt_store4(f32x4 v, OutT* __restrict__ C, int64_t idx, int accumulate) {
  if constexpr (sizeof(OutT) == 4) {
    f32x4* dst = reinterpret_cast<f32x4*>((float*)C + idx);
    if (accumulate) v += *dst;
    *dst = v;
  } else {
    *reinterpret_cast<bf16x4*>((bf16_t*)C + idx) = (bf16x4){(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
  }
}
template <typename OutT>
__device__ __forceinline__ void nt_store1(float v, OutT* __restrict__ C, int64_t idx, int accumulate) {
  if constexpr (sizeof(OutT) == 4) {
    float* dst = (float*)C + idx;
    *dst = accumulate ? *dst + v : v;
  } else {
    ((bf16_t*)C)[idx] = (bf16_t)v;
  }
}
__device__ __forceinline__ f32x4 nt_with_bias(f32x4 v, const float* __restrict__ bias, int64_t n) {
  if (bias) v += *reinterpret_cast<const f32x4*>(bias + n);
  return v;
}
// NT, one accumulator fragment of row m, columns n .. n + 3 of C[M, N]: bias first, then + old C, then the conversion.
// TAIL: N may end inside the four columns (otherwise the caller guarantees n + 3 < N).
template <typename OutT, bool TAIL>
__device__ __forceinline__ void nt_store_frag(f32x4 acc, const float* __restrict__ bias, OutT* __restrict__ C, int64_t m,
                                              int64_t n, int64_t N, int accumulate) {
  if (!TAIL || n + 3 < N) {
    nt_store4<OutT>(nt_with_bias(acc, bias, n), C, m * N + n, accumulate);
  } else {
    for (int r = 0; r < 4; ++r)
      if (n + r < N) nt_store1<OutT>(acc[r] + (bias ? bias[n + r] : 0.f), C, m * N + n + r, accumulate);
  }
}
// TN, the same for a float32 slab C[M, N]: no bias, no accumulation, and N need not be a multiple of 4
__device__ __forceinline__ void tn_store_frag(f32x4 acc, float* __restrict__ C, int64_t m, int64_t n, int64_t N) {
  if (n + 3 < N && (N & 3) == 0) {
    *reinterpret_cast<float4*>(C + m * N + n) = make_float4(acc[0], acc[1], acc[2], acc[3]);
  } else {
    for (int r = 0; r < 4; ++r)
      if (n + r < N) C[m * N + n + r] = acc[r];
  }
}

// Host: launch with `lds` bytes of dynamic LDS -- above the 64 KB every kernel may ask for, the attribute is raised first
template <auto Kernel, typename... Args>
static int launch_dyn_lds(dim3 grid, int threads, int lds, hipStream_t st, Args... args) {
  if (lds > 65536)
    if (int rc = ensure_dyn_lds<Kernel>(lds)) return rc;
  Kernel<<<grid, threads, lds, st>>>(args...);
  CSN_LAUNCH_CHECK();
  return CSN_OK;
}

}  // namespace csn
