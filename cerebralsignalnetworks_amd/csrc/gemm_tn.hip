// bf16 TN GEMMs of the LSTM path (weight gradients): C[M,N] = A[K,M]^T * B[K,N], the contraction over the T*B rows.
// Operands are staged row-major [k][m] / [k][n] in LDS and read column-major with ds_read_b64_tr_b16; split-K into
// float32 slabs that a fixed-order reduction combines (bitwise reproducible, no atomics).  tn_route() says which
// kernel a shape takes:
//
//  gemm_tn_bf16      128x128 tiles, 32 contraction rows per step, 4 waves, register-staged double buffer.
//  gemm_tn_256       256x256 tiles, 8 waves, ring of LDS-DMA stages (the reference form of the next one).
//  gemm_tn_256w4     256x256 / 256x128 tiles on four waves, the default for long contractions.
// Everything else goes to launch_generic (gemm_f32.hip).
#include "gemm_tile.h"

namespace csn {

// =====================================================================================
// bf16 TN GEMM (weight gradient), 128x128 output tile, BK = 32 rows of the contraction
// =====================================================================================
// Fragment of a 16(m) x 32(k) operand from the [k][m] LDS image: lane l (g = l>>4, i = l&15)
// ends with elements j = 0..7 = tile[k = 8g + j][m = mbase + i].
// ds_read_b64_tr_b16 (per 16-lane group): lane 4q+p supplies the address of k-row q, columns
// 4p..4p+3 of a 4x16 block; lane i receives column i, k-row q in element q.
template <bool USE_TR>
__device__ __forceinline__ bf16x8 tn_load_frag(const char* tile, int mbase, int lane) {
  const int g = lane >> 4, i = lane & 15;
  bf16x8 out;
  if constexpr (USE_TR) {
    const int q = i >> 2, p = i & 3;
    s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) s16x4*)(tile + tn_lds_off(8 * g + q, mbase + 4 * p)));
    s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) s16x4*)(tile + tn_lds_off(8 * g + 4 + q, mbase + 4 * p)));
    union { s16x4 s[2]; bf16x8 b; } u;
    u.s[0] = lo;
    u.s[1] = hi;
    out = u.b;
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) out[j] = *reinterpret_cast<const bf16_t*>(tile + tn_lds_off(8 * g + j, mbase + i));
  }
  return out;
}

template <bool USE_TR>
__global__ void __launch_bounds__(256)
gemm_tn_bf16_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ Bm, float* __restrict__ slabs,
                    int64_t M, int64_t N, int64_t K, int64_t k_per_split) {
  __shared__ __attribute__((aligned(16))) char smem[2 * 16384];  // 2 buffers x (A 8 KB + B 8 KB)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  // logical order [split][m tile][n tile]: an XCD gets whole K splits (or contiguous parts of one), so
  // the tiles that stream the same rows of A and B at the same time share one L2
  const unsigned ntn = (unsigned)((N + 127) / 128), ntm = (unsigned)((M + 127) / 128);
  const unsigned lid = xcd_remap(blockIdx.x, gridDim.x);
  const unsigned zsplit = lid / (ntm * ntn), rem = lid % (ntm * ntn);
  const int64_t m0 = (int64_t)(rem / ntn) * 128, n0 = (int64_t)(rem % ntn) * 128;
  const int64_t kbeg = (int64_t)zsplit * k_per_split;
  const int64_t kend = (kbeg + k_per_split < K) ? kbeg + k_per_split : K;
  const int nk = (int)((kend - kbeg + 31) / 32);

  // staging: tile = 32 k-rows x 16 chunks (16 B = 8 columns); q = tid + i*256, i<2: krow = q>>4, ch = q&15
  uint4 ra[2], rb[2];
  auto load_tile = [&](int kt) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int q = tid + i * 256;
      const int kr = q >> 4, ch = q & 15;
      const int64_t k = kbeg + (int64_t)kt * 32 + kr;
      const int64_t am = m0 + ch * 8, bn = n0 + ch * 8;
      ra[i] = (k < kend && am < M) ? *reinterpret_cast<const uint4*>(A + k * M + am) : make_uint4(0, 0, 0, 0);
      rb[i] = (k < kend && bn < N) ? *reinterpret_cast<const uint4*>(Bm + k * N + bn) : make_uint4(0, 0, 0, 0);
    }
  };
  auto store_tile = [&](int buf) {
    char* a_s = smem + buf * 16384;
    char* b_s = a_s + 8192;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int q = tid + i * 256;
      const int kr = q >> 4, ch = q & 15;
      *reinterpret_cast<uint4*>(a_s + tn_lds_off(kr, ch * 8)) = ra[i];
      *reinterpret_cast<uint4*>(b_s + tn_lds_off(kr, ch * 8)) = rb[i];
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  if (nk > 0) {
    load_tile(0);
    store_tile(0);
  }
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) load_tile(kt + 1);
    const char* a_s = smem + buf * 16384;
    const char* b_s = a_s + 8192;
    bf16x8 af[4], bfr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) af[i] = tn_load_frag<USE_TR>(a_s, wm * 64 + i * 16, lane);
#pragma unroll
    for (int j = 0; j < 4; ++j) bfr[j] = tn_load_frag<USE_TR>(b_s, wn * 64 + j * 16, lane);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[j], af[i], acc[i][j], 0, 0, 0);
    if (kt + 1 < nk) store_tile(buf ^ 1);
    __syncthreads();
  }

  float* C = slabs + (int64_t)zsplit * M * N;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t m = m0 + wm * 64 + i * 16 + (lane & 15);
    if (m >= M) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) tn_store_frag(acc[i][j], C, m, n0 + wn * 64 + j * 16 + (lane >> 4) * 4, N);
  }
}

// TN, 256 x 256 output tile, 8 waves (2 along M x 4 along N, 128 x 64 outputs per wave), LDS-DMA stages of
// 32 k-rows: per 64 contraction rows a workgroup moves 64 KB for 8.4 MFLOP -- half the L2 bytes per flop of the
// 128 x 128 tiles, whose ceiling is the aggregate L2 bandwidth (~14 TB/s measured => ~0.9 PFLOP/s).
// Stage image: tn256_lds_off (gemm_tile.h).
// Pipeline: a ring of NSTAGE stages of 32 k-rows (A 16 KB + B 16 KB each); before the MFMAs of stage h the
// stages h+1 .. h+NSTAGE-2 are already in flight and stage h+NSTAGE-1 is issued (into the slot of stage h-1,
// which every wave has left: it passed this step's barrier).  A wave waits for its own part of stage h with a
// COUNTED vmcnt (4 LDS-DMA instructions per stage and wave) and the raw barrier then covers everybody's part;
// __syncthreads() would drain the whole ring (it waits vmcnt(0) while LDS-DMA is outstanding).
// both ds_read_b64_tr_b16 of one 16 x 32 fragment (k-rows q and q + 4 of each 8-row group), LDS byte address
// relative to the workgroup's LDS base (the dynamic array is the kernel's only LDS object, at offset 0)
__device__ __forceinline__ bf16x8 tr_read_pair(unsigned addr) {
  union { s16x4 s[2]; bf16x8 b; } u;
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(u.s[0]) : "v"(addr) : "memory");
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:2048" : "=v"(u.s[1]) : "v"(addr) : "memory");
  return u.b;
}

template <int NSTAGE, bool COLSUM>
__global__ void __launch_bounds__(512)
gemm_tn_256_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ Bm, float* __restrict__ slabs,
                   int64_t M, int64_t N, int64_t K, int64_t k_per_split, float* __restrict__ colsum) {
  extern __shared__ __attribute__((aligned(1024))) char smem[];  // NSTAGE x (A 16 KB + B 16 KB)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 2, wn = wave & 3;
  const unsigned ntn = (unsigned)((N + 255) / 256), ntm = (unsigned)((M + 255) / 256);
  const unsigned lid = xcd_remap(blockIdx.x, gridDim.x);
  const unsigned zsplit = lid / (ntm * ntn), rem = lid % (ntm * ntn);
  const int64_t m0 = (int64_t)(rem / ntn) * 256, n0 = (int64_t)(rem % ntn) * 256;
  const int64_t kbeg = (int64_t)zsplit * k_per_split;
  const int64_t kend = (kbeg + k_per_split < K) ? kbeg + k_per_split : K;
  const int nh = kend > kbeg ? (int)((kend - kbeg) / 32) : 0;     // stages of 32 k-rows

  // staging: instruction i (0..1) of wave w fills k-rows 2 (8 i + w), +1 of a stage (2 rows x 32 chunks = 1 KB);
  // lane -> k-row r = lane >> 5, LDS chunk position c = lane & 31 <- global columns ((c >> 1) ^ s) * 16 + (c & 1) * 8
  // (written out here and in gemm_tn_256w4_kernel: through a shared function the compiler forms other addresses)
  const bf16_t* a_src[2];
  const bf16_t* b_src[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int kr = 2 * (8 * i + wave) + (lane >> 5);
    const int c = lane & 31;
    const int sw = (kr & 3) | (((kr >> 3) & 1) << 2);
    const int col = (((c >> 1) ^ sw) << 4) + (c & 1) * 8;
    int64_t am = m0 + col, bn = n0 + col;
    am = am + 8 <= M ? am : M - 8;
    bn = bn + 8 <= N ? bn : N - 8;
    a_src[i] = A + (kbeg + kr) * M + am;
    b_src[i] = Bm + (kbeg + kr) * N + bn;
  }
#if defined(CSN_TN_ROT)     // timing experiment (tools/abl_build.sh): every tile of a K slab starts its walk a few stages further on
  const int rot_ = nh > CSN_TN_ROT ? (int)(rem % (unsigned)(CSN_TN_ROT)) : 0;
#endif
  auto issue = [&](int h) {
    char* a_s = smem + (h % NSTAGE) * 32768;
    char* b_s = a_s + 16384;
#if defined(CSN_TN_ROT)
    const int hs_ = h + rot_;
    const int64_t hr = hs_ >= nh ? hs_ - nh : hs_;
#else
    const int64_t hr = h;
#endif
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      glds16(a_src[i] + hr * 32 * M, a_s + (8 * i + wave) * 1024);
      glds16(b_src[i] + hr * 32 * N, b_s + (8 * i + wave) * 1024);
    }
  };

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  // optional column sums of A (the bias gradient: sum over the contraction rows of dgates): in the workgroups of
  // the first column tile every wave multiplies two of its eight A fragments by a fragment of ones too (the four
  // waves that share the A rows split the eight fragments: + 6 % MFMAs there, nothing elsewhere)
  // (a template switch: the extra accumulators cost the plain kernel 8 % even when unused)
  // (the wave index goes through readfirstlane so that the condition around the extra MFMA is a SCALAR branch:
  // under a mere EXEC mask the MFMA would still execute -- MFMA ignores EXEC -- and add foreign fragments)
  const int wn_s = __builtin_amdgcn_readfirstlane(wn);
  const bool do_colsum = COLSUM && colsum != nullptr && n0 == 0;
  const bf16x8 ones = {(bf16_t)1.0f, (bf16_t)1.0f, (bf16_t)1.0f, (bf16_t)1.0f, (bf16_t)1.0f, (bf16_t)1.0f, (bf16_t)1.0f, (bf16_t)1.0f};
  f32x4 acc_cs[2];
  acc_cs[0] = acc_cs[1] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // byte address (inside a stage) of this lane's first ds_read_b64_tr_b16 of every fragment; the second one
  // (k-rows + 4) is 2048 bytes further
  unsigned a_addr[8], b_addr[4];
  {
    const int g = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
#pragma unroll
    for (int i = 0; i < 8; ++i) a_addr[i] = (unsigned)tn256_lds_off(8 * g + q, wm * 128 + i * 16 + 4 * pp);
#pragma unroll
    for (int j = 0; j < 4; ++j) b_addr[j] = (unsigned)tn256_lds_off(8 * g + q, wn * 64 + j * 16 + 4 * pp);
  }

#pragma unroll
  for (int h = 0; h < NSTAGE - 1; ++h)
    if (h < nh) issue(h);
  for (int h = 0; h < nh; ++h) {
    // stages issued after h and still allowed in flight: min(NSTAGE - 2, nh - 1 - h)
    const int ahead = nh - 1 - h;
    if (ahead >= NSTAGE - 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * (NSTAGE - 2)) : "memory");
    else if (NSTAGE > 3 && ahead == 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (ahead == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (h + NSTAGE - 1 < nh) issue(h + NSTAGE - 1);
    // Fragment reads in inline asm: for an LDS read it can see, the compiler waits vmcnt(0) while ANY LDS-DMA is
    // outstanding (it cannot tell the stages apart), which would drain the ring every step.  LDS operations
    // complete in order, so counted lgkmcnt waits release the MFMAs of A tile i while tiles i+1, i+2 are in flight.
    const unsigned sb = (unsigned)(h % NSTAGE) * 32768u;
    bf16x8 af[8], bfr[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) bfr[j] = tr_read_pair(b_addr[j] + sb + 16384u);
    af[0] = tr_read_pair(a_addr[0] + sb);
    af[1] = tr_read_pair(a_addr[1] + sb);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (i + 2 < 8) {
        af[i + 2] = tr_read_pair(a_addr[i + 2] + sb);
        asm volatile("s_waitcnt lgkmcnt(4)" ::: "memory");
      } else if (i + 1 < 8) {
        asm volatile("s_waitcnt lgkmcnt(2)" ::: "memory");
      } else {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      }
      __builtin_amdgcn_sched_barrier(0);
#ifdef CSN_TN_SETPRIO
      __builtin_amdgcn_s_setprio(1);
#endif
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[j], af[i], acc[i][j], 0, 0, 0);
#ifdef CSN_TN_SETPRIO
      __builtin_amdgcn_s_setprio(0);
#endif
      if constexpr (COLSUM)
        if (do_colsum && (i >> 1) == wn_s) acc_cs[i & 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, af[i], acc_cs[i & 1], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  if (COLSUM && do_colsum && (lane >> 4) == 0) {       // D[n][m]: every row n holds the same sum; lanes 0..15 write column m
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int64_t m = m0 + wm * 128 + (2 * wn + e) * 16 + (lane & 15);
      if (m < M) colsum[(int64_t)zsplit * M + m] = acc_cs[e][0];
    }
  }

  float* C = slabs + (int64_t)zsplit * M * N;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int64_t m = m0 + wm * 128 + i * 16 + (lane & 15);
    if (m >= M) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      // (tn_store_frag of gemm_tile.h written out, here and in gemm_tn_256w4_kernel: through the function three
      // instantiations of the two come out with other registers and another order of independent instructions, and
      // one line of the A/B was not inside the parent's own spread -- DESIGN.md section 6)
      const int64_t n = n0 + wn * 64 + j * 16 + (lane >> 4) * 4;
      if (n + 3 < N && (N & 3) == 0) {
        *reinterpret_cast<float4*>(C + m * N + n) = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
      } else {
        for (int r = 0; r < 4; ++r)
          if (n + r < N) C[m * N + n + r] = acc[i][j][r];
      }
    }
  }
}

// The same tile on FOUR waves (2 along M x 2 along N), the default: a wave owns 128 x BN/2 outputs, so at BN = 256 the
// 256 accumulator registers fill the AGPR half and a 32-row k-step reads 4 x (128 + 128) x 32 x 2 B = 64 KB of LDS
// for 1024 MFMA cycles per SIMD (the 8-wave form above reads 96 KB for the same MFMAs).  Stage image, swizzle, k walk,
// K splits and slab layout are those of gemm_tn_256_kernel, and every output element sees the same 16 x 16 x 32 MFMA
// k-blocks in the same order: the slabs and the column sums are bit-identical to the 8-wave kernels'.
// BN = 128 (N <= 128, the layer-0 input weight gradient): a 256 x 128 tile whose B stage is 8 KB of 256-byte k-rows
// (same block swizzle: a row is still a whole number of bank sets), so no clamped duplicate columns are staged,
// read or multiplied.
// One wave per SIMD: nothing hides a stall of that wave, so the overlap has to come from inside it (the k-loop below):
// every fragment register is refilled for the next stage right behind the last MFMA that uses it, and the 4 A + BN/64 B
// DMA pieces of stage h + PF are issued two to an MFMA group instead of in one burst behind the barrier.
// Measured (3072 x 768 x 128 000): 8-wave staggered ring 541 us, this kernel 523; N = 128: 208 -> 156.
// A ring of 4 stages beats one of 5 at every prefetch distance tried (537 against 553 - 558 us on one box).
#ifndef CSN_TN_W4_NSTAGE      // ring depth and prefetch distance (timing experiments override them: tools/abl_build.sh)
#define CSN_TN_W4_NSTAGE 4
#endif
#ifndef CSN_TN_W4_PF
#define CSN_TN_W4_PF 3
#endif
// A fragment as the kernel below carries it from one k-step into the next: four plain dwords.  (As a loop-carried
// bf16x8 the compiler rebuilds it from 16-bit halves with VALU instructions placed right behind the inline-asm read,
// which it cannot know to be asynchronous -- before the data has landed.)  ROW4: bytes from k-row q to k-row q + 4.
typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
template <int ROW4>
__device__ __forceinline__ i32x4 tr_read_frag(unsigned addr) {
  union { i32x2 s[2]; i32x4 v; } u;
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(u.s[0]) : "v"(addr) : "memory");
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(u.s[1]) : "v"(addr), "n"(ROW4) : "memory");
  return u.v;
}

template <int NSTAGE, int PF, bool COLSUM, int BN>
__global__ void __launch_bounds__(256)
gemm_tn_256w4_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ Bm, float* __restrict__ slabs,
                     int64_t M, int64_t N, int64_t K, int64_t k_per_split, float* __restrict__ colsum) {
  static_assert(BN == 256 || BN == 128, "256 x 256 or 256 x 128 tile");
  static_assert(PF >= 2 && PF <= 4 && PF < NSTAGE, "stage h + 1 is read in step h: its slot and stage h's are no DMA targets");
  constexpr bool NARROW = BN == 128;
  constexpr int NJ = BN / 32;                  // B fragments per wave
  constexpr int NBP = BN / 64;                 // B pieces per wave and stage
  constexpr int NP = 4 + NBP;                  // LDS-DMA instructions per wave and stage
  constexpr unsigned B_OFF = 16384u;
  constexpr unsigned STAGE = 16384u + BN * 64u;
  extern __shared__ __attribute__((aligned(1024))) char smem[];  // NSTAGE x (A 16 KB + B 16 / 8 KB)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);       // scalar: the LDS address of a DMA piece goes to M0
  const int wm = wave >> 1, wn = wave & 1;
  const unsigned ntn = (unsigned)((N + 255) / 256), ntm = (unsigned)((M + 255) / 256);
  const unsigned lid = xcd_remap(blockIdx.x, gridDim.x);
  const unsigned zsplit = lid / (ntm * ntn), rem = lid % (ntm * ntn);
  const int64_t m0 = (int64_t)(rem / ntn) * 256, n0 = (int64_t)(rem % ntn) * 256;
  const int64_t kbeg = (int64_t)zsplit * k_per_split;
  const int64_t kend = (kbeg + k_per_split < K) ? kbeg + k_per_split : K;
  const int nh = __builtin_amdgcn_readfirstlane(kend > kbeg ? (int)((kend - kbeg) / 32) : 0);     // stages of 32 k-rows

  // staging: A instruction i (0..3) of wave w fills k-rows 2 (4 i + w), +1 of a stage, as in gemm_tn_256_kernel; at
  // BN = 128 B instruction i (0..1) of wave w fills the four 256-byte k-rows 4 (4 i + w) .. + 3: lane -> k-row
  // lane >> 4, chunk position c = lane & 15 <- global columns ((c >> 1) ^ s) * 16 + (c & 1) * 8
  const bf16_t* a_src[4];
  const bf16_t* b_src[NBP];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int kr = 2 * (4 * i + wave) + (lane >> 5);
    const int c = lane & 31;
    const int sw = (kr & 3) | (((kr >> 3) & 1) << 2);
    const int col = (((c >> 1) ^ sw) << 4) + (c & 1) * 8;
    int64_t am = m0 + col;
    am = am + 8 <= M ? am : M - 8;
    a_src[i] = A + (kbeg + kr) * M + am;
    if constexpr (!NARROW) {
      int64_t bn = n0 + col;
      bn = bn + 8 <= N ? bn : N - 8;
      b_src[i] = Bm + (kbeg + kr) * N + bn;
    }
  }
  if constexpr (NARROW) {
#pragma unroll
    for (int i = 0; i < NBP; ++i) {
      const int kr = 4 * (4 * i + wave) + (lane >> 4);
      const int c = lane & 15;
      const int sw = (kr & 3) | (((kr >> 3) & 1) << 2);
      int64_t bn = n0 + (((c >> 1) ^ sw) << 4) + (c & 1) * 8;
      bn = bn + 8 <= N ? bn : N - 8;
      b_src[i] = Bm + (kbeg + kr) * N + bn;
    }
  }
  // piece p of stage h: p even -> A piece p / 2, p odd -> B piece p / 2 while B pieces last, then the A pieces left
  auto issue_piece = [&](int h, int p) {
    char* a_s = smem + (unsigned)(h % NSTAGE) * STAGE;
    const int ib = p >> 1;
    const bool is_b = (p & 1) && ib < NBP;
    if (is_b) glds16(b_src[ib] + (int64_t)h * 32 * N, a_s + B_OFF + (4 * ib + wave) * 1024);
    else {
      const int ia = p < 2 * NBP ? ib : p - NBP;
      glds16(a_src[ia] + (int64_t)h * 32 * M, a_s + (4 * ia + wave) * 1024);
    }
  };

  f32x4 acc[8][NJ];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  // column sums of A (the bias gradient), one more MFMA per owned A fragment and k-step against a fragment of ones,
  // behind a scalar branch.  Every workgroup of a tile row stages the same A rows, so the eight fragments of a wave
  // row are dealt out over ALL its column tiles' waves -- fragment i to slot i mod min(2 ntn, 8), slot = 2 x column
  // tile + wn: at three column tiles a wave owns at most two (with one wave per SIMD nothing hides the extra MFMAs;
  // four per wave in the first column tile's workgroups held the whole launch back).  Same fragment, same k order:
  // the same bits whoever computes them.
  unsigned own_cs = 0;
  if (COLSUM && colsum != nullptr) {
    const unsigned nslots = 2 * ntn < 8 ? 2 * ntn : 8, slot = 2 * (rem % ntn) + (unsigned)wn;
#pragma unroll
    for (unsigned i = 0; i < 8; ++i) own_cs |= (i % nslots == slot ? 1u : 0u) << i;
  }
  own_cs = __builtin_amdgcn_readfirstlane(own_cs);
  // (the fragment of ones goes through an empty asm: a constant the compiler can re-materialise it rebuilds with v_mov
  // right in front of every inline-asm MFMA that reads it, closer than the hardware allows -- tools/check_asm_hazards.py)
  i32x4 ones = {0x3f803f80, 0x3f803f80, 0x3f803f80, 0x3f803f80};      // eight bf16 1.0
  asm volatile("" : "+v"(ones));
  f32x4 acc_cs[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc_cs[e] = (f32x4){0.f, 0.f, 0.f, 0.f};

  unsigned a_addr[8], b_addr[NJ];
  {
    const int g = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
#pragma unroll
    for (int i = 0; i < 8; ++i) a_addr[i] = (unsigned)tn256_lds_off(8 * g + q, wm * 128 + i * 16 + 4 * pp);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int col = wn * (BN / 2) + j * 16 + 4 * pp;
      b_addr[j] = B_OFF + (unsigned)(NARROW ? tn256_lds_off(8 * g + q, col) - (8 * g + q) * 256 : tn256_lds_off(8 * g + q, col));
    }
  }

#if defined(CSN_TN_ABL) && CSN_TN_ABL == 2       // (ablation 2, timing only: no LDS reads)
#define W4_READ_A(i, sb) __builtin_bit_cast(i32x4, (f32x4){(float)(sb), 3.f, 2.f, (float)(i)})
#define W4_READ_B(j, sb) __builtin_bit_cast(i32x4, (f32x4){(float)(sb), 1.f, 2.f, (float)(j)})
#else
#define W4_READ_A(i, sb) tr_read_frag<2048>(a_addr[i] + (sb))
#define W4_READ_B(j, sb) tr_read_frag<NARROW ? 1024 : 2048>(b_addr[j] + (sb))
#endif
  // A burst of fragment reads in front of the MFMAs that need them is exposed in full here (the B fragments read behind
  // the barrier cost the first form of this kernel a quarter of the k-step).  So the reads are spread evenly over the
  // step -- one pair about every fourth MFMA -- and every fragment register is refilled from stage h + 1 (') as soon
  // as the last MFMA of stage h that uses it has been issued.  That takes two traversals:
  //   first half : A row-blocks 0 .. 3 one after the other against all B fragments  (A i is free behind group i),
  //   second half: B fragments one after the other against A row-blocks 4 .. 7       (B j is free behind column j);
  // A 4 .. 7 of stage h are read during the first half.  Reads of a step in issue order (pairs, BN = 256; 128 alike):
  //   A4 A5 | A0' A6 | A1' A7 | A2' || A3' | B0' | B1' | .. | B6' B7'
  // LDS reads retire in order, and the counted wait in front of an MFMA is the number of reads issued behind the last
  // pair it needs: only group 0 (B j' may still be in flight) and the first MFMA of the second half (A7) wait.
  //   read-after-DMA : a wave retires ITS pieces of stage h + 1 (counted vmcnt) in front of step h's barrier; the
  //                    first read of stage h + 1 is behind that barrier.
  //   DMA-after-read : stage s is last read in step s (A 4 .. 7, retired before the second half); its slot takes
  //                    stage s + NSTAGE, requested in step s + NSTAGE - PF >= s + 1, behind that step's barrier.
  // (The last step reads "stage nh" too, from a slot nobody fills any more, and nobody uses it: one sequence of reads,
  // one set of counted waits.)
  if (nh > 0) {
#pragma unroll
    for (int h = 0; h < PF; ++h)
      if (h < nh) {
#pragma unroll
        for (int p = 0; p < NP; ++p) issue_piece(h, p);
      }
    // stage 0: stages issued after it and still allowed in flight: min(PF, nh) - 1
    if (nh >= PF) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NP * (PF - 1)) : "memory");
    else if (PF > 2 && nh == PF - 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NP * (PF - 2)) : "memory");
    else if (PF > 3 && nh == PF - 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NP * (PF - 3)) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    i32x4 af[8], bfr[NJ];
#pragma unroll
    for (int i = 0; i < 4; ++i) af[i] = W4_READ_A(i, 0u);
#pragma unroll
    for (int j = 0; j < NJ; ++j) bfr[j] = W4_READ_B(j, 0u);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    for (int h = 0; h < nh; ++h) {
      // stage h + 1: stages issued after it and still allowed in flight: min(PF - 2, nh - 2 - h)
      const int ahead = nh - 2 - h;
      if (ahead >= PF - 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NP * (PF - 2)) : "memory");
      else if (PF > 3 && ahead == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NP) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
#if defined(CSN_TN_ABL) && CSN_TN_ABL == 1       // (ablation 1, timing only: no DMA after the prologue)
      const bool more = false;
#else
      const bool more = h + PF < nh;
#endif
      const unsigned sb = (unsigned)(h % NSTAGE) * STAGE, sbn = (unsigned)((h + 1) % NSTAGE) * STAGE;
#if defined(CSN_TN_W4_BURST)                     // (timing experiment: the stage's pieces in one burst behind the barrier)
      if (more) {
#pragma unroll
        for (int p = 0; p < NP; ++p) issue_piece(h + PF, p);
      }
#endif
      // ---- first half: A row-blocks 0 .. 3
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          // behind B j' of the last step: B j+1' .. ; of this step: A4 (from MFMA 1 on), A5 (from MFMA NJ / 2 + 1 on)
          if (i == 0) asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(2 * (NJ - 1 - j + (j >= 1) + (j >= NJ / 2 + 1))) : "memory");
          __builtin_amdgcn_sched_barrier(0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, bfr[j]), __builtin_bit_cast(bf16x8, af[i]), acc[i][j], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
          if (j == 0) {
            if (i == 0) af[4] = W4_READ_A(4, sb);
            else af[i - 1] = W4_READ_A(i - 1, sbn);
          }
          if (j == NJ / 2 && i < 3) af[5 + i] = W4_READ_A(5 + i, sb);
          __builtin_amdgcn_sched_barrier(0);
#if !defined(CSN_TN_W4_BURST)
          // two DMA pieces of stage h + PF inside each group, behind MFMAs that wait for nothing new
          if (j == NJ / 4 && 2 * i < NP && more) issue_piece(h + PF, 2 * i);
          if (j == (3 * NJ) / 4 && 2 * i + 1 < NP && more) issue_piece(h + PF, 2 * i + 1);
          __builtin_amdgcn_sched_barrier(0);
#endif
        }
        if constexpr (COLSUM)
          if (own_cs & (1u << i))     // (inline asm: the builtin's accumulator would have to be an AGPR, and all 256 are taken)
            asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc_cs[i]) : "v"(ones), "v"(af[i]));
        __builtin_amdgcn_sched_barrier(0);
      }
      // ---- second half: B fragments 0 .. NJ - 1 against A row-blocks 4 .. 7 (A7 has A2' behind it)
      asm volatile("s_waitcnt lgkmcnt(2)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          acc[4 + k][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, bfr[j]), __builtin_bit_cast(bf16x8, af[4 + k]), acc[4 + k][j], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
          if (k == 0) {
            if (j == 0) af[3] = W4_READ_A(3, sbn);
            else bfr[j - 1] = W4_READ_B(j - 1, sbn);
          }
          if (k == 3 && j == NJ - 1) bfr[j] = W4_READ_B(j, sbn);
          __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (COLSUM)
          if (j < 4 && (own_cs & (16u << j)))
            asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc_cs[4 + j]) : "v"(ones), "v"(af[4 + j]));
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the unused reads of "stage nh"
  }
#undef W4_READ_A
#undef W4_READ_B

  if (COLSUM && (lane >> 4) == 0) {       // D[n][m]: every row n holds the same sum; lanes 0..15 write column m
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int64_t m = m0 + wm * 128 + e * 16 + (lane & 15);
      if ((own_cs & (1u << e)) && m < M) colsum[(int64_t)zsplit * M + m] = acc_cs[e][0];
    }
  }

  float* C = slabs + (int64_t)zsplit * M * N;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int64_t m = m0 + wm * 128 + i * 16 + (lane & 15);
    if (m >= M) continue;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int64_t n = n0 + wn * (BN / 2) + j * 16 + (lane >> 4) * 4;      // (written out: see gemm_tn_256_kernel)
      if (n + 3 < N && (N & 3) == 0) {
        *reinterpret_cast<float4*>(C + m * N + n) = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
      } else {
        for (int r = 0; r < 4; ++r)
          if (n + r < N) C[m * N + n + r] = acc[i][j][r];
      }
    }
  }
}

static int tn_splits(int64_t M, int64_t N, int64_t K) {
  const int64_t tiles = ((M + 127) / 128) * ((N + 127) / 128);
  int64_t s = (1024 + tiles - 1) / tiles;          // aim at >= 4 workgroups per CU
  const int64_t max_by_k = (K + 511) / 512;        // keep >= 512 contraction rows per split
  if (s > max_by_k) s = max_by_k;
  if (s < 1) s = 1;
  if (s > 64) s = 64;
  return (int)s;
}
// the 256 x 256 kernel: one workgroup per CU (128 KB of LDS), so the K splits fill the 256 CUs once
static bool tn_use_256(int64_t M, int64_t N, int64_t K, const Options& opt) {
  // (N >= 128: at N = 128 -- the layer-0 input weight gradient -- half of every tile's columns are clamped duplicates
  // whose results are discarded, and it still beats the 128 x 128 register-staged kernel)
  return M >= 256 && N >= 128 && K % 64 == 0 && K >= 8192 && !opt.gemm_no_dma && !opt.gemm_no_256;
}
static int tn_splits_256(int64_t M, int64_t N, int64_t K) {
  const int64_t tiles = ((M + 255) / 256) * ((N + 255) / 256);
  int64_t s = 256 / tiles;
  const int64_t max_by_k = K / 2048;               // keep >= 32 k-steps per split
  if (s > max_by_k) s = max_by_k;
  if (s < 1) s = 1;
  if (s > 64) s = 64;
  return (int)s;
}
size_t gemm_tn_scratch_bytes(int64_t M, int64_t N, int64_t K, const Options& opt) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  const int a = tn_splits(M, N, K), b = tn_use_256(M, N, K, opt) ? tn_splits_256(M, N, K) : 0;
  return (size_t)(a > b ? a : b) * (size_t)M * (size_t)N * sizeof(float);
}

// ---- which kernel: pure host functions (csn_gemm_tn_route reports them to the tests; cabi.py names the values) ----
enum TnRoute { TN_GENERIC = 0, TN_TILE128 = 1, TN_TILE128_NOTR = 2, TN_RING3 = 3, TN_RING4 = 4, TN_RING5 = 5, TN_W4_128 = 6, TN_W4_256 = 7 };
struct TnChoice { TnRoute route; int tile; };      // the kernel and the tile its grid and K splits are counted in

// the bf16 kernels' precondition: operand type, divisibility, 16-byte aligned A and B
static bool tn_fast(int64_t M, int64_t N, int dtype, bool aligned16) {
  return dtype == CSN_BF16 && (M % 8 == 0) && (N % 8 == 0) && aligned16;
}

static TnChoice tn_route(int64_t M, int64_t N, int64_t K, bool fast, bool colsum, const Options& opt) {
  if (fast && tn_use_256(M, N, K, opt)) {
    // the default: the four-wave kernel.  CSN_TN_NO_STAGGER (a name from when the default was a staggered 8-wave ring)
    // and CSN_TN_STAGES=3|5 select the 8-wave single-phase rings, the reference form the tests compare it with.
    if (!opt.tn_no_stagger && opt.tn_stages == 4) return {N <= 128 ? TN_W4_128 : TN_W4_256, 256};   // 256 x 128 tile body: no clamped duplicate columns
    if (colsum) return {TN_RING4, 256};          // the only 8-wave ring with column sums
    return {opt.tn_stages == 3 ? TN_RING3 : opt.tn_stages == 5 ? TN_RING5 : TN_RING4, 256};
  }
  if (fast && !opt.gemm_generic) return {opt.tn_no_tr ? TN_TILE128_NOTR : TN_TILE128, 128};
  return {TN_GENERIC, 128};
}

// ---- how to launch it: the instantiation with or without the column sums of A ----
struct TnArgs {
  const bf16_t* A; const bf16_t* B; float* slabs;
  int64_t M, N, K, kper; float* colsum; hipStream_t st;
};
template <auto KernelColsum, auto KernelPlain>
static int launch_tn256(dim3 grid, int threads, int lds, const TnArgs& a) {
  if (a.colsum) return launch_dyn_lds<KernelColsum>(grid, threads, lds, a.st, a.A, a.B, a.slabs, a.M, a.N, a.K, a.kper, a.colsum);
  return launch_dyn_lds<KernelPlain>(grid, threads, lds, a.st, a.A, a.B, a.slabs, a.M, a.N, a.K, a.kper, (float*)nullptr);
}

// colsum (optional): device buffer of at least 64 * M floats; if the kernel that runs can produce the column sums
// of A on the way (one partial row of M values per K split), *colsum_done is set to 1.
int launch_gemm_tn_slabs(const void* A, const void* B, float* slabs, int64_t M, int64_t N, int64_t K, int dtype,
                         hipStream_t st, int* S_out, float* colsum, int* colsum_done, const Options& opt) {
  const bool aligned16 = ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(B)) & 15) == 0;
  const TnChoice r = tn_route(M, N, K, tn_fast(M, N, dtype, aligned16), colsum != nullptr, opt);
  const int S = r.tile == 256 ? tn_splits_256(M, N, K) : tn_splits(M, N, K);
  int64_t kper = (K + S - 1) / S;
  kper = (kper + 63) / 64 * 64;
  *S_out = S;
  if (colsum_done) *colsum_done = r.tile == 256 && colsum ? 1 : 0;
  const dim3 grid((unsigned)(((N + r.tile - 1) / r.tile) * ((M + r.tile - 1) / r.tile) * S));
  const TnArgs a = {(const bf16_t*)A, (const bf16_t*)B, slabs, M, N, K, kper, colsum, st};
  constexpr int NS = CSN_TN_W4_NSTAGE, PF = CSN_TN_W4_PF;
  switch (r.route) {
    case TN_W4_128: return launch_tn256<&gemm_tn_256w4_kernel<NS, PF, true, 128>, &gemm_tn_256w4_kernel<NS, PF, false, 128>>(grid, 256, NS * (16384 + 8192), a);
    case TN_W4_256: return launch_tn256<&gemm_tn_256w4_kernel<NS, PF, true, 256>, &gemm_tn_256w4_kernel<NS, PF, false, 256>>(grid, 256, NS * 32768, a);
    case TN_RING4: return launch_tn256<&gemm_tn_256_kernel<4, true>, &gemm_tn_256_kernel<4, false>>(grid, 512, 4 * 32768, a);
    case TN_RING3: return launch_dyn_lds<&gemm_tn_256_kernel<3, false>>(grid, 512, 3 * 32768, st, a.A, a.B, slabs, M, N, K, kper, (float*)nullptr);
    case TN_RING5: return launch_dyn_lds<&gemm_tn_256_kernel<5, false>>(grid, 512, 5 * 32768, st, a.A, a.B, slabs, M, N, K, kper, (float*)nullptr);
    case TN_TILE128: return launch_dyn_lds<&gemm_tn_bf16_kernel<true>>(grid, 256, 0, st, a.A, a.B, slabs, M, N, K, kper);
    case TN_TILE128_NOTR: return launch_dyn_lds<&gemm_tn_bf16_kernel<false>>(grid, 256, 0, st, a.A, a.B, slabs, M, N, K, kper);
    case TN_GENERIC: break;
  }
  // A(m,k) = A[k*M + m], B(k,n) = B[k*N + n]
  return launch_generic(A, 1, M, B, N, 1, nullptr, slabs, N, M, N, K, dtype, CSN_F32, 0, S, M * N, st);
}

}  // namespace csn

using namespace csn;

extern "C" size_t csn_gemm_tn_scratch_bytes(int64_t M, int64_t N, int64_t K) {
  return gemm_tn_scratch_bytes(M, N, K, options_from_env());
}
// Host-only diagnostic for the tests (bound on use by cabi.py, not part of the public header): the TnRoute that
// launch_gemm_tn_slabs takes under the current environment's switches, with (colsum = 1) or without a column-sum buffer.
extern "C" int csn_gemm_tn_route(int64_t M, int64_t N, int64_t K, int dtype, int aligned16, int colsum) {
  if (M <= 0 || N <= 0 || K <= 0) return -1;
  return (int)tn_route(M, N, K, tn_fast(M, N, dtype, aligned16 != 0), colsum != 0, options_from_env()).route;
}

extern "C" int csn_gemm_tn(const void* A, const void* B, float* C, int64_t M, int64_t N, int64_t K, int dtype,
                           void* scratch, csnStream_t stream) {
  CSN_REQUIRE(A && B && C && scratch, "csn_gemm_tn: null pointer");
  CSN_REQUIRE(M > 0 && N > 0 && K > 0, "csn_gemm_tn: bad shape");
  CSN_REQUIRE(dtype == CSN_F32 || dtype == CSN_BF16, "csn_gemm_tn: bad dtype %d", dtype);
  hipStream_t st = as_stream(stream);
  int S = 1;
  if (int rc = launch_gemm_tn_slabs(A, B, (float*)scratch, M, N, K, dtype, st, &S, nullptr, nullptr, options_from_env())) return rc;
  return launch_reduce_slabs((const float*)scratch, M * N, S, C, nullptr, M * N, 0, st);
}
