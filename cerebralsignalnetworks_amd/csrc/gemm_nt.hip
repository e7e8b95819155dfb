// bf16 NT GEMMs of the LSTM path (input projections, input gradients): C[M,N] (+)= A[M,K] * Bt[N,K]^T (+ bias), f32 or
// bf16 out, v_mfma_f32_16x16x32_bf16; algorithmic flops 2*M*N*K.  nt_route() says which kernel a shape takes:
//
//  gemm_nt_bf16      128x128x64 tiles, 4 waves (2x2) of 64x64, one LDS buffer with an XOR swizzle that makes the
//                    ds_read_b128 fragment reads conflict-free, register-staged prefetch: any K % 8 == 0.
//  gemm_nt_dma       the same tile through LDS-DMA, two buffers (K % 64 == 0).
//  gemm_nt_256       256x128 tiles, 8 waves, ring of three LDS-DMA stages, epilogue through LDS.
//  gemm_nt_wide      256x192 / 256x256 tiles, 8 waves, one workgroup per CU.
//  gemm_nt_w4        256x192 tiles on four waves, two workgroups per CU.
// Everything else goes to launch_generic (gemm_f32.hip).
#include "gemm_tile.h"

namespace csn {

// =====================================================================================
// bf16 NT GEMM, 128x128x64 tiles
// =====================================================================================
// One 32 KB LDS buffer, two barriers per k-tile -- small enough to co-reside on a CU with the weight-stationary
// LSTM kernel (100 KB LDS), which is how the input-projection GEMMs overlap the recurrence.
template <typename OutT>
__global__ void __launch_bounds__(256)
gemm_nt_bf16_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ Bt, const float* __restrict__ bias,
                    OutT* __restrict__ C, int64_t M, int64_t N, int64_t K, int accumulate) {
  extern __shared__ __attribute__((aligned(16))) char smem[];  // A 16 KB + B 16 KB
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  // logical order: N tiles fastest inside an M tile, so one XCD walks the N tiles of "its" M tiles and
  // the A panel of an M tile is fetched into a single L2
  const unsigned ntn = (unsigned)((N + 127) / 128);
  const unsigned lid = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t m0 = (int64_t)(lid / ntn) * 128, n0 = (int64_t)(lid % ntn) * 128;
  const int nk = (int)((K + 63) / 64);

  // global->register staging: each thread moves 4 chunks of A and 4 of B per k-tile.
  // chunk id q = tid + i*256 (0..1023): row = q >> 3, chunk = q & 7 (8 lanes cover one 128-B row).
  uint4 ra[4], rb[4];
  auto load_tile = [&](int kt) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int q = tid + i * 256;
      const int row = q >> 3, ch = q & 7;
      const int64_t k = (int64_t)kt * 64 + ch * 8;
      const int64_t am = m0 + row, bn = n0 + row;
      ra[i] = (am < M && k < K) ? *reinterpret_cast<const uint4*>(A + am * K + k) : make_uint4(0, 0, 0, 0);
      rb[i] = (bn < N && k < K) ? *reinterpret_cast<const uint4*>(Bt + bn * K + k) : make_uint4(0, 0, 0, 0);
    }
  };
  char* const a_s = smem;
  char* const b_s = a_s + 16384;
  auto store_tile = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int q = tid + i * 256;
      const int row = q >> 3, ch = q & 7;
      *reinterpret_cast<uint4*>(a_s + nt_lds_off(row, ch)) = ra[i];
      *reinterpret_cast<uint4*>(b_s + nt_lds_off(row, ch)) = rb[i];
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  load_tile(0);
  store_tile();
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) load_tile(kt + 1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 af[4], bfr[4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        af[i] = *reinterpret_cast<const bf16x8*>(a_s + nt_lds_off(wm * 64 + i * 16 + (lane & 15), kk * 4 + (lane >> 4)));
#pragma unroll
      for (int j = 0; j < 4; ++j)
        bfr[j] = *reinterpret_cast<const bf16x8*>(b_s + nt_lds_off(wn * 64 + j * 16 + (lane & 15), kk * 4 + (lane >> 4)));
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          // swapped operands: D[row = n][col = m]: lane holds m = lane&15, n = (lane>>4)*4 + r
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[j], af[i], acc[i][j], 0, 0, 0);
    }
    __syncthreads();                          // everyone has read the tile before it is overwritten
    if (kt + 1 < nk) store_tile();
    __syncthreads();
  }

#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t m = m0 + wm * 64 + i * 16 + (lane & 15);
    if (m >= M) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      nt_store_frag<OutT, true>(acc[i][j], bias, C, m, n0 + wn * 64 + j * 16 + (lane >> 4) * 4, N, accumulate);
  }
}

// The same tile through LDS-DMA (gemm_tile.h), two buffers
template <typename OutT>
__global__ void __launch_bounds__(256)
gemm_nt_dma_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ Bt, const float* __restrict__ bias,
                   OutT* __restrict__ C, int64_t M, int64_t N, int64_t K, int accumulate) {
  extern __shared__ __attribute__((aligned(1024))) char smem[];  // 2 buffers x (A 16 KB + B 16 KB)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const unsigned ntn = (unsigned)((N + 127) / 128);
  const unsigned ntiles = ntn * (unsigned)((M + 127) / 128);
  const int nk = (int)(K / 64);
  // (a grid smaller than the tile count would walk the tiles; gemm_nt() launches one workgroup per tile, so the loop
  // runs once -- the GEMM beside a persistent LSTM launch, for which it was written, is gemm_beside.h now.  The loop
  // and the barrier at its head stay: without them the kernel's code changes, and no measurement covers that)
  for (unsigned lid = xcd_remap(blockIdx.x, gridDim.x); lid < ntiles; lid += gridDim.x) {
  const int64_t m0 = (int64_t)(lid / ntn) * 128, n0 = (int64_t)(lid % ntn) * 128;
  __syncthreads();     // every wave has left the previous tile's last LDS buffer

  // staging: instruction i of wave w fills rows [(4 i + w) 8, +8) of a tile (8 rows x 8 chunks = 1 KB);
  // lane -> row r = lane >> 3, LDS chunk position c = lane & 7 <- global chunk c ^ ((row >> 1) & 7)
  // (nt_dma_src of gemm_tile.h written out: through the function this kernel's code comes out two s_nop longer)
  const bf16_t* a_src[4];
  const bf16_t* b_src[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = (4 * i + wave) * 8 + (lane >> 3);
    const int ch = (lane & 7) ^ ((row >> 1) & 7);
    int64_t am = m0 + row, bn = n0 + row;
    am = am < M ? am : M - 1;
    bn = bn < N ? bn : N - 1;
    a_src[i] = A + am * K + ch * 8;
    b_src[i] = Bt + bn * K + ch * 8;
  }
  auto issue = [&](int kt, int buf) {
    char* a_s = smem + buf * 32768;
    char* b_s = a_s + 16384;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      glds16(a_src[i] + (int64_t)kt * 64, a_s + (4 * i + wave) * 1024);
      glds16(b_src[i] + (int64_t)kt * 64, b_s + (4 * i + wave) * 1024);
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  issue(0, 0);
  for (int kt = 0; kt < nk; ++kt) {
    // tile kt has landed (own loads: vmcnt; everyone's: barrier) and every wave is done reading the other buffer
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (kt + 1 < nk) issue(kt + 1, (kt + 1) & 1);
    const char* a_s = smem + (kt & 1) * 32768;
    const char* b_s = a_s + 16384;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 af[4], bfr[4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        af[i] = *reinterpret_cast<const bf16x8*>(a_s + nt_lds_off(wm * 64 + i * 16 + (lane & 15), kk * 4 + (lane >> 4)));
#pragma unroll
      for (int j = 0; j < 4; ++j)
        bfr[j] = *reinterpret_cast<const bf16x8*>(b_s + nt_lds_off(wn * 64 + j * 16 + (lane & 15), kk * 4 + (lane >> 4)));
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[j], af[i], acc[i][j], 0, 0, 0);
    }
  }

#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t m = m0 + wm * 64 + i * 16 + (lane & 15);
    if (m >= M) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      nt_store_frag<OutT, true>(acc[i][j], bias, C, m, n0 + wn * 64 + j * 16 + (lane >> 4) * 4, N, accumulate);
  }
  }   // tile loop
}

// NT, 256 x 128 output tile, 8 waves (4 along M x 2 along N, 64 x 64 outputs per wave), ring of NSTAGE LDS-DMA
// stages of 64 contraction columns (A 32 KB + B 16 KB each, the 128-byte-row image and swizzle of nt_lds_off),
// counted vmcnt + raw barrier, fragment reads in inline asm (see gemm_tn_256_kernel for why).
template <typename OutT, int NSTAGE>
__global__ void __launch_bounds__(512)
gemm_nt_256_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ Bt, const float* __restrict__ bias,
                   OutT* __restrict__ C, int64_t M, int64_t N, int64_t K, int accumulate) {
  extern __shared__ __attribute__((aligned(1024))) char smem[];  // NSTAGE x (A 32 KB + B 16 KB)
  constexpr unsigned kStage = 49152;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const unsigned ntn = (unsigned)((N + 127) / 128);
  const unsigned ntiles = ntn * (unsigned)((M + 255) / 256);
  const int nk = (int)(K / 64);
  // (one workgroup per tile: the loop runs once, see gemm_nt_dma_kernel)
  for (unsigned lid = xcd_remap(blockIdx.x, gridDim.x); lid < ntiles; lid += gridDim.x) {
  const int64_t m0 = (int64_t)(lid / ntn) * 256, n0 = (int64_t)(lid % ntn) * 128;
  __syncthreads();     // every wave has left the previous tile's last stage

  // staging: a 1 KB instruction fills 8 rows x 8 chunks (nt_dma_src); A has 32 of them per stage (4 per wave), B 16
  // (2 per wave)
  const bf16_t* a_src[4];
  const bf16_t* b_src[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) a_src[i] = nt_dma_src<true>(A, m0, M, K, 8 * i + wave, lane);
#pragma unroll
  for (int i = 0; i < 2; ++i) b_src[i] = nt_dma_src<true>(Bt, n0, N, K, 8 * i + wave, lane);
  auto issue = [&](int kt) {
    char* a_s = smem + (kt % NSTAGE) * kStage;
    char* b_s = a_s + 32768;
#pragma unroll
    for (int i = 0; i < 4; ++i) glds16(a_src[i] + (int64_t)kt * 64, a_s + (8 * i + wave) * 1024);
#pragma unroll
    for (int i = 0; i < 2; ++i) glds16(b_src[i] + (int64_t)kt * 64, b_s + (8 * i + wave) * 1024);
  };

  // fragment addresses inside a stage: tile i of A is 2048 bytes further, the second k-half flips chunk bit 2
  const unsigned sw = (unsigned)((lane & 15) >> 1);
  const unsigned a_base = (unsigned)((wm * 64 + (lane & 15)) * 128) + ((((unsigned)lane >> 4) ^ sw) << 4);
  const unsigned b_base = 32768u + (unsigned)((wn * 64 + (lane & 15)) * 128) + ((((unsigned)lane >> 4) ^ sw) << 4);

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int h = 0; h < NSTAGE - 1; ++h)
    if (h < nk) issue(h);
  for (int kt = 0; kt < nk; ++kt) {
    const int ahead = nk - 1 - kt;            // stages issued after kt: min(NSTAGE - 2, ahead) stay in flight
    if (ahead >= NSTAGE - 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(6 * (NSTAGE - 2)) : "memory");
    else if (NSTAGE > 3 && ahead == 1) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (kt + NSTAGE - 1 < nk) issue(kt + NSTAGE - 1);
    const unsigned sb = (unsigned)(kt % NSTAGE) * kStage;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const unsigned xo = kk ? 64u : 0u;
      bf16x8 af[4], bfr[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) bfr[j] = lds_read_b128(((b_base ^ xo) + sb) + j * 2048u);
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = lds_read_b128(((a_base ^ xo) + sb) + i * 2048u);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (i == 0) asm volatile("s_waitcnt lgkmcnt(3)" ::: "memory");
        else if (i == 1) asm volatile("s_waitcnt lgkmcnt(2)" ::: "memory");
        else if (i == 2) asm volatile("s_waitcnt lgkmcnt(1)" ::: "memory");
        else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[j], af[i], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }

  // ---- epilogue through LDS: in the accumulator layout a wave's store instruction covers 16 rows x 64 bytes (16 half
  // cache lines); staged as a [256][128] f32 image in the ring's memory, every store instruction writes two full
  // 512-byte rows of the tile
  constexpr int LDC = 132;                    // padded row (floats): the 16 rows of a fragment column fall in 16 distinct bank groups
  static_assert(256 * LDC * 4 <= NSTAGE * 49152, "the C image lives in the staging ring");
  float* const cs = reinterpret_cast<float*>(smem);
  __syncthreads();                            // (every DMA has landed: the last k-step waited vmcnt(0)) all waves have left the ring
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      *reinterpret_cast<f32x4*>(cs + (wm * 64 + i * 16 + (lane & 15)) * LDC + wn * 64 + j * 16 + (lane >> 4) * 4) = acc[i][j];
  __syncthreads();
  {
    const int c4 = tid & 31, r0 = tid >> 5;
    const int64_t n = n0 + c4 * 4;
    const bool vec = n + 3 < N;
    f32x4 bz = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (bias) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (n + r < N) bz[r] = bias[n + r];
    }
#pragma unroll 4
    for (int pass = 0; pass < 16; ++pass) {
      const int row = pass * 16 + r0;
      const int64_t m = m0 + row;
      if (m >= M) continue;
      f32x4 v = *reinterpret_cast<const f32x4*>(cs + row * LDC + c4 * 4) + bz;
#if defined(CSN_NT_ABL) && CSN_NT_ABL == 1     // (ablation, timing only: no C stores unless a value is NaN)
      if (v[0] == v[0]) continue;
#endif
      // (nt_store4 / nt_store1 of gemm_tile.h written out: through them the float32 instantiation comes out with other
      // registers and another order of independent instructions, and on two lines of the A/B it was not inside the
      // parent's own spread -- DESIGN.md section 6)
      if (vec) {
        if constexpr (sizeof(OutT) == 4) {
          float4* dst = reinterpret_cast<float4*>((float*)C + m * N + n);
          if (accumulate) { const float4 o = *dst; v[0] += o.x; v[1] += o.y; v[2] += o.z; v[3] += o.w; }
          *dst = make_float4(v[0], v[1], v[2], v[3]);
        } else {
          bf16x4 o = {(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
          *reinterpret_cast<bf16x4*>((bf16_t*)C + m * N + n) = o;
        }
      } else {
        for (int r = 0; r < 4; ++r)
          if (n + r < N) {
            if constexpr (sizeof(OutT) == 4) {
              float* dst = (float*)C + m * N + n + r;
              *dst = accumulate ? *dst + v[r] : v[r];
            } else {
              ((bf16_t*)C)[m * N + n + r] = (bf16_t)v[r];
            }
          }
      }
    }
  }
  }   // tile loop
}

// NT, 256 x BN output tile, BN = 192 or 256 (N % BN == 0), 8 waves, one workgroup per CU.  The default at BN = 256 (cfg4's
// projection); at BN = 192 the four-wave gemm_nt_w4_kernel below is the default and this instantiation the reference form
// (CSN_NT_NO_W4, and operands outside that kernel's 32-bit offsets).  The 256 x 128 kernel with a wider tile -- at the LSTM's chunk shapes
// (8192 x 3072 x 768 with BN = 192, 8192 x 4096 x 1024 with BN = 256) 512 tiles = exactly two per CU instead of three /
// four, 21 % / 33 % fewer bytes through the L2 -> CU fabric, which is what the 256 x 128 form is bound by (DESIGN.md
// section 6: the vendor library's 192 x 256 kernel is faster by exactly that ratio).  8 waves (4 along M x 2 along N,
// 64 x BN/2 outputs per wave).  A stage of 64 contraction columns is 32 KB of A + 24 / 32 KB of B, three of which do not
// fit the 160 KB of LDS: A keeps a ring of THREE stages (two k-steps ahead: the streaming operand), B a ring of TWO (one
// k-step ahead: a few hundred KB per column tile, read by 16 workgroups at a time, L2-resident).  144 / 160 KB.
template <typename OutT, int BN>
__global__ void __launch_bounds__(512)
gemm_nt_wide_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ Bt, const float* __restrict__ bias,
                   OutT* __restrict__ C, int64_t M, int64_t N, int64_t K, int accumulate) {
  static_assert(BN == 192 || BN == 256, "column tile");
  extern __shared__ __attribute__((aligned(1024))) char smem[];  // A: 3 x 32 KB, then B: 2 x (24 | 32) KB
  constexpr unsigned kBBase = 3 * 32768, kBStage = BN * 128;
  constexpr int NBI = BN / 64;       // B staging instructions per wave and stage
  constexpr int NBF = BN / 32;       // B fragments (16 columns each) per wave
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const unsigned ntn = (unsigned)(N / BN);
  const unsigned ntiles = ntn * (unsigned)((M + 255) / 256);
  const int nk = (int)(K / 64);
#if defined(CSN_NT_STAGGER)      // timing experiment (tools/abl_build.sh): every second first-wave workgroup of an XCD starts late, so that
  if (blockIdx.x < 256u && ((blockIdx.x >> 3) & 1u)) {      // one half of the chip stores its tile while the other half streams operands
    const unsigned long long t0_ = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0_ < (unsigned long long)(CSN_NT_STAGGER)) __builtin_amdgcn_s_sleep(8);
  }
#endif
  // (one workgroup per tile: the loop runs once, see gemm_nt_dma_kernel)
  for (unsigned lid = xcd_remap(blockIdx.x, gridDim.x); lid < ntiles; lid += gridDim.x) {
  const int64_t m0 = (int64_t)(lid / ntn) * 256, n0 = (int64_t)(lid % ntn) * BN;
  __syncthreads();     // every wave has left the previous tile's last stage

  // staging as in gemm_nt_256_kernel; A has 32 instructions per stage (4 per wave), B 24 / 32 (3 / 4 per wave) and
  // needs no clamp (N % BN == 0)
  const bf16_t* a_src[4];
  const bf16_t* b_src[NBI];
#pragma unroll
  for (int i = 0; i < 4; ++i) a_src[i] = nt_dma_src<true>(A, m0, M, K, 8 * i + wave, lane);
#pragma unroll
  for (int i = 0; i < NBI; ++i) b_src[i] = nt_dma_src<false>(Bt, n0, N, K, 8 * i + wave, lane);
#if defined(CSN_NT_ROT)     // timing experiment: the column tiles that share an A panel (and the row tiles that share a B panel) start
  const int nrot_ = (int)(lid % (unsigned)nk);      // their k walk at different steps, so that they are not all on the same lines at once
#else
  const int nrot_ = 0;
#endif
  auto kpos = [&](int kt) { const int k = kt + nrot_; return (int64_t)(k >= nk ? k - nk : k) * 64; };
  auto issue_a = [&](int kt) {
    char* a_s = smem + (kt % 3) * 32768;
#pragma unroll
    for (int i = 0; i < 4; ++i) glds16(a_src[i] + kpos(kt), a_s + (8 * i + wave) * 1024);
  };
  auto issue_b = [&](int kt) {
    char* b_s = smem + kBBase + (kt % 2) * kBStage;
#pragma unroll
    for (int i = 0; i < NBI; ++i) glds16(b_src[i] + kpos(kt), b_s + (8 * i + wave) * 1024);
  };

  const unsigned sw = (unsigned)((lane & 15) >> 1);
  const unsigned a_base = (unsigned)((wm * 64 + (lane & 15)) * 128) + ((((unsigned)lane >> 4) ^ sw) << 4);
  const unsigned b_base = kBBase + (unsigned)((wn * (BN / 2) + (lane & 15)) * 128) + ((((unsigned)lane >> 4) ^ sw) << 4);

  f32x4 acc[4][NBF];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NBF; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // issue order: A(0) B(0) A(1) | step kt: B(kt+1) A(kt+2).  Behind B(kt) the wave has issued only A(kt+1) (4 pieces):
  // vmcnt(4) = "A(kt) and B(kt) have landed" (vector-memory operations retire in order)
  issue_a(0);
  issue_b(0);
  if (nk > 1) issue_a(1);
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();      // everybody's pieces of step kt are there; everybody has left step kt - 1
    if (kt + 1 < nk) issue_b(kt + 1);  // (slot of B(kt-1))
    if (kt + 2 < nk) issue_a(kt + 2);  // (slot of A(kt-1))
    const unsigned sa = (unsigned)(kt % 3) * 32768u, sb = (unsigned)(kt % 2) * kBStage;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const unsigned xo = kk ? 64u : 0u;
      bf16x8 af[4], bfr[NBF];
#pragma unroll
      for (int j = 0; j < NBF; ++j) bfr[j] = lds_read_b128(((b_base ^ xo) + sb) + j * 2048u);
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = lds_read_b128(((a_base ^ xo) + sa) + i * 2048u);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (i == 0) asm volatile("s_waitcnt lgkmcnt(3)" ::: "memory");
        else if (i == 1) asm volatile("s_waitcnt lgkmcnt(2)" ::: "memory");
        else if (i == 2) asm volatile("s_waitcnt lgkmcnt(1)" ::: "memory");
        else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < NBF; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[j], af[i], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }

  // epilogue from the accumulators: lane holds row m = .. + (lane & 15), columns n .. n + 3 (a store instruction covers 16
  // rows x 64 bytes)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t m = m0 + wm * 64 + i * 16 + (lane & 15);
    if (m >= M) continue;
#pragma unroll
    for (int j = 0; j < NBF; ++j) {
      const int64_t n = n0 + wn * (BN / 2) + j * 16 + (lane >> 4) * 4;
      const f32x4 v = nt_with_bias(acc[i][j], bias, n);
#if defined(CSN_NT_ABL) && CSN_NT_ABL == 1     // (ablation, timing only: no C stores unless a value is NaN)
      if (v[0] == v[0]) continue;
#endif
      nt_store4<OutT>(v, C, m * N + n, accumulate);
    }
  }
  }   // tile loop
}

// The 256 x 192 tile on FOUR waves (2 along M x 2 along N, 128 x 96 outputs per wave = 8 x 6 accumulator fragments), TWO
// workgroups to a CU, the default for BN = 192: the 192 store instructions of a tile's epilogue cost the CU about a quarter
// of the launch when nothing else runs on it, and with two independent workgroups resident one
// stores while the other multiplies.  Residency is a speed property only: no workgroup waits for another.
// Stage: 32 contraction columns, A 256 rows x 64 B = 16 KB, B 192 rows x 64 B = 12 KB.  LDS image: 64-byte rows, four
// 16-byte chunks per row, chunk ch of row r at position ch ^ nt64_sw(r): the 16 lanes of every ds_read_b128 lane group
// ({0-3,12-15,20-27}, ...) then hit the 16 distinct 16-byte slots of the 256-byte bank row when lane l reads row
// (l & 15), chunk (l >> 4).  A 1 KB LDS-DMA instruction fills 16 rows x 4 chunks, the swizzle on the source side.
// Rings as in gemm_nt_wide_kernel: A (the streaming operand) NA stages, two k-steps ahead at NA = 3; B (L2-resident)
// two stages, one k-step ahead; NA x 16 + 24 KB = 72 KB at NA = 3, two workgroups in a CU's 160 KB.  Counted vmcnt +
// raw barrier; the 3 B + 4 A pieces of a step go one to an MFMA group; the six B fragments of a stage are held, the A
// fragments streamed one ahead of the MFMA group that uses them.
// Same 16 x 16 x 32 k-blocks per output element in ascending k, same operand order, same epilogue arithmetic as
// gemm_nt_wide_kernel / gemm_nt_256_kernel: float32 results are bit-identical, bf16 the same rounding of them.
// Source offsets are 32-bit byte offsets per lane against the scalar operand base (7 registers instead of 14 at 243 of
// 256): the launcher takes this kernel only where nt_w4_offsets_fit().
#ifndef CSN_NT_W4_NA          // A ring depth (timing experiments override it: tools/abl_build.sh)
#define CSN_NT_W4_NA 3
#endif
template <typename OutT, int NA>
__global__ void __launch_bounds__(256, 2)
gemm_nt_w4_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ Bt, const float* __restrict__ bias,
                  OutT* __restrict__ C, int64_t M, int64_t N, int64_t K, int accumulate) {
  static_assert(NA == 2 || NA == 3, "A ring depth");
  constexpr unsigned kAStage = 16384u, kBStage = 12288u, kBBase = NA * kAStage;
  static_assert(kBBase + 2 * kBStage <= 81920u, "two workgroups per CU");
  extern __shared__ __attribute__((aligned(1024))) char smem[];  // A: NA x 16 KB, then B: 2 x 12 KB
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);       // scalar: the LDS address of a DMA piece goes to M0
  const int wm = wave >> 1, wn = wave & 1;
  const unsigned ntn = (unsigned)(N / 192);
  const unsigned lid = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t m0 = (int64_t)(lid / ntn) * 256, n0 = (int64_t)(lid % ntn) * 192;
  const int nk = __builtin_amdgcn_readfirstlane((int)(K / 32));

  // staging: instruction i of wave w fills rows [(4 i + w) 16, + 16) of a stage; lane -> row lane >> 2, LDS chunk
  // position c = lane & 3 <- global chunk c ^ nt64_sw(row); A has 16 instructions per stage (4 per wave), B 12 (3)
  unsigned a_off[4], b_off[3];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = (4 * i + wave) * 16 + (lane >> 2);
    const int ch = (lane & 3) ^ nt64_sw(row);
    int64_t am = m0 + row;
    am = am < M ? am : M - 1;
    a_off[i] = (unsigned)((am * K + ch * 8) * 2);
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int row = (4 * i + wave) * 16 + (lane >> 2);
    const int ch = (lane & 3) ^ nt64_sw(row);
    b_off[i] = (unsigned)(((n0 + row) * K + ch * 8) * 2);
  }
  auto issue_a = [&](int kt, int i) {
    glds16(reinterpret_cast<const char*>(A + (int64_t)kt * 32) + a_off[i], smem + (unsigned)(kt % NA) * kAStage + (4 * i + wave) * 1024);
  };
  auto issue_b = [&](int kt, int i) {
    glds16(reinterpret_cast<const char*>(Bt + (int64_t)kt * 32) + b_off[i], smem + kBBase + (unsigned)(kt & 1) * kBStage + (4 * i + wave) * 1024);
  };

  // fragment addresses inside a stage: fragment i is 16 rows = 1024 bytes further (the swizzle repeats every 16 rows)
  const unsigned frag = (unsigned)((lane & 15) * 64) + ((((unsigned)lane >> 4) ^ (unsigned)nt64_sw(lane & 15)) << 4);
  const unsigned a_base = (unsigned)(wm * 128 * 64) + frag;
  const unsigned b_base = kBBase + (unsigned)(wn * 96 * 64) + frag;
#define W4_READ(addr, off) ({ bf16x8 v_; asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v_) : "v"(addr), "n"(off) : "memory"); v_; })

  f32x4 acc[8][6];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 6; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // issue order: A(0) B(0) [A(1)] | step kt: B(kt+1), then A(kt+NA-1).  Behind B(kt) the wave has issued only A(kt+1)
  // at NA = 3 (4 pieces): vmcnt(4) = "my pieces of A(kt) and B(kt) have landed" (vector-memory operations retire in
  // order); at NA = 2 nothing: vmcnt(0).
  //   read-after-DMA : the wait sits in front of step kt's barrier, the first read of stage kt behind it.
  //   DMA-after-read : the slots of B(kt+1) and A(kt+NA-1) were last read in step kt - 1; a wave's reads of a step are
  //                    retired by that step's MFMAs' counted lgkmcnt, all of them in front of step kt's barrier.
#pragma unroll
  for (int i = 0; i < 4; ++i) issue_a(0, i);
#pragma unroll
  for (int i = 0; i < 3; ++i) issue_b(0, i);
  if (NA == 3 && nk > 1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) issue_a(1, i);
  }
  for (int kt = 0; kt < nk; ++kt) {
    if (NA == 3 && kt + 1 < nk) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    const bool more_b = kt + 1 < nk, more_a = kt + NA - 1 < nk;
    const unsigned aa = a_base + (unsigned)(kt % NA) * kAStage, ba = b_base + (unsigned)(kt & 1) * kBStage;
    bf16x8 af[2], bfr[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) bfr[j] = W4_READ(ba, j * 1024);
    af[0] = W4_READ(aa, 0);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (i < 7) af[(i + 1) & 1] = W4_READ(aa, (i + 1) * 1024);
      if (i < 7) asm volatile("s_waitcnt lgkmcnt(1)" ::: "memory");      // everything but A i+1
      else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[j], af[i & 1], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (j == 1) {        // one DMA piece per MFMA group, behind MFMAs that wait for nothing new
          if (i < 3) { if (more_b) issue_b(kt + 1, i); }
          else if (i < 7) { if (more_a) issue_a(kt + NA - 1, i - 3); }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
  }
#undef W4_READ

  // epilogue from the accumulators, as gemm_nt_wide_kernel (N % 192 == 0: no column tail)
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int64_t m = m0 + wm * 128 + i * 16 + (lane & 15);
    if (m >= M) continue;
#pragma unroll
    for (int j = 0; j < 6; ++j)
      nt_store_frag<OutT, false>(acc[i][j], bias, C, m, n0 + wn * 96 + j * 16 + (lane >> 4) * 4, N, accumulate);
  }
}

// gemm_nt_w4_kernel addresses its operands with 32-bit byte offsets per lane: both must be smaller than 4 GiB
static bool nt_w4_offsets_fit(int64_t M, int64_t N, int64_t K) {
  const int64_t lim = (int64_t)1 << 31;      // elements of 2 bytes
  return M <= lim / K && N <= lim / K && M * K < lim && N * K < lim;
}
static constexpr int kNtW4LdsBytes = CSN_NT_W4_NA * 16384 + 2 * 12288;
static_assert(kNtW4LdsBytes <= 81920, "two workgroups of gemm_nt_w4_kernel per CU");

// ---- which kernel: pure host functions (csn_gemm_nt_route reports them to the tests; cabi.py names the values) ----
enum NtRoute { NT_GENERIC = 0, NT_BF16 = 1, NT_DMA = 2, NT_TILE256X128 = 3, NT_WIDE192 = 4, NT_WIDE256 = 5, NT_WIDE192W4 = 6 };
struct NtChoice { NtRoute route; int bm, bn; };      // the kernel and its output tile

// the bf16 kernels' precondition: operand type, divisibility, 16-byte aligned A, Bt, C and bias
static bool nt_fast(int64_t N, int64_t K, int dtype, bool aligned16, const Options& opt) {
  return dtype == CSN_BF16 && (K % 8 == 0) && (N % 4 == 0) && aligned16 && !opt.gemm_generic;
}

static NtChoice nt_route(int64_t M, int64_t N, int64_t K, bool fast, const Options& opt) {
  if (!fast) return {NT_GENERIC, 64, 64};
  if (K % 64 == 0 && K >= 128 && M >= 256 && !opt.gemm_no_dma && !opt.gemm_no_256 && !opt.gemm_no_192) {
    // 256 x 256 or 256 x 192 tiles where they give every CU whole tiles: 33 % / 21 % fewer operand bytes per flop than
    // 256 x 128 (measured at 8192 x 3072 x 768: 53.2 vs 59.0 us, 39.4 vs 47.2 without the C stores; at 8192 x 768 x 3072
    // -- 128 tiles of 192 -- 66 vs 47: hence "at least one tile per CU, and at most 10 % of the last round empty")
    auto fills = [&](int bn) {
      if (N % bn != 0) return false;
      const int64_t t = (N / bn) * ((M + 255) / 256), rounds = (t + 255) / 256;
      return t >= 256 && t * 10 >= rounds * 256 * 9;
    };
    if (fills(256)) return {NT_WIDE256, 256, 256};
    // four waves, two workgroups per CU (CSN_NT_NO_W4: the 8-wave kernel, the reference form)
    if (fills(192)) return {!opt.nt_no_w4 && nt_w4_offsets_fit(M, N, K) ? NT_WIDE192W4 : NT_WIDE192, 256, 192};
  }
  // 256 x 128 tiles where the tile count still fills the chip a few times over (measured at the LSTM's chunk
  // shapes: 58 vs 67 us at N = 3072, 56 vs 51 us at N = 768)
  if (K % 64 == 0 && K >= 256 && M >= 256 && N >= 1024 && !opt.gemm_no_dma && !opt.gemm_no_256) return {NT_TILE256X128, 256, 128};
  if (K % 64 == 0 && !opt.gemm_no_dma) return {NT_DMA, 128, 128};
  return {NT_BF16, 128, 128};
}

// ---- how to launch it: the bf16-out or the f32-out instantiation of a kernel (a bf16 C never accumulates) ----
struct NtArgs {
  const bf16_t* A; const bf16_t* Bt; const float* bias; void* C;
  int64_t M, N, K; int out_dtype, accumulate; hipStream_t st;
};
template <auto KernelBf16, auto KernelF32>
static int launch_nt(dim3 grid, int threads, int lds, const NtArgs& a) {
  if (a.out_dtype == CSN_BF16) return launch_dyn_lds<KernelBf16>(grid, threads, lds, a.st, a.A, a.Bt, a.bias, (bf16_t*)a.C, a.M, a.N, a.K, 0);
  return launch_dyn_lds<KernelF32>(grid, threads, lds, a.st, a.A, a.Bt, a.bias, (float*)a.C, a.M, a.N, a.K, a.accumulate);
}

int gemm_nt(const void* A, const void* Bt, const float* bias, void* C, int64_t M, int64_t N, int64_t K, int dtype,
            int out_dtype, int accumulate, hipStream_t st, const Options& opt) {
  CSN_REQUIRE(A && Bt && C, "csn_gemm_nt: null pointer");
  CSN_REQUIRE(M > 0 && N > 0 && K > 0, "csn_gemm_nt: bad shape M=%lld N=%lld K=%lld", (long long)M, (long long)N,
              (long long)K);
  CSN_REQUIRE(dtype == CSN_F32 || dtype == CSN_BF16, "csn_gemm_nt: bad dtype %d", dtype);
  CSN_REQUIRE(out_dtype == CSN_F32 || out_dtype == CSN_BF16, "csn_gemm_nt: bad out_dtype %d", out_dtype);
  CSN_REQUIRE(!(accumulate && out_dtype != CSN_F32), "csn_gemm_nt: accumulate needs a float32 C");
  const bool aligned16 = ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(Bt) |
                           reinterpret_cast<uintptr_t>(C) | reinterpret_cast<uintptr_t>(bias)) & 15) == 0;
  const NtChoice r = nt_route(M, N, K, nt_fast(N, K, dtype, aligned16, opt), opt);
  const dim3 grid((unsigned)(((N + r.bn - 1) / r.bn) * ((M + r.bm - 1) / r.bm)));
  const NtArgs a = {(const bf16_t*)A, (const bf16_t*)Bt, bias, C, M, N, K, out_dtype, accumulate, st};
  switch (r.route) {
    case NT_WIDE256: return launch_nt<&gemm_nt_wide_kernel<bf16_t, 256>, &gemm_nt_wide_kernel<float, 256>>(grid, 512, 3 * 32768 + 2 * 256 * 128, a);
    case NT_WIDE192: return launch_nt<&gemm_nt_wide_kernel<bf16_t, 192>, &gemm_nt_wide_kernel<float, 192>>(grid, 512, 3 * 32768 + 2 * 192 * 128, a);
    case NT_WIDE192W4: return launch_nt<&gemm_nt_w4_kernel<bf16_t, CSN_NT_W4_NA>, &gemm_nt_w4_kernel<float, CSN_NT_W4_NA>>(grid, 256, kNtW4LdsBytes, a);
    case NT_TILE256X128: return launch_nt<&gemm_nt_256_kernel<bf16_t, 3>, &gemm_nt_256_kernel<float, 3>>(grid, 512, 3 * 49152, a);
    case NT_DMA: return launch_nt<&gemm_nt_dma_kernel<bf16_t>, &gemm_nt_dma_kernel<float>>(grid, 256, 65536, a);
    case NT_BF16: return launch_nt<&gemm_nt_bf16_kernel<bf16_t>, &gemm_nt_bf16_kernel<float>>(grid, 256, 32768, a);
    case NT_GENERIC: break;
  }
  return launch_generic(A, K, 1, Bt, 1, K, bias, C, N, M, N, K, dtype, out_dtype, accumulate, 1, 0, st);
}

}  // namespace csn

using namespace csn;

extern "C" int csn_gemm_nt(const void* A, const void* Bt, const float* bias, void* C, int64_t M, int64_t N, int64_t K,
                           int dtype, int out_dtype, int accumulate, csnStream_t stream) {
  return gemm_nt(A, Bt, bias, C, M, N, K, dtype, out_dtype, accumulate, as_stream(stream), options_from_env());
}

// Host-only diagnostics of the dispatch above for the tests (bound on use by cabi.py; not part of the public header, so
// a library from before them still loads for an A/B run): 1 where gemm_nt_w4_kernel's 32-bit offsets cover A[M, K] and
// Bt[N, K], the dynamic LDS bytes of its launches, and the NtRoute csn_gemm_nt takes under the current environment's
// switches for operands that are (aligned16 = 1) or are not all 16-byte aligned.
extern "C" int csn_gemm_nt_w4_offsets_fit(int64_t M, int64_t N, int64_t K) {
  return M > 0 && N > 0 && K > 0 && nt_w4_offsets_fit(M, N, K) ? 1 : 0;
}
extern "C" int csn_gemm_nt_w4_lds_bytes(void) { return kNtW4LdsBytes; }
extern "C" int csn_gemm_nt_route(int64_t M, int64_t N, int64_t K, int dtype, int aligned16) {
  const Options opt = options_from_env();
  return M > 0 && N > 0 && K > 0 ? (int)nt_route(M, N, K, nt_fast(N, K, dtype, aligned16 != 0, opt), opt).route : -1;
}

