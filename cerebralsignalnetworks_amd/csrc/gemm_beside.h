// A bf16 NT GEMM as a DEVICE function for a 256-thread workgroup that is alone on its CU: C[M,N] (f32) =
// A[M,K] * Bt[N,K]^T, all row-major, no bias, tiles dealt to `nworkers` workgroups.  It runs
// inside the weight-stationary backward launch (lstm_bwd_persist.hip) on the workgroups that launch would otherwise
// leave idle -- the input gradient dx of the chunk the layer above finished one launch ago -- so it needs no stream,
// event or flag: both of its dependencies are kernel boundaries.
//
// Two tile bodies, bit-identical results (an output element sees the same 16 x 16 x 32 k-blocks in ascending k in both):
//   wide   256 x 192 tiles where N % 192 == 0 (H = 768, 384), dealt XCD by XCD (beside_xcd_tiles); structure =
//          gemm_nt_w4_kernel (gemm_nt.hip): stages of 32 contraction columns (A 16 KB + B 12 KB, 64-byte rows, its
//          swizzle), 4 waves (2 x 2) of 128 x 96 outputs, the six B fragments of a stage held, the A fragments streamed,
//          one DMA piece per MFMA group; here A and B share one ring of kBesideWideStages stages.
//   narrow 256 x 128 tiles dealt round-robin, every other width and CSN_BESIDE_128=1; structure = gemm_nt_256_kernel:
//          ring of 3 stages of 64 contraction columns (A 32 KB + B 16 KB, 128-byte rows, XOR swizzle applied on the
//          source side), 4 waves (2 x 2) of 128 x 64 outputs each.
// Both: primitives from gemm_tile.h, counted vmcnt + raw barrier, fragment reads in inline asm with counted lgkmcnt.
// K % 64 == 0, N % 4 == 0.
#pragma once
#include "gemm_tile.h"
#include "lstm_cell_blk.h"

namespace csn {

static constexpr int kBesideStages = 3;
static constexpr unsigned kBesideStageBytes = 49152;
static constexpr unsigned kBesideLdsBytes = kBesideStages * kBesideStageBytes;

// ring depth of the wide body: 3 to 5 stages of 28 KB fit the workers' LDS (timing experiments override it:
// tools/abl_build.sh; depths tried: DESIGN.md section 6)
#ifndef CSN_BESIDE_WIDE_STAGES
#define CSN_BESIDE_WIDE_STAGES 4
#endif
static constexpr int kBesideWideStages = CSN_BESIDE_WIDE_STAGES;
static constexpr unsigned kBesideWideStageBytes = 16384 + 12288;
static_assert(kBesideWideStages >= 3 && kBesideWideStages * kBesideWideStageBytes <= kBesideLdsBytes, "wide ring depth");

// The XCD-local tile walk.  Tiles are numbered row panel by row panel, `ntn` column tiles each.  The workers
// [xbase, xbase + xcount) of the nworkers share an XCD (and its L2): that XCD takes the whole row panels
// [npanels * xbase / nworkers, npanels * (xbase + xcount) / nworkers), and its workers deal the tiles of that range
// round-robin among themselves -- at H = 768 (ntn = 4, 8 workers) two row panels at a time, so a panel of A is
// fetched by one XCD, once.  The panel ranges of the XCDs partition [0, npanels) because their worker ranges partition
// [0, nworkers): every tile is visited exactly once for any worker counts.  Worker `local` of the XCD walks
// first, first + step, ... < end.  (Pure: tests/test_beside_wide_cpu.py mirrors it.)
struct BesideWalk { unsigned first, end, step; };
__host__ __device__ __forceinline__ BesideWalk beside_xcd_tiles(unsigned npanels, unsigned ntn, unsigned xbase, unsigned xcount,
                                                                unsigned local, unsigned nworkers) {
  // (32-bit products: M is an int, so npanels < 2^23, and a launch has at most 256 workers)
  const unsigned p0 = npanels * xbase / nworkers, p1 = npanels * (xbase + xcount) / nworkers;
  return BesideWalk{p0 * ntn + local, p1 * ntn, xcount};
}

#define CSN_BESIDE_VMCNT(n) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(n) : "memory")

// the wide body: `smem` as below; N % 192 == 0, K % 32 == 0, 255 * K * 2 bytes below 4 GiB (launch_bwd_persist checks K)
__device__ __forceinline__ void beside_gemm_tiles_wide(const BesideGemm& g, char* smem, const BesideWalk walk) {
  constexpr int NS = kBesideWideStages;
  constexpr unsigned kStage = kBesideWideStageBytes, kBOff = 16384u;     // a stage: A 256 rows x 64 B, then B 192 rows x 64 B
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);             // scalar: the LDS address of a DMA piece goes to M0
  const int wm = wave >> 1, wn = wave & 1;
  const int64_t M = g.M, N = g.N, K = g.K;
  const unsigned ntn = (unsigned)(N / 192);
  const int nk = __builtin_amdgcn_readfirstlane((int)(K / 32));
  // fragment addresses inside a stage (gemm_nt_w4_kernel): fragment i is 16 rows = 1024 bytes further
  const unsigned frag = (unsigned)((lane & 15) * 64) + ((((unsigned)lane >> 4) ^ (unsigned)nt64_sw(lane & 15)) << 4);
  const unsigned a_base = (unsigned)(wm * 128 * 64) + frag;
  const unsigned b_base = kBOff + (unsigned)(wn * 96 * 64) + frag;
#define BESIDE_READ(addr, off) ({ bf16x8 v_; asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v_) : "v"(addr), "n"(off) : "memory"); v_; })

  for (unsigned lid = walk.first; lid < walk.end; lid += walk.step) {
    __syncthreads();     // every wave has left the previous tile's last stage
    const int64_t m0 = (int64_t)(lid / ntn) * 256, n0 = (int64_t)(lid % ntn) * 192;
    // staging: piece i of wave w fills rows [(4 i + w) 16, + 16) of a stage's operand; lane -> row lane >> 2, LDS chunk
    // position c = lane & 3 <- global chunk c ^ nt64_sw(row); A has 16 pieces per stage (4 per wave), B 12 (3).
    // Offsets are 32-bit, against the tile's first row; rows beyond M read the last row (the epilogue drops them)
    const char* const a_tile = reinterpret_cast<const char*>(g.A + m0 * K);
    const char* const b_tile = reinterpret_cast<const char*>(g.Bt + n0 * K);
    const int last = (int)(M - m0 < 256 ? M - m0 : 256) - 1;
    unsigned a_off[4], b_off[3];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = (4 * i + wave) * 16 + (lane >> 2);
      const int ch = (lane & 3) ^ nt64_sw(row);
      a_off[i] = (unsigned)(((int64_t)(row < last ? row : last) * K + ch * 8) * 2);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int row = (4 * i + wave) * 16 + (lane >> 2);
      const int ch = (lane & 3) ^ nt64_sw(row);
      b_off[i] = (unsigned)(((int64_t)row * K + ch * 8) * 2);
    }
    // piece p of the 7 a wave contributes to the stage in slot `slot` holding contraction columns [32 kt, + 32)
    auto issue = [&](int kt, unsigned slot, int p) {
      char* const s = smem + slot * kStage;
      if (p < 4) glds16(a_tile + (int64_t)kt * 64 + a_off[p], s + (4 * p + wave) * 1024);
      else glds16(b_tile + (int64_t)kt * 64 + b_off[p - 4], s + kBOff + (4 * (p - 4) + wave) * 1024);
    };

    f32x4 acc[8][6];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 6; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // issue order: stages 0 .. NS - 2, then in step kt stage kt + NS - 1, seven pieces per wave and stage.  Behind its
    // pieces of stage kt a wave has issued min(NS - 2, nk - 1 - kt) stages: the counted wait says "my pieces of stage
    // kt have landed" (vector-memory operations retire in order).
    //   read-after-DMA : the wait sits in front of step kt's barrier, the first read of stage kt behind it.
    //   DMA-after-read : the slot of stage kt + NS - 1 was last read in step kt - 1; a wave's reads of a step are
    //                    retired by that step's MFMAs' counted lgkmcnt, all of them in front of step kt's barrier.
#pragma unroll
    for (int h = 0; h < NS - 1; ++h)
      if (h < nk) {
#pragma unroll
        for (int p = 0; p < 7; ++p) issue(h, (unsigned)h, p);
      }
    unsigned cur = 0, nxt = NS - 1;      // slots of stage kt and of stage kt + NS - 1
    for (int kt = 0; kt < nk; ++kt) {
      const int ahead = nk - 1 - kt;
      if (ahead >= NS - 2) CSN_BESIDE_VMCNT(7 * (NS - 2));
      else if (NS > 4 && ahead == 2) CSN_BESIDE_VMCNT(14);
      else if (NS > 3 && ahead == 1) CSN_BESIDE_VMCNT(7);
      else CSN_BESIDE_VMCNT(0);
      __builtin_amdgcn_s_barrier();
      const bool more = kt + NS - 1 < nk;
      const unsigned aa = a_base + cur * kStage, ba = b_base + cur * kStage;
      bf16x8 af[2], bfr[6];
#pragma unroll
      for (int j = 0; j < 6; ++j) bfr[j] = BESIDE_READ(ba, j * 1024);
      af[0] = BESIDE_READ(aa, 0);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (i < 7) af[(i + 1) & 1] = BESIDE_READ(aa, (i + 1) * 1024);
        if (i < 7) asm volatile("s_waitcnt lgkmcnt(1)" ::: "memory");      // everything but A i+1
        else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[j], af[i & 1], acc[i][j], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
          if (j == 1 && i < 7) {     // one DMA piece per MFMA group, behind MFMAs that wait for nothing new
            if (more) issue(kt + NS - 1, nxt, i);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
      cur = cur + 1 == NS ? 0 : cur + 1;
      nxt = nxt + 1 == NS ? 0 : nxt + 1;
    }

#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int64_t m = m0 + wm * 128 + i * 16 + (lane & 15);
      if (m >= M) continue;
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        // (written out like the narrow body's stores below, for the same reason; N % 192 == 0: no column tail)
        const int64_t n = n0 + wn * 96 + j * 16 + (lane >> 4) * 4;
        *reinterpret_cast<float4*>(g.C + m * N + n) = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
      }
    }
  }
#undef BESIDE_READ
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// the narrow body; worker = this workgroup's index among the nworkers workgroups that share the GEMM: tile
// worker + i nworkers, column tiles fastest
__device__ __forceinline__ void beside_gemm_tiles_narrow(const BesideGemm& g, char* smem, unsigned worker, unsigned nworkers) {
  constexpr int NSTAGE = kBesideStages;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int64_t M = g.M, N = g.N, K = g.K;
  const unsigned ntn = (unsigned)((N + 127) / 128);
  const unsigned ntiles = ntn * (unsigned)((M + 255) / 256);
  const int nk = (int)(K / 64);
  const unsigned sw = (unsigned)((lane & 15) >> 1);
  const unsigned a_base = (unsigned)((wm * 128 + (lane & 15)) * 128) + ((((unsigned)lane >> 4) ^ sw) << 4);
  const unsigned b_base = 32768u + (unsigned)((wn * 64 + (lane & 15)) * 128) + ((((unsigned)lane >> 4) ^ sw) << 4);

  for (unsigned lid = worker; lid < ntiles; lid += nworkers) {
    __syncthreads();     // every wave has left the previous tile's last stage
    const int64_t m0 = (int64_t)(lid / ntn) * 256, n0 = (int64_t)(lid % ntn) * 128;
    // staging: a 1 KB instruction fills 8 rows x 8 chunks; A has 32 per stage (8 per wave), B 16 (4 per wave);
    // lane -> row r = lane >> 3, LDS chunk position c = lane & 7 <- global chunk c ^ ((row >> 1) & 7)
    // (nt_dma_src of gemm_tile.h written out: the addresses are formed per stage here, not held in registers)
    const int srow = lane >> 3;
    auto issue = [&](int kt) {
      char* a_s = smem + (kt % NSTAGE) * kBesideStageBytes;
      char* b_s = a_s + 32768;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int row = (4 * i + wave) * 8 + srow;
        const int ch = (lane & 7) ^ ((row >> 1) & 7);
        int64_t am = m0 + row;
        am = am < M ? am : M - 1;
        glds16(g.A + am * K + (int64_t)kt * 64 + ch * 8, a_s + (4 * i + wave) * 1024);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = (4 * i + wave) * 8 + srow;
        const int ch = (lane & 7) ^ ((row >> 1) & 7);
        int64_t bn = n0 + row;
        bn = bn < N ? bn : N - 1;
        glds16(g.Bt + bn * K + (int64_t)kt * 64 + ch * 8, b_s + (4 * i + wave) * 1024);
      }
    };

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

#pragma unroll
    for (int h = 0; h < NSTAGE - 1; ++h)
      if (h < nk) issue(h);
    for (int kt = 0; kt < nk; ++kt) {
      const int ahead = nk - 1 - kt;            // stages issued after kt: min(NSTAGE - 2, ahead) stay in flight
      if (ahead >= NSTAGE - 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(12 * (NSTAGE - 2)) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      if (kt + NSTAGE - 1 < nk) issue(kt + NSTAGE - 1);
      const unsigned sb = (unsigned)(kt % NSTAGE) * kBesideStageBytes;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const unsigned xo = kk ? 64u : 0u;
        bf16x8 af[8], bfr[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bfr[j] = lds_read_b128(((b_base ^ xo) + sb) + j * 2048u);
#pragma unroll
        for (int i = 0; i < 8; ++i) af[i] = lds_read_b128(((a_base ^ xo) + sb) + i * 2048u);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          switch (7 - i) {   // LDS reads complete in order: A tile i is ready once at most 7 - i younger reads are out
            case 7: asm volatile("s_waitcnt lgkmcnt(7)" ::: "memory"); break;
            case 6: asm volatile("s_waitcnt lgkmcnt(6)" ::: "memory"); break;
            case 5: asm volatile("s_waitcnt lgkmcnt(5)" ::: "memory"); break;
            case 4: asm volatile("s_waitcnt lgkmcnt(4)" ::: "memory"); break;
            case 3: asm volatile("s_waitcnt lgkmcnt(3)" ::: "memory"); break;
            case 2: asm volatile("s_waitcnt lgkmcnt(2)" ::: "memory"); break;
            case 1: asm volatile("s_waitcnt lgkmcnt(1)" ::: "memory"); break;
            default: asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); break;
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[j], af[i], acc[i][j], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }

#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int64_t m = m0 + wm * 128 + i * 16 + (lane & 15);
      if (m >= M) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        // (nt_store_frag of gemm_tile.h without bias and accumulation, written out: through the function the
        // compiler addresses g.C differently in all 36 instantiations of the backward kernel)
        const int64_t n = n0 + wn * 64 + j * 16 + (lane >> 4) * 4;
        if (n + 3 < N) {
          *reinterpret_cast<float4*>(g.C + m * N + n) = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
        } else {
          for (int r = 0; r < 4; ++r)
            if (n + r < N) g.C[m * N + n + r] = acc[i][j][r];
        }
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
#undef CSN_BESIDE_VMCNT

// Host: which body a GEMM of a grouped launch takes -- `ngroups` XCDs run a hand-off group on `nslices` of their
// `grid_slices` workgroups, the other workgroups are the workers.  A launch with such a GEMM ends with the GEMM's last
// round of tiles, and a wide tile takes about 1.3 times as long as a narrow one (80 against 62 us beside the recurrence
// at K = 3072): the wide body where N % 192 == 0, unless its busiest worker then has two or more
// tiles and 1.3 times its rounds exceed the narrow body's (cfg2's second-last launch: 20 row panels are 2 rounds either way).
static inline bool beside_takes_wide(int64_t M, int64_t N, int ngroups, int nslices, int grid_slices) {
  if (N % 192 != 0) return false;
  const unsigned idle = (unsigned)(grid_slices - nslices), nworkers = (unsigned)ngroups * idle + (unsigned)(8 - ngroups) * grid_slices;
  if (nworkers == 0) return false;
  const unsigned npanels = (unsigned)((M + 255) / 256), ntn = (unsigned)(N / 192);
  unsigned wide_rounds = 0, base = 0;
  for (int x = 0; x < 8; ++x) {
    const unsigned count = x < ngroups ? idle : (unsigned)grid_slices;
    if (count == 0) continue;
    const BesideWalk w = beside_xcd_tiles(npanels, ntn, base, count, 0, nworkers);
    const unsigned rounds = (w.end - w.first + count - 1) / count;
    wide_rounds = rounds > wide_rounds ? rounds : wide_rounds;
    base += count;
  }
  const unsigned narrow_rounds = (npanels * (unsigned)((N + 127) / 128) + nworkers - 1) / nworkers;
  return wide_rounds < 2 || 13 * wide_rounds <= 10 * narrow_rounds;
}

// `smem`: the workgroup's dynamic LDS (at LDS offset 0, >= kBesideLdsBytes).  The workgroup is worker xbase + local of
// nworkers; the workers [xbase, xbase + xcount) are those of its XCD.  wide: what beside_takes_wide() said of this GEMM.
__device__ __forceinline__ void beside_gemm_tiles(const BesideGemm& g, char* smem, unsigned xbase, unsigned xcount, unsigned local,
                                                  unsigned nworkers, bool wide) {
  if (wide) {
    const unsigned npanels = (unsigned)((g.M + 255) / 256), ntn = (unsigned)(g.N / 192);
#ifdef CSN_BESIDE_WIDE_RR      // (ablation, timing only: the wide body on the narrow body's round-robin walk)
    beside_gemm_tiles_wide(g, smem, BesideWalk{xbase + local, npanels * ntn, nworkers});
#else
    beside_gemm_tiles_wide(g, smem, beside_xcd_tiles(npanels, ntn, xbase, xcount, local, nworkers));
#endif
  } else
    beside_gemm_tiles_narrow(g, smem, xbase + local, nworkers);
}

}  // namespace csn
