// Argument blocks of the multi-problem cell kernels (lstm_cell_blk.hip) and their launchers.
#pragma once
#include "csn_common.h"
#include "lstm_schedule.h"      // fwd_persist_slices, fwd_ns_slices, bwd_persist_slices

// Debug library (-DCSN_SLAB_TAGS, `make tags`): bit 2 of data_polls = fault injection "do not re-arm the ring slots", so
// that consumers ARE served stale occupants and the tag check can be seen to fire.  The product build has neither.
#ifdef CSN_SLAB_TAGS
#define CSN_DPOLL_MODE(x) ((x) & 3)
#define CSN_DPOLL_NO_REARM(x) (((x) & 4) != 0)
#else
#define CSN_DPOLL_MODE(x) (x)
#define CSN_DPOLL_NO_REARM(x) false
#endif

namespace csn {

struct CellFwdProb {
  const bf16_t* h_prev_blk;  // fragment-major [Bpad, H] or null (zero state)
  const bf16_t* w_blk;       // fragment-major W_hh, interleaved rows [4H, H]
  const float* xproj;        // [B, 4H] interleaved columns (x W_ih^T + b), row stride 4H
  const float* c_prev;       // [B, H] or null
  bf16_t* gates_out;         // [B, 4H] interleaved, or null
  float* c_out;              // [B, H]
  bf16_t* h_out;             // [B, H] row-major
  bf16_t* h_out_blk;         // fragment-major [Bpad, H]
};
struct CellFwdArgs {
  CellFwdProb p[4];
  int B, H;
};

struct CellBwdProb {
  const bf16_t* dg_next_blk;  // fragment-major [Bpad, 4H'] or null
  const bf16_t* wt_blk;       // fragment-major W_hh^T [H, 4H'] (k interleaved)
  const float* dy;            // [B, H] (row stride dy_ld) or null
  int64_t dy_ld;
  const bf16_t* gates;        // [B, 4H] interleaved
  const float* c;             // [B, H]
  const float* c_prev;        // [B, H] or null
  float* dc_carry;            // [B, H] in/out
  bf16_t* dg_out;             // [B, 4H] interleaved, row-major
  bf16_t* dg_out_blk;         // fragment-major [Bpad, 4H']
};
struct CellBwdArgs {
  CellBwdProb p[4];
  int B, H;
};

// weight-stationary forward (lstm_fwd_persist.hip): ONE launch advances up to 4 layers, each through its
// own chunk of timesteps (a wavefront diagonal over chunks).
struct PersistFwdSlot {
  const bf16_t* w_blk;     // fragment-major W_hh, interleaved rows [4H, H]
  const float* xproj;      // [T, B, 4H] interleaved
  bf16_t* gates;           // [T, B, 4H] interleaved, or null
  float* c_all;            // [T+1, B, H]  (slot t+1 = c_t)
  bf16_t* h_all;           // [T+1, B, H]  row-major
  bf16_t* h_blk_all;       // [T+1][Bpad * H] fragment-major slabs (slot t+1 = h_t); never reused in a forward
  unsigned* flags;         // [T+1][MT][kPersistFlagLine]: word i of line (t, mt) != 0 once slice i has published h_{t-1}; zeroed per forward
  // fused input projection (layer 0, I % 32 == 0, I <= 128): xproj is ignored, the workgroup keeps its W_ih rows
  // in registers too and multiplies x_t itself
  const bf16_t* x_blk;     // [T][Bpad * I] fragment-major slabs of the input, or null
  const bf16_t* wih_blk;   // fragment-major W_ih, interleaved rows [4H, I]
  const float* bias;       // [4H] interleaved b_ih + b_hh
  int I;
  int t0, nsteps;
};
// C[M,N] (f32) = A[M,K] * Bt[N,K]^T, bf16 operands, row-major: run by the workgroups of a weight-stationary backward
// launch that have no recurrence work (gemm_beside.h)
struct BesideGemm {
  const bf16_t* A;
  const bf16_t* Bt;
  float* C;
  int M, N, K;
};
static constexpr int kPersistFlagLine = 32;    // one 128-byte line per (slot, M-tile): at most 32 slices
struct PersistFwdArgs {
  PersistFwdSlot slot[4];
  int nslots;
  int data_polls;          // K-split kernel: hand-off by sentinel data in a ring of 4 slabs (no flags, no store drain); the host fills the 4 slabs with 0xff per forward
  // xcd_groups != 0: 1-D grid of 8 * nslices workgroups; the workgroups that share (blockIdx.x % 8) form one
  // hand-off group (a slot's M-tile) -- under the round-robin dispatch they share an XCD, which each group
  // verifies at run time through agree[group] (zeroed, one set of 8 words per launch) before it uses the
  // L2-local hand-off.  xcd_groups == 0: groups are contiguous block ranges, placement-independent hand-off.
  int xcd_groups;
  int rotate;              // != 0: each workgroup walks the k-blocks from its own offset (changes the summation order)
  unsigned long long* agree;
  unsigned* error_flag;    // sticky: a bounded spin gave up
  int B, H, T, Bpad, MT;
  // != 0: an initial state (CSN_LSTM_STATE): step 0 multiplies h_{-1} = h0 from hand-off slot 0 (written by an earlier
  // kernel on the stream: read without a wait) and starts from c_all slot 0; 0: step 0 has no recurrent term, c = 0
  int state;
  // != 0: hand-off groups of 32 rows (MT = Bpad / 32) instead of 64; K-split kernel, grouped form only.  A workgroup
  // writes and re-arms exactly the (row, unit) pieces it owns at either height, so launches of both heights follow each
  // other on the same ring of slabs; the flag lines of the two heights are separate (slot.flags is the height's own)
  int half_tiles;
  // != 0 (K-split kernel, H = 768 with data polls; elsewhere ignored): two k-block groups of h in flight and the waiting
  // register set parked in LDS; 0 (CSN_NO_FWD_PARK): a ring of 4, everything in registers.  Bit-identical results
  int park;
};
// float4 slots per accumulator tile in the forward's reduction buffer: 64 + padding.  The epilogue's lanes walk (row, unit
// quad j) with j fastest and read slot (tile j, row): with 65 a lane's 16-byte bank group is (j + row) mod 16 -- three lanes
// of a 16-lane group on one group; with 71 it is (7 j + row) mod 16, distinct except for one rare pair.
static constexpr int kRedTile = 71;
static constexpr int kParkSlots = 6;     // float4 slots per thread of the parked form's region
// dynamic LDS request of lstm_fwd_persist_kernel<NQ, ...> in bytes, at either tile height: [4 waves][4 NQ tiles][kRedTile]
// partial sums, [NQ][4] bias, and in the parked form [kParkSlots][256 threads].  More than half of a CU's 160 KB on
// purpose: a workgroup stays alone on its CU
constexpr size_t fwd_persist_lds_bytes(int nq, bool park) {
  return (size_t)(4 * 4 * nq * kRedTile + 4 * nq + (park ? kParkSlots * 256 : 0)) * 16;
}
bool fwd_persist_supported(int B, int H, int dtype, const Options& opt);
// N-split weight-stationary forward (lstm_fwd_ns.hip): the default where it applies
bool fwd_ns_supported(int B, int H, int dtype, const Options& opt);
int launch_fwd_ns(const PersistFwdArgs& a, hipStream_t st);
int launch_fwd_persist(const PersistFwdArgs& a, hipStream_t st);

// weight-stationary backward recurrence (lstm_bwd_persist.hip): ONE launch walks up to 4 layers, each backwards
// through its own chunk of timesteps; grouping / hand-off as in PersistFwdArgs.
struct PersistBwdSlot {
  const bf16_t* wt_blk;    // fragment-major W_hh^T [H, 4H'] (k interleaved)
  const bf16_t* gates;     // [T, B, 4H] interleaved (saved by the forward)
  const float* c_all;      // [T+1, B, H]  (slot t+1 = c_t)
  const float* dy;         // [T, B, H] gradient w.r.t. this layer's output, or null
  const float* dy_last;    // [B, H] added at t = T-1 when dy is null, or null
  const float* zeros;      // [B, H] of zeros: what a step reads when it has no incoming gradient
  float* dc_carry;         // [B, H] carried dc, in/out across launches
  bf16_t* dgates;          // [T, B, 4H] interleaved, row-major (GEMM operand)
  bf16_t* dg_blk_all;      // [T][Bpad * 4H] fragment-major slabs (slot t = dgates_t); never reused in a backward
  unsigned* flags;         // [T][MT][kPersistFlagLine], zeroed per backward (MT = tiles of the launch's height; the two heights use lines of their own)
  int t_hi, nsteps;        // steps t_hi, t_hi - 1, ..., t_hi - nsteps + 1 (of a merged launch: those of its first round)
  // merged launches (PersistBwdArgs::nrounds > 1), indices into PersistBwdArgs::cnt or -1: in round r the layer's
  // workgroups add to word cnt_pub + r when they leave the round's chunk (rec_done of that chunk; -1: layer 0, nobody
  // multiplies its dgates inside the launch) and, from round 1 on, enter the chunk only once word cnt_wait + r has
  // counted every worker (gemm_done of the layer above at that chunk; -1: the top layer, its dy is the caller's)
  int cnt_pub, cnt_wait;
};
struct PersistBwdArgs {
  PersistBwdSlot slot[4];
  int nslots;
  BesideGemm gemm[3];      // input-gradient GEMMs of the chunks the layers above finished one launch ago
  int ngemm;
  int beside_narrow;       // != 0 (CSN_BESIDE_128): the GEMMs take 256 x 128 tiles at every width (gemm_beside.h); same bits
  int gemm_wide;           // bit i: gemm[i] takes 256 x 192 tiles; set by launch_bwd_persist from the launch's geometry
  int grid_slices;         // xcd_groups: the grid is 8 * grid_slices workgroups (>= slices per group)
  int xcd_groups;
  int rotate;              // != 0: each workgroup walks the k-blocks from its own offset (changes the summation order)
  int data_polls;          // hand-off by sentinel data in a ring of 4 slabs (the host fills them with 0xff per backward)
  unsigned long long* agree;
  unsigned* error_flag;
  int B, H, T, Bpad, MT;   // MT: M-tiles per layer at the launch's tile height
  int half_tiles;          // != 0: hand-off groups of 32 rows (MT = Bpad / 32), else 64 (MT = Bpad / 64); grouped form only
  // Merged launch: nrounds consecutive chunk diagonals in one launch (1: a launch of one diagonal, as ever; > 1 only in
  // the grouped form with data polls, every layer in range in every round and ngemm = nslots - 1 GEMMs of M = chunk * B
  // rows).  Round r is diagonal first + r: a slot's chunk lies `chunk` steps below that of round r - 1 (only the last
  // round's may be short), gemm[i] is the host's gemm[i] moved down r chunks (slot i's chunk of round r - 1, its output
  // the dy of slot i + 1 in round r + 1), and the two kernel boundaries that a GEMM stands between are the counters
  // cnt[] (zeroed per backward): see PersistBwdSlot::cnt_pub / cnt_wait.
  int nrounds, chunk;
  unsigned* cnt;
  // the same words as the GEMM workers index them (slot i is layer nslots - 1 - i, two chunks behind slot i - 1): GEMM i
  // of round r waits on word wk_wait + r - i * wk_stride and adds to word wk_pub + r - i * wk_stride
  int wk_wait, wk_pub, wk_stride;
};
static_assert(sizeof(PersistBwdArgs) <= 4096, "PersistBwdArgs is passed by value: the kernel-argument segment holds 4096 bytes");
bool bwd_persist_supported(int B, int H, int dtype, const Options& opt);
// lengths != NULL (variable-length batches): [B] device array; the masked instantiation of the kernel
int launch_bwd_persist(const PersistBwdArgs& a, hipStream_t st, const int* lengths = nullptr);

// one launch for all layout-preparation jobs of a forward (lstm_cell_blk.hip: prep_multi_kernel)
enum { kPrepBlockify = 0, kPrepPermRows, kPrepTransPerm, kPrepBias, kPrepCastX, kPrepBlockifyX };
static constexpr int kPrepMaxJobs = 32;
struct PrepJob {
  int kind;
  const float* a;
  const float* b;
  void* dst;
  int64_t n0, n1, n2, s0, s1, H;     // meaning per kind (see the kernel)
  int perm_r, perm_k;
  int64_t work;                      // work items (threads) of the job
  unsigned blk_begin, blk_count;     // filled by the launcher
  const int* len;                    // x jobs of reverse plans (perm_r != 0) and of calls with input windows: [B] valid steps per row, null = n1 for all
};
// vrow / vt0: the input windows of the call (csn_lstm_plan_set_views), [B] device arrays or null; they belong to the x
// jobs and sit here ONCE (a call has one x): a pointer pair per job would put the struct past the 4096 bytes a kernel's
// by-value arguments may take
struct PrepArgs {
  PrepJob job[kPrepMaxJobs];
  int njobs;
  const int* vrow;
  const int* vt0;
};
static_assert(sizeof(PrepArgs) <= 4096, "PrepArgs is passed by value: the kernel-argument segment holds 4096 bytes");
int launch_prep_multi(PrepArgs& A, hipStream_t st);

bool cell_blk_supported(int H, int dtype, const Options& opt);
int launch_cell_fwd_il(const CellFwdArgs& a, int nprob, hipStream_t st);
int launch_cell_bwd_il(const CellBwdArgs& a, int nprob, hipStream_t st, const CellMask* mask = nullptr);
int launch_blockify_x(const float* x, int64_t xsb, int64_t xst, int B, int T, int I, void* dst, hipStream_t st);
int launch_blockify(const float* src, int64_t ld_r, int64_t ld_k, int64_t R, int64_t K, int perm_r, int perm_k,
                    int64_t H, void* dst, hipStream_t st);
int launch_permute_rows_cast(const float* src, int64_t H, int64_t I, void* dst, hipStream_t st);
int launch_transpose_perm_cast(const float* src, int64_t H, int64_t I, void* dst, hipStream_t st);
int launch_bias_perm_sum(const float* a, const float* b, int64_t H, float* dst, hipStream_t st);
int launch_reduce_slabs_unperm(const float* slabs, int64_t slab_stride, int S, int64_t H, int64_t C, float* out,
                               float* out2, int accumulate, hipStream_t st);

}  // namespace csn
