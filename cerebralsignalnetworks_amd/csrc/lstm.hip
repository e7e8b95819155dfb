// K3 orchestration: stacked LSTM forward / backward over the whole sequence.
// Replaces nn.LSTM(batch_first=True).forward / autograd backward as called at
// /root/reference/LSTMDistill.py:118,132 and /root/reference/LSTMDistillRetreival.py:91,103.
//
// Six paths share the C entry points (csn_lstm_plan_path; make_layout decides at plan creation):
//
//  0  generic (forward_v1 / backward_v1): float32, or bf16 shapes the fast paths do not cover; cell kernels of
//     lstm_cell.hip, the layers as a wavefront of one launch per diagonal, lag = 1 chunk, everything on the caller's stream.
//  1  per-diagonal fast path (forward_il / backward_il; bf16, H % 128 == 0): lstm_cell_blk.hip kernels.  The layers
//     advance as a WAVEFRONT: one launch per diagonal runs layer 0 at step d, layer 1 at step d - lag, ...
//     (lag = 2 chunks), so a launch boundary (~2 us) and the launch ramp are paid once per
//     diagonal, not once per layer-step, and a 2-layer diagonal is exactly one workgroup per CU.
//     The non-recurrent contractions are big GEMMs on a second, plan-owned HIP stream:
//       forward : xproj_{l+1}[chunk] = h_l[chunk] W_ih^T + b   as soon as layer l finished a chunk;
//       backward: dx_l[chunk] = dgates_l[chunk] W_ih (input gradient of layer l = dy of layer l-1),
//                 then dW_hh, dW_ih, db of layer l once its recurrence is done
//     and HIP events order the two streams, so the MFMA-bound GEMMs run beside the
//     latency/bandwidth-bound recurrence of the other layer instead of after it.
//  2  weight-stationary forward (forward_persist: lstm_fwd_persist.hip or lstm_fwd_ns.hip, one launch per chunk
//     diagonal, or per layer and chunk on streams of their own), backward of path 1.
//  3  path 2 with the weight-stationary backward (backward_persist: lstm_bwd_persist.hip, one launch per chunk diagonal,
//     the input-gradient GEMM inside the next launch; the diagonals with every layer in range merged into one launch)
//     where its grouped form applies (bwd_grouped), else backward_il.
//  4  exact float32, weight-stationary (forward_f32p / backward_f32p: lstm_f32_persist.hip), layer after layer.
//  5  CU-resident recurrence (forward_resident / backward_resident: lstm_resident.hip), opt-in with CSN_LSTM_RESIDENT,
//     H <= 128, both dtypes: path 0's workspace and host flow with the step loop of a chunk inside the kernel -- one
//     launch per CHUNK diagonal, everything on the caller's stream, every result bit for bit that of path 0.
//
// Each path is one function over the per-call context (struct Call) and the caller's pointers (FwdArgs / BwdArgs); what
// more than one of them does -- slot 0, weight gradients, chunk GEMMs, dx out, the profile epilogue -- is one helper each.
// The layer wavefronts of paths 0, 1 and 5 are ONE schedule (wavefront_schedule, lstm_schedule.h: unit, lag, direction).
// The API boundary -- the caller's batch-first float32 tensors into the time-major workspace and back, whatever the plan's
// lengths, direction, pitches or output dropout -- is a file of its own (lstm_boundary.hip: one kernel per layout pass); this
// file launches none of it, and csn_lstm_forward / csn_lstm_backward are one flow each around run_forward / run_backward.
//
// Layout in HBM (inside the caller's workspace; [T,B,*] time-major so one timestep is one slab):
//   per layer: compute-dtype weight copies (+ transposes / fragment-major forms), bias,
//              xproj[T,B,4H] f32, gates[T,B,4H], c_all[T+1,B,H] f32, h_all[T+1,B,H],
//              dgates[T,B,4H], dx[T,B,I_l] f32; the fast paths add the fragment-major ping-pong / ring
//              buffers of h and dgates.  In paths 1 - 3 every 4H axis is gate-interleaved
//              (n' = 4 unit + gate); parameters and their gradients are (un)permuted at the API.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "csn_common.h"
#include "lstm_cell_blk.h"
#include "lstm_boundary.h"
#include "lstm_cell_common.h"
#include "lstm_dropout.h"
#include "lstm_f32_persist.h"
#include "lstm_handoff.h"
#include "lstm_resident.h"
#include "lstm_schedule.h"

namespace csn {

struct LayerWs {
  size_t wih, whh, whht, wiht, whh_blk, whht_blk, bias, xproj, gates, c_all, h_all, dgates, dx, dc_carry, hblk[2],
      dgblk[2], h_blk_all, counters, dg_blk_all, bflags;
  size_t h_drop;           // CSN_LSTM_DROPOUT plans, layers below the top: [T,B,H] compute dtype, what layer l + 1 reads in place of h_all
};
struct WsLayout {
  LayerWs layer[8];
  size_t x_c, x_blk, wih0_blk, dy_tm, tn_scratch, colsum, status, agree, agree_b, merge_cnt, zeros_bh, f32_bias_part, total;
  // weight-stationary paths: everything that must be zero at the start of a forward / a backward sits in ONE block each
  size_t zero_fwd, zero_fwd_bytes, zero_bwd, zero_bwd_bytes;
  bool fuse_x;
  bool il, persist, persist_bwd;
  bool fwd_ns;             // forward runs the N-split kernel (lstm_fwd_ns.hip), else the K-split one
  bool f32_persist;        // exact-float32 path: weight-stationary recurrence (lstm_f32_persist.hip), one launch per layer and row block
};

static bool whole_chip() {       // (asked when a layout is made -- plan creation --, not per launch)
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  return hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus >= 256;
}

static WsLayout make_layout(const csnLstmDesc& d, int training, bool dropout, const Options& opt) {
  WsLayout w{};
  w.il = cell_blk_supported(d.H, d.dtype, opt);
  // (the K-split weight-stationary kernels address their per-step hand-off slabs with 32-bit byte offsets from step 0: a
  // sequence whose slabs reach 4 GiB takes the per-diagonal launches; the N-split kernel bases its resources per launch)
  const bool slabs_fit = ((size_t)d.T + 1) * (((size_t)d.B + 63) / 64 * 64) * (size_t)d.H * 8 < ((size_t)1 << 32);
  w.fwd_ns = w.il && fwd_ns_supported(d.B, d.H, d.dtype, opt) && d.L <= 4;
  w.persist = w.fwd_ns || (w.il && slabs_fit && fwd_persist_supported(d.B, d.H, d.dtype, opt) && d.L <= 4);
  w.persist_bwd = w.persist && slabs_fit && training && bwd_persist_supported(d.B, d.H, d.dtype, opt);
  size_t off = 0;
  const size_t es = dtype_size(d.dtype);
  auto take = [&](size_t bytes) {
    size_t o = off;
    off += align_up(bytes, 256);
    return o;
  };
  const size_t TB = (size_t)d.T * d.B, H = d.H, G = 4 * (size_t)d.H;
  const size_t Bpad = ((size_t)d.B + 63) / 64 * 64;
  size_t tn_bytes = 0;
  for (int l = 0; l < d.L; ++l) {
    const size_t I = l == 0 ? d.I : d.H;
    LayerWs& L = w.layer[l];
    L.wih = take(G * I * es);
    L.wiht = take(G * I * es);
    L.bias = take(G * 4);
    if (w.il) {
      L.whh_blk = take(G * H * 2);
      L.whht_blk = take(G * H * 2);
      L.hblk[0] = take(Bpad * H * 2);
      L.hblk[1] = take(Bpad * H * 2);
      if (w.persist) L.h_blk_all = take(((size_t)(d.T < 3 ? 3 : d.T) + 1) * Bpad * H * 2);   // (>= 4: the data-poll hand-off uses the first 4 as a ring)
    } else {
      L.whh = take(G * H * es);
      L.whht = take(G * H * es);
    }
    L.xproj = take(TB * G * 4);
    L.gates = take(TB * G * es);
    L.c_all = take((TB + d.B) * H * 4);
    L.h_all = take((TB + d.B) * H * es);
    if (training) {
      L.dgates = take(TB * G * es);
      L.dx = take(TB * I * 4);
      if (!w.persist_bwd) L.dc_carry = take((size_t)d.B * H * 4);
      if (w.il) {
        L.dgblk[0] = take(Bpad * G * 2);
        L.dgblk[1] = take(Bpad * G * 2);
      }
      if (w.persist_bwd) L.dg_blk_all = take((size_t)(d.T < 4 ? 4 : d.T) * Bpad * G * 2);   // (>= 4: ring of the data-poll hand-off)
    }
    size_t a = gemm_tn_scratch_bytes(G, I, TB, opt), b = gemm_tn_scratch_bytes(G, H, TB, opt);
    if (a > tn_bytes) tn_bytes = a;
    if (b > tn_bytes) tn_bytes = b;
  }
  w.x_c = take(TB * d.I * es);
  w.status = take(kStatusBytes);
  // (H = 512 excluded: its 64 x 32-unit tile leaves no registers for the W_ih fragments.  N-split kernel at H = 1024: W_hh
  // fills the 256 AGPRs, W_ih's 32 registers are VGPR operands of their MFMAs -- round 3's fused instantiation asked for
  // AGPRs there too and the compiler's copies ran into an MFMA read hazard the recogniser cannot see inside inline asm
  // (wrong row group 0; tools/check_asm_hazards.py).  CSN_NO_FUSE_X keeps the projection GEMM.)
  w.fuse_x = w.persist && !opt.no_fuse_x &&
             (w.fwd_ns ? d.I == 128 : (d.I % 32 == 0 && d.I <= 128 && d.H != 512));
  if (w.fuse_x) {
    w.x_blk = take((size_t)d.T * Bpad * d.I * 2);
    w.wih0_blk = take(G * d.I * 2);
  }
  if (w.persist_bwd) w.zeros_bh = take((size_t)d.B * H * 4);
  // exact-float32 path, weight-stationary: needs a whole MI355X like the bf16 kernels (all workgroups of a launch co-resident)
  w.f32_persist = !w.il && d.dtype == CSN_F32 && !opt.no_persist && !opt.cell_v1 && f32_persist_supported(d.B, d.H) && whole_chip();
  if (w.f32_persist) {
    const size_t MTt = Bpad / 64;
    w.zero_fwd = off;
    for (int l = 0; l < d.L; ++l) w.layer[l].counters = take(((size_t)d.T + 1) * MTt * kF32FlagLine * 4);
    w.zero_fwd_bytes = off - w.zero_fwd;
    for (int l = 0; l < d.L; ++l) w.layer[l].h_blk_all = take(((size_t)d.T + 1) * Bpad * H * 4);       // fragment-major hand-off copies
    if (training) {
      for (int l = 0; l < d.L; ++l) w.layer[l].dg_blk_all = take((size_t)d.T * Bpad * G * 4);
      w.zeros_bh = take((size_t)d.B * H * 4);
      w.f32_bias_part = take(MTt * 4 * G * 4);      // per-row-group bias-gradient partial sums of ONE layer (consumed before the next launch)
      w.zero_bwd = off;
      for (int l = 0; l < d.L; ++l) w.layer[l].bflags = take((size_t)d.T * MTt * kF32FlagLine * 4);
      w.zero_bwd_bytes = off - w.zero_bwd;
    }
  }
  if (w.persist) {
    w.zero_fwd = off;
    // (x 4: room for four flag lines per (slot, M-tile): the first holds the lines of the 64-row tiles, the next two
    // those of the 32-row tiles of launches with few groups, twice as many; the last is unused)
    for (int l = 0; l < d.L; ++l) w.layer[l].counters = take(((size_t)d.T + 1) * (Bpad / 64) * 4 * kPersistFlagLine * 4);
    w.agree = take(((size_t)d.T + 8) * 8 * sizeof(unsigned long long));   // 8 words per launch
    w.zero_fwd_bytes = off - w.zero_fwd;
  }
  if (w.persist_bwd) {
    w.zero_bwd = off;
    for (int l = 0; l < d.L; ++l) {
      w.layer[l].dc_carry = take((size_t)d.B * H * 4);
      // (x 3: the lines of the 64-row tiles, then those of the 32-row tiles of launches with few groups -- twice as many)
      w.layer[l].bflags = take((size_t)d.T * (Bpad / 64) * 3 * kPersistFlagLine * 4);
    }
    w.agree_b = take(((size_t)d.T + 8) * 8 * sizeof(unsigned long long));
    // merged backward launches: rec_done[L][chunks] and gemm_done[L][chunks] (lstm_cell_blk.h), at most T chunks
    w.merge_cnt = take((2 * (size_t)d.L * d.T * sizeof(unsigned) + 15) / 16 * 16);
    w.zero_bwd_bytes = off - w.zero_bwd;
  }
  if (training) {
    w.dy_tm = take(TB * H * 4);
    w.tn_scratch = take(tn_bytes);
    w.colsum = take(colsum_scratch_bytes(G));
  }
  // (behind everything else: a plan without the bit is laid out as it always was)
  for (int l = 0; dropout && l + 1 < d.L; ++l) w.layer[l].h_drop = take(TB * H * es);
  w.total = off;
  return w;
}

// the bits of `training` that are not "training"
static const int kPlanBits = CSN_LSTM_STATE | CSN_LSTM_DROPOUT | CSN_LSTM_REVERSE | CSN_LSTM_RESIDENT;

// CSN_LSTM_RESIDENT: a whole layer's W_hh has to fit the registers of one workgroup
static int check_resident(const char* fn, const csnLstmDesc* d, int training) {
  if ((training & CSN_LSTM_RESIDENT) && !resident_supported(d->H))
    return fail(CSN_ERR_UNSUPPORTED, "%s: CSN_LSTM_RESIDENT takes H <= %d, not H=%d", fn, kResidentMaxH, d->H);
  return CSN_OK;
}
// ... and the plan is laid out as path 0 lays it out (il = persist = f32_persist = false)
static void resident_options(Options& opt) {
  opt.cell_v1 = true;
  opt.no_persist = true;
}

static int check_desc(const char* fn, const csnLstmDesc* d) {
  CSN_REQUIRE(d != nullptr, "%s: null descriptor", fn);
  CSN_REQUIRE(d->B > 0 && d->T > 0 && d->I > 0 && d->H > 0, "%s: bad shape B=%d T=%d I=%d H=%d", fn, d->B, d->T,
              d->I, d->H);
  CSN_REQUIRE(d->L >= 1 && d->L <= 8, "%s: L=%d outside 1..8", fn, d->L);
  CSN_REQUIRE(d->H % 32 == 0, "%s: H=%d must be a multiple of 32", fn, d->H);
  CSN_REQUIRE(d->dtype == CSN_F32 || d->dtype == CSN_BF16, "%s: bad dtype %d", fn, d->dtype);
  return CSN_OK;
}

// Gradient w.r.t. the initial hidden state of one layer (CSN_LSTM_STATE plans):
//   out[b][j] = sum_k dg[b][k] Wt(j, k),  k in [0, 4H), dg = dgates at t = 0 [B, 4H] row-major,
//   Wt = W_hh^T [H, 4H]: row-major (BLK = false, generic path) or fragment-major (BLK = true, per-diagonal path, 4H axis
//   gate-interleaved like dg).  The operands the recurrence multiplies (bf16 or float32), float32 accumulate in a fixed
//   k order.  Tile 32 rows x 64 units per workgroup, k in blocks of 32 through LDS.
template <typename T, bool BLK>
__global__ void __launch_bounds__(256) lstm_dh0_kernel(const T* __restrict__ dg, const T* __restrict__ wt, int B, int H,
                                                       float* __restrict__ out) {
  __shared__ float As[32][33];
  __shared__ float Ws[32][65];
  const int64_t G = 4 * (int64_t)H;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int b0 = blockIdx.y * 32, j0 = blockIdx.x * 64;
  float acc[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  for (int64_t k0 = 0; k0 < G; k0 += 32) {
    for (int i = threadIdx.x; i < 32 * 32; i += 256) {
      const int r = i >> 5, k = i & 31;
      As[r][k] = b0 + r < B ? to_f32(dg[(int64_t)(b0 + r) * G + k0 + k]) : 0.f;
    }
    for (int i = threadIdx.x; i < 64 * 32; i += 256) {
      const int j = i >> 5, k = i & 31;
      float v = 0.f;
      if (j0 + j < H) v = to_f32(wt[BLK ? blk_offset(j0 + j, k0 + k, G) : (int64_t)(j0 + j) * G + k0 + k]);
      Ws[k][j] = v;
    }
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < 32; ++k) {
      const float a0 = As[ty][k], a1 = As[ty + 16][k];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float wv = Ws[k][tx + 16 * c];
        acc[0][c] = fmaf(a0, wv, acc[0][c]);
        acc[1][c] = fmaf(a1, wv, acc[1][c]);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int b = b0 + ty + 16 * r, j = j0 + tx + 16 * c;
      if (b < B && j < H) out[(int64_t)b * H + j] = acc[r][c];
    }
}

// out[n] = part[0][n] + part[1][n] + ... (fixed order): the row groups' bias-gradient partial sums of the float32 backward;
// accumulate: each destination's own previous contents join last
__global__ void sum_rows_kernel(const float* __restrict__ part, int P, int64_t n, float* out, float* out2, int accumulate) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  for (int p = 0; p < P; ++p) s += part[(int64_t)p * n + i];
  out[i] = accumulate ? out[i] + s : s;
  out2[i] = accumulate ? out2[i] + s : s;
}

// ---- second stream + event pool: owned by the PLAN (created on first use, destroyed with it) -------
struct SideCtx {
  hipStream_t side = nullptr;           // GEMMs
  hipStream_t layer[8] = {nullptr};     // weight-stationary forward: one stream per layer >= 1
  std::vector<hipEvent_t> events;
  size_t next = 0;
};

static int side_ctx(SideCtx& c) {
  if (c.side == nullptr) {
    CSN_HIP_CHECK(hipStreamCreateWithFlags(&c.side, hipStreamNonBlocking));
    for (int l = 1; l < 8; ++l) CSN_HIP_CHECK(hipStreamCreateWithFlags(&c.layer[l], hipStreamNonBlocking));
  }
  c.next = 0;
  return CSN_OK;
}
static int next_event(SideCtx* c, hipEvent_t* ev) {
  if (c->next == c->events.size()) {
    hipEvent_t e;
    CSN_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    c->events.push_back(e);
  }
  *ev = c->events[c->next++];
  return CSN_OK;
}
// record on `from`, make `to` wait
static int hand_off(SideCtx* c, hipStream_t from, hipStream_t to) {
  hipEvent_t ev;
  if (int rc = next_event(c, &ev)) return rc;
  CSN_HIP_CHECK(hipEventRecord(ev, from));
  CSN_HIP_CHECK(hipStreamWaitEvent(to, ev, 0));
  return CSN_OK;
}

// ---- optional event timing of the recurrence window ----------------------------------------
struct Prof {
  bool on = false;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // fwd begin/end, bwd begin/end
  int launches[2] = {0, 0}, cells[2] = {0, 0};
  bool have[2] = {false, false};
  // grouped weight-stationary paths: the recurrence launches alternate with GEMMs on the same stream, so each
  // launch is bracketed by its own event pair and the reported time is the sum over the pairs
  std::vector<hipEvent_t> pair[2];
  size_t pairs_used[2] = {0, 0};
};
static int prof_mark(Prof& g_prof, int which, hipStream_t st) {
  if (!g_prof.on) return CSN_OK;
  if ((which & 1) == 0) g_prof.pairs_used[which >> 1] = 0;
  if (g_prof.ev[which] == nullptr) CSN_HIP_CHECK(hipEventCreate(&g_prof.ev[which]));
  CSN_HIP_CHECK(hipEventRecord(g_prof.ev[which], st));
  return CSN_OK;
}

static int prof_pair(Prof& g_prof, int k, bool end, hipStream_t st) {   // k: 0 forward, 1 backward
  if (!g_prof.on) return CSN_OK;
  const size_t i = 2 * g_prof.pairs_used[k] + (end ? 1 : 0);
  while (g_prof.pair[k].size() <= i) {
    hipEvent_t e;
    CSN_HIP_CHECK(hipEventCreate(&e));
    g_prof.pair[k].push_back(e);
  }
  CSN_HIP_CHECK(hipEventRecord(g_prof.pair[k][i], st));
  if (end) ++g_prof.pairs_used[k];
  return CSN_OK;
}

}  // namespace csn

// The plan: shapes, the switches read once at creation, the workspace layout, and every piece of host-side
// state a forward / backward needs (side streams, event pool, profiling events).  Nothing of it is global, so
// plans are independent: one per (stream, thread, device) as the caller likes.  A plan is not itself
// thread-safe -- do not call the same plan from two threads at once.
struct csnLstmPlan {
  csnLstmDesc d;
  int training;
  int dropout = 0;            // created with CSN_LSTM_DROPOUT: the workspace holds h_drop, csn_lstm_plan_set_dropout takes p > 0
  float drop_p = 0.f;         // csn_lstm_plan_set_dropout (sticky): 0 = off
  uint64_t drop_seed = 0;
  uint32_t drop_subsequence = 0;
  int state;                  // created with CSN_LSTM_STATE: accepts (h0, c0) / (h_n, c_n) and their gradients
  bool state_seen = false;    // a forward with a state has run: stateless forwards re-zero slot 0 (weight-stationary paths)
  int device;
  csn::Options opt;
  csn::WsLayout w;
  csn::SideCtx sc;
  csn::Prof prof;
  int dgates_copies = 0;      // what the last backward wrote per step (csn_lstm_plan_dgates_copies)
  int bwd_launches[2] = {0, 0};    // last backward: recurrence launches, diagonals the merged one covered (csn_lstm_plan_bwd_launches)
  int half_launches[2] = {0, 0};   // recurrence launches of the last forward / backward on 32-row groups (csn_lstm_plan_half_tile_launches)
  csnGradReadyFn grad_cb = nullptr;      // csn_lstm_plan_set_grad_callback
  void* grad_cb_user = nullptr;
  int grad_accumulate = 0;               // csn_lstm_plan_set_grad_mode: dw / db are added to, not overwritten
  int reverse = 0;                       // created with CSN_LSTM_REVERSE: the layout passes walk every row backwards in time
  int resident = 0;                      // created with CSN_LSTM_RESIDENT: path 0's layout, the recurrence of lstm_resident.hip
  int64_t y_pitch = 0, dy_pitch = 0;     // csn_lstm_plan_set_io: elements per (b, t) row of y_all / dy_all, 0 = dense (H)
  int dx_add = 0;                        // csn_lstm_plan_set_io: dx is added to over the valid steps, not overwritten
  int readout = CSN_READOUT_LAST;        // csn_lstm_plan_set_readout: what y_last is, and where dy_last enters
  int32_t* argmax_dev = nullptr;         // [B, H] int32 owned by the plan: the MAX backward's argmax, written and read in stream order
  // csn_lstm_plan_set_attention (sticky; q = null = off): the learned-query readout in place of the mode above.  attn_dev:
  // the [B, T] arrays and the dq partials of one call (AttnArgs), owned by the plan, allocated on first use, written and
  // read in stream order inside the one call like argmax_dev
  const float* attn_q = nullptr;
  float attn_scale = 0.f;
  float *attn_dq = nullptr, *attn_out = nullptr, *attn_dscore = nullptr;
  char* attn_dev = nullptr;
  // csn_lstm_plan_set_output_dropout (sticky; p = 0 = off): the mask the layout passes apply to y_all as they store it and
  // to dy_all as they load it, indexed on the caller's tensor
  float out_drop_p = 0.f;
  uint64_t out_drop_seed = 0, out_drop_first = 0;
  uint32_t out_drop_subsequence = 0;
  int64_t out_drop_pitch = 0;
  csn::OutDropCfg out_drop() const {
    return csn::OutDropCfg{csn::dropout_cfg(out_drop_p, out_drop_seed, out_drop_subsequence), out_drop_first, out_drop_pitch};
  }
  // csn_lstm_plan_set_lengths (empty = every row is T): the lengths of the next calls and the longest of them.  What a
  // call in progress derives from them lives in its Call, not here.  (len_dev: [B] int32 owned by the plan -- a state
  // plan's workspace is laid out exactly as a plain plan's)
  std::vector<int32_t> lengths;
  int t_eff = 0;
  int32_t* len_dev = nullptr;
  int32_t* len_pin = nullptr;            // pinned staging of the upload, and the event behind its last copy
  hipEvent_t len_ev = nullptr;
  // csn_lstm_plan_set_views (empty = off): per row the source row and the first source step of its input window, and
  // the source's extents.  view_dev / view_pin: [2 B] int32 (rows, then starts), uploaded by every forward like the lengths
  std::vector<int32_t> view_row, view_t0;
  int view_src_rows = 0, view_src_T = 0;
  int32_t* view_dev = nullptr;
  int32_t* view_pin = nullptr;
  hipEvent_t view_ev = nullptr;
  void grads_ready(int layer) const {
    if (grad_cb != nullptr) grad_cb(grad_cb_user, layer);
  }
};

using namespace csn;
typedef csnLstmPlan Plan;

extern "C" int csn_lstm_plan_create(const csnLstmDesc* d, int training, csnLstmPlan** out) {
  if (int rc = check_desc("csn_lstm_plan_create", d)) return rc;
  CSN_REQUIRE(out != nullptr, "csn_lstm_plan_create: null output pointer");
  if (int rc = check_resident("csn_lstm_plan_create", d, training)) return rc;
  Plan* P = new Plan();
  P->d = *d;
  P->state = (training & CSN_LSTM_STATE) != 0;
  P->dropout = (training & CSN_LSTM_DROPOUT) != 0;
  P->reverse = (training & CSN_LSTM_REVERSE) != 0;
  P->resident = (training & CSN_LSTM_RESIDENT) != 0;
  P->training = (training & ~kPlanBits) != 0;
  if (hipGetDevice(&P->device) != hipSuccess) {
    delete P;
    return fail(CSN_ERR_HIP, "csn_lstm_plan_create: hipGetDevice failed");
  }
  P->opt = options_from_env();
  // (the exact-float32 weight-stationary path (4) takes no state: a float32 state plan runs the per-step cells)
  if (P->state && d->dtype == CSN_F32) P->opt.no_persist = true;
  if (P->resident) resident_options(P->opt);
  {
    // the weight-stationary kernels address the steps of ONE launch with 32-bit byte offsets from the launch's base
    // (lstm_fwd_ns.hip; launch_fwd_ns refuses more): a CSN_LSTM_CHUNK that large is clamped here, not left to wrap
    const unsigned long long Bp = ((unsigned long long)d->B + 63) / 64 * 64;
    const unsigned long long per_step = std::max({(unsigned long long)d->B * d->H * 16ull, Bp * (unsigned long long)d->I * 2ull, Bp * (unsigned long long)d->H * 2ull});
    const unsigned long long cmax = ((1ull << 32) - 1ull) / per_step;
    if (cmax >= 3 && (unsigned long long)P->opt.chunk > cmax - 2) P->opt.chunk = (int)(cmax - 2);
  }
  P->w = make_layout(*d, P->training, P->dropout != 0, P->opt);
  *out = P;
  return CSN_OK;
}

extern "C" void csn_lstm_plan_destroy(csnLstmPlan* P) {
  if (P == nullptr) return;
  int cur = 0;
  const bool switched = hipGetDevice(&cur) == hipSuccess && cur != P->device && hipSetDevice(P->device) == hipSuccess;
  for (hipEvent_t e : P->sc.events) (void)hipEventDestroy(e);
  if (P->sc.side) (void)hipStreamDestroy(P->sc.side);
  for (int l = 1; l < 8; ++l)
    if (P->sc.layer[l]) (void)hipStreamDestroy(P->sc.layer[l]);
  for (int i = 0; i < 4; ++i)
    if (P->prof.ev[i]) (void)hipEventDestroy(P->prof.ev[i]);
  for (int k = 0; k < 2; ++k)
    for (hipEvent_t e : P->prof.pair[k]) (void)hipEventDestroy(e);
  if (P->len_ev) (void)hipEventDestroy(P->len_ev);
  if (P->len_pin) (void)hipHostFree(P->len_pin);
  if (P->len_dev) (void)hipFree(P->len_dev);
  if (P->view_ev) (void)hipEventDestroy(P->view_ev);
  if (P->view_pin) (void)hipHostFree(P->view_pin);
  if (P->view_dev) (void)hipFree(P->view_dev);
  if (P->argmax_dev) (void)hipFree(P->argmax_dev);
  if (P->attn_dev) (void)hipFree(P->attn_dev);
  if (switched) (void)hipSetDevice(cur);
  delete P;
}

extern "C" size_t csn_lstm_plan_workspace_bytes(const csnLstmPlan* P) { return P ? P->w.total : 0; }

extern "C" int csn_lstm_plan_path(const csnLstmPlan* P) {
  if (P == nullptr) return -1;
  if (P->resident) return 5;
  return P->w.f32_persist ? 4 : (P->w.persist_bwd ? 3 : (P->w.persist ? 2 : (P->w.il ? 1 : 0)));
}

extern "C" int csn_lstm_plan_dgates_copies(const csnLstmPlan* P) { return P == nullptr ? -1 : P->dgates_copies; }

// Host-only diagnostic for the tests, exported beside the public header like csn_gemm_nt_w4_offsets_fit (cabi.py binds it
// on use): the weight-stationary recurrence launches of the plan's LAST backward (which = 0), and how many chunk
// diagonals the merged one of them covered (which = 1; 0 = none was merged: CSN_BWD_NO_MERGE=1, dropout, lengths, dh_n,
// flags in place of data polls, H = 1024, one layer, fewer than two diagonals with every layer in range).  0 / 0 before
// any backward and on the other paths; -1 for a null plan / other `which`.
extern "C" int csn_lstm_plan_bwd_launches(const csnLstmPlan* P, int which) {
  return (P == nullptr || which < 0 || which > 1) ? -1 : P->bwd_launches[which];
}
extern "C" int csn_lstm_plan_half_tile_launches(const csnLstmPlan* P, int which) {
  return (P == nullptr || which < 0 || which > 1) ? -1 : P->half_launches[which];
}

// does a backward of this plan over T steps take the grouped weight-stationary form?  (a call passes the steps it runs --
// with lengths the longest row --, csn_lstm_plan_kernel_name the plan's T)
static bool bwd_grouped(const csnLstmPlan* P, int T) {
  return csn::bwd_grouped(P->w.persist_bwd, P->d.B, P->d.L, T, P->opt.chunk, P->opt.persist_streams);
}

extern "C" const char* csn_lstm_plan_kernel_name(const csnLstmPlan* P, int which) {
  if (P == nullptr) return nullptr;
  const bool ks = (P->d.dtype == CSN_F32 ? P->d.H % 128 == 0 : P->d.H % 256 == 0);      // K-split cell kernels (lstm_cell.hip)
  if (P->resident) return which == 0 ? "lstm_resident_fwd_kernel" : (which == 1 ? "lstm_resident_bwd_kernel" : nullptr);
  if (P->w.f32_persist) return which == 0 ? "lstm_fwd_f32_persist_kernel" : (which == 1 ? "lstm_bwd_f32_persist_kernel" : nullptr);
  if (which == 0) {
    if (P->w.fwd_ns) return "lstm_fwd_ns_kernel";
    if (P->w.persist) return "lstm_fwd_persist_kernel";
    if (P->w.il) return "lstm_cell_fwd_il_kernel";
    return ks ? "lstm_cell_fwd_ks_kernel" : "lstm_cell_fwd_kernel";
  }
  if (which == 1) {
    if (bwd_grouped(P, P->d.T)) return "lstm_bwd_persist_kernel";
    if (P->w.il) return "lstm_cell_bwd_il_kernel";
    return ks ? "lstm_cell_bwd_ks_kernel" : "lstm_cell_bwd_kernel";
  }
  return nullptr;
}

extern "C" int csn_lstm_plan_set_grad_callback(csnLstmPlan* P, csnGradReadyFn fn, void* user) {
  CSN_REQUIRE(P != nullptr, "csn_lstm_plan_set_grad_callback: null plan");
  P->grad_cb = fn;
  P->grad_cb_user = fn ? user : nullptr;
  return CSN_OK;
}

extern "C" int csn_lstm_plan_set_grad_mode(csnLstmPlan* P, int mode) {
  CSN_REQUIRE(P != nullptr, "csn_lstm_plan_set_grad_mode: null plan");
  CSN_REQUIRE(mode == CSN_GRAD_OVERWRITE || mode == CSN_GRAD_ACCUMULATE, "csn_lstm_plan_set_grad_mode: unknown mode %d", mode);
  P->grad_accumulate = mode == CSN_GRAD_ACCUMULATE;
  return CSN_OK;
}

extern "C" int csn_lstm_plan_set_lengths(csnLstmPlan* P, const int32_t* lengths) {
  CSN_REQUIRE(P != nullptr, "csn_lstm_plan_set_lengths: null plan");
  CSN_REQUIRE(P->state, "csn_lstm_plan_set_lengths: the plan was created without CSN_LSTM_STATE");
  if (lengths == nullptr) {
    P->lengths.clear();
    P->t_eff = 0;
    return CSN_OK;
  }
  int longest = 0;
  for (int b = 0; b < P->d.B; ++b) {
    CSN_REQUIRE(lengths[b] >= 0 && lengths[b] <= P->d.T, "csn_lstm_plan_set_lengths: lengths[%d] = %d outside [0, %d]", b,
                (int)lengths[b], P->d.T);
    longest = std::max(longest, (int)lengths[b]);
  }
  P->lengths.assign(lengths, lengths + P->d.B);
  P->t_eff = longest;
  return CSN_OK;
}

extern "C" int csn_lstm_plan_set_views(csnLstmPlan* P, const int32_t* src_row, const int32_t* t0, int32_t src_rows,
                                       int32_t src_T) {
  CSN_REQUIRE(P != nullptr, "csn_lstm_plan_set_views: null plan");
  CSN_REQUIRE((src_row == nullptr) == (t0 == nullptr), "csn_lstm_plan_set_views: exactly one of src_row and t0 is null");
  if (src_row == nullptr) {
    P->view_row.clear();
    P->view_t0.clear();
    P->view_src_rows = P->view_src_T = 0;
    return CSN_OK;
  }
  CSN_REQUIRE(src_rows >= 1, "csn_lstm_plan_set_views: src_rows = %d", (int)src_rows);
  CSN_REQUIRE(src_T >= 1, "csn_lstm_plan_set_views: src_T = %d", (int)src_T);
  for (int b = 0; b < P->d.B; ++b) {
    CSN_REQUIRE(src_row[b] >= 0 && src_row[b] < src_rows, "csn_lstm_plan_set_views: src_row[%d] = %d outside [0, %d)", b,
                (int)src_row[b], (int)src_rows);
    CSN_REQUIRE(t0[b] >= 0, "csn_lstm_plan_set_views: t0[%d] = %d is negative", b, (int)t0[b]);
  }
  P->view_row.assign(src_row, src_row + P->d.B);
  P->view_t0.assign(t0, t0 + P->d.B);
  P->view_src_rows = src_rows;
  P->view_src_T = src_T;
  return CSN_OK;
}

extern "C" int csn_lstm_plan_set_dropout(csnLstmPlan* P, float p, uint64_t seed, uint32_t subsequence) {
  CSN_REQUIRE(P != nullptr, "csn_lstm_plan_set_dropout: null plan");
  CSN_REQUIRE(p >= 0.f && p <= 1.f, "csn_lstm_plan_set_dropout: p = %g outside [0, 1]", (double)p);      // (NaN fails both)
  CSN_REQUIRE(p == 0.f || P->dropout, "csn_lstm_plan_set_dropout: p = %g, but the plan was created without CSN_LSTM_DROPOUT", (double)p);
  P->drop_p = p;
  P->drop_seed = seed;
  P->drop_subsequence = subsequence;
  return CSN_OK;
}

extern "C" int csn_lstm_plan_set_output_dropout(csnLstmPlan* P, float p, uint64_t seed, uint32_t subsequence, uint64_t first,
                                                int64_t index_pitch) {
  CSN_REQUIRE(P != nullptr, "csn_lstm_plan_set_output_dropout: null plan");
  CSN_REQUIRE(p >= 0.f && p <= 1.f, "csn_lstm_plan_set_output_dropout: p = %g outside [0, 1]", (double)p);      // (NaN fails both)
  CSN_REQUIRE(p == 0.f || (first % 4 == 0 && index_pitch % 4 == 0 && index_pitch >= P->d.H),
              "csn_lstm_plan_set_output_dropout: first = %llu and index_pitch = %lld must be multiples of 4, index_pitch >= H = %d",
              (unsigned long long)first, (long long)index_pitch, P->d.H);
  P->out_drop_p = p;
  P->out_drop_seed = seed;
  P->out_drop_subsequence = subsequence;
  P->out_drop_first = first;
  P->out_drop_pitch = index_pitch;
  return CSN_OK;
}

extern "C" int csn_lstm_plan_set_io(csnLstmPlan* P, int64_t y_all_pitch, int64_t dy_all_pitch, int dx_add) {
  CSN_REQUIRE(P != nullptr, "csn_lstm_plan_set_io: null plan");
  const int64_t pitch[2] = {y_all_pitch, dy_all_pitch};
  const char* const names[2] = {"y_all_pitch", "dy_all_pitch"};
  for (int i = 0; i < 2; ++i)
    CSN_REQUIRE(pitch[i] == 0 || (pitch[i] >= P->d.H && pitch[i] % 4 == 0),
                "csn_lstm_plan_set_io: %s = %lld is neither 0 (dense) nor a multiple of 4 that is >= H = %d", names[i],
                (long long)pitch[i], P->d.H);
  P->y_pitch = y_all_pitch == P->d.H ? 0 : y_all_pitch;
  P->dy_pitch = dy_all_pitch == P->d.H ? 0 : dy_all_pitch;
  P->dx_add = dx_add != 0;
  return CSN_OK;
}

extern "C" int csn_lstm_plan_set_attention(csnLstmPlan* P, const float* q, float scale, float* dq, float* attn_out, float* dscore_out) {
  CSN_REQUIRE(P != nullptr, "csn_lstm_plan_set_attention: null plan");
  CSN_REQUIRE(std::isfinite(scale), "csn_lstm_plan_set_attention: scale is not finite");
  CSN_REQUIRE(q != nullptr || (dq == nullptr && attn_out == nullptr && dscore_out == nullptr),
              "csn_lstm_plan_set_attention: dq, attn_out or dscore_out without q");
  P->attn_q = q;
  P->attn_scale = scale;
  P->attn_dq = dq;
  P->attn_out = attn_out;
  P->attn_dscore = dscore_out;
  return CSN_OK;
}

extern "C" int csn_lstm_plan_set_readout(csnLstmPlan* P, int mode) {
  CSN_REQUIRE(P != nullptr, "csn_lstm_plan_set_readout: null plan");
  CSN_REQUIRE(mode == CSN_READOUT_LAST || mode == CSN_READOUT_MEAN || mode == CSN_READOUT_MAX, "csn_lstm_plan_set_readout: unknown mode %d", mode);
  P->readout = mode;
  return CSN_OK;
}

// lengths of the call in progress -> the plan's device array, in stream order (every forward and backward that runs with
// lengths uploads what the plan holds, so the kernels of a call read the lengths of that call); *dlen: that array, or null
// for a plan without lengths
static int upload_lengths(csnLstmPlan* P, hipStream_t st, const int** dlen) {
  *dlen = nullptr;
  if (P->lengths.empty()) return CSN_OK;
  // through a pinned staging array of the plan: the copy is asynchronous, and the array is rewritten only once the copy
  // before has left it (long ago, as a rule: the wait is for one small copy, not for the stream)
  const size_t bytes = (size_t)P->d.B * 4;
  if (P->len_pin == nullptr) {
    CSN_HIP_CHECK(hipMalloc((void**)&P->len_dev, bytes));
    CSN_HIP_CHECK(hipHostMalloc((void**)&P->len_pin, bytes, hipHostMallocDefault));
    CSN_HIP_CHECK(hipEventCreateWithFlags(&P->len_ev, hipEventDisableTiming));
  } else {
    CSN_HIP_CHECK(hipEventSynchronize(P->len_ev));
  }
  memcpy(P->len_pin, P->lengths.data(), bytes);
  CSN_HIP_CHECK(hipMemcpyAsync(P->len_dev, P->len_pin, bytes, hipMemcpyHostToDevice, st));
  CSN_HIP_CHECK(hipEventRecord(P->len_ev, st));
  *dlen = P->len_dev;
  return CSN_OK;
}

// input windows of the forward in progress -> the plan's device arrays, in stream order, exactly as upload_lengths does
// (the backward reads no x and uploads nothing); *vrow / *vt0: the [B] arrays, or null for a plan without windows
static int upload_views(csnLstmPlan* P, hipStream_t st, const int** vrow, const int** vt0) {
  *vrow = *vt0 = nullptr;
  if (P->view_row.empty()) return CSN_OK;
  const size_t B = (size_t)P->d.B, bytes = 2 * B * 4;
  if (P->view_pin == nullptr) {
    CSN_HIP_CHECK(hipMalloc((void**)&P->view_dev, bytes));
    CSN_HIP_CHECK(hipHostMalloc((void**)&P->view_pin, bytes, hipHostMallocDefault));
    CSN_HIP_CHECK(hipEventCreateWithFlags(&P->view_ev, hipEventDisableTiming));
  } else {
    CSN_HIP_CHECK(hipEventSynchronize(P->view_ev));
  }
  memcpy(P->view_pin, P->view_row.data(), B * 4);
  memcpy(P->view_pin + B, P->view_t0.data(), B * 4);
  CSN_HIP_CHECK(hipMemcpyAsync(P->view_dev, P->view_pin, bytes, hipMemcpyHostToDevice, st));
  CSN_HIP_CHECK(hipEventRecord(P->view_ev, st));
  *vrow = P->view_dev;
  *vt0 = P->view_dev + B;
  return CSN_OK;
}

// One forward or backward call: lives on the stack of csn_lstm_forward / csn_lstm_backward and is handed to every path and
// helper below.  What holds for the duration of a call only is here, not in the plan: P.d is never written after
// csn_lstm_plan_create.  A call with lengths runs every path over the steps of the longest row (all saved tensors are
// time-major, so T enters extents only, never a stride -- the workspace layout is that of d.T).
struct Call {
  Plan& P;
  const csnLstmDesc& d;
  const WsLayout& w;
  char* ws;
  hipStream_t st;       // the caller's stream
  const int* dlen;      // device copy of the lengths ([B] int32, owned by the plan), null without lengths
  const int* vrow = nullptr;      // device copies of the input windows of a forward ([B] int32 each, owned by the plan),
  const int* vt0 = nullptr;       // null without windows
  int T;                // the steps this call runs: the longest row with lengths, else d.T
  int T_full;           // d.T: the steps per row of the caller's batch-first tensors
  int B, H, NL, dt, Cz; // Cz: steps per chunk
  int64_t G, TB;        // 4 H; T * B
  size_t es;            // bytes per element of the compute dtype
  Call(Plan& P_, void* workspace, hipStream_t st_, const int* dlen_)
      : P(P_), d(P_.d), w(P_.w), ws((char*)workspace), st(st_), dlen(dlen_), T(dlen_ ? P_.t_eff : P_.d.T), T_full(P_.d.T),
        B(P_.d.B), H(P_.d.H), NL(P_.d.L), dt(P_.d.dtype), Cz(P_.opt.chunk), G(4 * (int64_t)P_.d.H), TB((int64_t)T * P_.d.B),
        es(dtype_size(P_.d.dtype)) {}
  int64_t in_width(int l) const { return l == 0 ? d.I : H; }
};
// what the caller passes to a forward / a backward (state pointers null unless the plan takes them)
struct FwdArgs {
  const float* x;
  int64_t xsb, xst;
  const float* const* w_ih;
  const float* const* w_hh;
  const float* const* b_ih;
  const float* const* b_hh;
  const float* h0;
  const float* c0;
};
struct BwdArgs {
  const float* dy_last;       // gradient w.r.t. the top layer's output: at the last step, and / or
  const float* dy_tm;         // time-major for every step (workspace copy)
  const float* dh_n;
  const float* dc_n;
  float* const* dw_ih;
  float* const* dw_hh;
  float* const* db_ih;
  float* const* db_hh;
  float* dx;
};

// this call's rows for a layout pass of lstm_boundary.hip over a caller's tensor `width` wide, `pitch` elements from row to row (0: dense)
static RowMap row_map(const Call& C, int64_t width, int64_t pitch) {
  return RowMap{C.dlen, C.B, C.T_full, C.T, (int)width, pitch ? pitch : width, C.P.reverse, C.P.dx_add};
}
// input gradient out of its time-major workspace form (the caller's rows have T_full steps)
static int emit_dx(const Call& C, const float* dx_tm, float* dx, int64_t I, hipStream_t st) {
  return launch_dx_out(dx_tm, dx, row_map(C, I, 0), st);
}
// gradient w.r.t. h_n of the layer below, into this layer's time-major input gradient `dx_tm` whose steps [t_lo, t_hi] were
// just written: at each row's own last step
static int add_dh_n_rows(const Call& C, const float* dh_below, float* dx_tm, int t_lo, int t_hi, hipStream_t st) {
  return launch_add_at_end(dh_below, dx_tm, C.dlen, C.T, t_lo, t_hi, C.B, C.H, st);
}

extern "C" int csn_lstm_profile_enable(csnLstmPlan* P, int on) {
  CSN_REQUIRE(P != nullptr, "csn_lstm_profile_enable: null plan");
  P->prof.on = on != 0;
  P->prof.have[0] = P->prof.have[1] = false;
  return CSN_OK;
}

extern "C" int csn_lstm_profile_read(csnLstmPlan* P, double* fwd_ms, int* fwd_launches, int* fwd_cells, double* bwd_ms,
                                     int* bwd_launches, int* bwd_cells) {
  CSN_REQUIRE(P && fwd_ms && fwd_launches && fwd_cells && bwd_ms && bwd_launches && bwd_cells,
              "csn_lstm_profile_read: null pointer");
  Prof& g_prof = P->prof;
  *fwd_ms = *bwd_ms = 0.0;
  *fwd_launches = *fwd_cells = *bwd_launches = *bwd_cells = 0;
  for (int k = 0; k < 2; ++k) {
    if (!g_prof.have[k]) continue;
    float ms = 0.f;
    CSN_HIP_CHECK(hipEventSynchronize(g_prof.ev[2 * k + 1]));
    if (g_prof.pairs_used[k] > 0) {
      for (size_t i = 0; i < g_prof.pairs_used[k]; ++i) {
        float one = 0.f;
        CSN_HIP_CHECK(hipEventElapsedTime(&one, g_prof.pair[k][2 * i], g_prof.pair[k][2 * i + 1]));
        ms += one;
      }
    } else {
      CSN_HIP_CHECK(hipEventElapsedTime(&ms, g_prof.ev[2 * k], g_prof.ev[2 * k + 1]));
    }
    (k == 0 ? *fwd_ms : *bwd_ms) = ms;
    (k == 0 ? *fwd_launches : *bwd_launches) = g_prof.launches[k];
    (k == 0 ? *fwd_cells : *bwd_cells) = g_prof.cells[k];
  }
  return CSN_OK;
}

// Once per workspace, before its first forward: the status word and everything the kernels only ever READ as zero
// (slot 0 of h_all / c_all of every layer = the zero initial state; the zero row the backward reads where a step has
// no incoming gradient)
extern "C" int csn_lstm_workspace_init(const csnLstmPlan* P, void* workspace, csnStream_t stream) {
  CSN_REQUIRE(P && workspace, "csn_lstm_workspace_init: null pointer");
  CSN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "csn_lstm_workspace_init: workspace must be 256-B aligned");
  hipStream_t st = as_stream(stream);
  char* ws = (char*)workspace;
  const WsLayout& w = P->w;
  const size_t es = dtype_size(P->d.dtype);
  CSN_HIP_CHECK(hipMemsetAsync(ws + w.status, 0, kStatusBytes, st));
  for (int l = 0; l < P->d.L; ++l) {
    CSN_HIP_CHECK(hipMemsetAsync(ws + w.layer[l].h_all, 0, (size_t)P->d.B * P->d.H * es, st));
    CSN_HIP_CHECK(hipMemsetAsync(ws + w.layer[l].c_all, 0, (size_t)P->d.B * P->d.H * 4, st));
  }
  if (w.persist_bwd || (w.f32_persist && P->training))
    CSN_HIP_CHECK(hipMemsetAsync(ws + w.zeros_bh, 0, (size_t)P->d.B * P->d.H * 4, st));
  return CSN_OK;
}

// The workspace's status word (sticky; see include/csn_hip.h)
extern "C" int csn_lstm_status_clear(const csnLstmPlan* P, void* workspace, csnStream_t stream) {
  CSN_REQUIRE(P && workspace, "csn_lstm_status_clear: null pointer");
  CSN_HIP_CHECK(hipMemsetAsync((char*)workspace + P->w.status, 0, kStatusBytes, as_stream(stream)));
  return CSN_OK;
}
extern "C" int csn_lstm_status_raise(const csnLstmPlan* P, void* workspace, csnStream_t stream) {
  CSN_REQUIRE(P && workspace, "csn_lstm_status_raise: null pointer");
  CSN_HIP_CHECK(hipMemsetAsync((char*)workspace + P->w.status + 4 * kStatusTimeout, 1, 1, as_stream(stream)));   // word = 1, as a timed-out wait leaves it
  return CSN_OK;
}
extern "C" int csn_lstm_status_read(const csnLstmPlan* P, const void* workspace, int* status) {
  CSN_REQUIRE(P && workspace && status, "csn_lstm_status_read: null pointer");
  // the status words of lstm_handoff.h: a bounded wait timed out; a non-finite gradient reached the backward; (debug
  // library built with -DCSN_SLAB_TAGS only) a consumer was served a stale occupant of a hand-off ring slot
  unsigned flag[kStatusStaleSlot + 1] = {};
  CSN_HIP_CHECK(hipMemcpy(flag, (const char*)workspace + P->w.status, sizeof(flag), hipMemcpyDeviceToHost));
  *status = (flag[kStatusTimeout] ? CSN_STATUS_TIMEOUT : 0) | (flag[kStatusNonFinite] ? CSN_STATUS_NONFINITE : 0) |
            (flag[kStatusStaleSlot] ? CSN_STATUS_STALE_SLOT : 0);
#ifdef CSN_SLAB_TAGS
  if (flag[kStatusStaleSlot] && getenv("CSN_TAGS_VERBOSE")) {
    unsigned dbg[24];      // the claim word, then the dump
    static_assert(kStatusDump == kStatusDumpClaim + 1 && 4 * kStatusDumpClaim + sizeof(dbg) <= kStatusBytes, "the dump follows its claim");
    CSN_HIP_CHECK(hipMemcpy(dbg, (const char*)workspace + P->w.status + 4 * kStatusDumpClaim, sizeof(dbg), hipMemcpyDeviceToHost));
    if (dbg[0])
      fprintf(stderr, "stale piece (backward): t=%u step-in-launch=%u group=%u slice=%u wave=%u lane=%u kb*4+rg=%u u0=%08x local=%u redone=%u "
              "single=%u phase=%u rot=%u nsteps=%u xcc=%u lanes=%u\n", dbg[1], dbg[2], dbg[3], dbg[4], dbg[5], dbg[6], dbg[7], dbg[8],
              dbg[9], dbg[10], dbg[11], dbg[12], dbg[13], dbg[14], dbg[15], dbg[16]);
  }
#endif
  return CSN_OK;
}

extern "C" size_t csn_lstm_workspace_bytes(const csnLstmDesc* d, int training) {
  if (check_desc("csn_lstm_workspace_bytes", d) != CSN_OK) return 0;
  if (check_resident("csn_lstm_workspace_bytes", d, training) != CSN_OK) return 0;
  Options opt = options_from_env();
  if ((training & CSN_LSTM_STATE) && d->dtype == CSN_F32) opt.no_persist = true;
  if (training & CSN_LSTM_RESIDENT) resident_options(opt);
  return make_layout(*d, (training & ~kPlanBits) != 0, (training & CSN_LSTM_DROPOUT) != 0, opt).total;
}

// C[M,N] = A[K,M]^T B[K,N] through the split-K slabs + their fixed-order reduction (the body of csn_gemm_tn)
// accumulate: C's previous contents join the reduced sum last (CSN_GRAD_ACCUMULATE)
static int gemm_tn_full(const void* A, const void* B, float* C, int64_t M, int64_t N, int64_t K, int dtype, void* scratch,
                        int accumulate, hipStream_t st, const Options& opt) {
  int S = 1;
  if (int rc = launch_gemm_tn_slabs(A, B, (float*)scratch, M, N, K, dtype, st, &S, nullptr, nullptr, opt)) return rc;
  return launch_reduce_slabs((const float*)scratch, M * N, S, C, nullptr, M * N, accumulate, st);
}

// lengths: zeros over the padding of the re-laid-out input (x_c, and the fragment-major slabs of the fused projection)
static int mask_x(const Call& C, hipStream_t st) {
  if (C.dlen == nullptr) return CSN_OK;
  const csnLstmDesc& d = C.d;
  if (int rc = launch_mask_tm(C.ws + C.w.x_c, d.dtype, C.dlen, d.B, C.T, d.I, st)) return rc;
  if (C.w.fuse_x) return launch_mask_x_blk((bf16_t*)(C.ws + C.w.x_blk), C.dlen, d.B, ((int64_t)d.B + 63) / 64 * 64, C.T, d.I, st);
  return CSN_OK;
}

// =============================================================================================
// jobs every path shares
// =============================================================================================
// what layer l multiplies by W_ih, time-major from step 0: the re-laid-out x, or the outputs of the layer below (h_all from slot 1)
// (with dropout on: the masked and scaled copy of those outputs, h_drop, which has no slot 0)
static bool drop_on(const Call& C) { return C.P.dropout && C.P.drop_p > 0.f && C.NL > 1; }
static const void* layer_input(const Call& C, int l) {
  if (l > 0 && drop_on(C)) return C.ws + C.w.layer[l - 1].h_drop;
  return l == 0 ? (const void*)(C.ws + C.w.x_c) : (const void*)(C.ws + C.w.layer[l - 1].h_all + (size_t)C.B * C.H * C.es);
}

// Inter-layer dropout (csn_lstm_plan_set_dropout; lstm_dropout.hip), interface l = between layers l and l + 1, steps
// [t_lo, t_hi]; both are no-ops unless the plan has the bit and p > 0.  The element index runs over the PLAN's T, so a
// call with lengths draws the mask of the same call without them.
//   forward : h_drop[l] <- mask * h_all[l] / (1 - p), in front of the GEMM that reads it
//   backward: dx of layer l + 1 *= mask / (1 - p) in place, between its GEMM and the dh_n term of layer l
static int drop_fwd(const Call& C, int l, int t_lo, int t_hi, hipStream_t on) {
  if (!drop_on(C)) return CSN_OK;
  const size_t BH = (size_t)C.B * C.H;
  return launch_lstm_dropout_fwd(C.ws + C.w.layer[l].h_all + (size_t)(t_lo + 1) * BH * C.es, C.ws + C.w.layer[l].h_drop + (size_t)t_lo * BH * C.es,
                                 (int64_t)(t_hi - t_lo + 1) * (int64_t)BH, ((uint64_t)l * C.T_full + t_lo) * BH, C.dt,
                                 dropout_cfg(C.P.drop_p, C.P.drop_seed, C.P.drop_subsequence), on);
}
static int drop_bwd(const Call& C, int l, int t_lo, int t_hi, hipStream_t on) {
  if (!drop_on(C)) return CSN_OK;
  const size_t BH = (size_t)C.B * C.H;
  return launch_lstm_dropout_bwd((float*)(C.ws + C.w.layer[l + 1].dx) + (size_t)t_lo * BH, (int64_t)(t_hi - t_lo + 1) * (int64_t)BH,
                                 ((uint64_t)l * C.T_full + t_lo) * BH, dropout_cfg(C.P.drop_p, C.P.drop_seed, C.P.drop_subsequence), on);
}

// slot 0 of h_all / c_all of layer l = the initial state (the cells read it at t = 0; the dW_hh GEMM reads h_all slot 0
// too): the caller's (h0, c0), or zeros
static int install_slot0(const Call& C, int l, const float* h0, const float* c0) {
  const LayerWs& L = C.w.layer[l];
  const size_t BH = (size_t)C.B * C.H;
  if (h0) {
    if (int rc = launch_cast(h0 + l * BH, C.ws + L.h_all, (int64_t)BH, C.dt, C.st)) return rc;
  } else {
    CSN_HIP_CHECK(hipMemsetAsync(C.ws + L.h_all, 0, BH * C.es, C.st));
  }
  if (c0)
    CSN_HIP_CHECK(hipMemcpyAsync(C.ws + L.c_all, c0 + l * BH, BH * 4, hipMemcpyDeviceToDevice, C.st));
  else
    CSN_HIP_CHECK(hipMemsetAsync(C.ws + L.c_all, 0, BH * 4, C.st));
  return CSN_OK;
}

// the carried dc of layer l starts as the gradient w.r.t. c_n; after step 0 it is the gradient w.r.t. c0
// (zeroed: a fill of the workspace has cleared it already)
static int seed_dc_carry(const Call& C, int l, const float* dc_n, bool zeroed) {
  const size_t BH = (size_t)C.B * C.H;
  if (dc_n)
    CSN_HIP_CHECK(hipMemcpyAsync(C.ws + C.w.layer[l].dc_carry, dc_n + l * BH, BH * 4, hipMemcpyDeviceToDevice, C.st));
  else if (!zeroed)
    CSN_HIP_CHECK(hipMemsetAsync(C.ws + C.w.layer[l].dc_carry, 0, BH * 4, C.st));
  return CSN_OK;
}

// Row-major paths (0 and 4): time-major x, the compute-dtype copies of the parameters (transposes for a training plan),
// b_ih + b_hh, slot 0 of every layer
static int prep_row_major(const Call& C, const FwdArgs& A) {
  const WsLayout& w = C.w;
  char* ws = C.ws;
  hipStream_t st = C.st;
  const int H = C.H, dt = C.dt;
  const int64_t G = C.G;
  int rc;
  if ((rc = launch_cast_strided(A.x, A.xsb, A.xst, C.B, C.T, C.d.I, ws + w.x_c, dt, st, C.dlen, C.P.reverse, C.vrow, C.vt0))) return rc;
  if ((rc = mask_x(C, st))) return rc;
  for (int l = 0; l < C.NL; ++l) {
    const LayerWs& L = w.layer[l];
    const int64_t I = C.in_width(l);
    if ((rc = launch_cast(A.w_ih[l], ws + L.wih, G * I, dt, st))) return rc;
    if ((rc = launch_cast(A.w_hh[l], ws + L.whh, G * H, dt, st))) return rc;
    if (C.P.training) {
      if ((rc = launch_transpose_cast(A.w_hh[l], G, H, ws + L.whht, dt, st))) return rc;
      if ((rc = launch_transpose_cast(A.w_ih[l], G, I, ws + L.wiht, dt, st))) return rc;
    }
    if ((rc = launch_add_vec(A.b_ih[l], A.b_hh[l], (float*)(ws + L.bias), G, st))) return rc;
    if ((rc = install_slot0(C, l, A.h0, A.c0))) return rc;
  }
  return CSN_OK;
}

// chunk c of this call's steps (lstm_schedule.h)
static Chunk chunk_at(const Call& C, int c) { return chunk_at(C.T, C.Cz, c); }

// layer l finished chunk c -> xproj_{l+1}[chunk c] = h_l[chunk c] W_ih^T + b
static int xproj_chunk_gemm(const Call& C, int l, int c, hipStream_t on) {
  const LayerWs& Ln = C.w.layer[l + 1];
  const Chunk k = chunk_at(C, c);
  if (int rc = drop_fwd(C, l, k.t0, k.t0 + k.nsteps - 1, on)) return rc;
  return gemm_nt((const char*)layer_input(C, l + 1) + (size_t)k.t0 * C.B * C.H * C.es, C.ws + Ln.wih, (const float*)(C.ws + Ln.bias),
                 (float*)(C.ws + Ln.xproj) + (size_t)k.t0 * C.B * C.G, (int64_t)k.nsteps * C.B, C.G, C.H, C.dt, CSN_F32, 0, on, C.P.opt);
}

// layer l >= 1 finished reverse chunk c -> dx_l[chunk] = dgates_l[chunk] W_ih (the dy of the layer below; Bt = W_ih^T [H, 4H]),
// then the gradient w.r.t. h_n of the layer below joins it at t = T-1 (with lengths: at each row's last step)
static int dx_chunk_gemm(const Call& C, int l, int c, const float* dh_n, hipStream_t on) {
  const LayerWs& L = C.w.layer[l];
  const Chunk k = chunk_at(C, c);
  const int t_hi = C.T - 1 - k.t0, t_lo = t_hi - k.nsteps + 1;
  if (int rc = gemm_nt(C.ws + L.dgates + (size_t)t_lo * C.B * C.G * C.es, C.ws + L.wiht, nullptr, (float*)(C.ws + L.dx) + (size_t)t_lo * C.B * C.H,
                       (int64_t)k.nsteps * C.B, C.H, C.G, C.dt, CSN_F32, 0, on, C.P.opt))
    return rc;
  if (int rc = drop_bwd(C, l - 1, t_lo, t_hi, on)) return rc;
  if (dh_n) return add_dh_n_rows(C, dh_n + (size_t)(l - 1) * C.B * C.H, (float*)(C.ws + L.dx), t_lo, t_hi, on);
  return CSN_OK;
}

// input gradient of layer 0, whole sequence, out to the caller (batch-first)
static int dx_out(const Call& C, float* dx, hipStream_t on) {
  const LayerWs& L = C.w.layer[0];
  if (int rc = gemm_nt(C.ws + L.dgates, C.ws + L.wiht, nullptr, C.ws + L.dx, C.TB, C.d.I, C.G, C.dt, CSN_F32, 0, on, C.P.opt)) return rc;
  return emit_dx(C, (const float*)(C.ws + L.dx), dx, C.d.I, on);
}

// weight / bias gradients of layer l (its recurrence complete), row-major paths.  colsum: db_ih and db_hh as the column
// sums of dgates (the float32 weight-stationary kernel has summed the bias gradient itself)
static int weight_grads_rm(const Call& C, const BwdArgs& A, int l, bool colsum) {
  const WsLayout& w = C.w;
  const LayerWs& L = w.layer[l];
  char* ws = C.ws;
  const int acc = C.P.grad_accumulate;
  int rc;
  if ((rc = gemm_tn_full(ws + L.dgates, ws + L.h_all, A.dw_hh[l], C.G, C.H, C.TB, C.dt, ws + w.tn_scratch, acc, C.st, C.P.opt))) return rc;
  if ((rc = gemm_tn_full(ws + L.dgates, layer_input(C, l), A.dw_ih[l], C.G, C.in_width(l), C.TB, C.dt, ws + w.tn_scratch, acc, C.st, C.P.opt))) return rc;
  // db_ih and db_hh both come out of the reduction (each adds to its own previous contents under CSN_GRAD_ACCUMULATE)
  if (colsum) return launch_colsum(ws + L.dgates, C.TB, C.G, C.dt, A.db_ih[l], A.db_hh[l], acc, ws + w.colsum, C.st);
  return CSN_OK;
}

// weight / bias gradients of layer l (its recurrence complete), fast paths: two split-K GEMMs, the reductions that
// un-permute the gate-interleaved 4H axis, the bias gradient -- four or five launches on `on`
static int weight_grads_blk(const Call& C, const BwdArgs& A, int l, hipStream_t on) {
  const WsLayout& w = C.w;
  const LayerWs& L = w.layer[l];
  char* ws = C.ws;
  const int H = C.H;
  const int64_t G = C.G, TB = C.TB, I = C.in_width(l);
  float* slabs = (float*)(ws + w.tn_scratch);
  const int acc = C.P.grad_accumulate;
  int S = 1, r;
  int cs_done = 0, S_cs = 1;
  if ((r = launch_gemm_tn_slabs(ws + L.dgates, ws + L.h_all, slabs, G, H, TB, CSN_BF16, on, &S, (float*)(ws + w.colsum), &cs_done, C.P.opt))) return r;
  S_cs = S;
  if ((r = launch_reduce_slabs_unperm(slabs, G * H, S, H, H, A.dw_hh[l], nullptr, acc, on))) return r;
  if ((r = launch_gemm_tn_slabs(ws + L.dgates, layer_input(C, l), slabs, G, I, TB, CSN_BF16, on, &S, nullptr, nullptr, C.P.opt))) return r;
  if ((r = launch_reduce_slabs_unperm(slabs, G * I, S, H, I, A.dw_ih[l], nullptr, acc, on))) return r;
  // bias gradient = column sums of dgates: partial sums come out of the dW_hh GEMM when its kernel provides them
  if (!cs_done) {
    if ((r = launch_colsum_partial(ws + L.dgates, TB, G, CSN_BF16, ws + w.colsum, on))) return r;
    S_cs = colsum_chunks();
  }
  // db_ih and db_hh both come out of the reduction (each adds to its own previous contents under CSN_GRAD_ACCUMULATE)
  return launch_reduce_slabs_unperm((const float*)(ws + w.colsum), G, S_cs, H, 1, A.db_ih[l], A.db_hh[l], acc, on);
}

// end of the recurrence window of a forward (k = 0) / a backward (k = 1): its closing event and what csn_lstm_profile_read reports
static int prof_end(Call& C, int k, int launches, int cells) {
  Prof& g_prof = C.P.prof;
  if (int rc = prof_mark(g_prof, 2 * k + 1, C.st)) return rc;
  g_prof.launches[k] = launches;
  g_prof.cells[k] = cells;
  g_prof.have[k] = g_prof.on;
  return CSN_OK;
}

// gradient w.r.t. the initial hidden state of layer l (lstm_dh0_kernel: dgates of step 0 times W_hh), in the form this
// plan's backward left the two
static int launch_dh0(const Call& C, int l, float* out) {
  const LayerWs& L = C.w.layer[l];
  const int B = C.B, H = C.H;
  const dim3 grid((unsigned)((H + 63) / 64), (unsigned)((B + 31) / 32));
  if (C.w.il)
    lstm_dh0_kernel<bf16_t, true><<<grid, 256, 0, C.st>>>((const bf16_t*)(C.ws + L.dgates), (const bf16_t*)(C.ws + L.whht_blk), B, H, out);
  else if (C.dt == CSN_BF16)
    lstm_dh0_kernel<bf16_t, false><<<grid, 256, 0, C.st>>>((const bf16_t*)(C.ws + L.dgates), (const bf16_t*)(C.ws + L.whht), B, H, out);
  else
    lstm_dh0_kernel<float, false><<<grid, 256, 0, C.st>>>((const float*)(C.ws + L.dgates), (const float*)(C.ws + L.whht), B, H, out);
  CSN_LAUNCH_CHECK();
  return CSN_OK;
}

// =============================================================================================
// path 0: generic cells (lstm_cell.hip)
// =============================================================================================
// Wavefront over the layers, as in path 1: diagonal d runs layer l at step d - l * lag in ONE launch (blockIdx.z =
// layer; round 3 ran layer after layer, one launch per layer-step: 2 T L launches per pass, each bound by its launch
// boundary and its own fill, not by the float32 MFMA rate).  The input projection of layer l + 1 follows layer l chunk by
// chunk (GEMM over `chunk` steps on the same stream), so lag = chunk.  Which cells a launch holds and which chunks a
// diagonal finished is wavefront_schedule (lstm_schedule.h), here and in paths 1 and 5: each of the six functions fills one
// problem of its kernel's batch from a cell and enqueues the launches, the chunk GEMMs behind one that closes a diagonal.
static int forward_v1(Call& C, const FwdArgs& A) {
  const WsLayout& w = C.w;
  char* ws = C.ws;
  hipStream_t st = C.st;
  const int B = C.B, T = C.T, H = C.H, dt = C.dt, NL = C.NL;
  const int64_t G = C.G;
  const size_t es = C.es;
  const int training = C.P.training;
  int rc;
  if ((rc = prep_row_major(C, A))) return rc;
  // layer 0: projection of every step in one GEMM
  if ((rc = gemm_nt(ws + w.x_c, ws + w.layer[0].wih, (const float*)(ws + w.layer[0].bias), ws + w.layer[0].xproj, C.TB, G,
                    C.d.I, dt, CSN_F32, 0, st, C.P.opt)))
    return rc;
  auto cell = [&](const WaveCell& s) {
    const LayerWs& L = w.layer[s.layer];
    const int t = s.t;
    return CellFwdOne{ws + L.h_all + (size_t)t * B * H * es, ws + L.whh, (const float*)(ws + L.xproj) + (size_t)t * B * G, G,
                      (const float*)(ws + L.c_all) + (size_t)t * B * H,
                      training ? ws + L.gates + (size_t)t * B * G * es : nullptr,
                      (float*)(ws + L.c_all) + (size_t)(t + 1) * B * H, ws + L.h_all + (size_t)(t + 1) * B * H * es};
  };
  return wavefront_schedule(WaveIn{T, NL, C.Cz, WaveUnit::step, 1, false}, [&](const WaveLaunch& q) -> int {
    CellFwdBatch b{};
    for (int i = 0; i < q.ncells; ++i) b.p[i] = cell(q.cell[i]);
    if (int rc = launch_cell_fwd_batch(b, q.ncells, B, H, dt, st)) return rc;
    // a layer that just finished a chunk feeds the next layer's input projection
    for (int i = 0; i < q.ndone; ++i)
      if (q.done[i].layer + 1 < NL)
        if (int rc = xproj_chunk_gemm(C, q.done[i].layer, q.done[i].chunk, st)) return rc;
    return CSN_OK;
  });
}

static int backward_v1(Call& C, const BwdArgs& A) {
  const WsLayout& w = C.w;
  char* ws = C.ws;
  hipStream_t st = C.st;
  const int B = C.B, T = C.T, H = C.H, dt = C.dt, NL = C.NL;
  const int64_t G = C.G;
  const size_t es = C.es;
  int rc;
  for (int l = 0; l < NL; ++l)
    if ((rc = seed_dc_carry(C, l, A.dc_n, false))) return rc;
  auto cell = [&](const WaveCell& s) {
    const int l = s.layer, t = s.t;
    const LayerWs& L = w.layer[l];
    const float* dy_t = l == NL - 1 ? (A.dy_tm ? A.dy_tm + (size_t)t * B * H : (t == T - 1 ? A.dy_last : nullptr))
                                    : (const float*)(ws + w.layer[l + 1].dx) + (size_t)t * B * H;
    return CellBwdOne{(t == T - 1) ? nullptr : (const void*)(ws + L.dgates + (size_t)(t + 1) * B * G * es), ws + L.whht, dy_t, H,
                      ws + L.gates + (size_t)t * B * G * es, (const float*)(ws + L.c_all) + (size_t)(t + 1) * B * H,
                      (const float*)(ws + L.c_all) + (size_t)t * B * H, (float*)(ws + L.dc_carry),
                      ws + L.dgates + (size_t)t * B * G * es};
  };
  // the gradient w.r.t. a layer's input (= dy of the layer below) follows chunk by chunk
  rc = wavefront_schedule(WaveIn{T, NL, C.Cz, WaveUnit::step, 1, true}, [&](const WaveLaunch& q) -> int {
    CellBwdBatch b{};
    CellMask mask{C.dlen, {0, 0, 0, 0}};
    for (int i = 0; i < q.ncells; ++i) {
      mask.t[i] = q.cell[i].t;
      b.p[i] = cell(q.cell[i]);
    }
    if (int rc = launch_cell_bwd_batch(b, q.ncells, B, H, dt, st, C.dlen ? &mask : nullptr)) return rc;
    for (int i = 0; i < q.ndone; ++i)
      if (q.done[i].layer > 0)
        if (int rc = dx_chunk_gemm(C, q.done[i].layer, q.done[i].chunk, A.dh_n, st)) return rc;
    return CSN_OK;
  });
  if (rc) return rc;
  for (int l = NL - 1; l >= 0; --l) {
    if ((rc = weight_grads_rm(C, A, l, true))) return rc;
    C.P.grads_ready(l);
  }
  if (A.dx) return dx_out(C, A.dx, st);
  return CSN_OK;
}

// =============================================================================================
// path 5: CU-resident recurrence, H <= 128 (lstm_resident.hip; CSN_LSTM_RESIDENT plans)
// =============================================================================================
// forward_v1 / backward_v1 with the step loop of a chunk moved into the kernel: the wavefront runs over CHUNKS, diagonal
// d runs layer l at chunk d - l in one launch (up to four (layer, chunk) problems, a second launch beyond), and the same
// chunk GEMMs follow it.  ceil(T / Cz) + L - 1 recurrence launches per pass for L <= 4, against T + Cz (L - 1).
static int forward_resident(Call& C, const FwdArgs& A) {
  const WsLayout& w = C.w;
  char* ws = C.ws;
  hipStream_t st = C.st;
  const int B = C.B, T = C.T, H = C.H, dt = C.dt, NL = C.NL;
  int rc;
  C.P.half_launches[0] = 0;
  if ((rc = prep_row_major(C, A))) return rc;
  if ((rc = gemm_nt(ws + w.x_c, ws + w.layer[0].wih, (const float*)(ws + w.layer[0].bias), ws + w.layer[0].xproj, C.TB, C.G,
                    C.d.I, dt, CSN_F32, 0, st, C.P.opt)))
    return rc;
  if ((rc = prof_mark(C.P.prof, 0, st))) return rc;
  auto cell = [&](const WaveCell& s) {
    const LayerWs& L = w.layer[s.layer];
    return ResFwdOne{ws + L.whh, (const float*)(ws + L.xproj), (float*)(ws + L.c_all), ws + L.h_all,
                     C.P.training ? ws + L.gates : nullptr, s.t, s.nsteps};
  };
  int n_launch = 0;
  rc = wavefront_schedule(WaveIn{T, NL, C.Cz, WaveUnit::chunk, 1, false}, [&](const WaveLaunch& q) -> int {
    ResFwdBatch b{};
    for (int i = 0; i < q.ncells; ++i) b.p[i] = cell(q.cell[i]);
    if (int rc = launch_resident_fwd(b, q.ncells, B, H, dt, st)) return rc;
    ++n_launch;
    // a layer that just finished a chunk feeds the next layer's input projection
    for (int i = 0; i < q.ndone; ++i)
      if (q.done[i].layer + 1 < NL)
        if (int rc = xproj_chunk_gemm(C, q.done[i].layer, q.done[i].chunk, st)) return rc;
    return CSN_OK;
  });
  if (rc) return rc;
  return prof_end(C, 0, n_launch, T * NL);
}

static int backward_resident(Call& C, const BwdArgs& A) {
  const WsLayout& w = C.w;
  char* ws = C.ws;
  hipStream_t st = C.st;
  const int B = C.B, T = C.T, H = C.H, dt = C.dt, NL = C.NL;
  int rc;
  C.P.dgates_copies = 0;
  C.P.half_launches[1] = 0;
  for (int l = 0; l < NL; ++l)
    if ((rc = seed_dc_carry(C, l, A.dc_n, false))) return rc;
  if ((rc = prof_mark(C.P.prof, 2, st))) return rc;
  auto cell = [&](const WaveCell& s) {      // (reverse chunk: the steps [t_hi - nsteps + 1, t_hi])
    const int l = s.layer;
    const LayerWs& L = w.layer[l];
    const bool top = (l == NL - 1);
    return ResBwdOne{ws + L.whht, top ? A.dy_tm : (const float*)(ws + w.layer[l + 1].dx), top ? A.dy_last : nullptr,
                     ws + L.gates, (const float*)(ws + L.c_all), (float*)(ws + L.dc_carry), ws + L.dgates,
                     s.t, s.nsteps};
  };
  int n_launch = 0;
  rc = wavefront_schedule(WaveIn{T, NL, C.Cz, WaveUnit::chunk, 1, true}, [&](const WaveLaunch& q) -> int {
    ResBwdBatch b{};
    for (int i = 0; i < q.ncells; ++i) b.p[i] = cell(q.cell[i]);
    if (int rc = launch_resident_bwd(b, q.ncells, B, T, H, dt, C.dlen, st)) return rc;
    ++n_launch;
    for (int i = 0; i < q.ndone; ++i)
      if (q.done[i].layer > 0)
        if (int rc = dx_chunk_gemm(C, q.done[i].layer, q.done[i].chunk, A.dh_n, st)) return rc;
    return CSN_OK;
  });
  if (rc) return rc;
  if ((rc = prof_end(C, 1, n_launch, T * NL))) return rc;
  for (int l = NL - 1; l >= 0; --l) {
    if ((rc = weight_grads_rm(C, A, l, true))) return rc;
    C.P.grads_ready(l);
  }
  if (A.dx) return dx_out(C, A.dx, st);
  return CSN_OK;
}

// =============================================================================================
// path 4: exact float32, weight-stationary (lstm_f32_persist.hip)
// =============================================================================================
// Layer after layer, ONE recurrence launch per layer and block of M-tiles, the non-recurrent contractions as
// whole-sequence GEMMs between them (the same GEMM kernels, the same K order per output element as the chunked calls of
// forward_v1: row chunking does not enter a row's sum).
static int forward_f32p(Call& C, const FwdArgs& A) {
  const WsLayout& w = C.w;
  Prof& g_prof = C.P.prof;
  char* ws = C.ws;
  hipStream_t st = C.st;
  const int B = C.B, T = C.T, H = C.H, NL = C.NL;
  const int MTt = (B + 63) / 64, per = f32_persist_tiles_per_launch(H);
  int rc;
  if ((rc = prep_row_major(C, A))) return rc;
  CSN_HIP_CHECK(hipMemsetAsync(ws + w.zero_fwd, 0, w.zero_fwd_bytes, st));      // the flag lines of every layer
  int n_launch = 0;
  if ((rc = prof_mark(g_prof, 0, st))) return rc;
  for (int l = 0; l < NL; ++l) {
    const LayerWs& L = w.layer[l];
    if (l > 0 && (rc = drop_fwd(C, l - 1, 0, T - 1, st))) return rc;
    if ((rc = gemm_nt(layer_input(C, l), ws + L.wih, (const float*)(ws + L.bias), ws + L.xproj, C.TB, C.G, C.in_width(l), CSN_F32, CSN_F32, 0, st, C.P.opt)))
      return rc;
    F32PersistFwdArgs a{};
    a.w_hh = (const float*)(ws + L.whh);
    a.xproj = (const float*)(ws + L.xproj);
    a.gates = C.P.training ? (float*)(ws + L.gates) : nullptr;
    a.c_all = (float*)(ws + L.c_all);
    a.h_all = (float*)(ws + L.h_all);
    a.h_blk = (float*)(ws + L.h_blk_all);
    a.flags = (unsigned*)(ws + L.counters);
    a.error_flag = (unsigned*)(ws + w.status);
    a.B = B; a.T = T; a.MT_total = MTt;
    for (int m = 0; m < MTt; m += per) {
      a.mt0 = m;
      a.MT = MTt - m < per ? MTt - m : per;
      if ((rc = prof_pair(g_prof, 0, false, st))) return rc;
      if ((rc = launch_fwd_f32_persist(a, H, st))) return rc;
      if ((rc = prof_pair(g_prof, 0, true, st))) return rc;
      ++n_launch;
    }
  }
  return prof_end(C, 0, n_launch, T * NL);
}

static int backward_f32p(Call& C, const BwdArgs& A) {
  const WsLayout& w = C.w;
  Prof& g_prof = C.P.prof;
  char* ws = C.ws;
  hipStream_t st = C.st;
  const int B = C.B, T = C.T, H = C.H, NL = C.NL;
  const int64_t G = C.G;
  const int MTt = (B + 63) / 64, per = f32_persist_tiles_per_launch(H);
  int rc;
  CSN_HIP_CHECK(hipMemsetAsync(ws + w.zero_bwd, 0, w.zero_bwd_bytes, st));
  int n_launch = 0;
  if ((rc = prof_mark(g_prof, 2, st))) return rc;
  for (int l = NL - 1; l >= 0; --l) {
    const LayerWs& L = w.layer[l];
    const bool top = (l == NL - 1);
    F32PersistBwdArgs a{};
    a.w_hh_t = (const float*)(ws + L.whht);
    a.gates = (const float*)(ws + L.gates);
    a.c_all = (const float*)(ws + L.c_all);
    a.dy = top ? A.dy_tm : (const float*)(ws + w.layer[l + 1].dx);
    a.dy_last = (top && A.dy_tm == nullptr) ? A.dy_last : nullptr;
    a.zeros = (const float*)(ws + w.zeros_bh);
    a.dgates = (float*)(ws + L.dgates);
    a.dg_blk = (float*)(ws + L.dg_blk_all);
    a.bias_part = (float*)(ws + w.f32_bias_part);
    a.flags = (unsigned*)(ws + L.bflags);
    a.error_flag = (unsigned*)(ws + w.status);
    a.B = B; a.T = T; a.MT_total = MTt;
    for (int m = 0; m < MTt; m += per) {
      a.mt0 = m;
      a.MT = MTt - m < per ? MTt - m : per;
      if ((rc = prof_pair(g_prof, 1, false, st))) return rc;
      if ((rc = launch_bwd_f32_persist(a, H, st))) return rc;
      if ((rc = prof_pair(g_prof, 1, true, st))) return rc;
      ++n_launch;
    }
    // bias gradients: the row groups' partial sums in fixed order (db_ih = db_hh)
    sum_rows_kernel<<<(unsigned)((G + 255) / 256), 256, 0, st>>>((const float*)(ws + w.f32_bias_part), MTt * 4, G, A.db_ih[l], A.db_hh[l], C.P.grad_accumulate);
    CSN_LAUNCH_CHECK();
    // gradient w.r.t. this layer's input = dy of the layer below, whole sequence
    if (l > 0 && (rc = gemm_nt(ws + L.dgates, ws + L.wiht, nullptr, ws + L.dx, C.TB, H, G, CSN_F32, CSN_F32, 0, st, C.P.opt))) return rc;
    if (l > 0 && (rc = drop_bwd(C, l - 1, 0, T - 1, st))) return rc;
  }
  if ((rc = prof_end(C, 1, n_launch, T * NL))) return rc;
  for (int l = NL - 1; l >= 0; --l) {
    if ((rc = weight_grads_rm(C, A, l, false))) return rc;
    C.P.grads_ready(l);
  }
  if (A.dx) return dx_out(C, A.dx, st);
  return CSN_OK;
}

// =============================================================================================
// paths 1 - 3: bf16 fast paths, every 4H axis gate-interleaved (lstm_cell_blk.hip and the weight-stationary kernels)
// =============================================================================================
// Layout preparation of both fast forwards: time-major x, permuted / fragment-major parameters, bias sums, the zeroed
// hand-off buffers of the per-diagonal path, and layer 0's input projection unless the recurrence kernel multiplies x itself
static int prep_fast(Call& C, const FwdArgs& A) {
  const csnLstmDesc& d = C.d;
  const WsLayout& w = C.w;
  char* ws = C.ws;
  hipStream_t st = C.st;
  const int B = C.B, T = C.T, H = C.H, NL = C.NL;
  const int64_t G = C.G, TB = C.TB;
  const size_t Bpad = ((size_t)B + 63) / 64 * 64;
  int rc;
  // all layout preparation in one launch (prep_multi_kernel); a training plan with more than 6 layers has more jobs
  // than one launch holds (1 + 5 L): a full batch is launched and a new one started -- the jobs are independent
  PrepArgs pa{};
  pa.vrow = C.vrow;
  pa.vt0 = C.vt0;
  int prep_rc = CSN_OK;
  auto job = [&](int kind, const float* a_, const float* b_, void* dst, int64_t n0, int64_t n1, int64_t n2, int64_t s0,
                 int64_t s1, int64_t Hh, int pr, int pk, int64_t work) {
    if (prep_rc != CSN_OK) return;
    if (pa.njobs == kPrepMaxJobs) {
      if ((prep_rc = launch_prep_multi(pa, st)) != CSN_OK) return;
      pa.njobs = 0;
    }
    PrepJob& J = pa.job[pa.njobs++];
    J = PrepJob{kind, a_, b_, dst, n0, n1, n2, s0, s1, Hh, pr, pk, work, 0u, 0u, nullptr};
  };
  // (the two x jobs of a reverse plan: perm_r = 1 and the lengths -- each row is read backwards from its own last step)
  job(kPrepCastX, A.x, nullptr, ws + w.x_c, B, T, d.I, A.xsb, A.xst, 0, C.P.reverse, 0, TB * d.I);
  pa.job[pa.njobs - 1].len = C.dlen;
  for (int l = 0; l < NL; ++l) {
    const LayerWs& L = w.layer[l];
    const int64_t I = C.in_width(l);
    job(kPrepPermRows, A.w_ih[l], nullptr, ws + L.wih, 0, I, 0, 0, 0, H, 0, 0, G * I);
    job(kPrepBlockify, A.w_hh[l], nullptr, ws + L.whh_blk, G, H, 0, H, 1, H, 1, 0, G * H / 8);
    job(kPrepBias, A.b_ih[l], A.b_hh[l], ws + L.bias, 0, 0, 0, 0, 0, H, 0, 0, G);
    if (C.P.training) {
      job(kPrepTransPerm, A.w_ih[l], nullptr, ws + L.wiht, 0, I, 0, 0, 0, H, 0, 0, G * I);
      // W_hh^T [H rows = unit][k' = 4u'+g]: element (u, k') = W_hh[std_row(k')][u]
      job(kPrepBlockify, A.w_hh[l], nullptr, ws + L.whht_blk, H, G, 0, 1, H, H, 0, 1, H * G / 8);
    }
    if (!w.persist) {       // ping-pong hand-off buffers of the per-timestep launches
      CSN_HIP_CHECK(hipMemsetAsync(ws + L.hblk[0], 0, Bpad * H * 2, st));
      CSN_HIP_CHECK(hipMemsetAsync(ws + L.hblk[1], 0, Bpad * H * 2, st));
      // initial state (CSN_LSTM_STATE plans): bf16 h0 fragment-major into the ping-pong buffer step 0 reads, behind its
      // memset.  (weight-stationary paths: forward_persist installs the state; a stateless plan never writes slot 0,
      // csn_lstm_workspace_init zeroed it)
      if (A.h0 && (rc = launch_blockify_x(A.h0 + (size_t)l * B * H, H, 0, B, 1, H, ws + L.hblk[0], st))) return rc;
      if ((rc = install_slot0(C, l, A.h0, A.c0))) return rc;
    }
  }
  if (w.fuse_x) {
    // layer 0 multiplies x_t itself inside the weight-stationary kernel: fragment-major x and W_ih instead of
    // a [T, B, 4H] float32 projection written to and re-read from HBM
    job(kPrepBlockifyX, A.x, nullptr, ws + w.x_blk, B, T, d.I, A.xsb, A.xst, (int64_t)Bpad, C.P.reverse, 0, (int64_t)T * Bpad * d.I / 8);
    pa.job[pa.njobs - 1].len = C.dlen;
    job(kPrepBlockify, A.w_ih[0], nullptr, ws + w.wih0_blk, G, d.I, 0, d.I, 1, H, 1, 0, G * d.I / 8);
  }
  if (prep_rc != CSN_OK) return prep_rc;
  if ((rc = launch_prep_multi(pa, st))) return rc;
  if ((rc = mask_x(C, st))) return rc;
  if (!w.fuse_x) {
    // layer 0 input projection for every step, main stream
    if ((rc = gemm_nt(ws + w.x_c, ws + w.layer[0].wih, (const float*)(ws + w.layer[0].bias), ws + w.layer[0].xproj,
                      TB, G, d.I, CSN_BF16, CSN_F32, 0, st, C.P.opt)))
      return rc;
  }
  return CSN_OK;
}

// Path 1, per-diagonal cells: the WAVEFRONT of the file header, lag = 2 chunks, input projections on the side stream
static int forward_il(Call& C, const FwdArgs& A) {
  const WsLayout& w = C.w;
  char* ws = C.ws;
  hipStream_t st = C.st;
  SideCtx* sc = &C.P.sc;
  int rc;
  if ((rc = side_ctx(C.P.sc))) return rc;
  hipStream_t side = C.P.opt.no_side_stream ? st : sc->side;
  const int B = C.B, T = C.T, H = C.H, NL = C.NL;
  const int64_t G = C.G;
  const int Cz = C.Cz;
  const int training = C.P.training;
  if ((rc = prep_fast(C, A))) return rc;
  if (NL > 1 && (rc = hand_off(sc, st, side))) return rc;   // side stream sees the prepared weights

  const int nch = (T + Cz - 1) / Cz;
  std::vector<hipEvent_t> xproj_ready((size_t)NL * nch, nullptr);
  int n_launch = 0, n_cells = 0;
  if ((rc = prof_mark(C.P.prof, 0, st))) return rc;
  auto cell = [&](CellFwdProb& q, const WaveCell& s) {
    const LayerWs& L = w.layer[s.layer];
    const int t = s.t;
    q.h_prev_blk = (t == 0 && !A.h0) ? nullptr : (const bf16_t*)(ws + L.hblk[t & 1]);
    q.w_blk = (const bf16_t*)(ws + L.whh_blk);
    q.xproj = (const float*)(ws + L.xproj) + (size_t)t * B * G;
    q.c_prev = (t == 0 && !A.c0) ? nullptr : (const float*)(ws + L.c_all) + (size_t)t * B * H;
    q.gates_out = training ? (bf16_t*)(ws + L.gates) + (size_t)t * B * G : nullptr;
    q.c_out = (float*)(ws + L.c_all) + (size_t)(t + 1) * B * H;
    q.h_out = (bf16_t*)(ws + L.h_all) + (size_t)(t + 1) * B * H;
    q.h_out_blk = (bf16_t*)(ws + L.hblk[(t + 1) & 1]);
  };
  rc = wavefront_schedule(WaveIn{T, NL, Cz, WaveUnit::step, 2, false}, [&](const WaveLaunch& q) -> int {
    CellFwdArgs a{};  a.B = B; a.H = H;
    for (int i = 0; i < q.ncells; ++i) {
      const WaveCell& s = q.cell[i];      // entering a chunk: its projection has to be there
      if (s.layer > 0 && s.enters) CSN_HIP_CHECK(hipStreamWaitEvent(st, xproj_ready[(size_t)s.layer * nch + s.chunk], 0));
      cell(a.p[i], s);
    }
    if (int rc = launch_cell_fwd_il(a, q.ncells, st)) return rc;
    ++n_launch;
    n_cells += q.ncells;
    // a layer that just finished a chunk feeds the next layer's input projection (side stream)
    for (int i = 0; i < q.ndone; ++i) {
      const int l = q.done[i].layer, c = q.done[i].chunk;
      if (l + 1 == NL) continue;
      if (int rc = hand_off(sc, st, side)) return rc;
      if (int rc = xproj_chunk_gemm(C, l, c, side)) return rc;
      hipEvent_t ev;
      if (int rc = next_event(sc, &ev)) return rc;
      CSN_HIP_CHECK(hipEventRecord(ev, side));
      xproj_ready[(size_t)(l + 1) * nch + c] = ev;
    }
    return CSN_OK;
  });
  if (rc) return rc;
  return prof_end(C, 0, n_launch, n_cells);
}

// Paths 2 and 3, weight-stationary forward (lstm_fwd_persist.hip, lstm_fwd_ns.hip).
//
// Grouped form (the fast one, taken when slots * M-tiles <= 8): ONE launch per chunk diagonal advances layer
// l through chunk (dg - l) for every layer in range -- at cfg2 two layers x four 64-row M-tiles = 8 hand-off
// groups of 32 workgroups, one group per XCD under the round-robin dispatch, so a group's h hand-off stays
// inside one L2 (verified per launch by the kernel; otherwise it uses the placement-independent protocol).
// The input projection of layer l+1 for the chunk layer l just finished is a GEMM between two launches, on
// the same stream: the persistent workgroups own every CU (408 VGPRs, 100 KB LDS), nothing co-resides.
//
// Stream form (any number of layers / M-tiles): layer l runs chunk after chunk on its own stream, the GEMMs
// on the side stream, ordered by events; placement-independent hand-off.
//
// Which form a call takes and what each launch holds is fwd_persist_form / fwd_persist_schedule (lstm_schedule.h); this
// function sets up the call, then enqueues that schedule entry by entry.
static int forward_persist(Call& C, const FwdArgs& A) {
  Plan& P = C.P;
  const WsLayout& w = C.w;
  Prof& g_prof = P.prof;
  char* ws = C.ws;
  hipStream_t st = C.st;
  SideCtx* sc = &P.sc;
  int rc;
  if ((rc = side_ctx(P.sc))) return rc;
  hipStream_t side = P.opt.no_side_stream ? st : sc->side;
  const float* h0 = A.h0;
  const float* c0 = A.c0;
  const int B = C.B, T = C.T, H = C.H, NL = C.NL;
  const int Bpad = (B + 63) / 64 * 64, MT = Bpad / 64;
  const int training = P.training;
  if ((rc = prep_fast(C, A))) return rc;
  // one fill: the flag lines of every layer, the XCD agreement words
  CSN_HIP_CHECK(hipMemsetAsync(ws + w.zero_fwd, 0, w.zero_fwd_bytes, st));
  auto fill_slot = [&](PersistFwdSlot& S, const FwdSlot& s) {
    const int l = s.layer;
    const LayerWs& L = w.layer[l];
    S.w_blk = (const bf16_t*)(ws + L.whh_blk);
    S.xproj = (const float*)(ws + L.xproj);
    S.gates = training ? (bf16_t*)(ws + L.gates) : nullptr;
    S.c_all = (float*)(ws + L.c_all);
    S.h_all = (bf16_t*)(ws + L.h_all);
    S.h_blk_all = (bf16_t*)(ws + L.h_blk_all);
    S.flags = (unsigned*)(ws + L.counters);
    S.x_blk = nullptr;
    S.wih_blk = nullptr;
    S.bias = nullptr;
    S.I = 0;
    if (l == 0 && w.fuse_x) {
      S.x_blk = (const bf16_t*)(ws + w.x_blk);
      S.wih_blk = (const bf16_t*)(ws + w.wih0_blk);
      S.bias = (const float*)(ws + L.bias);
      S.I = C.d.I;
    }
    S.t0 = s.t0;
    S.nsteps = s.nsteps;
  };
  PersistFwdArgs a{};
  a.error_flag = (unsigned*)(ws + w.status);
  a.B = B; a.H = H; a.T = T; a.Bpad = Bpad; a.MT = MT;
  a.rotate = !P.opt.no_rotate;
  a.park = !P.opt.no_fwd_park;
  // (forward: no hint words by default -- the first k-block's own pieces are what the wave spins on; measured 205 -> 200 us
  // per launch; CSN_FWD_HINT restores them)
  a.data_polls = (!w.fwd_ns && !P.opt.fwd_flags) ? (P.opt.fwd_hint && !P.opt.dpoll_no_hint ? 1 : 2) : 0;
#ifdef CSN_SLAB_TAGS
  if (a.data_polls && P.opt.tags_no_rearm) a.data_polls |= 4;
#endif
  if (a.data_polls)        // the ring of 4 hand-off slabs of every layer starts as sentinel (lstm_fwd_persist.hip)
    for (int l = 0; l < NL; ++l)
      CSN_HIP_CHECK(hipMemsetAsync(ws + w.layer[l].h_blk_all, 0xff, (size_t)4 * Bpad * H * 2, st));
  // initial state: h0 fragment-major into hand-off slot 0 (behind the ring's sentinel fill) and row-major into h_all
  // slot 0 (the dW_hh GEMM), c0 into c_all slot 0 (the forward's step 0 and the backward's df_0).  A stateless forward
  // of a plan that has seen a state re-zeroes both slots 0, which it does not otherwise write.
  a.state = (h0 || c0) ? 1 : 0;
  if (a.state) P.state_seen = true;
  for (int l = 0; l < NL && P.state_seen; ++l) {
    const LayerWs& L = w.layer[l];
    if (h0) {
      if ((rc = launch_blockify_x(h0 + (size_t)l * B * H, H, 0, B, 1, H, ws + L.h_blk_all, st))) return rc;
    } else if (a.state) {
      CSN_HIP_CHECK(hipMemsetAsync(ws + L.h_blk_all, 0, (size_t)Bpad * H * 2, st));
    }
    if ((rc = install_slot0(C, l, h0, c0))) return rc;
  }
  int n_launch = 0;
  P.half_launches[0] = 0;

  auto launch_fwd = [&](const PersistFwdArgs& args, hipStream_t on) {
    return w.fwd_ns ? launch_fwd_ns(args, on) : launch_fwd_persist(args, on);
  };
  const FwdSchedIn in{T, B, H, NL, C.Cz, w.fwd_ns, P.opt.persist_streams, P.opt.no_half_tiles};
  const FwdForm form = fwd_persist_form(in);
  const std::vector<FwdLaunch> sched = fwd_persist_schedule(in);
  if (form == FwdForm::grouped) {
    const bool try_local = !P.opt.no_xcd_local;
    if ((rc = prof_mark(g_prof, 0, st))) return rc;
    a.xcd_groups = 1;
    for (const FwdLaunch& q : sched) {
      for (int i = 0; i < q.nslots; ++i) {
        fill_slot(a.slot[i], q.slot[i]);
        if (q.half) a.slot[i].flags += ((size_t)T + 1) * MT * kPersistFlagLine;      // the 32-row tiles' own lines
      }
      a.nslots = q.nslots;
      a.half_tiles = q.half ? 1 : 0;
      a.MT = q.MT;
      if (q.half) ++P.half_launches[0];
      a.agree = try_local ? (unsigned long long*)(ws + w.agree) + (size_t)q.agree * 8 : nullptr;
      if ((rc = prof_pair(g_prof, 0, false, st))) return rc;
      if ((rc = launch_fwd(a, st))) return rc;
      if ((rc = prof_pair(g_prof, 0, true, st))) return rc;
      ++n_launch;
      for (int i = 0; i < q.nslots; ++i)      // layer l finished chunk c -> xproj_{l+1}[chunk c], before the next launch
        if (q.slot[i].feeds_next && (rc = xproj_chunk_gemm(C, q.slot[i].layer, q.slot[i].chunk, st))) return rc;
    }
    return prof_end(C, 0, n_launch, T * NL);
  }

  if (form == FwdForm::caller_stream) side = st;
  hipStream_t ls[8];
  ls[0] = st;
  for (int l = 1; l < NL; ++l) {
    ls[l] = (side == st) ? st : sc->layer[l];
    if (ls[l] != st && (rc = hand_off(sc, st, ls[l]))) return rc;
  }
  if (side != st && (rc = hand_off(sc, st, side))) return rc;
  if ((rc = prof_mark(g_prof, 0, st))) return rc;
  a.nslots = 1;
  a.xcd_groups = 0;
  a.agree = nullptr;
  a.half_tiles = 0;
  a.MT = MT;
  for (const FwdLaunch& q : sched) {
    const FwdSlot& s = q.slot[0];
    const int l = s.layer;
    fill_slot(a.slot[0], s);
    if ((rc = launch_fwd(a, ls[l]))) return rc;
    ++n_launch;
    if (s.feeds_next) {
      // layer l finished chunk c -> GEMM xproj_{l+1}[chunk] on the side stream -> layer l+1 may start it
      if ((rc = hand_off(sc, ls[l], side))) return rc;
      if ((rc = xproj_chunk_gemm(C, l, s.chunk, side))) return rc;
      if (side != ls[l + 1] && (rc = hand_off(sc, side, ls[l + 1]))) return rc;
    }
  }
  // the caller's stream resumes after every layer stream (and the side stream) has drained
  for (int l = 1; l < NL; ++l)
    if (ls[l] != st && (rc = hand_off(sc, ls[l], st))) return rc;
  if (side != st && (rc = hand_off(sc, side, st))) return rc;
  return prof_end(C, 0, n_launch, T * NL);
}

// Paths 1 and 2, and path 3 where its grouped form does not apply: per-diagonal backward cells, lag = 2 chunks, the input
// gradients and the weight gradients on the side stream
static int backward_il(Call& C, const BwdArgs& A) {
  const WsLayout& w = C.w;
  char* ws = C.ws;
  hipStream_t st = C.st;
  SideCtx* sc = &C.P.sc;
  int rc;
  if ((rc = side_ctx(C.P.sc))) return rc;
  hipStream_t side = C.P.opt.no_side_stream ? st : sc->side;
  const int B = C.B, T = C.T, H = C.H, NL = C.NL;
  const int64_t G = C.G;
  const size_t Bpad = ((size_t)B + 63) / 64 * 64;
  const int Cz = C.Cz;
  const int nch = (T + Cz - 1) / Cz;
  const bool state = C.P.state != 0;

  for (int l = 0; l < NL; ++l) {
    const LayerWs& L = w.layer[l];
    if ((rc = seed_dc_carry(C, l, A.dc_n, false))) return rc;
    CSN_HIP_CHECK(hipMemsetAsync(ws + L.dgblk[0], 0, Bpad * G * 2, st));
    CSN_HIP_CHECK(hipMemsetAsync(ws + L.dgblk[1], 0, Bpad * G * 2, st));
  }
  if ((rc = hand_off(sc, st, side))) return rc;

  std::vector<hipEvent_t> dx_ready((size_t)NL * nch, nullptr);
  int n_launch = 0, n_cells = 0;
  if ((rc = prof_mark(C.P.prof, 2, st))) return rc;
  auto cell = [&](CellBwdProb& q, const WaveCell& s) {
    const int l = s.layer, t = s.t;
    const LayerWs& L = w.layer[l];
    q.dg_next_blk = (t == T - 1) ? nullptr : (const bf16_t*)(ws + L.dgblk[(t + 1) & 1]);
    q.wt_blk = (const bf16_t*)(ws + L.whht_blk);
    if (l == NL - 1) {
      q.dy = A.dy_tm ? A.dy_tm + (size_t)t * B * H : (t == T - 1 ? A.dy_last : nullptr);
    } else {
      q.dy = (const float*)(ws + w.layer[l + 1].dx) + (size_t)t * B * H;
    }
    q.dy_ld = H;
    q.gates = (const bf16_t*)(ws + L.gates) + (size_t)t * B * G;
    q.c = (const float*)(ws + L.c_all) + (size_t)(t + 1) * B * H;
    // (a CSN_LSTM_STATE plan reads c_all slot 0 at t = 0: c0, or the zeros its forward wrote there)
    q.c_prev = (t == 0 && !state) ? nullptr : (const float*)(ws + L.c_all) + (size_t)t * B * H;
    q.dc_carry = (float*)(ws + L.dc_carry);
    q.dg_out = (bf16_t*)(ws + L.dgates) + (size_t)t * B * G;
    q.dg_out_blk = (bf16_t*)(ws + L.dgblk[t & 1]);
  };
  rc = wavefront_schedule(WaveIn{T, NL, Cz, WaveUnit::step, 2, true}, [&](const WaveLaunch& q) -> int {
    CellBwdArgs a{};  a.B = B; a.H = H;
    CellMask mask{C.dlen, {0, 0, 0, 0}};
    for (int i = 0; i < q.ncells; ++i) {
      const WaveCell& s = q.cell[i];      // entering a chunk: its dy (the dx of the layer above) has to be there
      mask.t[i] = s.t;
      if (s.layer < NL - 1 && s.enters) CSN_HIP_CHECK(hipStreamWaitEvent(st, dx_ready[(size_t)(s.layer + 1) * nch + s.chunk], 0));
      cell(a.p[i], s);
    }
    if (int rc = launch_cell_bwd_il(a, q.ncells, st, C.dlen ? &mask : nullptr)) return rc;
    ++n_launch;
    n_cells += q.ncells;
    for (int i = 0; i < q.ndone; ++i) {
      const int l = q.done[i].layer, cr = q.done[i].chunk;
      const bool last = q.done[i].last;
      if (l > 0 || last)
        if (int rc = hand_off(sc, st, side)) return rc;
      if (l > 0) {
        if (int rc = dx_chunk_gemm(C, l, cr, A.dh_n, side)) return rc;
        hipEvent_t ev;
        if (int rc = next_event(sc, &ev)) return rc;
        CSN_HIP_CHECK(hipEventRecord(ev, side));
        dx_ready[(size_t)l * nch + cr] = ev;
      } else if (last && A.dx != nullptr) {
        if (int rc = dx_out(C, A.dx, side)) return rc;
      }
      // the weight gradients of a layer follow on the side stream once its recurrence is complete
      if (last)
        if (int rc = weight_grads_blk(C, A, l, side)) return rc;
    }
    return CSN_OK;
  });
  if (rc) return rc;
  if ((rc = prof_end(C, 1, n_launch, n_cells))) return rc;
  if ((rc = hand_off(sc, side, st))) return rc;   // the caller's stream resumes after all side-stream work
  // (the weight gradients of this path run on the side stream: only now are they ordered before the caller's stream)
  for (int l = NL - 1; l >= 0; --l) C.P.grads_ready(l);
  return CSN_OK;
}

// Path 3, weight-stationary backward recurrence (lstm_bwd_persist.hip), grouped form: ONE launch per chunk diagonal
// walks every layer in range backwards through one chunk.  The input gradient of a layer's chunk
// (dx_l = dgates_l W_ih, the dy of the layer below) is a GEMM, and it runs INSIDE the next launch: the backward
// kernel's groups occupy 24 of the 32 CUs of their XCD (24 slices of 32 units at H = 768), so the launch is
// widened to 32 workgroups per XCD and the 8 extra ones (plus all workgroups of XCDs without a group) walk
// the GEMM's tiles (gemm_beside.h).  Both of the GEMM's dependencies are then kernel boundaries: its input was
// written by the launch before, its output is read by the launch after -- for which the layer below lags TWO
// chunks: diagonal dg holds layer l at reverse chunk dg - 2 (L-1-l).  (A GEMM kernel on a second stream beside
// the launch was measured too: the event waits between the streams cost ~30 us per launch, most of the gain.)
// CSN_NO_BESIDE: lag one chunk, GEMM between two launches.
// The weight / bias gradients follow once the recurrence is complete.
//
// What each launch holds, which diagonals merge and what follows a launch on the stream is bwd_persist_schedule
// (lstm_schedule.h); this function sets up the call, then enqueues that schedule entry by entry.
static int backward_persist(Call& C, const BwdArgs& A) {
  Plan& P = C.P;
  const WsLayout& w = C.w;
  Prof& g_prof = P.prof;
  char* ws = C.ws;
  hipStream_t st = C.st;
  const float* dh_n = A.dh_n;
  const int B = C.B, T = C.T, H = C.H, NL = C.NL;
  const int64_t G = C.G;
  const int Bpad = (B + 63) / 64 * 64, MT = Bpad / 64;
  const int Cz = C.Cz;
  int rc;
  // one fill: carried dc and flag lines of every layer, the XCD agreement words (zeros_bh: csn_lstm_workspace_init)
  CSN_HIP_CHECK(hipMemsetAsync(ws + w.zero_bwd, 0, w.zero_bwd_bytes, st));
  // (the kernel reads the carried dc at launch start and writes it back at launch end, so after the last launch it holds
  // the gradient w.r.t. c0)
  for (int l = 0; l < NL; ++l)
    if ((rc = seed_dc_carry(C, l, A.dc_n, true))) return rc;
  const bool try_local = !P.opt.no_xcd_local;

  PersistBwdArgs a{};
  a.error_flag = (unsigned*)(ws + w.status);
  a.B = B; a.H = H; a.T = T; a.Bpad = Bpad; a.MT = MT;
  a.xcd_groups = 1;
  a.grid_slices = 32;
  a.beside_narrow = P.opt.beside_128 ? 1 : 0;
  a.rotate = !P.opt.no_rotate;
  a.data_polls = P.opt.bwd_flags ? 0 : (P.opt.dpoll_no_hint ? 2 : 1);
#ifdef CSN_SLAB_TAGS
  if (a.data_polls && P.opt.tags_no_rearm) a.data_polls |= 4;
#endif
  a.chunk = Cz;
  a.cnt = (unsigned*)(ws + w.merge_cnt);     // merged launches: rec_done[NL][nch], then gemm_done[NL][nch]
  P.dgates_copies = 2;     // hand-off slabs + the row-major copy the GEMMs read (csn_lstm_plan_dgates_copies)
  if (a.data_polls)        // the ring of 4 hand-off slabs of every layer starts as sentinel
    for (int l = 0; l < NL; ++l) CSN_HIP_CHECK(hipMemsetAsync(ws + w.layer[l].dg_blk_all, 0xff, (size_t)4 * Bpad * G * 2, st));
  int n_launch = 0;
  P.half_launches[1] = 0;
  P.bwd_launches[0] = P.bwd_launches[1] = 0;

  const std::vector<BwdLaunch> sched =
      bwd_persist_schedule(BwdSchedIn{T, B, H, NL, Cz, C.dlen != nullptr, drop_on(C), dh_n != nullptr, a.data_polls != 0,
                                      P.opt.no_beside, P.opt.bwd_no_merge, P.opt.no_half_tiles});
  auto beside_gemm = [&](const BwdGemm& g) {
    const LayerWs& L = w.layer[g.layer];
    return BesideGemm{(const bf16_t*)(ws + L.dgates) + (size_t)g.t_lo * B * G, (const bf16_t*)(ws + L.wiht),
                      (float*)(ws + L.dx) + (size_t)g.t_lo * B * H, (g.t_hi - g.t_lo + 1) * B, H, (int)G};
  };
  // what follows GEMM g on the stream: the dropout mask of its steps, then the gradient w.r.t. h_n of the layer below
  auto mask = [&](const BwdGemm& g) -> int { return g.mask ? drop_bwd(C, g.layer - 1, g.t_lo, g.t_hi, st) : CSN_OK; };
  auto add_dh_n = [&](const BwdGemm& g) -> int {
    if (!g.add) return CSN_OK;
    return add_dh_n_rows(C, dh_n + (size_t)(g.layer - 1) * B * H, (float*)(ws + w.layer[g.layer].dx), g.t_lo, g.t_hi, st);
  };
  if ((rc = prof_mark(g_prof, 2, st))) return rc;
  for (const BwdLaunch& q : sched) {
    if (q.nslots == 0) {      // no layer in range: the GEMMs the previous launch left behind, stand-alone
      for (int i = 0; i < q.ngemm; ++i) {
        const BesideGemm g = beside_gemm(q.gemm[i]);
        if ((rc = gemm_nt(g.A, g.Bt, nullptr, g.C, g.M, g.N, g.K, CSN_BF16, CSN_F32, 0, st, P.opt))) return rc;
        if ((rc = mask(q.gemm[i]))) return rc;
        if ((rc = add_dh_n(q.gemm[i]))) return rc;
      }
      continue;
    }
    for (int i = 0; i < q.nslots; ++i) {
      const BwdSlot& s = q.slot[i];
      const LayerWs& L = w.layer[s.layer];
      PersistBwdSlot& S = a.slot[i];
      S.wt_blk = (const bf16_t*)(ws + L.whht_blk);
      S.gates = (const bf16_t*)(ws + L.gates);
      S.c_all = (const float*)(ws + L.c_all);
      if (s.layer == NL - 1) {
        S.dy = A.dy_tm;
        S.dy_last = A.dy_tm ? nullptr : A.dy_last;
      } else {
        S.dy = (const float*)(ws + w.layer[s.layer + 1].dx);
        S.dy_last = nullptr;
      }
      S.zeros = (const float*)(ws + w.zeros_bh);
      S.dc_carry = (float*)(ws + L.dc_carry);
      S.dgates = (bf16_t*)(ws + L.dgates);
      S.dg_blk_all = (bf16_t*)(ws + L.dg_blk_all);
      S.flags = (unsigned*)(ws + L.bflags);
      if (q.half) S.flags += (size_t)T * MT * kPersistFlagLine;      // the 32-row tiles' own lines
      S.t_hi = s.t_hi;
      S.nsteps = s.nsteps;
      S.cnt_pub = s.cnt_pub;
      S.cnt_wait = s.cnt_wait;
    }
    a.nslots = q.nslots;
    a.ngemm = q.ngemm;
    for (int i = 0; i < q.ngemm; ++i) a.gemm[i] = beside_gemm(q.gemm[i]);
    a.nrounds = q.nrounds;
    if (q.nrounds > 1) {
      CSN_REQUIRE(q.nslots == NL && q.ngemm == NL - 1, "backward_persist: merged launch without every layer");
      for (int i = 0; i < q.ngemm; ++i) CSN_REQUIRE(a.gemm[i].M == Cz * B, "backward_persist: merged launch with a short GEMM");
      a.wk_wait = q.wk_wait;
      a.wk_pub = q.wk_pub;
      a.wk_stride = q.wk_stride;
      for (int i = 1; i + 1 < q.nslots; ++i)
        CSN_REQUIRE(q.slot[i].cnt_pub == q.slot[0].cnt_pub - i * q.wk_stride && q.slot[i + 1].cnt_wait == q.slot[1].cnt_wait - i * q.wk_stride,
                    "backward_persist: merged launch whose counters are not evenly spaced");
      P.bwd_launches[1] = q.nrounds;
    }
    a.half_tiles = q.half ? 1 : 0;
    a.MT = q.MT;
    if (q.half) P.half_launches[1] += q.nrounds;      // (a merged launch: once per diagonal it covers)
    a.agree = try_local ? (unsigned long long*)(ws + w.agree_b) + (size_t)q.agree * 8 : nullptr;
    if ((rc = prof_pair(g_prof, 1, false, st))) return rc;
    if ((rc = launch_bwd_persist(a, st, C.dlen))) return rc;
    if ((rc = prof_pair(g_prof, 1, true, st))) return rc;
    ++n_launch;
    for (int i = 0; i < q.ngemm; ++i)
      if ((rc = mask(q.gemm[i]))) return rc;
    for (int i = 0; i < q.ngemm; ++i)
      if ((rc = add_dh_n(q.gemm[i]))) return rc;
    for (int i = 0; q.inline_gemms && i < q.nslots; ++i)
      if (q.slot[i].layer > 0 && (rc = dx_chunk_gemm(C, q.slot[i].layer, q.slot[i].chunk, dh_n, st))) return rc;
  }
  P.bwd_launches[0] = n_launch;
  if ((rc = prof_end(C, 1, n_launch, T * NL))) return rc;

  if (A.dx != nullptr && (rc = dx_out(C, A.dx, st))) return rc;
  // (every recurrence launch has been enqueued by now: what a gradient-ready callback starts -- a collective on another
  // stream -- runs beside the remaining layers' weight-gradient GEMMs, never beside a one-workgroup-per-CU launch)
  for (int l = NL - 1; l >= 0; --l) {
    if ((rc = weight_grads_blk(C, A, l, st))) return rc;
    P.grads_ready(l);
  }
  return CSN_OK;
}

// =============================================================================================
// the path of a call (csn_lstm_plan_path: the forward of paths 2 and 3 is one, the backward of path 3 falls back to that of
// paths 1 and 2 where its grouped form does not apply)
static int run_forward(Call& C, const FwdArgs& A) {
  if (C.P.resident) return forward_resident(C, A);
  if (C.w.persist) return forward_persist(C, A);
  if (C.w.il) return forward_il(C, A);
  if (C.w.f32_persist) return forward_f32p(C, A);
  return forward_v1(C, A);
}
static int run_backward(Call& C, const BwdArgs& A) {
  C.P.bwd_launches[0] = C.P.bwd_launches[1] = 0;     // (only the weight-stationary backward counts them)
  if (C.P.resident) return backward_resident(C, A);
  if (bwd_grouped(&C.P, C.T)) return backward_persist(C, A);
  if (C.w.il) return backward_il(C, A);
  if (C.w.f32_persist) return backward_f32p(C, A);
  return backward_v1(C, A);
}

// state arguments ([L,B,H] float32): only on a CSN_LSTM_STATE plan, 16-B aligned (read / written as float4)
static int check_state_args(const Plan& P, const char* fn, const void* const* ptrs, const char* const* names, int n) {
  for (int i = 0; i < n; ++i) {
    if (ptrs[i] == nullptr) continue;
    CSN_REQUIRE(P.state, "%s: %s given, but the plan was created without CSN_LSTM_STATE", fn, names[i]);
    CSN_REQUIRE((reinterpret_cast<uintptr_t>(ptrs[i]) & 15) == 0, "%s: %s must be 16-B aligned", fn, names[i]);
  }
  return CSN_OK;
}

// ---- what a forward hands back, out of the saved states (slot n of h_all / c_all is a row's state after its n steps: its
// final state, and slot 0 the initial one, which is all a call whose rows are all empty reads)
static const OutDropCfg* out_drop_of(const Call& C, OutDropCfg& od) {      // csn_lstm_plan_set_output_dropout, or null
  od = C.P.out_drop();
  return C.P.out_drop_p > 0.f ? &od : nullptr;
}
static int emit_state(const Call& C, int l, float* h_n, float* c_n) {
  const LayerWs& L = C.w.layer[l];
  const size_t at = (size_t)l * C.B * C.H;
  if (h_n)
    if (int rc = launch_gather_state(C.ws + L.h_all, C.dt, C.dlen, C.T, h_n + at, C.B, C.H, C.st)) return rc;
  if (c_n) return launch_gather_state(C.ws + L.c_all, CSN_F32, C.dlen, C.T, c_n + at, C.B, C.H, C.st);
  return CSN_OK;
}
// the attention readout's arrays of this call: the caller's attn_out / dscore_out where given, else plan-owned like the rest
static int attn_args(const Call& C, AttnArgs& A) {
  Plan& P = C.P;
  const size_t BT = (size_t)C.B * C.T_full, r8 = (BT * 8 + 255) / 256 * 256, r4 = (BT * 4 + 255) / 256 * 256;
  if (P.attn_dev == nullptr) CSN_HIP_CHECK(hipMalloc((void**)&P.attn_dev, 2 * r8 + 2 * r4 + (size_t)kAttnDqParts * C.H * 8));
  char* p = P.attn_dev;
  A.q = P.attn_q;
  A.scale = P.attn_scale;
  A.a64 = (double*)p;
  A.g64 = (double*)(p + r8);
  A.a32 = P.attn_out ? P.attn_out : (float*)(p + 2 * r8);
  A.w32 = P.attn_dscore ? P.attn_dscore : (float*)(p + 2 * r8 + r4);
  A.dq_part = (double*)(p + 2 * r8 + 2 * r4);
  return CSN_OK;
}
static int emit_y_last(const Call& C, float* y_last) {
  if (C.P.attn_q != nullptr) {
    AttnArgs A;
    if (int rc = attn_args(C, A)) return rc;
    return launch_attn_forward(C.ws + C.w.layer[C.NL - 1].h_all, C.dt, A, y_last, row_map(C, C.H, 0), C.st);
  }
  if (C.P.readout != CSN_READOUT_LAST)
    return launch_pool_readout(C.ws + C.w.layer[C.NL - 1].h_all, C.dt, C.P.readout, y_last, row_map(C, C.H, 0), C.st);
  return launch_gather_state(C.ws + C.w.layer[C.NL - 1].h_all, C.dt, C.dlen, C.T, y_last, C.B, C.H, C.st);
}
static int emit_y_all(const Call& C, float* y_all) {
  OutDropCfg od;
  return launch_y_out(C.ws + C.w.layer[C.NL - 1].h_all, C.dt, y_all, row_map(C, C.H, C.P.y_pitch), out_drop_of(C, od), C.st);
}

extern "C" int csn_lstm_forward(csnLstmPlan* Pp, const float* x, int64_t x_stride_b, int64_t x_stride_t,
                                const float* const* w_ih, const float* const* w_hh, const float* const* b_ih,
                                const float* const* b_hh, const float* h0, const float* c0, void* workspace,
                                float* y_last, float* y_all, float* h_n, float* c_n, csnStream_t stream) {
  CSN_REQUIRE(Pp != nullptr, "csn_lstm_forward: null plan");
  Plan& P = *Pp;
  const csnLstmDesc* d = &P.d;
  CSN_REQUIRE(x && w_ih && w_hh && b_ih && b_hh && workspace, "csn_lstm_forward: null pointer");
  CSN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "csn_lstm_forward: workspace must be 256-B aligned");
  CSN_REQUIRE(y_last || y_all || h_n || c_n, "csn_lstm_forward: no output requested");
  CSN_REQUIRE(P.out_drop_p == 0.f || (reinterpret_cast<uintptr_t>(y_all) & 15) == 0,
              "csn_lstm_forward: y_all must be 16-B aligned under csn_lstm_plan_set_output_dropout");
  {
    const void* ptrs[4] = {h0, c0, h_n, c_n};
    const char* names[4] = {"h0", "c0", "h_n", "c_n"};
    if (int rc = check_state_args(P, "csn_lstm_forward", ptrs, names, 4)) return rc;
  }
  for (int l = 0; l < d->L; ++l)
    CSN_REQUIRE(w_ih[l] && w_hh[l] && b_ih[l] && b_hh[l], "csn_lstm_forward: null parameter pointer, layer %d", l);
  int dev = -1;
  CSN_HIP_CHECK(hipGetDevice(&dev));
  CSN_REQUIRE(dev == P.device, "csn_lstm_forward: plan was created on device %d, current device is %d", P.device, dev);
  // input windows: every row's window lies inside the source (checked per call -- the lengths may be newer than the views)
  for (int b = 0; b < d->B && !P.view_row.empty(); ++b) {
    const int n = P.lengths.empty() ? d->T : P.lengths[b];
    CSN_REQUIRE((int64_t)P.view_t0[b] + n <= P.view_src_T,
                "csn_lstm_forward: the window of row %d, steps [%d, %d), ends past the source's %d steps", b,
                (int)P.view_t0[b], (int)P.view_t0[b] + n, P.view_src_T);
  }
  hipStream_t st = as_stream(stream);
  int rc;
  // (the status word is NOT cleared here: it stays raised from the first timed-out hand-off until
  // csn_lstm_status_clear, so a check at the end of an epoch / a timed region covers every step in it)
  const int* dlen = nullptr;
  if ((rc = upload_lengths(Pp, st, &dlen))) return rc;
  Call C(P, workspace, st, dlen);
  if ((rc = upload_views(Pp, st, &C.vrow, &C.vt0))) return rc;
  const FwdArgs A{x, x_stride_b, x_stride_t, w_ih, w_hh, b_ih, b_hh, h0, c0};
  // Every path runs its kernels over steps 0 .. C.T - 1 of ALL rows (with lengths: the longest row's, short rows run on
  // over zeroed padding), then each row's results are selected
  if (C.T > 0) {
    if ((rc = run_forward(C, A))) return rc;
  } else {
    // every row is empty: no recurrence launch; slot 0 (the initial state) is all the gathers below read
    for (int l = 0; l < d->L; ++l)
      if ((rc = install_slot0(C, l, h0, c0))) return rc;
    if (h0 || c0) P.state_seen = true;      // (slot 0 is no longer the zeros csn_lstm_workspace_init left)
    P.prof.have[0] = false;
  }
  for (int l = 0; l < d->L && (h_n || c_n); ++l)
    if ((rc = emit_state(C, l, h_n, c_n))) return rc;
  if (y_last && (rc = emit_y_last(C, y_last))) return rc;
  if (y_all && (rc = emit_y_all(C, y_all))) return rc;
  return CSN_OK;
}

// ---- the gradient w.r.t. the top layer's outputs as the paths take it: A.dy_tm, dense and time-major in the workspace
// (dy_all, zero over the padding; then dy_last and the top layer's dh_n added at each row's last step, in this order), or,
// for a call without lengths and without dy_all, A.dy_last alone: no T B H buffer is filled
static int assemble_top_dy(const Call& C, BwdArgs& A, const float* dy_all) {
  float* buf = (float*)(C.ws + C.w.dy_tm);
  const size_t BH = (size_t)C.B * C.H;
  const float* dh_top = A.dh_n ? A.dh_n + (C.NL - 1) * BH : nullptr;
  int rc;
  if (A.dy_last && (C.P.attn_q != nullptr || C.P.readout != CSN_READOUT_LAST)) {
    // the pooled readout: dy_last reaches every valid step (MEAN) or the first maximum (MAX, found again in the saved h),
    // inside the layout pass; then the top layer's dh_n at each row's end, as below
    PoolIn pool{C.P.readout, A.dy_last, nullptr, nullptr, nullptr, nullptr};
    const RowMap m = row_map(C, C.H, C.P.dy_pitch);
    if (C.P.attn_q != nullptr) {
      // the attention readout: the weights are computed again from the saved h and q, with the score gradients and dq
      // (all of it in front of the recurrence: dq is complete when the first gradient-ready callback fires)
      AttnArgs at;
      if ((rc = attn_args(C, at))) return rc;
      if ((rc = launch_attn_backward(C.ws + C.w.layer[C.NL - 1].h_all, C.dt, at, A.dy_last, C.P.attn_dq, C.P.grad_accumulate, m, C.st))) return rc;
      pool = PoolIn{kPoolAttention, A.dy_last, nullptr, at.a32, at.w32, at.q};
    } else if (pool.mode == CSN_READOUT_MAX) {
      if (C.P.argmax_dev == nullptr) CSN_HIP_CHECK(hipMalloc((void**)&C.P.argmax_dev, BH * 4));
      if ((rc = launch_pool_argmax(C.ws + C.w.layer[C.NL - 1].h_all, C.dt, C.P.argmax_dev, m, C.st))) return rc;
      pool.argmax = C.P.argmax_dev;
    }
    OutDropCfg od;
    if ((rc = launch_dy_in(dy_all, buf, m, out_drop_of(C, od), &pool, C.st))) return rc;
    if (dh_top && (rc = launch_add_at_end(dh_top, buf, C.dlen, C.T, 0, C.T - 1, C.B, C.H, C.st))) return rc;
    A.dy_last = nullptr;
    A.dy_tm = buf;
  } else if (dy_all || C.dlen) {
    OutDropCfg od;
    if ((rc = launch_dy_in(dy_all, buf, row_map(C, C.H, C.P.dy_pitch), out_drop_of(C, od), nullptr, C.st))) return rc;
    if (A.dy_last && (rc = launch_add_at_end(A.dy_last, buf, C.dlen, C.T, 0, C.T - 1, C.B, C.H, C.st))) return rc;
    if (dh_top && (rc = launch_add_at_end(dh_top, buf, C.dlen, C.T, 0, C.T - 1, C.B, C.H, C.st))) return rc;
    A.dy_last = nullptr;
    A.dy_tm = buf;
  } else if (dh_top && A.dy_last) {
    // (dy_last is caller memory: the sum goes into a workspace copy of it, one step at the front of the unused dy_tm region)
    CSN_HIP_CHECK(hipMemcpyAsync(buf, A.dy_last, BH * 4, hipMemcpyDeviceToDevice, C.st));
    if ((rc = launch_add_at_end(dh_top, buf, nullptr, 1, 0, 0, C.B, C.H, C.st))) return rc;
    A.dy_last = buf;
  } else if (dh_top) {
    A.dy_last = dh_top;
  }
  return CSN_OK;
}
// every row is empty: no recurrence, no parameter contribution
static int backward_all_empty(const Call& C, const BwdArgs& A) {
  Plan& P = C.P;
  if (A.dx && !P.dx_add) CSN_HIP_CHECK(hipMemsetAsync(A.dx, 0, (size_t)C.T_full * C.B * C.d.I * 4, C.st));
  for (int l = C.NL - 1; l >= 0; --l) {
    if (!P.grad_accumulate) {
      CSN_HIP_CHECK(hipMemsetAsync(A.dw_ih[l], 0, (size_t)(C.G * C.in_width(l)) * 4, C.st));
      CSN_HIP_CHECK(hipMemsetAsync(A.dw_hh[l], 0, (size_t)(C.G * C.H) * 4, C.st));
      CSN_HIP_CHECK(hipMemsetAsync(A.db_ih[l], 0, (size_t)C.G * 4, C.st));
      CSN_HIP_CHECK(hipMemsetAsync(A.db_hh[l], 0, (size_t)C.G * 4, C.st));
    }
    P.grads_ready(l);
  }
  P.prof.have[1] = false;
  return CSN_OK;
}

extern "C" int csn_lstm_backward(csnLstmPlan* Pp, const float* dy_last, const float* dy_all, const float* dh_n,
                                 const float* dc_n, void* workspace, float* const* dw_ih, float* const* dw_hh,
                                 float* const* db_ih, float* const* db_hh, float* dx, float* dh0, float* dc0,
                                 csnStream_t stream) {
  CSN_REQUIRE(Pp != nullptr, "csn_lstm_backward: null plan");
  Plan& P = *Pp;
  const csnLstmDesc* d = &P.d;
  CSN_REQUIRE(P.training, "csn_lstm_backward: the plan was created with training = 0");
  CSN_REQUIRE(workspace && dw_ih && dw_hh && db_ih && db_hh, "csn_lstm_backward: null pointer");
  CSN_REQUIRE(dy_last || dy_all || dh_n || dc_n, "csn_lstm_backward: no incoming gradient");
  CSN_REQUIRE(P.out_drop_p == 0.f || (reinterpret_cast<uintptr_t>(dy_all) & 15) == 0,
              "csn_lstm_backward: dy_all must be 16-B aligned under csn_lstm_plan_set_output_dropout");
  {
    const void* ptrs[4] = {dh_n, dc_n, dh0, dc0};
    const char* names[4] = {"dh_n", "dc_n", "dh0", "dc0"};
    if (int rc = check_state_args(P, "csn_lstm_backward", ptrs, names, 4)) return rc;
  }
  for (int l = 0; l < d->L; ++l) {
    CSN_REQUIRE(dw_ih[l] && dw_hh[l] && db_ih[l] && db_hh[l], "csn_lstm_backward: null gradient pointer, layer %d", l);
    // (accumulating, one buffer for both biases would receive the sum twice)
    CSN_REQUIRE(!P.grad_accumulate || db_ih[l] != db_hh[l],
                "csn_lstm_backward: db_ih and db_hh of layer %d are one buffer under CSN_GRAD_ACCUMULATE", l);
  }
  int dev = -1;
  CSN_HIP_CHECK(hipGetDevice(&dev));
  CSN_REQUIRE(dev == P.device, "csn_lstm_backward: plan was created on device %d, current device is %d", P.device, dev);
  hipStream_t st = as_stream(stream);
  int rc;
  const int* dlen = nullptr;
  if ((rc = upload_lengths(Pp, st, &dlen))) return rc;
  Call C(P, workspace, st, dlen);
  BwdArgs A{dy_last, nullptr, dh_n, dc_n, dw_ih, dw_hh, db_ih, db_hh, dx};
  const size_t BH = (size_t)C.B * C.H;
  // (the attention readout without a dy_last, or with every row empty: nothing reaches the query, and the weights are zero)
  if (P.attn_q != nullptr && (dy_last == nullptr || C.T == 0)) {
    const size_t BT = (size_t)C.B * C.T_full;
    if (P.attn_dq && !P.grad_accumulate) CSN_HIP_CHECK(hipMemsetAsync(P.attn_dq, 0, (size_t)C.H * 4, st));
    if (dy_last && P.attn_out) CSN_HIP_CHECK(hipMemsetAsync(P.attn_out, 0, BT * 4, st));
    if (dy_last && P.attn_dscore) CSN_HIP_CHECK(hipMemsetAsync(P.attn_dscore, 0, BT * 4, st));
  }
  if (C.T > 0) {
    if ((rc = assemble_top_dy(C, A, dy_all))) return rc;
    if ((rc = run_backward(C, A))) return rc;
  } else if ((rc = backward_all_empty(C, A))) {
    return rc;
  }
  // gradients w.r.t. the initial state (CSN_LSTM_STATE plans only: paths 0 and 1, everything on `stream` by now)
  for (int l = 0; l < C.NL && (dh0 || dc0); ++l) {
    if (dh0) {
      float* out = dh0 + l * BH;
      if (C.T > 0) {
        if ((rc = launch_dh0(C, l, out))) return rc;
      } else {
        CSN_HIP_CHECK(hipMemsetAsync(out, 0, BH * 4, st));
      }
      // an empty row's dgates are zero at step 0: its dh0 is the gradient w.r.t. its h_n
      if (dlen && dh_n && (rc = launch_add_rows_len0(dh_n + l * BH, out, dlen, C.B, C.H, st))) return rc;
      // ... and y_last of an empty row is h_n of the top layer, that is its h0: dy_last reaches dh0 there (a pooled
      // readout of an empty row is zero instead)
      if (dlen && dy_last && P.readout == CSN_READOUT_LAST && P.attn_q == nullptr && l == C.NL - 1 && (rc = launch_add_rows_len0(dy_last, out, dlen, C.B, C.H, st))) return rc;
    }
    if (dc0) {
      // the carried dc (an empty row's passed every masked step as it was); without a step, dc_n itself
      if (C.T > 0)
        CSN_HIP_CHECK(hipMemcpyAsync(dc0 + l * BH, C.ws + C.w.layer[l].dc_carry, BH * 4, hipMemcpyDeviceToDevice, st));
      else if (dc_n)
        CSN_HIP_CHECK(hipMemcpyAsync(dc0 + l * BH, dc_n + l * BH, BH * 4, hipMemcpyDeviceToDevice, st));
      else
        CSN_HIP_CHECK(hipMemsetAsync(dc0 + l * BH, 0, BH * 4, st));
    }
  }
  return CSN_OK;
}
