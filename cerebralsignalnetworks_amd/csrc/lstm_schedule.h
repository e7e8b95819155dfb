// Launch schedules of the LSTM host paths (lstm.hip) as pure functions of (T, B, H, L, chunk) and a few booleans.
// Weight-stationary paths (forward_persist / backward_persist): which (layer, chunk) cells a launch holds, which
// input-gradient GEMMs ride in it, its tile height, which diagonals merge into one launch and which counter words that
// launch uses.  Per-diagonal and CU-resident paths (the _v1, _il and _resident pairs): the layer wavefront -- which cells a
// launch holds, which launch closes its diagonal and which chunks the diagonal finished.  The host functions build a
// schedule and enqueue it entry by entry.  Standard headers only, no HIP, no workspace pointers: a host-only program
// includes this file and prints what the library runs (tests/lstm_schedule_probe.py).
#pragma once
#include <vector>

namespace csn {

// chunk c of the sequence: steps [t0, t0 + nsteps).  The backward walks the chunks from the end: its reverse chunk c
// covers the steps [t_hi - nsteps + 1, t_hi] with t_hi = T - 1 - t0.
struct Chunk { int t0, nsteps; };
inline Chunk chunk_at(int T, int chunk, int c) {
  const int t0 = c * chunk;
  return Chunk{t0, t0 + chunk <= T ? chunk : T - t0};
}
// is step (or reverse step) t the last one of its chunk?
inline bool ends_chunk(int T, int chunk, int t) { return (t + 1) % chunk == 0 || t == T - 1; }

// workgroups per hand-off group of the three weight-stationary recurrence kernels
inline int fwd_persist_slices(int H) { return H / (4 * ((H % 24 == 0) ? 6 : 8)); }
inline int fwd_ns_slices(int H) { return H / 32; }
inline int bwd_persist_slices(int H) { return H / 32; }

// does a backward over `steps` steps take the grouped weight-stationary form?  (a call passes the steps it runs -- with
// lengths the longest row --, csn_lstm_plan_kernel_name the plan's T)
inline bool bwd_grouped(bool persist_bwd, int B, int L, int steps, int chunk, bool persist_streams) {
  if (!persist_bwd) return false;
  const int MTg = (B + 63) / 64, nchg = (steps + chunk - 1) / chunk;
  const int slots = L < nchg ? L : nchg;
  return slots <= 4 && slots * MTg <= 8 && !persist_streams;
}

// ---- layer wavefront of the per-diagonal and CU-resident paths (0, 1, 5 and the backward_il fall-back of 2 / 3) ------------
// One machine, six drivers.  The layers advance as a wavefront: diagonal dg holds the i-th layer (forward: counted from
// the bottom, backward: from the top) at unit dg - lag * i, a unit being a step (the _v1 and _il pairs) or a whole chunk
// (the _resident pair), and a layer that finished a chunk is followed by a chunk job (forward: the input projection of
// the layer above, backward: the input gradient = dy of the layer below) that the next layer's entry into that chunk
// needs -- hence the lag, in chunks: 1 where the job runs on the caller's stream in front of the next diagonal (_v1,
// _resident), 2 where it runs on the side stream beside the next chunk (_il).
enum class WaveUnit { step, chunk };
constexpr int kWaveMaxLayers = 8;       // (csn_lstm_plan_create takes L <= 8)
struct WaveIn { int T, L, chunk; WaveUnit unit; int lag; bool backward; };      // T: the steps this call runs; lag in chunks
struct WaveCell {
  int layer, chunk;           // backward: the reverse chunk
  int t, nsteps;              // forward: the steps [t, t + nsteps); backward: t, t - 1, ..., t - nsteps + 1 (t = BwdSlot's t_hi)
  bool enters, ends;          // the first / the last unit of its chunk (ends_chunk); both always for whole-chunk units
  bool last;                  // ... and the last of its layer: the layer's recurrence is complete
};
struct WaveLaunch {
  WaveCell cell[4]; int ncells;       // 1 to 4, never two cells of one layer
  bool closes;                // the last launch of its diagonal: the chunk jobs go behind it, never between the two launches of
  WaveCell done[kWaveMaxLayers];      // a diagonal with more than four layers in range.  done: the cells of the WHOLE
  int ndone;                  // diagonal that ended a chunk, in the diagonal's layer order (only on a closing launch)
};

// The recurrence launches in enqueue order, one call of visit(const WaveLaunch&) each; a non-zero return stops the walk
// and is returned.  A diagonal without a layer in range (T < lag: the layers further apart than the sequence is long)
// is not a launch.  A visitor, not a vector: the host functions consume each launch once, in order; nothing is allocated.
template <class Visit>
inline int wavefront_schedule(const WaveIn& in, Visit&& visit) {
  const int T = in.T, L = in.L, nch = (T + in.chunk - 1) / in.chunk;
  const bool by_step = in.unit == WaveUnit::step;
  const int units = by_step ? T : nch, lag = by_step ? in.lag * in.chunk : in.lag;
  const int ndiag = units + lag * (L - 1);
  for (int dg = 0; dg < ndiag; ++dg) {
    WaveCell on[kWaveMaxLayers];      // the cells of this diagonal
    int n = 0;
    for (int i = 0; i < L; ++i) {
      const int u = dg - lag * i, layer = in.backward ? L - 1 - i : i;
      if (u < 0 || u >= units) continue;
      const Chunk k = by_step ? Chunk{u, 1} : chunk_at(T, in.chunk, u);
      on[n++] = WaveCell{layer, by_step ? u / in.chunk : u, in.backward ? T - 1 - k.t0 : k.t0, k.nsteps,
                         !by_step || u % in.chunk == 0, !by_step || ends_chunk(T, in.chunk, u), u == units - 1};
    }
    for (int first = 0; first < n; first += 4) {      // (more than 4 layers on one diagonal: a second launch, the problems are independent)
      WaveLaunch q{};
      q.ncells = n - first < 4 ? n - first : 4;
      for (int i = 0; i < q.ncells; ++i) q.cell[i] = on[first + i];
      q.closes = first + 4 >= n;
      for (int i = 0; q.closes && i < n; ++i)
        if (on[i].ends) q.done[q.ndone++] = on[i];
      if (int rc = visit(q)) return rc;
    }
  }
  return 0;
}

// ---- forward ------------------------------------------------------------------------------------------------------------
struct FwdSchedIn {
  int T, B, H, L, chunk;      // T: the steps this call runs
  bool fwd_ns;                // the N-split kernel (no 32-row groups), else the K-split one
  bool persist_streams;       // CSN_PERSIST_STREAMS
  bool no_half_tiles;         // CSN_NO_HALF_TILES
};
// grouped: ONE launch per chunk diagonal (at most 4 slots, slots x 64-row tiles <= 8 groups -- one per XCD --, at most
// 32 slices per group).  Otherwise one launch per layer and chunk: every launch needs ALL its workgroups resident (one
// per CU), so the layers run on streams of their own only while together they fit the chip's 256 CUs; else everything
// goes down the caller's stream, layer after layer.
enum class FwdForm { grouped, layer_streams, caller_stream };
inline FwdForm fwd_persist_form(const FwdSchedIn& in) {
  const int MT = (in.B + 63) / 64, nch = (in.T + in.chunk - 1) / in.chunk;
  const int max_slots = in.L < nch ? in.L : nch;
  const int slices = in.fwd_ns ? fwd_ns_slices(in.H) : fwd_persist_slices(in.H);
  if (max_slots <= 4 && max_slots * MT <= 8 && slices <= 32 && !in.persist_streams) return FwdForm::grouped;
  return in.L * slices * MT > 256 ? FwdForm::caller_stream : FwdForm::layer_streams;
}

struct FwdSlot {
  int layer, chunk, t0, nsteps;
  bool feeds_next;            // the projection GEMM of layer + 1 for this chunk follows the launch
};
struct FwdLaunch {
  FwdSlot slot[4];
  int nslots;
  bool half;                  // 32-row groups
  int MT;                     // row tiles per layer at the launch's tile height
  int agree;                  // which set of XCD agreement words the launch uses (grouped form; -1: none)
};
// The recurrence launches of a forward in enqueue order.  Grouped form: diagonal dg holds layer l at chunk dg - l (the
// projection of layer l + 1 for a chunk is a GEMM between the launch that finished it below and the next one, so the
// layers lag ONE chunk).  A launch with few groups -- the wavefront's fill and drain, small batches -- runs on 32-row
// groups, twice as many, so that it spreads over all eight XCDs and every step of its chain handles half the rows
// (K-split kernel only).  The two stream forms: chunk after chunk, layer after layer, one slot per launch.
inline std::vector<FwdLaunch> fwd_persist_schedule(const FwdSchedIn& in) {
  const int MT = (in.B + 63) / 64, nch = (in.T + in.chunk - 1) / in.chunk, L = in.L;
  std::vector<FwdLaunch> out;
  auto slot_at = [&](int l, int c) {
    const Chunk k = chunk_at(in.T, in.chunk, c);
    return FwdSlot{l, c, k.t0, k.nsteps, l + 1 < L};
  };
  if (fwd_persist_form(in) != FwdForm::grouped) {
    out.reserve((size_t)nch * L);
    for (int c = 0; c < nch; ++c)
      for (int l = 0; l < L; ++l) {
        FwdLaunch q{};
        q.slot[q.nslots++] = slot_at(l, c);
        q.MT = MT;
        q.agree = -1;
        out.push_back(q);
      }
    return out;
  }
  const int ndiag = nch + L - 1;
  out.reserve(ndiag);
  for (int dg = 0; dg < ndiag; ++dg) {
    FwdLaunch q{};
    for (int l = 0; l < L; ++l) {
      const int c = dg - l;
      if (c >= 0 && c < nch) q.slot[q.nslots++] = slot_at(l, c);
    }
    q.half = !in.fwd_ns && !in.no_half_tiles && 2 * q.nslots * MT <= 8;
    q.MT = q.half ? 2 * MT : MT;
    q.agree = dg;
    out.push_back(q);
  }
  return out;
}

// ---- backward, grouped form ---------------------------------------------------------------------------------------------
struct BwdSchedIn {
  int T, B, H, L, chunk;      // T: the steps this call runs
  bool lengths;               // a batch with per-row lengths: the masked kernel, 64-row groups
  bool dropout;               // inter-layer dropout is on (plan bit, p > 0, more than one layer)
  bool dh_n;                  // the caller passes a gradient w.r.t. h_n
  bool data_polls;            // hand-off by sentinel data, not flags (CSN_BWD_FLAGS off)
  bool no_beside, no_merge, no_half_tiles;      // CSN_NO_BESIDE, CSN_BWD_NO_MERGE, CSN_NO_HALF_TILES
};
struct BwdSlot {
  int layer, chunk;           // reverse chunk index (of a merged launch: that of its first round)
  int t_hi, nsteps;           // steps t_hi, t_hi - 1, ..., t_hi - nsteps + 1 (of a merged launch: its first round)
  int cnt_pub, cnt_wait;      // PersistBwdSlot (lstm_cell_blk.h): indices into the merge counters, -1 = none
};
// dx_layer[t_lo .. t_hi] = dgates_layer[t_lo .. t_hi] W_ih, M = (t_hi - t_lo + 1) B rows: the dy of layer - 1
struct BwdGemm {
  int layer, t_lo, t_hi;
  bool mask;                  // the dropout mask of interface layer - 1 over these steps follows the GEMM
  bool add;                   // then the gradient w.r.t. h_n of layer - 1 joins those rows
};
struct BwdLaunch {
  BwdSlot slot[4];
  int nslots;                 // 0: a diagonal without a layer in range -- its GEMMs run stand-alone, each followed by its mask and term
  BwdGemm gemm[3];            // the GEMMs inside the launch (of a merged launch: those of its first round); behind the launch
  int ngemm;                  // come their masks, then their dh_n terms
  bool inline_gemms;          // CSN_NO_BESIDE and shapes without the beside form: dx_chunk_gemm of every slot above layer 0 follows
  int nrounds;                // > 1: a merged launch of as many diagonals
  bool half;                  // 32-row groups
  int MT;                     // row tiles per layer at the launch's tile height
  int agree;                  // which set of XCD agreement words: the (last) diagonal the launch covers
  int wk_wait, wk_pub, wk_stride;     // PersistBwdArgs: the merge counters as the GEMM workers index them
};

// What a grouped backward enqueues, in enqueue order.
//
// ONE launch per chunk diagonal walks every layer in range backwards through one chunk.  The input gradient of a layer's
// chunk is a GEMM that runs INSIDE the next launch, on the workgroups the recurrence leaves idle (gemm_beside.h), so
// both of its dependencies are kernel boundaries: its input was written by the launch before, its output is read by the
// launch after -- for which the layer below lags TWO chunks: diagonal dg holds layer l at reverse chunk
// dg - 2 (L - 1 - l).  Where the beside form does not apply (one layer or more than four, more than 28 slices per group,
// CSN_NO_BESIDE) the lag is one chunk and the GEMMs run between two launches.
//
// What follows a GEMM on the stream: under dropout the mask of its steps, then the gradient w.r.t. h_n of the layer
// below -- at step T - 1, i.e. behind the GEMM of reverse chunk 0, and with lengths behind EVERY GEMM (each row's own
// last step).  Both sit behind the launch that ran the GEMM and in front of the one that reads its output.
//
// A diagonal without a layer in range (one chunk per layer and the layers two launches apart) has nothing to recur
// over, but the GEMMs the previous launch left behind still have to run: stand-alone.
//
// Merged launch: the diagonals on which EVERY layer is in range, [lag (L - 1), nch - 1], hold the same workgroups with
// the same W_hh^T slices, carried dc and ring position (the tile height depends only on the layer count), and where
// nothing is enqueued between their launches (no dropout mask, no dh_n term, no lengths) they run as ONE launch of as
// many rounds: the two kernel boundaries around each GEMM become chunk-level counters, rec_done[L][nch] then
// gemm_done[L][nch].  A layer publishes rec_done of the chunk it leaves and waits for gemm_done of the layer above at the
// chunk it enters; layer 0 never publishes (nobody multiplies its dgates inside the launch) and the top layer never
// waits (its dy is the caller's), so there is no cycle.  The GEMMs of a merged launch all have chunk * B rows: the short
// chunk is the top layer's on the last of its diagonals, multiplied one launch later.
inline std::vector<BwdLaunch> bwd_persist_schedule(const BwdSchedIn& in) {
  const int T = in.T, L = in.L, MT = (in.B + 63) / 64;
  const int nch = (T + in.chunk - 1) / in.chunk;
  const bool beside = L > 1 && L <= 4 && bwd_persist_slices(in.H) <= 28 && (4 * in.H) % 64 == 0 && !in.no_beside;
  const int lag = beside ? 2 : 1;
  const int ndiag = nch + lag * (L - 1);
  const int m_first = lag * (L - 1), m_count = nch - m_first;
  const bool merge = beside && !in.no_merge && in.data_polls && !in.lengths && !in.dropout && !in.dh_n && m_count >= 2;
  std::vector<BwdLaunch> out;
  out.reserve(ndiag);
  BwdGemm left[3];            // the GEMMs of the chunks the previous launch finished
  int nleft = 0;
  for (int dg = 0; dg < ndiag;) {
    BwdLaunch q{};
    q.nrounds = (merge && dg == m_first) ? m_count : 1;
    q.agree = dg + q.nrounds - 1;
    for (int l = L - 1; l >= 0; --l) {
      const int c = dg - lag * (L - 1 - l);
      if (c < 0 || c >= nch) continue;
      const Chunk k = chunk_at(T, in.chunk, c);
      q.slot[q.nslots++] = BwdSlot{l, c, T - 1 - k.t0, k.nsteps, -1, -1};
    }
    q.ngemm = nleft;
    for (int i = 0; i < nleft; ++i) q.gemm[i] = left[i];
    nleft = 0;
    if (q.nslots > 0) {
      q.inline_gemms = !beside;
      // few groups: 32-row groups, twice as many (as in the forward).  The grid and the GEMM workers stay what they
      // are.  A batch with lengths stays on 64 rows: the masked kernel has no 32-row form.
      q.half = !in.no_half_tiles && !in.lengths && 2 * q.nslots * MT <= 8;
      q.MT = q.half ? 2 * MT : MT;
      if (q.nrounds > 1) {
        for (int i = 0; i < q.nslots; ++i) {
          BwdSlot& S = q.slot[i];
          if (S.layer > 0) S.cnt_pub = S.layer * nch + S.chunk;
          if (S.layer < L - 1) S.cnt_wait = (L + S.layer + 1) * nch + S.chunk;
        }
        q.wk_wait = q.slot[0].cnt_pub - 1;
        q.wk_pub = q.slot[1].cnt_wait + 1;
        q.wk_stride = nch + lag;
      }
      // the chunks the launch's last diagonal finished above layer 0: the GEMMs of the next entry
      for (int i = 0; beside && i < q.nslots; ++i) {
        const BwdSlot& S = q.slot[i];
        if (S.layer == 0) continue;
        const int c = S.chunk + q.nrounds - 1;
        const Chunk k = chunk_at(T, in.chunk, c);
        const int t_hi = T - 1 - k.t0;
        left[nleft++] = BwdGemm{S.layer, t_hi - k.nsteps + 1, t_hi, in.dropout, in.dh_n && (c == 0 || in.lengths)};
      }
    }
    if (q.nslots > 0 || q.ngemm > 0) out.push_back(q);
    dg += q.nrounds;
  }
  return out;
}

}  // namespace csn
