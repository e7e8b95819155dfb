// The API boundary of the stacked LSTM (lstm_boundary.hip): everything that turns the caller's batch-first float32 tensors
// into the time-major workspace and back around the recurrence -- one kernel per layout pass (y_all out, dy_all in, dx out)
// whatever the plan's lengths, direction, pitch, adding store or output dropout (DESIGN.md sections 10, 16 and 23), the
// pooled readout (mean / max over time in place of the last step, section 26), the attention readout (a learned-query
// weighted mean over time, section 28), and the small per-row helpers of variable-length batches.  lstm.hip calls the
// launchers below and launches none of this itself.
#pragma once
#include "lstm_dropout.h"

namespace csn {

// One layout pass over rows of the caller's [B, Tn, .] tensor and steps of the time-major workspace.
struct RowMap {
  const int* len;      // [B] device, valid steps per row; null: every row has Tn
  int B, Tn, Te, H;    // Tn: steps per row of the caller's tensor; Te: the steps the call ran (dy_in fills only those); H: row width
  int64_t pitch;       // elements between two (b, t) rows of the caller's tensor (y_out, dy_in; dx is dense)
  int rev;             // CSN_LSTM_REVERSE plan: the recurrence walked each row from its own last step
  int add;             // dx_out: add to what the caller's tensor holds, and leave its padding alone
};

// THE index rule.  Row b has n = len[b] valid steps (Tn without lengths).  Step s of the recurrence
// is the caller's t = rev ? n - 1 - s : s -- the same expression turns t into s --, and the output at t is slot
// rev ? n - t : t + 1 of h_all (slot 0 is the initial state, slot n the final one).  Nothing at t >= n was computed.
struct RowSteps {
  int64_t n;
  int rev;
  __device__ __forceinline__ RowSteps(const int* __restrict__ len, int64_t b, int Tn, int rev_) : n(len != nullptr ? len[b] : Tn), rev(rev_) {}
  __device__ __forceinline__ bool valid(int64_t t) const { return t < n; }
  __device__ __forceinline__ int64_t flip(int64_t t) const { return rev ? n - 1 - t : t; }       // t <-> s
  __device__ __forceinline__ int64_t slot(int64_t t) const { return rev ? n - t : t + 1; }
};

// The pooled term of dy_in (csn_lstm_plan_set_readout): the gradient w.r.t. the pooled y_last, and under MAX the caller time
// per (b, h) that receives it (launch_pool_argmax)
struct PoolIn {
  int mode;                // CSN_READOUT_*, or kPoolAttention
  const float* dy_last;    // [B, H]
  const int* argmax;       // [B, H] int32, MAX only
  const float* a32;        // [B, Tn] attention weights, w32: [B, Tn] score gradients, q: [H] the query -- kPoolAttention only
  const float* w32;
  const float* q;
};
// the attention readout's tag in PoolIn::mode (csn_lstm_plan_set_attention): internal, not a CSN_READOUT_* value
constexpr int kPoolAttention = 16;

// The attention readout (csn_lstm_plan_set_attention): the query, and the [B, Tn] arrays of one call.
// a64 / g64 / dq_part are plan-owned scratch; a32 / w32 are the caller's attn_out / dscore_out, or plan-owned scratch too.
struct AttnArgs {
  const float* q;      // [H]
  float scale;
  double* a64;         // [B, Tn]: the scaled scores z, then exp(z - max), then the weights, in place
  double* g64;         // [B, Tn]: <dy_last[b], v[b, t]> (backward)
  float* a32;          // [B, Tn]: fl32 of the weights, 0 from a row's length on
  float* w32;          // [B, Tn]: fl32(scale a (g - s)), 0 from a row's length on (backward)
  double* dq_part;     // [kAttnDqParts, H]: the query gradient's partial sums (backward with dq)
};
constexpr int kAttnDqParts = 64;

// The launchers.  od: output dropout (csn_lstm_plan_set_output_dropout), or null.  With it a thread moves four consecutive h
// under one Philox call with 16-byte accesses of the caller's tensor, which must be 16-B aligned with pitch % 4 == 0;
// without it one element, and the caller's tensor needs the 4 bytes of a float.  A dropped element is a selected zero.
// y[(b Tn + t) pitch + h] = t < n ? [keep ? scale *] float(h_all[slot(t)][b][h]) : 0      (h_all: dtype, time-major)
int launch_y_out(const void* h_all, int dtype, float* y, const RowMap& m, const OutDropCfg* od, hipStream_t st);
// dy_tm[s][b][h], s < Te  =  s < n && dy ? [keep ? scale *] dy[(b Tn + t) pitch + h] : 0      (dy null: all zeros)
// pool (or null): + dy_last[b][h] / n (MEAN), + (argmax[b][h] == t ? dy_last[b][h] : 0) (MAX) for s < n, one float32 add behind
// the dy element -- the term itself where dy is null; kPoolAttention: + fl32(fl32(a32[b][t] dy_last[b][h]) + fl32(w32[b][t] q[h]))
int launch_dy_in(const float* dy, float* dy_tm, const RowMap& m, const OutDropCfg* od, const PoolIn* pool, hipStream_t st);
// y[b][h] = mean (float64 sums, one rounding) or max (first maximum, a NaN wins) over t < n of float(h_all[slot(t)][b][h]);
// zeros for n = 0.  m.pitch and m.Te are not read.  A fixed split of the steps: the same bits every call
int launch_pool_readout(const void* h_all, int dtype, int mode, float* y, const RowMap& m, hipStream_t st);
// argmax[b][h] = the first caller time t < n that attains that maximum (-1 for n = 0)
int launch_pool_argmax(const void* h_all, int dtype, int* argmax, const RowMap& m, hipStream_t st);
// The attention readout, forward: z[b][t] = scale <v[b][t], q> (float64 partials per lane, a fixed lane tree), its softmax
// over t < n (float64, max-subtracted) into A.a64 and A.a32, and y[b][h] = fl32(sum over t < n of a64 v) with the split and
// the LDS combine of the pooled readout.  Three launches, two reads of h_all; zeros for n = 0; the same bits every call
int launch_attn_forward(const void* h_all, int dtype, const AttnArgs& A, float* y, const RowMap& m, hipStream_t st);
// ... and the backward's pre-passes: the scores again with g[b][t] = <dy_last[b], v[b][t]> from the same load, the row
// kernel with s = sum a g and A.w32 = fl32(scale a (g - s)), then (dq != null) dq[h] = or += fl32(sum over b, t < n of
// w32 v): float64 partials per workgroup into A.dq_part, combined in a fixed order.  Two or four launches, at most two
// reads of h_all.  What dy_in adds comes through PoolIn{kPoolAttention, dy_last, nullptr, A.a32, A.w32, A.q}
int launch_attn_backward(const void* h_all, int dtype, const AttnArgs& A, const float* dy_last, float* dq, int accumulate, const RowMap& m,
                         hipStream_t st);
// dx[b][t][i] = or += dx_tm[s][b][i] for t < n; from n on zero, or with add left as it is      (m.H: the input width)
int launch_dx_out(const float* dx_tm, float* dx, const RowMap& m, hipStream_t st);

// out[b][h] (f32) = all[n][b][h], n = len ? len[b] : T: slot n of h_all / c_all is the state after step n - 1, slot 0 the initial state
int launch_gather_state(const void* all, int dtype, const int* len, int T, float* out, int B, int H, hipStream_t st);
// dst_tm[n-1][b][:] += src[b][:] for the rows whose last step n - 1 lies in [t_lo, t_hi]: a gradient that enters at the
// row's end.  Without lengths every row ends at T - 1, and no kernel is launched when that lies outside the window.
int launch_add_at_end(const float* src, float* dst_tm, const int* len, int T, int t_lo, int t_hi, int B, int H, hipStream_t st);
// dst[b][:] += src[b][:] for the rows of length 0 (their dh0 is dh_n)
int launch_add_rows_len0(const float* src, float* dst, const int* len, int B, int H, hipStream_t st);
// buf[t][b][:] = 0 where t >= len[b] (time-major input copy [Tn, B, W] in dtype: padding is never multiplied) ...
int launch_mask_tm(void* buf, int dtype, const int* len, int B, int Tn, int W, hipStream_t st);
// ... and the same on the fragment-major slabs [Tn][Bpad * I] of the fused input projection
int launch_mask_x_blk(bf16_t* x_blk, const int* len, int B, int64_t Bpad, int Tn, int I, hipStream_t st);

}  // namespace csn
