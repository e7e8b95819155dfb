/*
 * csn_hip.h -- C ABI of libcsn_hip.so: the MI355X (gfx950) implementation of the
 * EEG -> stacked-LSTM -> distillation hot path of Vi-Sri/CerebralSignalNetworks.
 *
 * The reference is pure Python and has no FFI/plugin interface of its own (SURVEY.md
 * section 8b): its boundary is a set of Python call sites that reach third-party native code
 * (scipy.signal, torch.nn.LSTM/ATen, faiss).  Each entry point below replaces one of
 * those call sites and cites it.  Signatures carry only plain pointers and sizes:
 * every `const T*` / `T*` is a DEVICE pointer unless marked [host]; `stream` is a
 * hipStream_t passed as void* (NULL = the default stream).  All work is enqueued on
 * `stream` or ordered by it, and only the calls listed there wait for the device
 * ("Stream contract" below).  Return value: 0 on success, non-zero csnStatus otherwise,
 * with a message in csn_last_error().  Shape / alignment violations are rejected on the
 * host before any launch.
 *
 * Tensors are dense row-major unless strides are given.  dtype codes: CSN_F32, CSN_BF16.
 */
#ifndef CSN_HIP_H
#define CSN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* csnStream_t;

/* ------------------------------------------------------------------------------------
 * Stream contract of every entry point that takes a csnStream_t (tests/test_gpu_stream_order.py runs each of them with
 * inputs produced late on `stream`, outputs read and inputs overwritten on it directly behind the call and no other
 * synchronisation -- evidence where it fails, not proof where it passes: DESIGN.md section 14).
 *
 * ORDER.  Everything the call enqueues -- kernels, memsets, copies, and the work the LSTM puts on streams of its own
 * (a plan owns a side stream and seven per-layer streams) -- runs after everything the caller enqueued on `stream`
 * before the call and before everything the caller enqueues on `stream` after it.  Work on the plan's own streams is
 * forked from `stream` by an event and joined back to it by an event before the call returns.  The caller synchronises
 * no other stream, and no entry point that takes a `stream` uses the default (NULL) stream unless it is `stream`.  (The one
 * call that does use the NULL stream takes no `stream`: csn_lstm_status_read, under BLOCKING.)
 *
 * HOST.  The calls return once their work is enqueued; none waits for the device, except as listed under BLOCKING.
 * [host] arguments (sos, the arrays of layer pointers, seg_end, flags, lengths) are read before the call returns and may
 * be freed then.
 *
 * OVERWRITE.  When a call has returned, work enqueued on `stream` may overwrite or free EVERY device argument of it:
 * inputs, scratch and -- once read -- outputs.  For the LSTM in particular:
 *   csn_lstm_forward   copies x, every weight and bias, h0 and c0 into the workspace (re-laid out, in the compute dtype).
 *                      Nothing later reads the caller's copies: csn_lstm_backward takes the weights, the transposes, the
 *                      initial state and the input from the workspace, so an optimiser step enqueued on `stream` right
 *                      behind the forward may already rewrite the parameters the matching backward is still to use.
 *   csn_lstm_backward  reads from caller memory only its own arguments dy_last, dy_all, dh_n, dc_n (and, accumulating,
 *                      the previous dw / db; under dx_add of csn_lstm_plan_set_io the previous dx, which is then an input
 *                      as well as an output: what it holds must be there in stream order in front of the call); all four
 *                      may be overwritten behind it.  dw, db, dx, dh0, dc0 are complete
 *                      in stream order behind it (the gradient-ready callback marks an earlier point per layer).
 *   A pitched y_all / dy_all (csn_lstm_plan_set_io) follows the same rule as the dense one: the forward writes, and the
 *                      backward reads, only the H elements of every (b, t) row of the half it was given, in stream order;
 *                      the rest of the wider buffer is neither read nor written and belongs to the caller (or to the
 *                      other direction's plan) throughout, and the whole buffer may be overwritten behind the backward.
 *   The workspace belongs to the plan's calls from a forward to its backward; the lengths are host memory (above).
 *
 * ANOTHER STREAM.  A plan (and its workspace) may be called on another stream than its previous call used, provided the
 * new stream is ordered behind the old one (an event wait, or a synchronisation): every call leaves all of its work
 * joined to the stream it was given.  Calls of one plan on streams NOT so ordered race on the workspace and on the
 * plan's event pool.
 *
 * BLOCKING (the only entry points that wait for the device on the host):
 *   csn_lstm_status_read   hipMemcpy to the host on the NULL stream: returns when the word has arrived.  The NULL stream
 *                          does not wait for streams created with hipStreamNonBlocking (PyTorch's side streams are):
 *                          the caller synchronises such a stream first if the word is to cover the work on it.
 *   csn_lstm_profile_read  waits for the closing profile event of the last forward / backward.
 *   csn_lstm_forward / csn_lstm_backward ON A PLAN WITH LENGTHS wait for the lengths upload of the plan's PREVIOUS call
 *                          with lengths (a copy of 4 * B bytes; they reuse its pinned staging array) -- hence until `stream`
 *                          has reached that copy; the first such call allocates the staging and device arrays.
 *                          csn_lstm_plan_set_lengths itself only stores the lengths on the host.
 *   csn_lstm_forward ON A PLAN WITH INPUT WINDOWS waits in the same way for the windows upload (8 * B bytes) of the
 *                          plan's previous forward with windows; csn_lstm_plan_set_views only stores them on the host.
 *   csn_lstm_plan_destroy  frees the plan's streams and events (and, after lengths, device memory, which waits for the
 *                          device): call it when the plan's work has completed.
 * Not blocking, but host work beyond the launches: csn_lstm_plan_create computes the workspace layout and reads the
 * environment (no device work); the first forward / backward of a plan creates its streams, and a call grows the event
 * pool when it needs more events than any call before it; the first launch of a kernel with a large dynamic LDS
 * allocation sets that function attribute once per process.
 * ---------------------------------------------------------------------------------- */

enum csnStatus {
  CSN_OK = 0,
  CSN_ERR_INVALID_ARGUMENT = 1,
  CSN_ERR_HIP = 2,
  CSN_ERR_UNSUPPORTED = 3
};

enum csnDtype { CSN_F32 = 0, CSN_BF16 = 1 };

/* ABI version of this header; bumped on any signature change.  A symbol added beside the existing ones
 * (csn_lstm_plan_set_grad_mode, csn_lstm_plan_set_lengths, csn_lstm_plan_set_views, csn_lstm_plan_set_io, csn_lstm_plan_set_readout, csn_lstm_plan_set_attention, csn_lstm_plan_half_tile_launches, the
 * csn_flat_* family, csn_adam_step, csn_lars_step, csn_eeg_bandpass_stream and its _path, csn_distill_loss,
 * csn_dino_loss, csn_barlow_corr, csn_barlow_grad, csn_contrastive_lse, csn_contrastive_grad, csn_bank_norms, csn_bank_contrastive and its _scratch_bytes, csn_topk_merge and its _staged_max, csn_topk_class_metrics, csn_grad_guard, its _scratch_bytes and the three
 * csn_*_step_guarded) breaks no caller and does not bump it; neither does a new bit of csn_lstm_plan_create's `training` word. */
#define CSN_ABI_VERSION 6
int csn_abi_version(void);
/* Thread-local message for the last non-zero status returned on this thread. */
const char* csn_last_error(void);
/* Name of the device code object's target ("gfx950"). */
const char* csn_target_arch(void);

/* ------------------------------------------------------------------------------------
 * K1+K2  fused band-pass + per-channel z-score.
 * Replaces: scipy.signal.butter/lfilter design+apply named by utils/EEGFilters.py:2,26
 * (applied causally, in second-order sections) followed by EEGDataset.normlizeEEG,
 * utils/PerilsEEGDataset.py:454-461, for every channel of a segment, and the
 * `.t()` re-layout of EEGDataset.__getitem__, utils/PerilsEEGDataset.py:549.
 *   x      [B,C,T] float32 (channel-first, as stored on disk: ConvertToPth.py:170-201)
 *   sos    [host] [nsec,6] float64 rows (b0,b1,b2,a0,a1,a2), nsec <= 8; nsec == 0 = no filter
 *   ddof   0 (numpy path, PerilsEEGDataset.py:555-562) or 1 (torch path, :576-579)
 *   y      out_dtype, laid out [B,T,C] (time_major=0) or [T,B,C] (time_major=1)
 * IIR state and statistics are carried in float64.  Stateless: what depends on the coefficients alone (the
 * chunk-scan basis) is computed on the host per call and travels with the kernel arguments -- no device buffer is
 * kept between calls, so calls with different coefficients on different streams / threads / devices are independent.
 * ---------------------------------------------------------------------------------- */
int csn_eeg_bandpass_znorm(const float* x, int B, int C, int T,
                           const double* sos, int nsec, int ddof,
                           void* y, int out_dtype, int time_major, csnStream_t stream);

/* Zero-phase variant.  Replaces: signal.filtfilt(b, a, eeg[s, :, c]) for every (s, c) in
 * Utilities.remove_noise, utils/Utilities.py:411-428 (Butterworth order 4, 1-50 Hz; scipy defaults:
 * odd extension, padlen = 3*max(len(a),len(b)) = 3*(2*nsec+1), steady-state initial conditions),
 * evaluated on the second-order-section cascade in float64.
 *   x, y    [S,T,C] float32 (samples x time x channels, the layout remove_noise takes), T > padlen
 *   scratch csn_eeg_filtfilt_scratch_bytes(S,T,C,nsec) bytes of device memory */
size_t csn_eeg_filtfilt_scratch_bytes(int S, int T, int C, int nsec);
int csn_eeg_filtfilt(const float* x, int S, int T, int C, const double* sos, int nsec,
                     float* y, void* scratch, csnStream_t stream);

/* Causal band-pass of a recording delivered in pieces: scipy.signal.sosfilt(sos, x, zi) per (segment, channel) row.
 *   x          piece [B,C,T] float32, T >= 1; row (b,c) starts at x + (b*C + c) * x_row_stride, x_row_stride >= T
 *              (a piece may be a time slice of a longer [B,C,Ttotal] buffer: no copy)
 *   sos, nsec  as csn_eeg_bandpass_znorm (nsec 0..8; 0 = no filter)
 *   state_in   [B,C,nsec,2] float64, the direct-form-II-transposed (s1, s2) of every section = scipy's zi[nsec,B,C,2]
 *              with the section axis moved inward; NULL = zeros (start of a recording)
 *   state_out  same layout, the state after the last sample of the piece; may be NULL; may alias state_in
 *   mean, inv_std  optional [C] float32 (both or neither): y = (filtered - mean[c]) * inv_std[c], formed in float64,
 *              rounded once
 *   y          out_dtype, [B,T,C] (time_major = 0) or [T,B,C]
 * With nsec == 0 there is no state: state_in and state_out are ignored and only the affine applies.
 * Stateless like every other entry point: the state lives in the caller's buffers, the library keeps nothing between
 * calls, and what depends on the coefficients alone travels with the kernel arguments.  Two kernels: a tile-walking
 * chunk scan (nsec <= 5, C, T and x_row_stride multiples of 4, x 16-byte aligned) whose tiles of 512 samples are
 * left-aligned in the piece -- pieces that are whole tiles give the bits of the one-shot call -- and a stateful
 * row-walking kernel for everything else (any T, C, stride, alignment; nsec <= 8).  Neither computes statistics: the
 * z-score of csn_eeg_bandpass_znorm is per call, this normalisation is the caller's fixed per-channel affine. */
int csn_eeg_bandpass_stream(const float* x, int64_t x_row_stride, int B, int C, int T,
                            const double* sos, int nsec, const double* state_in, double* state_out,
                            const float* mean, const float* inv_std,
                            void* y, int out_dtype, int time_major, csnStream_t stream);
/* Which kernel a call with these arguments runs: 1 = tile-walking scan, 0 = stateful row-walking kernel.  Host only. */
int csn_eeg_bandpass_stream_path(const float* x, int64_t x_row_stride, int C, int T, int nsec);

/* ------------------------------------------------------------------------------------
 * K3  stacked LSTM, gate order i,f,g,o, nn.LSTM parameter layout; zero initial state, or (h0, c0) on a plan
 * created with CSN_LSTM_STATE.
 * Replaces: nn.LSTM(input, hidden, num_layers, batch_first=True) forward/backward at
 * LSTMDistill.py:118,132 and LSTMDistillRetreival.py:91,103 (the body of the absent
 * models.lstm.Model, LstmDistillFromDinoV2Train.py:323).
 * ---------------------------------------------------------------------------------- */
typedef struct csnLstmDesc {
  int32_t B;      /* batch                                       */
  int32_t T;      /* time steps                                  */
  int32_t I;      /* input features (EEG channels)               */
  int32_t H;      /* hidden size; multiple of 32                 */
  int32_t L;      /* stacked layers, 1..8                        */
  int32_t dtype;  /* CSN_BF16: bf16 MFMA operands, f32 accumulate/state; CSN_F32: exact f32 MFMA */
} csnLstmDesc;

/* A PLAN holds everything host-side that a stacked-LSTM problem of one shape needs: the workspace layout, the
 * diagnostic switches (environment, read once here), library-owned side streams, an event pool, profiling events.
 * The library keeps NO mutable global state: plans are independent of each other, so different host threads /
 * streams / devices use different plans freely.  One plan must not be used from two threads at once, and it is
 * bound to the device that was current when it was created.  training != 0: the forward keeps what
 * csn_lstm_backward needs.  (There is nothing like this in the reference: torch's nn.LSTM hides the same state in
 * cuDNN/MIOpen descriptors and the autograd graph.) */
typedef struct csnLstmPlan csnLstmPlan;
/* `training` may carry CSN_LSTM_STATE: the plan accepts the state arguments of csn_lstm_forward / csn_lstm_backward
 * (h0, c0, h_n, c_n, dh_n, dc_n, dh0, dc0).  A CSN_BF16 state plan takes the path a plan without the bit takes
 * (0-3); a CSN_F32 one runs as under CSN_NO_PERSIST (path 0): the exact-float32 weight-stationary path (4) takes no
 * state.  A plan without the bit rejects every state argument and runs exactly as before.  The remaining bits:
 * != 0 = training. */
#define CSN_LSTM_STATE 0x100
/* `training` may also carry CSN_LSTM_DROPOUT: the plan can apply nn.LSTM's inter-layer dropout (csn_lstm_plan_set_dropout
 * below).  Its workspace gains h_drop[l], [T,B,H] in the compute dtype, for every layer l < L-1 (197 MB at B 256, T 500,
 * H 768, L 2, bf16, on 10 GB), laid out behind everything else.  Valid on training and inference plans, with or
 * without CSN_LSTM_STATE.  Until a p > 0 is set the plan runs the launches and writes the bits of a plan without it. */
#define CSN_LSTM_DROPOUT 0x200
/* `training` may also carry CSN_LSTM_REVERSE: the plan walks every row BACKWARDS in time -- the reverse direction of a
 * bidirectional LSTM.  Valid with or without the other two bits, for any L, on every path: a reverse
 * plan takes the path, runs the recurrence kernels and has the workspace of a plan without the bit.  Only the layout
 * passes around the recurrence differ: with n = lengths[b] (T when no lengths are set), recurrence step s of row b
 * consumes x[b, n-1-s] and its top-layer output lands at y_all[b, n-1-s]; (h0, c0) is the state in front of time n-1;
 * y_last, h_n, c_n are taken after step n-1, that is at time 0; dy_all[b, t] is read and dx[b, t] written under the same
 * map, dy_last / dh_n / dc_n enter at the last step as on any plan.  x[b, t >= n] and dy_all[b, t >= n] are never read,
 * y_all and dx are zero there, n = 0 passes through.  With R = "reverse each row's first n steps, leave the rest":
 * y_all = R(y_all of a plan without the bit on R(x)) and dx = R(its dx for R(dy_all)); every other result -- y_last, h_n,
 * c_n, dh0, dc0, all weight gradients -- is that plan's, and all of it holds bit for bit (the workspace behind the
 * layout passes has the same contents).  (tests/test_gpu_bilstm.py) */
#define CSN_LSTM_REVERSE 0x400
/* `training` may also carry CSN_LSTM_RESIDENT: the plan runs the CU-resident recurrence (path 5)
 * instead of the path it would take.  H in {32, 64, 96, 128}, CSN_BF16 and CSN_F32, any B, T, I, L 1..8, training and
 * inference plans, with every other bit; with H > 128 csn_lstm_plan_create returns CSN_ERR_UNSUPPORTED and
 * csn_lstm_workspace_bytes 0.  The workspace is that of the same descriptor on path 0 (the generic per-step cells; what
 * CSN_CELL_V1=1 selects), nothing added, and so are the host flow and every plan feature: state, lengths, dropout,
 * reverse, windows, io, gradient accumulation, the gradient-ready callback.  What changes is the recurrence: the steps
 * of a chunk (CSN_LSTM_CHUNK, default 32) of a layer run inside ONE launch, W_hh in the registers of a workgroup that
 * owns 16 batch rows, h in LDS -- ceil(T / chunk) + L - 1 recurrence launches per pass (L <= 4) against
 * T + chunk (L - 1).  Every output and gradient equals, BIT FOR BIT, that of the same plan on path 0: same MFMA, same
 * k order per element, same gate expressions.  Opt-in: a plan without the bit is what it was.
 * (tests/test_gpu_lstm_resident.py) */
#define CSN_LSTM_RESIDENT 0x800
int csn_lstm_plan_create(const csnLstmDesc* d, int training, csnLstmPlan** out);
void csn_lstm_plan_destroy(csnLstmPlan* plan);
/* Bytes of device scratch ("workspace") a forward (+ backward) of this plan needs; 256-B aligned base.  The
 * caller owns it; one plan may be used with several workspaces (e.g. several forwards awaiting their backward). */
size_t csn_lstm_plan_workspace_bytes(const csnLstmPlan* plan);
/* Which kernels the plan runs: 0 generic per-step cells (exact f32 / odd shapes), 1 per-diagonal bf16 launches,
 * 2 weight-stationary forward, 3 weight-stationary forward and backward (bf16), 4 weight-stationary forward and
 * backward of the exact-float32 path (CSN_F32, H in {128, 256, 384, 512, 768, 1024}, a whole MI355X: one launch per layer and
 * block of batch rows; its workspace also holds fragment-major copies of h and of the gate gradients), 5 the CU-resident
 * recurrence of a CSN_LSTM_RESIDENT plan (H <= 128, both dtypes: path 0's workspace, one launch per chunk diagonal). */
int csn_lstm_plan_path(const csnLstmPlan* plan);
/* Copies of the gate gradients the plan's LAST csn_lstm_backward wrote per step: 2 = the fragment-major hand-off slab
 * and a row-major copy for the GEMMs behind the recurrence, which every weight-stationary bf16 backward writes; 0 = no
 * backward has run, or a path without hand-off slabs.  Kept for ABI stability: it never returns anything else (the
 * single-copy form that returned 1 was removed). */
int csn_lstm_plan_dgates_copies(const csnLstmPlan* plan);
/* How many weight-stationary recurrence launches of the plan's LAST forward (which = 0) / backward (which = 1) ran on
 * hand-off groups of 32 rows instead of 64 (launches whose 64-row groups would cover at most half of the XCDs;
 * CSN_NO_HALF_TILES=1 keeps 64 rows everywhere: 0; a merged backward launch counts once per chunk diagonal it covers, so
 * the figure does not depend on CSN_BWD_NO_MERGE).  Diagnostic; -1 for a null plan / other `which`. */
int csn_lstm_plan_half_tile_launches(const csnLstmPlan* plan, int which);
/* Name of the device function that advances the recurrence on this plan's path: which = 0 forward, 1 backward
 * ("lstm_fwd_persist_kernel", "lstm_fwd_ns_kernel", "lstm_bwd_persist_kernel", "lstm_cell_fwd_il_kernel", ... -- the
 * names a rocprofv3 kernel trace shows, without template arguments).  Diagnostic: bench.py labels its roofline object
 * and looks up the committed counter passes with it.  Static storage; NULL for a null plan / other `which`. */
const char* csn_lstm_plan_kernel_name(const csnLstmPlan* plan, int which);
/* Same number without a plan (what csn_lstm_plan_workspace_bytes would return for a plan created now). */
size_t csn_lstm_workspace_bytes(const csnLstmDesc* d, int training);

/* Once per workspace, before its first forward (enqueued on `stream`): zeroes the status word and the regions the
 * kernels only ever read as zero (the zero initial state h_0 / c_0 of every layer, ...).  A forward / backward
 * re-zeroes per call only what it dirties (flag lines, carried dc). */
int csn_lstm_workspace_init(const csnLstmPlan* plan, void* workspace, csnStream_t stream);

/* x: element (b,t,i) at x[b*x_stride_b + t*x_stride_t + i] (float32).  The strides are in ELEMENTS and may be any
 *   non-negative values, 0 included (a broadcast row), in either order (x_stride_b < x_stride_t is a time-major
 *   buffer); the innermost stride is 1.  x needs the 4-byte alignment of a float only: a base on 16 bytes with
 *   both strides multiples of 4 (and, for the row-major copy, I % 8 == 0) merely selects 16-byte loads.  x is never
 *   written, and it is not read after csn_lstm_forward has returned its work to `stream`: the forward re-lays it out
 *   into the workspace and everything else, csn_lstm_backward included (which takes no x), reads those copies, so work
 *   enqueued on `stream` behind the call may overwrite x.  (tests/test_gpu_lstm_input_views.py)
 * w_ih/w_hh/b_ih/b_hh: [host] arrays of L device pointers to float32 parameters
 *   weight_ih_l{k}[4H,I_k], weight_hh_l{k}[4H,H], bias_ih_l{k}[4H], bias_hh_l{k}[4H].
 * h0, c0: optional [L,B,H] float32 initial state (NULL = zeros), dense, 16-B aligned.
 * y_last: [B,H] float32 = output of the top layer at t = T-1, or its mean / maximum over time (csn_lstm_plan_set_readout).
 * y_all : optional (may be NULL) [B,T,H] float32, every step of the top layer.
 * h_n, c_n: optional [L,B,H] float32 final state of every layer (may be NULL), dense, 16-B aligned.
 * At least one of y_last, y_all, h_n, c_n must be given.
 * State (only on a CSN_LSTM_STATE plan; any non-NULL state argument on another plan is CSN_ERR_INVALID_ARGUMENT):
 *   CSN_BF16: h0 is rounded to bf16 as every h is; c0 stays float32.  h_n[l] is the upcast of the bf16 h that layer
 *   l+1 and y_all consumed, so under CSN_READOUT_LAST h_n[L-1] == y_last bit for bit; c_n is the float32 cell state.  Feeding (h_n, c_n) of
 *   one call into the next as (h0, c0) is therefore exact: a sequence run as consecutive chunks carries the same
 *   state as one run over all of it.  CSN_F32: everything float32.
 *   With every state argument NULL, a CSN_BF16 state plan computes the same bits as a plan without the bit (a float32
 *   one those of a plan under CSN_NO_PERSIST); once it has run a forward with a state, its later stateless forwards
 *   on paths 2-3 re-zero slot 0 of h and c (two memsets per layer). */
int csn_lstm_forward(csnLstmPlan* plan,
                     const float* x, int64_t x_stride_b, int64_t x_stride_t,
                     const float* const* w_ih, const float* const* w_hh,
                     const float* const* b_ih, const float* const* b_hh,
                     const float* h0, const float* c0,
                     void* workspace, float* y_last, float* y_all,
                     float* h_n, float* c_n, csnStream_t stream);

/* dy_last: [B,H] float32 gradient w.r.t. y_last (may be NULL); it enters where the plan's readout took y_last from.
 * dy_all : optional [B,T,H] float32 gradient w.r.t. y_all (may be NULL).
 * dh_n, dc_n: optional [L,B,H] float32 gradients w.r.t. h_n / c_n (may be NULL).
 * At least one of dy_last, dy_all, dh_n, dc_n must be given.
 * dw_ih/dw_hh/db_ih/db_hh: [host] arrays of L device pointers, float32, OVERWRITTEN, or added to under
 *   CSN_GRAD_ACCUMULATE (csn_lstm_plan_set_grad_mode).
 * dx: optional [B,T,I] float32 (dense), gradient w.r.t. x (may be NULL).
 * dh0, dc0: optional [L,B,H] float32 gradients w.r.t. h0 / c0, OVERWRITTEN (may be NULL); written whether or not the
 *   forward had a state (the gradient w.r.t. a zero state).  dh0[l] = dgates_l[t=0] W_hh_l from the operands the
 *   recurrence uses (bf16 on CSN_BF16), float32 accumulate; dc0[l] = the cell-state gradient carried past step 0.
 *   dW_hh includes dgates_0^T h0 and df_0 uses c0.  State arguments need a CSN_LSTM_STATE plan; all 16-B aligned. */
int csn_lstm_backward(csnLstmPlan* plan,
                      const float* dy_last, const float* dy_all,
                      const float* dh_n, const float* dc_n,
                      void* workspace,
                      float* const* dw_ih, float* const* dw_hh,
                      float* const* db_ih, float* const* db_hh,
                      float* dx, float* dh0, float* dc0, csnStream_t stream);

/* Gradient-ready notification (data-parallel training: the reference gets the overlap of its gradient all-reduce with
 * the backward from DistributedDataParallel's autograd hooks, LstmDistillation.py:445; this is the same hook at the C
 * boundary).  csn_lstm_backward calls fn(user, layer) on the CALLING host thread, once per layer, top layer first,
 * each time at a point where every kernel that writes dw_ih/dw_hh/db_ih/db_hh of `layer` has been enqueued on (or
 * ordered before) `stream`: work the callback enqueues behind `stream` -- e.g. an all-reduce of that layer's gradients
 * on a communication stream that waits on an event recorded there -- then runs beside the remaining layers' weight-
 * gradient GEMMs.  The weight-stationary recurrence launches (one workgroup per CU, all co-resident) are all enqueued
 * BEFORE the first call, so nothing the callback starts can share the device with them.  The callback must not call
 * back into this plan.  fn = NULL removes it. */
typedef void (*csnGradReadyFn)(void* user, int layer);
int csn_lstm_plan_set_grad_callback(csnLstmPlan* plan, csnGradReadyFn fn, void* user);

/* Gradient mode of the plan's later csn_lstm_backward calls; sticky until set again.  It governs dw_ih, dw_hh, db_ih and
 * db_hh only: dx, dh0 and dc0 are overwritten in both modes.  CSN_GRAD_OVERWRITE (the default) stores each gradient g.
 * CSN_GRAD_ACCUMULATE stores fl32(prev + g) into every element, where g is exactly the float32 value the overwrite mode
 * stores for the same inputs and prev is what the buffer held: one rounding, prev joins last -- bit for bit what
 * `p.grad += g` gives, so a backward that writes straight into a gradient buffer cannot be told from one that goes through
 * a temporary.  db_ih and db_hh each add to their OWN previous contents (in this mode one buffer for both is refused on the host).
 * Every path (csn_lstm_plan_path 0-5), with and without CSN_LSTM_STATE and the gradient-ready callback, whose meaning
 * is unchanged: the accumulating kernels of a layer are enqueued before it fires for that layer.  Uses: several forwards
 * through one set of parameters in a step (multi-crop views), micro-batches summed into one optimiser step, the chunks
 * of a recording chained through their state.  Null plan / unknown mode: CSN_ERR_INVALID_ARGUMENT. */
#define CSN_GRAD_OVERWRITE  0
#define CSN_GRAD_ACCUMULATE 1
int csn_lstm_plan_set_grad_mode(csnLstmPlan* plan, int mode);

/* Variable-length batches: per-row numbers of valid steps.  `lengths` is a HOST array of B
 * entries, each in [0, T]; NULL = every row is T (the default; such a plan runs exactly the kernels it ran before this
 * symbol existed).  Sticky until set again, like the gradient mode.  Only on a CSN_LSTM_STATE plan.
 * Semantics = nn.LSTM on pack_padded_sequence(enforce_sorted=False) + pad_packed_sequence(total_length=T).  For row b,
 * n = lengths[b]:  y_all[b, t >= n] = 0;  h_n[l, b], c_n[l, b] = the state after step n-1 (CSN_BF16: the bf16 h every
 * consumer saw);  y_last[b] = h_n[L-1, b];  nothing at t >= n enters any gradient: dx[b, t >= n] = 0, dy_all[b, t >= n]
 * is ignored, dh_n[l, b] / dc_n[l, b] / dy_last[b] enter at step n-1.  n = 0 (beyond torch): the row passes through --
 * h_n = h0 (bf16-rounded on CSN_BF16), c_n = c0, zero output, dh0 = dh_n (+ dy_last in the top layer, whose h_n is y_last),
 * dc0 = dc_n, no parameter contribution; with
 * every row 0 no recurrence kernel is launched.  x[b, t >= n] and dy_all[b, t >= n] are never read as data: whatever
 * they hold (NaN, Inf), every result has the bits of the same call with zeros there.
 * The recurrence and every GEMM behind it cover max(lengths) steps, not T.
 * Contract: a forward uses the lengths the plan holds when it is called and uploads them to the device in stream order
 * (into a [B] array the plan owns: a state plan's workspace stays laid out as a plain plan's); the matching backward must
 * be called with the same lengths set, and uploads them again (a wrapper that shares plans between calls keeps them with
 * the forward's autograd node and sets them again before the backward).  Calls of one plan that carry lengths are
 * ordered on one stream, or by the caller.
 * Null plan, a plan without CSN_LSTM_STATE, an entry outside [0, T]: CSN_ERR_INVALID_ARGUMENT (the setting is kept). */
int csn_lstm_plan_set_lengths(csnLstmPlan* plan, const int32_t* lengths);

/* Input windows: every row of the LSTM batch names the row of a SOURCE tensor it is cut from and the source step it
 * starts at.  `src_row` and `t0` are HOST arrays of B entries; the `x` of csn_lstm_forward is then
 * the source, [src_rows, src_T, I] under the call's own x_stride_b / x_stride_t.  With n = lengths[b] (T on a plan
 * without lengths), step t < n of row b reads  x[src_row[b] * x_stride_b + (t0[b] + t) * x_stride_t + i];  on a
 * CSN_LSTM_REVERSE plan recurrence step s reads time t0[b] + n - 1 - s.  Many rows may share a source row: all the
 * multi-crop views of a batch run as ONE call on the uncopied batch.
 * src_row = t0 = NULL: windows off (the default; such a plan enqueues the launches and writes the bits it did before
 * this symbol existed).  Host only and sticky until set again, like the lengths; every forward uploads the arrays in
 * stream order into device arrays the plan owns (the backward reads no x and uploads nothing).
 * IDENTITY.  A call with windows has, bit for bit, every output and every gradient of the same plan called with the same
 * lengths on the dense input  xm[b, t] = x[src_row[b], t0[b] + t]  for t < n, anything at all (NaN) for t >= n.  Only the
 * layout pass in front of the recurrence differs; dx stays the dense [B, T, I] gradient of the gathered rows.
 * NO READ PAST A WINDOW.  Nothing at t >= n is loaded (t0[b] + t may lie past the end of the source there): the layout
 * kernels store a zero instead.
 * Every plan, every path, training and inference; the lengths still need a CSN_LSTM_STATE plan.
 * Null plan, exactly one array NULL, src_row[b] outside [0, src_rows), t0[b] < 0, src_rows < 1 or src_T < 1:
 * CSN_ERR_INVALID_ARGUMENT (the setting is kept).  csn_lstm_forward returns CSN_ERR_INVALID_ARGUMENT, before it
 * enqueues anything, when t0[b] + n > src_T for some row (the lengths may be newer than the views). */
int csn_lstm_plan_set_views(csnLstmPlan* plan, const int32_t* src_row, const int32_t* t0, int32_t src_rows,
                            int32_t src_T);

/* Where the plan's later calls find y_all and dy_all, and how they store dx; host only, sticky until set again like the
 * gradient mode, and a call uses the setting it finds when it is CALLED.
 *   y_all_pitch, dy_all_pitch   elements per (b, t) row: element (b, t, h) is at base[(b T + t) pitch + h].  0 = dense (H);
 *                               otherwise pitch >= H and pitch % 4 == 0.  Only the H elements of a row are written / read.
 *   dx_add != 0                 dx[b, t, :] += ... over the valid steps (t < lengths[b]) instead of =; the padding of dx is
 *                               left as it is and nothing is zeroed.  fl32(prev + g), g the value the storing form writes.
 * For the two directions of a bidirectional layer: each plan writes its half of one [B, T, 2H] tensor (y_all = base + H
 * for the second, pitch 2H) and reads its half of that tensor's gradient in place, and the second direction adds its
 * input gradient to the first's -- no concatenation, split or sum pass.  Every path, every plan.  With (0, 0, 0), the
 * default, a plan without CSN_LSTM_REVERSE enqueues the launches and writes the bits it did before this symbol existed.
 * Null plan or a pitch that is neither 0 nor a multiple of 4 >= H: CSN_ERR_INVALID_ARGUMENT (the setting is kept). */
int csn_lstm_plan_set_io(csnLstmPlan* plan, int64_t y_all_pitch, int64_t dy_all_pitch, int dx_add);

/* What y_last is: the readout of the top layer's output sequence.  Host only and sticky until set again, like
 * csn_lstm_plan_set_io; a call uses the setting it finds when it is CALLED, and the matching backward must run with its
 * forward's setting.  Every plan and every path (0-5), training and inference, with or without CSN_LSTM_STATE,
 * CSN_LSTM_DROPOUT, CSN_LSTM_REVERSE or CSN_LSTM_RESIDENT.  The mode changes only the meaning of y_last in csn_lstm_forward
 * and of dy_last in csn_lstm_backward: y_all, h_n, c_n, every workspace buffer, csn_lstm_plan_workspace_bytes and the
 * workspace layout keep their bits.  Under CSN_READOUT_LAST (the default) a plan enqueues the launches and writes the bits
 * it did before this symbol existed.  
 * With v[b, t, h] the float32 upcast of the top layer's h at the CALLER's time t (what a y_all without output dropout
 * holds) and n = lengths[b] (T without lengths):
 *   FORWARD.   MEAN: y_last[b, h] = fl32((sum over t < n of (double)v[b, t, h]) / n): float64 partial sums over a fixed
 *              split of the steps (the same call gives the same bits every time), one rounding at the end.
 *              MAX:  y_last[b, h] = max over t < n of v[b, t, h], exact; a NaN wins, as in torch.max.
 *              Rows with n = 0 give zeros in both modes (NOT the h0 pass-through of LAST).  Output dropout does not touch
 *              the pooled value, as it does not touch y_last under LAST.
 *   BACKWARD.  dy_last enters every valid step of its row.  MEAN: each step t < n receives g = dy_last[b, h] / (float)n,
 *              an IEEE float32 division.  MAX: dy_last[b, h] enters at the FIRST caller time t that attains the maximum
 *              (the smallest t, also on a CSN_LSTM_REVERSE plan -- torch's tie rule; with a NaN the first NaN), and +0
 *              joins the other valid steps.  The argmax is recomputed from the workspace's h at backward time into a
 *              [B, H] int32 array the plan owns, under the ordering contract of the lengths upload; the forward saves
 *              nothing.  Into the top layer's gradient go, in this order: the (masked) dy_all element or 0; the pooled
 *              term, as one float32 add; the top layer's dh_n at the row's end.  Rows with n = 0 receive nothing from
 *              dy_last.
 *   IDENTITY.  A backward under MEAN or MAX has, bit for bit, every gradient of the same plan called under LAST with
 *              dy_last = NULL and dy_all' = fl32(dy_all + G), G[b, t, :] the expanded term above (plain G where dy_all is
 *              NULL).
 * Cost: the forward launches one reduction over the top layer's saved h in place of the gather of the last step; the
 * backward's term rides in the dy_all layout pass (a further instantiation of dy_in), plus for MAX one argmax pre-pass.
 * Null plan or unknown mode: CSN_ERR_INVALID_ARGUMENT (the setting is kept). */
#define CSN_READOUT_LAST 0
#define CSN_READOUT_MEAN 1
#define CSN_READOUT_MAX  2
int csn_lstm_plan_set_readout(csnLstmPlan* plan, int mode);

/* The attention readout: y_last as a weighted mean over time whose weights come from a learned query,
 * a[b, t] = softmax over t < n of scale <v[b, t, :], q>, in place of the last / mean / max of csn_lstm_plan_set_readout.
 * Host only and sticky until set again, like the other setters; it takes no stream.  All pointers are device memory:
 * q [H]; dq [H] or NULL (a frozen query); attn_out and dscore_out dense [B, T] float32 (T the descriptor's) or NULL.
 * q != NULL turns the attention readout on: it then defines y_last in csn_lstm_forward and dy_last in csn_lstm_backward,
 * whatever csn_lstm_plan_set_readout says; q == NULL turns it off and the plan's readout mode governs again.  Every plan
 * and every path (0-5), training and inference, with every plan bit and feature (state and lengths, reverse, dropout and
 * output dropout, views and io pitches, accumulation and the callback).  y_all, h_n, c_n, the workspace layout and
 * csn_lstm_plan_workspace_bytes do not change, and a plan that never calls this enqueues the launches and writes the bits
 * it did before this symbol existed.  q is read at forward and again at backward: keeping it unchanged between the two
 * is the caller's contract, as for the weights.  A forward computes the readout (and writes attn_out) only when y_last
 * is asked for.  
 * With v and n as above:
 *   FORWARD.   z64[b, t] = (double)scale * sum over h of (double)v (double)q[h]; a64 = softmax of z64 over t < n,
 *              max-subtracted, in float64; y_last[b, h] = fl32(sum over t < n of a64[b, t] (double)v[b, t, h]), one rounding;
 *              attn_out[b, t] = a32 = fl32(a64), and 0 for t >= n.  Rows with n = 0 give zero y_last and zero weights.
 *              Output dropout does not touch the pooled value.  Nothing past a row's length is read.
 *   BACKWARD.  g64[b, t] = sum over h of (double)dy_last[b, h] (double)v[b, t, h]; s64[b] = sum over t of a64 g64;
 *              dscore_out[b, t] = w32 = fl32((double)scale a64 (g64 - s64)), 0 for t >= n.  Every valid step receives
 *              G[b, t, h] = fl32(fl32(a32 dy_last[b, h]) + fl32(w32 q[h])): three separately rounded float32 operations.
 *              Into the top layer's gradient go, in this order: the (masked) dy_all element or 0; G, as ONE float32 add;
 *              the top layer's dh_n at the row's end.  dq[h] = fl32(sum over b, t < n of (double)w32[b, t] (double)v[b, t, h]),
 *              under CSN_GRAD_ACCUMULATE fl32(dq[h] + that); it is enqueued in front of the recurrence, so it is complete
 *              when the first gradient-ready callback fires.  Rows with n = 0 receive nothing from dy_last.  A backward
 *              without dy_last (or with every row empty) zeroes dq (leaves it, accumulating).
 *   RECOMPUTE. The backward computes a again from the workspace and q -- the forward saves nothing -- and writes the same
 *              attn_out bits the forward wrote.  The [B, T] scratch the plan owns is allocated on first use and written and
 *              read in stream order inside the one call.  Every split of a sum is fixed: the same call gives the same bits.
 *   IDENTITY.  A backward under attention has, bit for bit, every LSTM gradient (dx, dh0, dc0, all weight and bias
 *              gradients) of the same plan with attention off under CSN_READOUT_LAST, called with dy_last = NULL and
 *              dy_all' = fl32(dy_all + G) (plain G where dy_all is NULL).
 * Cost: three launches in the forward (scores, rows, weighted sum; two reads of the top layer's saved h), two pre-pass
 * launches in the backward plus two for dq (two reads), and the term rides in the dy_all layout pass.
 * Null plan, a non-finite scale, or dq / attn_out / dscore_out without q: CSN_ERR_INVALID_ARGUMENT (the setting is kept). */
int csn_lstm_plan_set_attention(csnLstmPlan* plan, const float* q, float scale, float* dq, float* attn_out, float* dscore_out);

/* Inter-layer dropout, with torch.nn.LSTM(dropout=p)'s meaning: for every layer l < L-1 the output sequence of layer l is
 * multiplied element-wise by an independent Bernoulli(1-p) mask and by 1/(1-p) before layer l+1's input projection.
 * NOT dropped: y_all, y_last, h_n, c_n, the recurrent h, the top layer's output.  With L = 1 it does nothing.  p = 0 is
 * off (always accepted); p = 1 drops everything.  Sticky until set again, like the lengths, and it takes no stream: the
 * setting a forward / backward finds when it is CALLED is the one it uses, and the matching backward must run with the
 * setting of its forward (a wrapper that shares plans keeps (p, seed, subsequence) with the forward's autograd node and
 * sets them again before the backward).  The caller decides when it is on (training mode); the library does not know.
 * The mask is fully specified, the same on every path, and reproducible on a CPU (csn_lstm_dropout_keep):
 *   element (l, t, b, u) of interface l (between layers l and l+1) has the 64-bit index e = ((l T + t) B + b) H + u with
 *   the PLAN's T, B, H (a call with lengths draws the mask of the same call without them);
 *   on a CSN_LSTM_REVERSE plan t is the recurrence step s (the caller's time n-1-s), as the mask is applied in the workspace:
 *   this is what makes a reverse dropout plan equal the plain dropout plan on reversed data, bit for bit;
 *   words = Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85) of
 *   counter (lo32(e >> 2), hi32(e >> 2), subsequence, 0) under key (lo32(seed), hi32(seed)); the word used is e & 3;
 *   keep iff word >= thr, thr = floor(float32(p) 2^32); at p = 1 nothing is kept, whatever the word.
 * Forward, float32 arithmetic with s = 1.0f / (1.0f - p):  h_drop = keep ? (compute dtype)(float(h) * s) : 0 -- on a
 * CSN_BF16 plan one more bf16 rounding.  Backward: the gradient that reaches layer l from layer l+1 (dgates W_ih,
 * float32) becomes keep ? dx * s : 0 BEFORE dh_n[l] is added (h_n is not dropped); dW_ih of layer l+1 is taken against
 * h_drop.  A dropped element is a selected zero, not a product: NaN / Inf there do not get through.  The gradient
 * w.r.t. x (layer 0) is never masked.  With lengths the mask covers the steps the GEMMs cover.
 * Cost: one element-wise launch in front of every next-layer input-projection GEMM and one behind every input-gradient
 * GEMM of a layer >= 1 (lstm_dropout.hip); no recurrence or GEMM kernel differs.
 * `subsequence` separates streams that share a seed (data-parallel ranks).
 * Null plan, p outside [0, 1] or NaN, p > 0 on a plan without CSN_LSTM_DROPOUT: CSN_ERR_INVALID_ARGUMENT (the setting is
 * kept). */
int csn_lstm_plan_set_dropout(csnLstmPlan* plan, float p, uint64_t seed, uint32_t subsequence);
/* The published definition of that mask, on the host: keep_host[i] = 1 if element e = first + i is kept, else 0, for
 * i in [0, n).  Host code filling a host array: no device, no stream, usable on a machine without a GPU. */
int csn_lstm_dropout_keep(uint64_t seed, uint32_t subsequence, float p, int64_t first, int64_t n, uint8_t* keep_host);

/* Output dropout: a dropout mask on y_all as the plan STORES it and on dy_all as the plan READS it, for a caller that
 * stacks single-layer plans itself (the 2L plans of a bidirectional stack, which share one [B, T, 2H] tensor per layer
 * through csn_lstm_plan_set_io).  Host only, no stream, sticky until set again like
 * csn_lstm_plan_set_io; it needs no plan bit and changes no workspace, and it is independent of
 * csn_lstm_plan_set_dropout (a plan may carry both).
 *   INDEX.  Element (b, t, h) of y_all has the 64-bit index  e = first + (b T + t) index_pitch + h,  T the plan's T and t
 *   the CALLER's time -- also on a CSN_LSTM_REVERSE plan, because this mask lives on the caller's tensor.  (NOT as in
 *   csn_lstm_plan_set_dropout, whose mask lives in the workspace and whose t is the recurrence step.)  With
 *   first = l B T 2H + d H and index_pitch = 2H the two directions d of layer l draw the halves of ONE stream over the
 *   concatenated [B, T, 2H] interface.
 *   KEEP.  csn_lstm_dropout_keep(seed, subsequence, p, e, 1): the same Philox4x32-10 words, threshold and p = 1 rule.
 *   FORWARD.  y_all[b, t, h] = t < n ? (keep ? float(h_top) * s : 0.f) : 0.f  with s = 1.0f / (1.0f - p) in float32
 *   arithmetic and n the row's length (T without lengths): a selected zero.  y_last, h_n, c_n, the recurrent h and
 *   everything inside the plan are untouched.
 *   BACKWARD.  dy_all is READ as keep ? dy * s : 0.f with the same index; NaN / Inf at a dropped or padded element do not
 *   get through.  dy_last, dh_n, dc_n are untouched.  The matching backward must run with its forward's setting, as for
 *   the lengths.
 * With p = 0 (the default) the plan enqueues the launches and writes the bits it did before this symbol existed.  With
 * p > 0 the two layout passes are the masked instantiations of the same kernels (y_out and dy_in of lstm_boundary.hip),
 * whatever the plan's pitch or direction: no extra pass and no extra launch.  They move 16 bytes per access, so with p > 0 csn_lstm_forward / csn_lstm_backward return
 * CSN_ERR_INVALID_ARGUMENT, before enqueueing anything, for a y_all / dy_all that is not 16-byte aligned.
 * Null plan, p outside [0, 1] or NaN, or with p > 0: first % 4 != 0, index_pitch % 4 != 0, index_pitch < H:
 * CSN_ERR_INVALID_ARGUMENT (the setting is kept). */
int csn_lstm_plan_set_output_dropout(csnLstmPlan* plan, float p, uint64_t seed, uint32_t subsequence, uint64_t first,
                                     int64_t index_pitch);

/* The workspace's status word: 0 = ok.  Bit CSN_STATUS_TIMEOUT: a bounded in-kernel wait of a weight-stationary
 * kernel gave up at some point since the word was last cleared (the results of that forward / backward and of every
 * later one are invalid).  Bit CSN_STATUS_NONFINITE: a NaN / Inf gradient reached the backward recurrence (the
 * operand was proven to be data, its product was not finite): the gradients are non-finite exactly as the reference's
 * autograd would leave them -- a diverged run, not a device fault.  Only the weight-stationary backward with the
 * hand-off by data (csn_lstm_plan_path() == 3, not under CSN_BWD_FLAGS) inspects its operands and can raise this bit;
 * on every other path (exact-f32, odd shapes, sequences too long for the slab ring) non-finite gradients simply
 * propagate into dw / dx, and a caller that wants the check on every path tests its gradient buffer itself
 * (trainer.check_device_status does).  It is STICKY: no forward or backward clears it.  csn_lstm_status_clear zeroes it (enqueued on
 * `stream`): call it once after allocating a workspace and after a reported error has been handled.
 * csn_lstm_status_read is a blocking device -> host read.  csn_lstm_status_raise is fault injection for tests of
 * the error path: it leaves the word exactly as a timed-out wait does (every later bounded wait then returns at
 * once, so nothing hangs; results are garbage by construction). */
#define CSN_STATUS_TIMEOUT 1
#define CSN_STATUS_NONFINITE 2
#define CSN_STATUS_STALE_SLOT 4   /* debug library (make tags) only: a hand-off ring slot served its previous occupant */
int csn_lstm_status_clear(const csnLstmPlan* plan, void* workspace, csnStream_t stream);
int csn_lstm_status_read(const csnLstmPlan* plan, const void* workspace, int* status);
int csn_lstm_status_raise(const csnLstmPlan* plan, void* workspace, csnStream_t stream);

/* Optional timing of the plan's recurrence kernels with HIP events recorded on the caller's stream in its most
 * recent forward / backward: around every weight-stationary launch (the time reported is the sum over the
 * launches, the GEMMs between them excluded), or around the whole launch loop of the per-timestep cell
 * kernels.  csn_lstm_profile_read synchronises on those events; *_launches = recurrence launches;
 * *_cells = cell problems (layer-steps) those launches advanced. */
int csn_lstm_profile_enable(csnLstmPlan* plan, int on);
int csn_lstm_profile_read(csnLstmPlan* plan, double* fwd_ms, int* fwd_launches, int* fwd_cells,
                          double* bwd_ms, int* bwd_launches, int* bwd_cells);

/* ------------------------------------------------------------------------------------
 * Building blocks of K3, exported so that each can be parity-tested on its own.
 * ---------------------------------------------------------------------------------- */
/* C[M,N] (+)= A[M,K] * Bt[N,K]^T (+ bias[N]).  dtype = type of A and Bt; C is out_dtype.
 * accumulate != 0 adds into C (float32 C only).  Replaces the input-projection /
 * input-gradient GEMMs inside ATen's LSTM. */
int csn_gemm_nt(const void* A, const void* Bt, const float* bias, void* C,
                int64_t M, int64_t N, int64_t K, int dtype, int out_dtype, int accumulate,
                csnStream_t stream);
/* C[M,N] = A[K,M]^T * B[K,N]  (weight-gradient form; float32 C, overwritten).
 * scratch: device buffer of csn_gemm_tn_scratch_bytes(M,N,K) bytes (split-K slabs). */
size_t csn_gemm_tn_scratch_bytes(int64_t M, int64_t N, int64_t K);
int csn_gemm_tn(const void* A, const void* B, float* C,
                int64_t M, int64_t N, int64_t K, int dtype, void* scratch, csnStream_t stream);

/* One LSTM cell step.  h_prev/h_out/gates are `dtype`; xproj (= x_t W_ih^T + b_ih + b_hh),
 * c_prev, c_out float32.  gates_out (may be NULL) receives post-activation i,f,g,o [B,4H]. */
int csn_lstm_cell_forward(const void* h_prev, const void* w_hh, const float* xproj, int64_t xproj_ld,
                          const float* c_prev, void* gates_out, float* c_out, void* h_out,
                          int B, int H, int dtype, csnStream_t stream);
/* One backward cell step: dh = dy + dgates_next * W_hh (w_hh_t = W_hh^T [H,4H]); writes
 * dgates_out [B,4H] and updates dc_carry [B,H] in place.  dgates_next / dy may be NULL. */
int csn_lstm_cell_backward(const void* dgates_next, const void* w_hh_t,
                           const float* dy, int64_t dy_ld,
                           const void* gates, const float* c, const float* c_prev,
                           float* dc_carry, void* dgates_out,
                           int B, int H, int dtype, csnStream_t stream);

/* ------------------------------------------------------------------------------------
 * K5  1 - mean_b cos(student_b, teacher_b), dim=1, eps=1e-8, and its gradient.
 * Replaces: CosineSimilarityLoss.forward, LstmDistillFromDinoV2Train.py:36-43.
 *   loss: [1] float32; dstudent: optional [B,D] float32 = grad_scale * dloss/dstudent.
 *   scratch: csn_cosine_loss_scratch_bytes(B) bytes of device memory owned by the caller (the per-row cosines; 8-byte
 *   aligned) -- like csn_l2_topk's: the library holds no buffer of its own between calls.
 * ---------------------------------------------------------------------------------- */
size_t csn_cosine_loss_scratch_bytes(int B);
int csn_cosine_loss(const float* student, const float* teacher, int B, int D,
                    float* loss, float* dstudent, float grad_scale, void* scratch, csnStream_t stream);

/* ------------------------------------------------------------------------------------
 * K5b  the distillation losses of the training scripts, value and gradient in two launches.
 * Both entry points follow csn_cosine_loss: float32 inputs, float64 arithmetic, each float32 output rounded once;
 * caller-owned scratch of *_scratch_bytes (8-byte aligned), no library state; everything enqueued on `stream`.  Every
 * softmax and log-softmax subtracts the row maximum first.  One wave per row; a row of D <= 1024 stays in registers, a
 * longer one is re-read in every pass.  Per-row float64 partial sums are added by a finishing launch in an order that
 * depends on the row count only: two calls on the same input give the same bits.
 *
 * csn_distill_loss: student[B,D], teacher[B,D]; logits[B,K] and labels int64[B], both or neither (NULL).
 *     loss = fl32( w_soft/B * sum_b soft_b + w_ce/B * sum_b ce_b )        (without logits: the first term alone)
 *   soft_mode CSN_SOFT_KL:          soft_b = sum_o p_t (log p_t - log_softmax(student_b / T)_o), p_t = softmax(teacher_b / T).
 *     A term with p_t == 0 is 0: nn.KLDivLoss's convention.  The explicit torch formula
 *     sum(p_t * (p_t.log() - log_q)) gives NaN there (0 * -inf) and the same value everywhere else.
 *   soft_mode CSN_SOFT_CE_OF_PROBS: soft_b = - sum_o softmax(student_b / T)_o * log_softmax(p_t)_o -- the reference's
 *     F.cross_entropy(teacher_probabilities, student_probabilities): probabilities used as logits.
 *   ce_b = - log_softmax(logits_b)[labels_b].  A label outside [0, K) makes that row's ce_b -- hence the loss -- and the
 *     row's CE gradient NaN; the label is checked before it is used, nothing outside the row is read.
 *   `logits` may be `student` itself (the KD case: one tensor distilled and classified); then K == D is required, the CE
 *     gradient is added to the soft gradient in float64 before the one rounding into dstudent, and dlogits must be NULL.
 *   Gradients (both optional), multiplied by grad_scale:
 *     KL:          dstudent = w_soft/(B T) (softmax(s/T) - p_t)
 *     CE_OF_PROBS: dstudent = - w_soft/(B T) q o (a - sum_o q a),  a = log_softmax(p_t), q = softmax(s/T)
 *     CE:          dlogits (or, aliased, added into dstudent) = w_ce/B (softmax(logits) - onehot(labels))
 *   An output passed as NULL is not written.
 *   Refused on the host before any launch: a null student / teacher / loss / scratch, B <= 0 or D <= 0, T not finite or
 *   not positive, an unknown soft_mode, logits without labels or with K <= 0, the alias with K != D, dlogits without
 *   logits or together with the alias, misaligned scratch.
 *   The library's losses:  FeatureDistributionLoss   CE_OF_PROBS, logits = pred_label, w_soft = beta, w_ce = alpha
 *                          loss_fn_kd                KL, alias, w_soft = alpha T^2 / D, w_ce = 1 - alpha
 *                          FeatureDistributionLossKD KL, alias, w_soft = 0.25 T^2, w_ce = 0.75
 *                          FeatureDistributionLossSoft KL, no logits, w_soft = T^2
 *   Replaces: LstmDistillFromDinoV2Train.py:107-140, LstmDistillFromDinoV2TrainSpampinato.py:107-184,
 *   LstmDistillFromDinoV2Eval.py:106-146.
 *
 * csn_dino_loss: student[V,B,D], teacher[G,B,D]; center + b * center_stride_b is the centre of batch row b:
 *   center_stride_b 0 = one shared [D] centre, D = the per-sample [B,D] centre the reference's update_center makes of it.
 *     q[g,b] = softmax((teacher[g,b] - center_b) / teacher_temp),  logp[v,b] = log_softmax(student[v,b] / student_temp)
 *     loss = fl32( - c * sum_{g,b} sum_{v in S_g} q[g,b] . logp[v,b] ),  c = 1 / (G B (V - 1))
 *   pairing CSN_DINO_SKIP_FIRST: S_g = {1 .. V-1} (the reference's chunk(1), LstmDistillation.py:128);
 *   pairing CSN_DINO_SKIP_SAME:  S_g = {v != g} (the pairing of the DINO paper).
 *   dstudent[V,B,D] (optional) = grad_scale * (-c / student_temp) (sum_{g: v in S_g} q[g,b] - n_v softmax(student[v,b] / student_temp)),
 *   n_v = |{g : v in S_g}|; a view that no pair uses gets an explicit zero row.
 *   Refused on the host: null pointers (other than dstudent), B <= 0 or D <= 0, V < 2, G outside [1, V], a
 *   center_stride_b other than 0 or D, temperatures not finite or not positive, an unknown pairing, misaligned scratch.
 *   The centre update (and its all-reduce) is not part of the call.  Replaces: DINOLoss.forward, LstmDistillation.py:118-148.
 * ---------------------------------------------------------------------------------- */
enum csnSoftMode { CSN_SOFT_KL = 0, CSN_SOFT_CE_OF_PROBS = 1 };
enum csnDinoPairing { CSN_DINO_SKIP_FIRST = 0, CSN_DINO_SKIP_SAME = 1 };
size_t csn_distill_loss_scratch_bytes(int B);
int csn_distill_loss(const float* student, const float* teacher, int B, int D, const float* logits, int K,
                     const int64_t* labels, int soft_mode, double T, double w_soft, double w_ce, float* loss,
                     float* dstudent, float* dlogits, float grad_scale, void* scratch, csnStream_t stream);
size_t csn_dino_loss_scratch_bytes(int B, int D);
int csn_dino_loss(const float* student, const float* teacher, int V, int G, int B, int D, const float* center,
                  int64_t center_stride_b, double teacher_temp, double student_temp, int pairing, float* loss,
                  float* dstudent, float grad_scale, void* scratch, csnStream_t stream);

/* ------------------------------------------------------------------------------------
 * Optimiser step of the hot loop over ONE flat float32 parameter / gradient / state buffer (16-byte aligned).
 * Replaces: torch.optim.RMSprop(model.parameters(), lr=...).step(), LstmDistillFromDinoV2Train.py:329,373, with
 * that call's defaults: square_avg <- alpha square_avg + (1 - alpha) g^2 ; p <- p - lr g / (sqrt(square_avg) + eps)
 * (alpha 0.99, eps 1e-8; no momentum, not centred, no weight decay).
 * ---------------------------------------------------------------------------------- */
int csn_rmsprop_step(float* params, const float* grads, float* square_avg, int64_t n,
                     float lr, float alpha, float eps, csnStream_t stream);

/* ------------------------------------------------------------------------------------
 * Optimiser tails over flat float32 buffers cut into SEGMENTS, one per parameter tensor (trainer.FlatGrads packs
 * tensors back to back: a segment boundary is an arbitrary element offset; only the buffer bases are 16-byte aligned).
 * Every call takes (n, nseg, table): n elements, nseg segments, and a SEGMENT TABLE in caller-owned device memory of
 * csn_flat_segments_scratch_bytes(nseg, n) bytes (16-byte aligned), filled once by csn_flat_segments_prepare and then
 * used by any number of calls ordered behind it.  It also holds the float64 partial sums of the norm passes, so two
 * calls that share a table must be ordered on one stream (one table per optimiser).  The library keeps no state.
 * Per-segment flags: CSN_SEG_DECAYED = weight decay applies, CSN_SEG_SCALED = the clip (Adam) / the LARS trust ratio
 * applies.  All sums of squares are two-stage: one float64 partial per (segment, 2048-element chunk), added per segment
 * in a fixed order -- no floating-point atomics, two runs on the same input give the same bits.
 * ---------------------------------------------------------------------------------- */
#define CSN_SEG_DECAYED 1
#define CSN_SEG_SCALED  2
size_t csn_flat_segments_scratch_bytes(int nseg, int64_t n);
/* seg_end: [host] nseg exclusive end offsets, strictly ascending from above 0, the last one == n.  flags: [host] nseg
 * flag words, or NULL = both flags on every segment.  Enqueues the table's construction on `stream`. */
int csn_flat_segments_prepare(const int64_t* seg_end, const int32_t* flags, int nseg, int64_t n, void* table,
                              csnStream_t stream);
/* Per-segment L2 norms.  b == NULL: |a_s|.  b != NULL: |a_s| and |d_s|, d = b + weight_decay a on decayed segments and
 * d = b elsewhere (LARS: a = params, b = grads).  norms_out: optional [nseg] (b == NULL) or [2, nseg] float32.
 * Replaces: torch._foreach_norm / p.grad.norm(2) per parameter, utils/utils.py:136, EEG-BarlowNetworks/optim.py:30-31. */
int csn_flat_segment_norms(const float* a, const float* b, float weight_decay, int64_t n, int nseg, void* table,
                           float* norms_out, csnStream_t stream);
/* g_s <- min(1, clip / (|g_s| + 1e-6)) g_s in place on every segment; norms_out: optional [nseg] float32 pre-clip norms
 * (stays on the device: no host round trip).  Replaces: clip_gradients, utils/utils.py:132-141. */
int csn_flat_clip(float* grads, int64_t n, int nseg, void* table, float clip, float* norms_out, csnStream_t stream);
/* One Adam (decoupled == 0) / AdamW (decoupled != 0) step, t >= 1 the number of this step, with the arithmetic of
 * torch's single-tensor path:  m <- m + (1 - beta1)(g - m);  v <- beta2 v + (1 - beta2) g^2;
 * p <- p - (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps), bc_i = 1 - beta_i^t (the scalar quotients are formed here in
 * double and rounded to float once); on decayed segments p <- p (1 - lr weight_decay) first (AdamW) or
 * g <- g + weight_decay p (Adam).  clip > 0: a norm pass over grads runs first and the step uses
 * g <- min(1, clip / (|g_s| + 1e-6)) g on scaled segments (the DINO per-tensor clip); norms_out as in csn_flat_clip.
 * grads is read, never written.  One launch (three with clip).
 * Replaces: torch.optim.AdamW(...).step(), LstmDistillFromDinoV2TrainSpampinato.py:378 and LstmDistillation.py:150
 * (behind the clip loop of utils/utils.py:132-141); torch.optim.Adam(...).step(), LSTMDistill.py:322. */
int csn_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, int nseg,
                  void* table, int64_t t, double lr, double beta1, double beta2, double eps, double weight_decay,
                  int decoupled, double clip, float* norms_out, csnStream_t stream);
/* One LARS step: d = g + weight_decay p (decayed segments); d <- d eta |p_s| / |d_s| where both norms are > 0 (scaled
 * segments); mu <- momentum mu + d; p <- p - lr mu.  The norm pass and the step: three launches.
 * Replaces: LARS.step, EEG-BarlowNetworks/optim.py:17-44. */
int csn_lars_step(float* params, const float* grads, float* mu, int64_t n, int nseg, void* table, double lr,
                  double weight_decay, double momentum, double eta, csnStream_t stream);

/* ------------------------------------------------------------------------------------
 * Global-norm gradient clipping and the non-finite step skip, decided ON THE DEVICE: one pass
 * over the flat gradient buffer leaves a 16-byte record, and the guarded optimiser steps read their coefficient from it.
 * The host never sees the norm, so the feature costs no round trip.
 * Replaces: torch.nn.utils.clip_grad_norm_(params, max_norm) (its coefficient min(1, max_norm / (|g| + 1e-6))), and the
 * step that fp16_scaler.step(optimizer) does NOT take when a gradient is non-finite, LstmDistillation.py:606-613.
 *
 * csnStepGuard: 16 bytes of caller-owned device memory, 16-byte aligned, zeroed ONCE by the caller (skipped counts up
 * over the record's life; the other three words are overwritten by every csn_grad_guard).
 * ---------------------------------------------------------------------------------- */
typedef struct { float norm; float scale; uint32_t finite; uint32_t skipped; } csnStepGuard;
/* Bytes of caller-owned device scratch (16-byte aligned) for a buffer of n elements; 0 (and an error message) for n <= 0. */
size_t csn_grad_guard_scratch_bytes(int64_t n);
/* S = sum (double)g_i^2, two-stage: one float64 partial per 2048-element chunk, the partials added in ascending chunk
 * order by one wave -- no floating-point atomics, two runs give the same bits; a float squared is exact in double, so S is
 * non-finite exactly when some g_i is.  Two launches.  The record then holds
 *     norm = (float)sqrt(S),  finite = isfinite(S),  skipped += !finite,
 *     scale = finite ? (float)min(1.0, max_norm / (sqrt(S) + 1e-6)) : 0     (clip_grad_norm_'s coefficient).
 * max_norm = +INFINITY: measure and gate only (scale is exactly 1.0f or 0).  max_norm <= 0 and NaN are refused.
 * grads (16-byte aligned) is read, never written. */
int csn_grad_guard(const float* grads, int64_t n, double max_norm, void* scratch, csnStepGuard* guard, csnStream_t stream);
/* The steps above behind a record that a csn_grad_guard earlier on `stream` filled.  Wherever the unguarded step reads g
 * -- the norm passes of LARS and of Adam's per-tensor clip included -- the guarded one reads g' = fl32(scale g), rounded
 * once (never contracted into a following multiply-add), then runs the identical arithmetic:
 *     step_guarded(g) == step(g') bit for bit.
 * Adam with a finite max_norm and clip > 0 is the sequential composition: the global clip, then the per-tensor clip of g'.
 * finite == 0: the step writes NOTHING -- parameters, every state buffer, norms_out and the table's sums keep their bits.
 * grads is never written.  guard == NULL is refused (the unguarded entry points exist for that).
 * csn_adam_step_guarded: t stays the HOST's count of calls, skipped calls included (the bias corrections of the steps
 * after a skip are those of t, not of the number of steps taken): the host does not read the record back.
 * Replaces: clip_grad_norm_ + optimizer.step(), and the skip of fp16_scaler.step(optimizer), LstmDistillation.py:606-613. */
int csn_rmsprop_step_guarded(float* params, const float* grads, float* square_avg, int64_t n, float lr, float alpha,
                             float eps, const csnStepGuard* guard, csnStream_t stream);
int csn_adam_step_guarded(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, int nseg,
                          void* table, int64_t t, double lr, double beta1, double beta2, double eps, double weight_decay,
                          int decoupled, double clip, float* norms_out, const csnStepGuard* guard, csnStream_t stream);
int csn_lars_step_guarded(float* params, const float* grads, float* mu, int64_t n, int nseg, void* table, double lr,
                          double weight_decay, double momentum, double eta, const csnStepGuard* guard, csnStream_t stream);

/* ------------------------------------------------------------------------------------
 * K7  Barlow-Twins reduction over the cross-correlation matrix c[D,D] (float32):
 *   out[0] = sum_i (c_ii - 1)^2,  out[1] = sum_{i!=j} c_ij^2      (float32[2])
 * Replaces: EEG-BarlowNetworks/net.py:6-9,39-40.
 * ---------------------------------------------------------------------------------- */
int csn_barlow_offdiag_sqsum(const float* c, int D, float* out, csnStream_t stream);

/* ------------------------------------------------------------------------------------
 * K7b  the Barlow-Twins loss itself, value and both gradients: BatchNorm1d(affine=False) in training
 * mode on z1[B,D] and z2[B,D] (float32), the cross-correlation, on + lambd * off, and the closed-form backward through the
 * batch norm.  Float64 arithmetic on the float32 inputs, every float32 output rounded once; caller-owned `saved`
 * (csn_barlow_saved_bytes) and `scratch` (csn_barlow_scratch_bytes), both 8-byte aligned; no library state; everything is
 * enqueued on `stream`.  Two calls, because the reference all-reduces c between them (net.py:38) outside autograd: each rank
 * back-propagates d loss(c summed) / d c through its own term c_local only.
 *
 * csn_barlow_corr, for z = z1 and z = z2 and every column i:
 *     mean_i = sum_b z[b,i] / B,   var_i = sum_b (z[b,i] - mean_i)^2 / B   (two passes, biased),   rstd_i = 1 / sqrt(var_i + eps)
 *     zn[b,i] = (z[b,i] - mean_i) rstd_i
 *     c[i,j] = inv_batch * sum_b z1n[b,i] z2n[b,j]          float64 [D,D] row-major, THIS rank's term;
 *   inv_batch = 1 / the GLOBAL batch (all ranks).  saved = mean1[D], rstd1[D], mean2[D], rstd2[D] (float64).
 *   running_mean / running_var (float32 [D], both NULL or both set): the ONE buffer pair is updated twice, for z1 and then
 *   for z2, as one nn.BatchNorm1d called twice:   rm <- fl32((1 - momentum) rm + momentum mean)
 *                                                 rv <- fl32((1 - momentum) rv + momentum var B / (B - 1))
 * csn_barlow_grad, c = the sum of every rank's term, c_local = this rank's (the same pointer on one rank):
 *     G[i,j] = 2 (c[i,i] - 1) on the diagonal, 2 lambd c[i,j] off it
 *     loss = fl32( sum_i (c_ii - 1)^2 + lambd sum_{i != j} c_ij^2 )                       (not scaled by grad_scale)
 *     k1[i] = sum_j G[i,j] c_local[i,j] / B,      k2[j] = sum_i G[i,j] c_local[i,j] / B
 *     dz1[b,i] = fl32( grad_scale rstd1[i] (inv_batch sum_j G[i,j] z2n[b,j] - z1n[b,i] k1[i]) )
 *     dz2[b,j] = fl32( grad_scale rstd2[j] (inv_batch sum_i G[i,j] z1n[b,i] - z2n[b,j] k2[j]) )
 *   -- the batch-norm backward (dzn - mean_b dzn - zn mean_b(dzn zn)) rstd in closed form: mean_b(dzn zn) is k, and
 *   mean_b dzn is identically zero because zn is column-centred.  dz1 / dz2 passed as NULL are not written.
 *   Every contraction is one fma chain per result in ascending order; the sums over c are added in an order that depends on
 *   D only: two calls on the same input give the same bits.  NaN / Inf in the inputs propagate.
 * Launches: corr 2, grad 3 (2 without a gradient).
 * Refused on the host before any launch: a null z1 / z2 / c / c_local / saved / loss / scratch; B < 2 (BatchNorm1d refuses
 * one row in training) or D < 1; eps, inv_batch or lambd not finite, eps or inv_batch <= 0; momentum outside [0, 1];
 * exactly one running pointer; c, c_local, saved or scratch not 8-byte aligned.
 * Replaces: BarlowTwins.forward and its autograd backward, EEG-BarlowNetworks/net.py:33-42.
 * ---------------------------------------------------------------------------------- */
size_t csn_barlow_saved_bytes(int D);
size_t csn_barlow_scratch_bytes(int B, int D);
int csn_barlow_corr(const float* z1, const float* z2, int B, int D, double eps, double inv_batch, double* c, void* saved,
                    float* running_mean, float* running_var, double momentum, csnStream_t stream);
int csn_barlow_grad(const float* z1, const float* z2, int B, int D, const double* c, const double* c_local,
                    const void* saved, double inv_batch, double lambd, float grad_scale, float* loss, float* dz1,
                    float* dz2, void* scratch, csnStream_t stream);

/* ------------------------------------------------------------------------------------
 * K7c  the symmetric in-batch contrastive (InfoNCE / CLIP) loss of a student against a frozen teacher, exact over the
 * GLOBAL batch of all ranks.  s_all / t_all [N,D] float32: every rank's rows in rank order (the
 * all-gathered batch); this rank owns rows row0 .. row0+B-1.  group_all [N] int32 or NULL: key j is left out of query i's
 * softmax when group[i] == group[j] and j != i (duplicates of the positive); NULL leaves nothing out.  a = logit_scale.
 *     s^_i = s_i / max(|s_i|, 1e-12),  t^ likewise                         (F.normalize)
 *     lA_i = log sum_{j allowed} exp(a s^_i . t^_j)      lB_i = log sum_{j allowed} exp(a t^_i . s^_j)      p_i = a s^_i . t^_i
 *     L    = (1/N) sum_i [ w_a (lA_i - p_i) + w_b (lB_i - p_i) ]
 *     dL/ds^_i = (a/N) [ w_a (sum_j PA_ij t^_j - t^_i) + w_b (sum_k PB_ki t^_k - t^_i) ]
 *         PA_ij = exp(a s^_i . t^_j - lA_i),   PB_ki = exp(a t^_k . s^_i - lB_k),   both 0 where the key is left out
 *     ds_i = grad_scale (dL/ds^_i - s^_i (s^_i . dL/ds^_i)) / max(|s_i|, 1e-12)      the projection only where |s_i| > 1e-12
 *     dL/da, the local rows' part = (1/N) sum_{i local} [ w_a (sum_j PA_ij s^_i . t^_j - s^_i . t^_i)
 *                                                        + w_b (sum_j PB_ij t^_i . s^_j - s^_i . t^_i) ]
 * Two calls, because PB_ki needs lB_k of rows other ranks own and nothing else from them: between the calls the host
 * all-gathers lB (N float64) and all-reduces the loss partial.  On one rank lse_a_local and lse_b_all are rows 0 and 1 of
 * rows_out on the device.  The teacher gets no gradient.
 *   csn_contrastive_lse   rows_out float64 [3][B]: lA, lB, p of the local rows; loss_part float64 [1]: the local rows' part of
 *                         L, added in an order that depends on B only.  3 launches.
 *   csn_contrastive_grad  ds float32 [B,D], holding grad_scale; dscale_part float64 [1] or NULL: the local rows' part of
 *                         dL/da, not scaled by grad_scale.  4 launches, 5 with dscale_part.
 * Float64 arithmetic on the float32 inputs, every float32 output rounded once; every log-sum-exp subtracts its maximum.  A
 * row's lA, lB, p and ds depend on (N, D) and the data alone, not on B or row0; partial sums over key tiles (64 keys) and the
 * splits of the ds contraction (256 keys) are merged in ascending order; two calls give the same bits.  NaN / Inf propagate
 * as in the torch expression (a key that is left out propagates nothing).  Any int32 is a group id; a query whose every
 * other key is left out has loss term 0 and a zero gradient.
 * scratch: caller-owned, 8-byte aligned, csn_contrastive_scratch_bytes(B, N, D) =
 *     8 * (3 N + 4 ceil(N/64) B + B + B N + ceil(N/256) B D)  bytes
 *   (norms | per-tile (max, sum exp) pairs or row sums | the diagonal | the B x N weight block | the ds splits); the same
 *   buffer serves both calls, neither reads what the other wrote.  0 for arguments the calls refuse.  No library state;
 *   everything is enqueued on `stream`.
 * Refused on the host before any launch: a null pointer other than group_all / dscale_part; N, D or B <= 0, row0 < 0,
 * row0 + B > N; logit_scale not finite or <= 0; w_a or w_b not finite; rows_out, loss_part, lse_a_local, lse_b_all,
 * dscale_part or scratch not 8-byte aligned.
 * Replaces: nothing in the reference (its scripts have no contrastive objective); the torch expression is
 * F.normalize x 2, one matmul, two cross_entropy and autograd.
 * ---------------------------------------------------------------------------------- */
size_t csn_contrastive_scratch_bytes(int B, int N, int D);
int csn_contrastive_lse(const float* s_all, const float* t_all, const int* group_all, int N, int D, int row0, int B,
                        double logit_scale, double w_a, double w_b, double* rows_out, double* loss_part, void* scratch,
                        csnStream_t stream);
int csn_contrastive_grad(const float* s_all, const float* t_all, const int* group_all, int N, int D, int row0, int B,
                         double logit_scale, const double* lse_a_local, const double* lse_b_all, double w_a, double w_b,
                         double grad_scale, float* ds, double* dscale_part, void* scratch, csnStream_t stream);

/* ------------------------------------------------------------------------------------
 * K7d  the contrastive (InfoNCE) loss of student rows against a fixed BANK of frozen teacher rows: every row of the bank
 * is a key of every query, so every image of the dataset is a negative at every step.
 * bank [M,D] float32; bank_inv_norm [M] float64 = 1 / max(|t_m|, 1e-12), computed once per bank by csn_bank_norms (a NaN
 * norm stays NaN); bank_group [M] int32 or NULL; s [B,D] float32; pos [B] int32: row i's positive as an index into the
 * bank; a = logit_scale.  Key m is left out of query i when bank_group[m] == bank_group[pos_i] and m != pos_i (the
 * positive itself never is); NULL leaves nothing out.
 *     s^_i = s_i / max(|s_i|, 1e-12),  t^_m = t_m bank_inv_norm[m]          (F.normalize)
 *     l_i = log sum_{m allowed} exp(a s^_i . t^_m)        p_i = a s^_i . t^_pos_i
 *     loss_part = inv_rows sum_i (l_i - p_i)
 *     dL/ds^_i = a inv_rows (sum_m P_im t^_m - t^_pos_i),      P_im = exp(a s^_i . t^_m - l_i), 0 where left out
 *     ds_i = grad_scale (dL/ds^_i - s^_i (s^_i . dL/ds^_i)) / max(|s_i|, 1e-12)      the projection only where |s_i| > 1e-12
 *     dscale_part = inv_rows sum_i (sum_m P_im s^_i . t^_m - s^_i . t^_pos_i)        not scaled by grad_scale
 * One call: against a fixed bank the loss is a plain mean over rows, nothing crosses ranks (inv_rows = 1 / the rows the
 * mean is over: the local batch, or the whole batch when the call sees a micro-batch of it).  The bank gets no gradient.
 *   rows_out float64 [2][B]: l, p;  loss_part float64 [1];  ds float32 [B,D] or NULL: the value part only (4 launches
 *   instead of 6);  dscale_part float64 [1] or NULL.
 * Float64 arithmetic on the float32 inputs, every float32 output rounded once; the logit is the product a (s^ . t^) rounded
 * on its own; every log-sum-exp subtracts its maximum.  A row's l, p and ds depend on (M, D), the scalars and the data
 * alone, not on B or on the row's place in the batch: the sums over keys run per row, thread x of 256 over keys x, x + 256,
 * ... in ascending order and then a fixed tree, and the ds contraction in ceil(M / w) splits of w = max(64, 32 ceil(M / 2048))
 * keys merged in ascending order.  loss_part and dscale_part add the rows in an order that depends on B only.  Two calls
 * give the same bits.
 * A key that is left out never goes through exp (a NaN there propagates nothing, into no output); a NaN in an allowed
 * key makes that query's l, p-term and ds row NaN and no other row's; a pos_i outside [0, M) gives row i a NaN l, p and
 * ds row and indexes nothing (csn_distill_loss's convention for a bad label; no device assert).  A query whose only
 * allowed key is its positive has l == p bit for bit, loss term 0 and a ds row of zeros.
 * scratch: caller-owned, 8-byte aligned, csn_bank_contrastive_scratch_bytes(B, M, D) =
 *     8 * (4 B + B M + ceil(M / w) B D)  bytes,  w as above
 *   (norms and per-row terms | the B x M dot products, then weights | the ds splits).  0 for arguments the call refuses.
 *   No library state; everything is enqueued on `stream`.
 * Refused on the host before any launch: a null pointer other than bank_group / ds / dscale_part; B, M or D <= 0 (B above
 * 1 048 560); logit_scale not finite or <= 0; inv_rows or grad_scale not finite; bank_inv_norm, rows_out, loss_part,
 * dscale_part or scratch not 8-byte aligned (csn_bank_norms: inv_norm).
 * Replaces: nothing in the reference; the torch expression is F.normalize x 2, one matmul, masked_fill, cross_entropy.
 * ---------------------------------------------------------------------------------- */
int csn_bank_norms(const float* bank, int M, int D, double* inv_norm, csnStream_t stream);
size_t csn_bank_contrastive_scratch_bytes(int B, int M, int D);
int csn_bank_contrastive(const float* s, int B, int D, const float* bank, const double* bank_inv_norm,
                         const int32_t* bank_group, int M, const int32_t* pos, double logit_scale, double inv_rows,
                         double grad_scale, double* rows_out, double* loss_part, float* ds, double* dscale_part, void* scratch,
                         csnStream_t stream);

/* ------------------------------------------------------------------------------------
 * K8  exact squared-L2 top-k.  Replaces: faiss.IndexFlatL2(d).add / .search(k),
 * utils/Utilities.py:45-55.  gallery [Ng,D], query [Nq,D] float32; out_idx [Nq,k]
 * int64, out_dist [Nq,k] float32, ascending, ties -> lower gallery index.
 * scratch: device buffer of csn_l2_topk_scratch_bytes(Ng,Nq) bytes.  1 <= k <= min(64, Ng): anything else is refused.
 * The selection runs on the float64 distances; out_dist is their float32 rounding (inf where that overflows).
 * ---------------------------------------------------------------------------------- */
size_t csn_l2_topk_scratch_bytes(int64_t Ng, int64_t Nq);
int csn_l2_topk(const float* gallery, const float* query, int64_t Ng, int64_t Nq, int D, int k,
                int64_t* out_idx, float* out_dist, void* scratch, csnStream_t stream);

/* K8, tiled form: the same search (utils/Utilities.py:45-55) without the [Nq,Ng] distance matrix, for k up to 1024.
 * A workgroup owns 64 queries and one of `splits` contiguous ranges of gallery rows; it computes 64 x 64 distance tiles
 * in registers, keeps a sorted list of the k best per query, and a second kernel merges the ranges' lists.
 *   1 <= k <= min(1024, Ng); inputs finite float32; splits = 0: the library chooses (at most 64), > 0: forced (tests,
 *   tuning; more than the gallery allows is clamped).  Null pointers (other than out_dist64), splits < 0 and sizes <= 0
 *   are refused on the host before any launch; the scratch function returns 0 for arguments the call refuses.
 *   Distances: acc = 0.0; for d = 0 .. D-1 ascending: df = (double)q[d] - (double)g[d]; acc = fma(df, df, acc) -- one chain
 *   per pair, the bits of csn_l2_topk.  Selection: the k smallest under (float64 distance, gallery index), ascending.
 *   out_dist64 (may be NULL) holds those float64 distances, out_dist their float32 rounding (inf where that overflows).
 *   For k <= 64 out_idx and out_dist equal csn_l2_topk's exactly, for every value of splits.
 *   scratch: csn_l2_topk_tiled_scratch_bytes(Ng, Nq, k) bytes = 2 buffers x S x Nq x k x 16 + S x Nq x 8 (rounded up to
 *   256), S = min(ceil(Ng / 64), max(8, the library's choice of splits)) -- independent of Ng beyond 64 tiles. */
size_t csn_l2_topk_tiled_scratch_bytes(int64_t Ng, int64_t Nq, int k);
int csn_l2_topk_tiled(const float* gallery, const float* query, int64_t Ng, int64_t Nq, int D, int k, int splits,
                      int64_t* out_idx, float* out_dist, double* out_dist64, void* scratch, csnStream_t stream);

/* K8, channel discovery: the greedy forward selection of EEG channels of
 * TestRetrieval_Perils_DiscoverChannels.py:125-351 without one index build and search per candidate.  The squared L2
 * distance over a channel subset is the sum of the per-channel distances: csn_chan_l2_dist computes those once,
 * csn_chan_l2_select runs one round's selection for every candidate at once, csn_chan_l2_accumulate adds the accepted
 * channel to the running sum.  All three refuse on the host, before any launch: null pointers (other than the ones
 * marked nullable), sizes <= 0, and what each lists below.
 *
 * csn_chan_l2_dist: gallery / query are float32 recordings, channel-first: element (n, c, t) at base[n*ld_n + c*ld_c + t]
 *   (strides in elements, time stride 1), n < Ng / Nq, c < C, t < T.  ld_c >= T and ld_n >= (C-1)*ld_c + T (a slice of a
 *   larger tensor is fine); only float alignment is needed.  Window [t0, t1): 0 <= t0 < t1 <= T.  channels: HOST array of
 *   nch channel numbers in [0, C), in any order, repeats allowed; NULL = all C channels ascending (nch ignored).
 *   Dc[nch, Nq, Ng] float64, dense:
 *     Dc[j,q,g] = acc, acc = 0.0; for t = t0 .. t1-1: df = (double)Q[q,c_j,t] - (double)G[g,c_j,t]; acc = fma(df, df, acc)
 *   -- one chain per (channel, pair), never split: the bits csn_l2_topk_tiled's out_dist64 holds for the feature matrix
 *   X[:, c_j, t0:t1].  Inputs finite.  Ng <= 64 * 65535.
 * csn_chan_l2_select: base[Nq,Ng] float64 (NULL: no fixed channel yet), Dc[nc,Nq,Ng] float64, gallery_class[Ng] /
 *   query_class[Nq] int32 (device; needed only by out_hits / out_top1).  For every candidate j and query q: the k
 *   smallest of v[g] = base[q,g] + Dc[j,q,g] (one float64 add; Dc[j,q,g] itself without base) under (value, gallery index)
 *   ascending, ties -> lower index.  1 <= k <= min(64, Ng); nc <= 65535.  Outputs, each nullable, at least one given:
 *   out_idx[nc,Nq,k] int64, out_dist[nc,Nq,k] float64 (the v of the chosen rows),
 *   out_hits[nc,Nq] int32 = how many of the k have gallery_class == query_class[q],
 *   out_top1[nc,Nq] int32 = gallery_class of the first.
 * csn_chan_l2_accumulate: base[i] = first ? D_one[i] : base[i] + D_one[i], i < n, float64.  A subset's matrix is therefore
 *   ((D_s1 + D_s2) + ...) + D_cand in selection order. */
int csn_chan_l2_dist(const float* gallery, int64_t g_ld_n, int64_t g_ld_c, const float* query, int64_t q_ld_n,
                     int64_t q_ld_c, int64_t Ng, int64_t Nq, int C, int T, int t0, int t1, const int32_t* channels, int nch,
                     double* Dc, csnStream_t stream);
int csn_chan_l2_select(const double* base, const double* Dc, int nc, int64_t Nq, int64_t Ng, const int32_t* gallery_class,
                       const int32_t* query_class, int k, int64_t* out_idx, double* out_dist, int32_t* out_hits,
                       int32_t* out_top1, csnStream_t stream);
int csn_chan_l2_accumulate(double* base, const double* D_one, int64_t n, int first, csnStream_t stream);

/* K8, retrieval evaluation behind the search: the exact merge of sharded candidate lists and the
 * per-class hit counts of utils/Utilities.py:57-99 on the device.  Both are stateless, run on `stream`, and refuse on the
 * host, before any launch: null pointers (other than the ones marked nullable), sizes <= 0, and the limits listed.
 *
 * csn_topk_merge: D_parts[P,Nq,k_in] float64 and I_parts[P,Nq,k_in] int64, dense; a padding entry is (+inf, -1) -- any
 *   entry with a negative index is padding, whatever its distance.  For every query the k smallest real entries of its
 *   P * k_in candidates under (float64 distance, index), ascending, ties -> lower index (equal pairs: the lower part, then
 *   the lower place); a real distance may be +inf.  1 <= k <= 1024, 1 <= k_in <= 1024, 1 <= P <= 64, P * k_in >= k.
 *   out_idx[Nq,k] int64; out_dist64[Nq,k] float64 and out_dist[Nq,k] float32 (its float32 rounding, inf where that
 *   overflows) may each be NULL.  A query with fewer than k real candidates gets (+inf, -1) in the remaining places.
 *   csn_topk_merge_staged_max: up to this many candidates per query (P * k_in) are kept in LDS, more are re-read from L2.
 * csn_topk_class_metrics: idx[Nq,k] int64 neighbour lists (1 <= k <= 1024; an index outside [0, Ng) counts as a miss and
 *   is never dereferenced), gallery_class[Ng] / query_class[Nq] int32 class ids in [0, n_classes), n_classes <= 65536 (a
 *   query whose class is outside adds to no class row).  Outputs, each nullable, at least one given:
 *   out_hits[Nq] int32 = how many of the k have the query's class; out_top1[Nq] int32 = class of the first (-1: none);
 *   out_pred[Nq] int32 = the query's class where hits > 0, else out_top1;
 *   out_class[n_classes,4] int64 = per class {queries, queries with hits > 0, sum of hits, lowest query index or -1};
 *   out_top1_correct[1] int64 = queries whose first neighbour has their class.
 *   Integer sums and a minimum only: the result does not depend on the grid, the order of execution or the stream. */
int csn_topk_merge_staged_max(void);
int csn_topk_merge(const double* D_parts, const int64_t* I_parts, int P, int64_t Nq, int k_in, int k, int64_t* out_idx,
                   double* out_dist64, float* out_dist, csnStream_t stream);
int csn_topk_class_metrics(const int64_t* idx, int64_t Nq, int k, const int32_t* gallery_class, int64_t Ng,
                           const int32_t* query_class, int n_classes, int32_t* out_hits, int32_t* out_top1,
                           int32_t* out_pred, int64_t* out_class, int64_t* out_top1_correct, csnStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CSN_HIP_H */
