// CU-resident LSTM recurrence for hidden sizes up to 128 (lstm_resident.hip; path 5, CSN_LSTM_RESIDENT plans): the steps
// of one chunk of one layer run inside ONE launch, W_hh in the registers of one workgroup, h / dgates of its 16 batch
// rows in LDS.  Workspace, operand layout and arithmetic are those of the per-step cells of lstm_cell.hip (path 0).
#pragma once
#include "csn_common.h"

namespace csn {

constexpr int kResidentMaxH = 128;

// One (layer, chunk) problem of a launch.  The saved tensors are the layer's, based at step 0 / slot 0 (time-major
// [T,B,*] or [T+1,B,H]); the kernel walks steps t0 .. t0 + nsteps - 1.
struct ResFwdOne {
  const void* w_hh;       // [4H,H] compute dtype
  const float* xproj;     // [T,B,4H]
  float* c_all;           // [T+1,B,H]: slot t0 read, slots t0+1 .. written
  void* h_all;            // [T+1,B,H] compute dtype, likewise
  void* gates;            // [T,B,4H] compute dtype, NULL on an inference plan
  int t0, nsteps;
};
struct ResFwdBatch { ResFwdOne p[4]; };
// backward: steps t_hi, t_hi - 1, .. t_hi - nsteps + 1
struct ResBwdOne {
  const void* w_hh_t;     // [H,4H] compute dtype
  const float* dy;        // [T,B,H] gradient w.r.t. the layer's output at every step, or NULL:
  const float* dy_last;   // [B,H] the one at step T-1 (may be NULL too)
  const void* gates;      // [T,B,4H]
  const float* c_all;     // [T+1,B,H]
  float* dc_carry;        // [B,H]: read at the start of the launch, written at its end
  void* dgates;           // [T,B,4H]: step t_hi + 1 read (absent at T-1), steps of the launch written
  int t_hi, nsteps;
};
struct ResBwdBatch { ResBwdOne p[4]; };

bool resident_supported(int H);
int launch_resident_fwd(const ResFwdBatch& b, int np, int B, int H, int dtype, hipStream_t st);
// lengths: [B] device, or NULL (every row runs all T steps)
int launch_resident_bwd(const ResBwdBatch& b, int np, int B, int T, int H, int dtype, const int* lengths, hipStream_t st);

}  // namespace csn
