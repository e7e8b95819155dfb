// CU-resident LSTM recurrence, H <= 128 (path 5; a plan created with CSN_LSTM_RESIDENT).
//
// At these widths the per-step cells of lstm_cell.hip pay one launch per step diagonal for a W_hh of at most 256 KB.
// Here the step loop of one chunk of one layer runs inside the kernel: a workgroup owns 16 batch rows and ALL H units of
// one (layer, chunk) problem, grid = (ceil(B / 16), problems).  It has one wave per unit tile of 16 (H / 16 waves: 2, 4, 6
// or 8); wave w loads the W_hh fragments of the four gates of its tile (backward: the W_hh^T rows of its units, K = 4H)
// once per launch and keeps them in registers -- 64 VGPRs in bf16 and 128 in float32 at H = 128, out of the 256 a lane
// has at two waves per SIMD.  (Four waves with two tiles each, the first form, hold the same registers per CU but run
// the gate math of two tiles one after the other in every wave: with the exact expf / tanhf of the cells that math, not
// the MFMA chain, is most of a step -- 3.9 us per step and layer at H 96 in bf16.)  h_{t-1} (backward: dgates_{t+1}) of
// the 16 rows goes from step to step through a double buffer in LDS, in the compute dtype, rows padded by 16 bytes so
// that the 16 rows of a fragment read fall on different banks; c (backward: the carried dc) stays in registers.  One
// barrier per step: a step reads buffer s & 1 and writes the other, and a wave reaches the barrier only after its reads.
// What step t + 1 (backward: t - 1) reads from the workspace is requested before step t's barrier.  No workgroup waits
// on another.
//
// Every saved tensor is written per step exactly as path 0 writes it (gates, c_all, h_all; dgates): the GEMMs around the
// recurrence, the backward and the next launch read them in the workspace, so the host flow, the workspace and every plan
// feature are those of path 0.
//
// Bit identity with path 0 by construction: the same MFMA (Frag<T>::mma, W as A, h as B), per output element the same k
// order, and the gate math of lstm_cell_common.h.  Where path 0 runs the K-split cells (float32, H % 128 == 0: the sum
// over k is formed from 4 / 8 partial sums, each a chain from 0.0, added in k order to 0.0), the same partial sums are
// formed here one after the other.
#include "lstm_resident.h"

#include "lstm_cell_common.h"

namespace csn {

template <int H> constexpr int kResThreads = 64 * (H / 16);      // one wave per unit tile of 16
template <typename T, int H> struct ResGeom {
  typedef Frag<T> F;
  static constexpr int kThreads = kResThreads<H>;
  static constexpr int kKs = H / F::kStep;                    // fragment steps over k = H (forward)
  static constexpr int kKsB = 4 * H / F::kStep;               // ... over k = 4H (backward)
  static constexpr int kPad = 16 / (int)sizeof(T);            // one 16-byte slot per row
  static constexpr int kLdH = H + kPad;                       // row strides of the LDS tiles, in elements
  static constexpr int kLdG = 4 * H + kPad;
  static constexpr bool kSplit = sizeof(T) == 4 && H % 128 == 0;      // path 0 runs the K-split cells (cell_ks_ok)
  static constexpr int kBwdLds = 2 * 16 * kLdG * (int)sizeof(T);
};

// LDS only: the saved tensors a step stores are read by later launches, never by this one, so the barrier waits for
// the LDS traffic alone and the stores stay in flight across it
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

__device__ __forceinline__ void zero4(float (&v)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = 0.f;
}
__device__ __forceinline__ void copy4(float (&dst)[4], const float (&src)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) dst[r] = src[r];
}

// ------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------
template <typename T, int H>
__global__ void __launch_bounds__(kResThreads<H>)
lstm_resident_fwd_kernel(ResFwdBatch batch, int B) {
  typedef Frag<T> F;
  typedef ResGeom<T, H> Gm;
  const ResFwdOne& q_ = batch.p[blockIdx.y];
  const T* __restrict__ w_hh = (const T*)q_.w_hh;
  const float* __restrict__ xproj = q_.xproj;
  float* __restrict__ c_all = q_.c_all;
  T* __restrict__ h_all = (T*)q_.h_all;
  T* __restrict__ gates_out = (T*)q_.gates;
  const int t0 = q_.t0, nsteps = q_.nsteps;

  __shared__ __attribute__((aligned(16))) T hbuf[2][16][Gm::kLdH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.x * 16, mrow = m0 + (lane & 15);     // the batch row of this lane's fragment column and results
  const bool row_ok = mrow < B;
  const int ub = wave * 16 + (lane >> 4) * 4;                  // lane holds units ub + r, r = 0..3, of batch row mrow
  const int64_t BH = (int64_t)B * H, G = 4 * (int64_t)H;

  // W_hh fragments of this wave's tile, all four gates, all of k
  typename F::type wf[4][Gm::kKs];
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int ks = 0; ks < Gm::kKs; ++ks)
      wf[g][ks] = F::load(w_hh + ((int64_t)g * H + wave * 16 + (lane & 15)) * H, ks * F::kStep, lane);
  // h_{t0 - 1} of the 16 rows (slot t0 of h_all: the installed state, or what the previous chunk's launch stored); rows
  // beyond B are zeros, their columns of the products are never stored
  for (int i = tid; i < 16 * (H / 4); i += Gm::kThreads) {
    const int r = i / (H / 4), c4 = (i % (H / 4)) * 4;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (m0 + r < B) Vec4<T>::load(h_all + (int64_t)t0 * BH + (int64_t)(m0 + r) * H + c4, v);
    Vec4<T>::store(&hbuf[0][r][c4], v);
  }
  float cst[4], xp[4][4];
  auto load_xp = [&](int t, float (&dst)[4][4]) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      zero4(dst[g]);
      if (row_ok) Vec4<float>::load(xproj + ((int64_t)t * B + mrow) * G + (int64_t)g * H + ub, dst[g]);
    }
  };
  zero4(cst);
  if (row_ok) Vec4<float>::load(c_all + (int64_t)t0 * BH + (int64_t)mrow * H + ub, cst);
  load_xp(t0, xp);
  __syncthreads();

  for (int s = 0; s < nsteps; ++s) {
    const int t = t0 + s, cur = s & 1;
    // step t + 1's xproj rows are requested now: their latency is off the chain of step t
    float xn[4][4];
    load_xp(s + 1 < nsteps ? t + 1 : t, xn);
    typename F::type hf[Gm::kKs];
#pragma unroll
    for (int ks = 0; ks < Gm::kKs; ++ks)
      hf[ks] = *reinterpret_cast<const typename F::type*>(&hbuf[cur][lane & 15][ks * F::kStep + F::kLane * (lane >> 4)]);
    f32x4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if constexpr (!Gm::kSplit) {
#pragma unroll
      for (int ks = 0; ks < Gm::kKs; ++ks)
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = F::mma(wf[g][ks], hf[ks], acc[g]);   // D[row = unit][col = batch]
    } else {
      // lstm_cell_fwd_ks_kernel: four K slices, each summed from zero, added in k order
      constexpr int per = Gm::kKs / 4;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        f32x4 part[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) part[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = w * per; ks < (w + 1) * per; ++ks)
#pragma unroll
          for (int g = 0; g < 4; ++g) part[g] = F::mma(wf[g][ks], hf[ks], part[g]);
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] += part[g];
      }
    }
    float pre[4][4];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int r = 0; r < 4; ++r) pre[g][r] = acc[g][r] + xp[g][r];
    float gi[4], gf[4], gg[4], go[4], cn[4], hn[4];
    cell_fwd_point(pre, cst, gi, gf, gg, go, cn, hn);
    Vec4<T>::store(&hbuf[cur ^ 1][lane & 15][ub], hn);       // h_t in the compute dtype: what path 0 reads back from h_all
    if (row_ok) {
      if (gates_out != nullptr) {
        T* gp = gates_out + ((int64_t)t * B + mrow) * G + ub;
        Vec4<T>::store(gp, gi);
        Vec4<T>::store(gp + H, gf);
        Vec4<T>::store(gp + 2 * (int64_t)H, gg);
        Vec4<T>::store(gp + 3 * (int64_t)H, go);
      }
      Vec4<float>::store(c_all + (int64_t)(t + 1) * BH + (int64_t)mrow * H + ub, cn);
      Vec4<T>::store(h_all + (int64_t)(t + 1) * BH + (int64_t)mrow * H + ub, hn);
    }
    copy4(cst, cn);
#pragma unroll
    for (int g = 0; g < 4; ++g) copy4(xp[g], xn[g]);
    lds_barrier();
  }
}

// ------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------
// MASK: as in lstm_cell_bwd_kernel -- a cell at t >= lengths[row] stores zero gate gradients and keeps the carried dc
template <typename T, int H, bool MASK>
__global__ void __launch_bounds__(kResThreads<H>)
lstm_resident_bwd_kernel(ResBwdBatch batch, int B, int Tn, const int* __restrict__ lengths) {
  typedef Frag<T> F;
  typedef ResGeom<T, H> Gm;
  const ResBwdOne& q_ = batch.p[blockIdx.y];
  const T* __restrict__ w_hh_t = (const T*)q_.w_hh_t;
  const float* __restrict__ dy = q_.dy;
  const float* __restrict__ dy_last = q_.dy_last;
  const T* __restrict__ gates = (const T*)q_.gates;
  const float* __restrict__ c_all = q_.c_all;
  float* __restrict__ dc_carry = q_.dc_carry;
  T* __restrict__ dgates = (T*)q_.dgates;
  const int t_hi = q_.t_hi, nsteps = q_.nsteps;

  extern __shared__ __attribute__((aligned(16))) char res_smem[];
  T (*dgb)[16][Gm::kLdG] = reinterpret_cast<T (*)[16][Gm::kLdG]>(res_smem);      // [2][16][4H + pad]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.x * 16, mrow = m0 + (lane & 15);
  const bool row_ok = mrow < B;
  const int ub = wave * 16 + (lane >> 4) * 4;
  constexpr int K = 4 * H;
  const int64_t BH = (int64_t)B * H, BK = (int64_t)B * K;

  // W_hh^T rows of this wave's units, all of k = 4H
  typename F::type wt[Gm::kKsB];
#pragma unroll
  for (int ks = 0; ks < Gm::kKsB; ++ks) wt[ks] = F::load(w_hh_t + (int64_t)(wave * 16 + (lane & 15)) * K, ks * F::kStep, lane);
  // dgates_{t_hi + 1} of the 16 rows, as the previous launch of this layer stored it (absent at the last step)
  if (t_hi != Tn - 1) {
    for (int i = tid; i < 16 * (K / 4); i += Gm::kThreads) {
      const int r = i / (K / 4), c4 = (i % (K / 4)) * 4;
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (m0 + r < B) Vec4<T>::load(dgates + (int64_t)(t_hi + 1) * BK + (int64_t)(m0 + r) * K + c4, v);
      Vec4<T>::store(&dgb[0][r][c4], v);
    }
  }
  float dcn[4];
  zero4(dcn);
  if (row_ok) Vec4<float>::load(dc_carry + (int64_t)mrow * H + ub, dcn);
  int len = 0x7fffffff;
  if constexpr (MASK) {
    if (row_ok) len = lengths[mrow];
  }
  // what a step reads from the workspace: gates, c_{t-1} (c_t is the c_{t-1} of the step before) and dy
  auto dy_at = [&](int t) { return dy != nullptr ? dy + (int64_t)t * BH : (t == Tn - 1 ? dy_last : nullptr); };
  auto load_step = [&](int t, float (&gi)[4], float (&gf)[4], float (&gg)[4], float (&go)[4], float (&cp)[4], float (&dyv)[4]) {
    zero4(gi), zero4(gf), zero4(gg), zero4(go), zero4(cp), zero4(dyv);
    if (!row_ok) return;
    const T* gp = gates + (int64_t)t * BK + (int64_t)mrow * K + ub;
    Vec4<T>::load(gp, gi);
    Vec4<T>::load(gp + H, gf);
    Vec4<T>::load(gp + 2 * (int64_t)H, gg);
    Vec4<T>::load(gp + 3 * (int64_t)H, go);
    Vec4<float>::load(c_all + (int64_t)t * BH + (int64_t)mrow * H + ub, cp);
    const float* dyp = dy_at(t);
    if (dyp != nullptr) Vec4<float>::load(dyp + (int64_t)mrow * H + ub, dyv);
  };
  float gi[4], gf[4], gg[4], go[4], cc[4], cp[4], dyv[4];
  zero4(cc);
  if (row_ok) Vec4<float>::load(c_all + (int64_t)(t_hi + 1) * BH + (int64_t)mrow * H + ub, cc);
  load_step(t_hi, gi, gf, gg, go, cp, dyv);
  __syncthreads();

  for (int s = 0; s < nsteps; ++s) {
    const int t = t_hi - s, cur = s & 1;
    // step t - 1's operands are requested now: their latency is off the chain of step t
    float ngi[4], ngf[4], ngg[4], ngo[4], ncp[4], ndy[4];
    load_step(s + 1 < nsteps ? t - 1 : t, ngi, ngf, ngg, ngo, ncp, ndy);
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (t != Tn - 1) {      // (uniform over the workgroup)
      const T* drow = &dgb[cur][lane & 15][F::kLane * (lane >> 4)];
      if constexpr (!Gm::kSplit) {
#pragma unroll
        for (int ks = 0; ks < Gm::kKsB; ++ks) {
          const typename F::type df = *reinterpret_cast<const typename F::type*>(drow + ks * F::kStep);
          acc = F::mma(wt[ks], df, acc);   // D[unit][batch] = sum_k W_hh^T[u][k] dg_next[b][k]
        }
      } else {
        // lstm_cell_bwd_ks_kernel: eight K slices, each summed from zero, added in k order
        constexpr int per = Gm::kKsB / 8;
#pragma unroll
        for (int w = 0; w < 8; ++w) {
          f32x4 part = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = w * per; ks < (w + 1) * per; ++ks) {
            const typename F::type df = *reinterpret_cast<const typename F::type*>(drow + ks * F::kStep);
            part = F::mma(wt[ks], df, part);
          }
          acc += part;
        }
      }
    }
    float dh[4] = {acc[0], acc[1], acc[2], acc[3]};
    if (dy_at(t) != nullptr) {
#pragma unroll
      for (int r = 0; r < 4; ++r) dh[r] += dyv[r];
    }
    float dai[4], daf[4], dag[4], dao[4], dcarry[4];
    cell_bwd_point(dh, gi, gf, gg, go, cc, cp, dcn, dai, daf, dag, dao, dcarry);
    if constexpr (MASK) {
      if (t >= len) cell_bwd_dead(dcn, dai, daf, dag, dao, dcarry);
    }
    T* lp = &dgb[cur ^ 1][lane & 15][ub];                  // the stored values, for step t - 1
    Vec4<T>::store(lp, dai);
    Vec4<T>::store(lp + H, daf);
    Vec4<T>::store(lp + 2 * H, dag);
    Vec4<T>::store(lp + 3 * H, dao);
    if (row_ok) {
      T* op = dgates + (int64_t)t * BK + (int64_t)mrow * K + ub;
      Vec4<T>::store(op, dai);
      Vec4<T>::store(op + H, daf);
      Vec4<T>::store(op + 2 * (int64_t)H, dag);
      Vec4<T>::store(op + 3 * (int64_t)H, dao);
    }
    copy4(dcn, dcarry);
    copy4(cc, cp);                                         // c_{t-1} is the c_t of step t - 1
    copy4(gi, ngi), copy4(gf, ngf), copy4(gg, ngg), copy4(go, ngo), copy4(cp, ncp), copy4(dyv, ndy);
    lds_barrier();
  }
  if (row_ok) Vec4<float>::store(dc_carry + (int64_t)mrow * H + ub, dcn);
}

bool resident_supported(int H) { return H >= 32 && H <= kResidentMaxH && H % 32 == 0; }

template <typename T, int H>
static int launch_fwd_one(const ResFwdBatch& b, dim3 grid, int B, hipStream_t st) {
  lstm_resident_fwd_kernel<T, H><<<grid, ResGeom<T, H>::kThreads, 0, st>>>(b, B);
  CSN_LAUNCH_CHECK();
  return CSN_OK;
}
template <typename T, int H>
static int launch_bwd_one(const ResBwdBatch& b, dim3 grid, int B, int Tn, const int* lengths, hipStream_t st) {
  constexpr int lds = ResGeom<T, H>::kBwdLds, threads = ResGeom<T, H>::kThreads;
  if (lengths != nullptr) {
    if (int rc = ensure_dyn_lds<lstm_resident_bwd_kernel<T, H, true>>(lds)) return rc;
    lstm_resident_bwd_kernel<T, H, true><<<grid, threads, lds, st>>>(b, B, Tn, lengths);
  } else {
    if (int rc = ensure_dyn_lds<lstm_resident_bwd_kernel<T, H, false>>(lds)) return rc;
    lstm_resident_bwd_kernel<T, H, false><<<grid, threads, lds, st>>>(b, B, Tn, nullptr);
  }
  CSN_LAUNCH_CHECK();
  return CSN_OK;
}

int launch_resident_fwd(const ResFwdBatch& b, int np, int B, int H, int dtype, hipStream_t st) {
  CSN_REQUIRE(np >= 1 && np <= 4, "launch_resident_fwd: %d problems", np);
  const dim3 grid((unsigned)((B + 15) / 16), (unsigned)np);
  const bool bf = dtype == CSN_BF16;
  switch (H) {
    case 32: return bf ? launch_fwd_one<bf16_t, 32>(b, grid, B, st) : launch_fwd_one<float, 32>(b, grid, B, st);
    case 64: return bf ? launch_fwd_one<bf16_t, 64>(b, grid, B, st) : launch_fwd_one<float, 64>(b, grid, B, st);
    case 96: return bf ? launch_fwd_one<bf16_t, 96>(b, grid, B, st) : launch_fwd_one<float, 96>(b, grid, B, st);
    case 128: return bf ? launch_fwd_one<bf16_t, 128>(b, grid, B, st) : launch_fwd_one<float, 128>(b, grid, B, st);
  }
  return fail(CSN_ERR_UNSUPPORTED, "launch_resident_fwd: no kernel for H=%d", H);
}

int launch_resident_bwd(const ResBwdBatch& b, int np, int B, int T, int H, int dtype, const int* lengths, hipStream_t st) {
  CSN_REQUIRE(np >= 1 && np <= 4, "launch_resident_bwd: %d problems", np);
  const dim3 grid((unsigned)((B + 15) / 16), (unsigned)np);
  const bool bf = dtype == CSN_BF16;
  switch (H) {
    case 32: return bf ? launch_bwd_one<bf16_t, 32>(b, grid, B, T, lengths, st) : launch_bwd_one<float, 32>(b, grid, B, T, lengths, st);
    case 64: return bf ? launch_bwd_one<bf16_t, 64>(b, grid, B, T, lengths, st) : launch_bwd_one<float, 64>(b, grid, B, T, lengths, st);
    case 96: return bf ? launch_bwd_one<bf16_t, 96>(b, grid, B, T, lengths, st) : launch_bwd_one<float, 96>(b, grid, B, T, lengths, st);
    case 128: return bf ? launch_bwd_one<bf16_t, 128>(b, grid, B, T, lengths, st) : launch_bwd_one<float, 128>(b, grid, B, T, lengths, st);
  }
  return fail(CSN_ERR_UNSUPPORTED, "launch_resident_bwd: no kernel for H=%d", H);
}

}  // namespace csn
