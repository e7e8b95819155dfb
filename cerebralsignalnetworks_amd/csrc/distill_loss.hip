// K5b: the losses the training scripts actually use, value and gradient in two launches each.
//   FeatureDistributionLoss      LstmDistillFromDinoV2Train.py:107-140           (CSN_SOFT_CE_OF_PROBS + CE of pred_label)
//   loss_fn_kd                   LstmDistillFromDinoV2TrainSpampinato.py:107-121 (CSN_SOFT_KL + CE of the same tensor)
//   FeatureDistributionLoss (KD) LstmDistillFromDinoV2TrainSpampinato.py:125-184 (CSN_SOFT_KL + CE of the same tensor)
//   FeatureDistributionLoss (Eval) LstmDistillFromDinoV2Eval.py:106-146          (CSN_SOFT_KL alone)
//   DINOLoss.forward             LstmDistillation.py:118-148
// The formulas are in include/csn_hip.h.  Shape of both row kernels, as cosine_rows_kernel (loss.hip): one wave per row
// (per batch row b for DINO), four rows per 256-thread workgroup, float32 in, float64 arithmetic, each float32 output
// rounded once.  A row of D <= DL_RESIDENT_D = 1024 elements is loaded once into DL_REG = 16 registers per lane (element i
// in lane i % 64, register i / 64) and every pass runs on the registers; a longer row is re-read from memory in each pass
// (the <false> instantiations).  The register arrays are only ever indexed by the counter of a fully unrolled loop: a
// dynamic index would put them in scratch memory, which tools/check_spills.py refuses.
// Per-row float64 partial sums go to caller-owned scratch; dl_finish_kernel (one wave) adds them, lane l taking rows
// l, l + 64, ... ascending and the lanes combined by the xor butterfly of dl_wave_sum -- an order that depends on the row
// count only, so two calls on the same input give the same bits.  No atomics, no waits between workgroups; every loop is
// bounded by D, K, V or G.
#include <math.h>

#include "csn_common.h"

namespace csn {

constexpr int DL_REG = 16;
constexpr int DL_RESIDENT_D = 64 * DL_REG;

__device__ __forceinline__ double dl_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ float dl_wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// f(j, i) for every element i = j * 64 + lane < D of this lane.  RES: j is the counter of an unrolled loop (a constant
// in every copy of f's body); otherwise j is 0 and unused.
template <bool RES, class F>
__device__ __forceinline__ void dl_each(int D, int lane, F&& f) {
  if constexpr (RES) {
#pragma unroll
    for (int j = 0; j < DL_REG; ++j) {
      const int i = j * 64 + lane;
      if (i < D) f(j, i);
    }
  } else {
    for (int i = lane; i < D; i += 64) f(0, i);
  }
}

// A float32 row: in registers (RES) or read where it lies.
template <bool RES>
struct DlRow {
  float r[RES ? DL_REG : 1];
  const float* p;
  __device__ __forceinline__ void load(const float* row, int D, int lane) {
    p = row;
    if constexpr (RES) {
#pragma unroll
      for (int j = 0; j < DL_REG; ++j) {
        const int i = j * 64 + lane;
        r[j] = i < D ? row[i] : 0.0f;
      }
    }
  }
  __device__ __forceinline__ double at(int j, int i) const {
    if constexpr (RES) return (double)r[j];
    else return (double)p[i];
  }
};

// A float64 row that a lane both writes and reads at its own elements only: registers (RES) or caller-owned scratch.
template <bool RES>
struct DlAcc {
  double r[RES ? DL_REG : 1];
  double* p;
  __device__ __forceinline__ void set(int j, int i, double v) {
    if constexpr (RES) r[j] = v;
    else p[i] = v;
  }
  __device__ __forceinline__ double get(int j, int i) const {
    if constexpr (RES) return r[j];
    else return p[i];
  }
};

template <bool RES>
__device__ __forceinline__ float dl_row_max(const DlRow<RES>& x, int D, int lane) {
  float m = -INFINITY;
  dl_each<RES>(D, lane, [&](int j, int i) { m = fmaxf(m, (float)x.at(j, i)); });
  return dl_wave_max(m);
}

struct DistillArgs {
  const float* student;
  const float* teacher;
  const float* logits;      // NULL: no CE term; == student: the alias (K == D)
  const int64_t* labels;
  int B, D, K, mode;
  double inv_T;
  double g_soft;            // grad_scale * w_soft / (B * T)
  double g_ce;              // grad_scale * w_ce / B
  double* soft_rows;        // [B]
  double* ce_rows;          // [B]
  float* dstudent;          // may be NULL
  float* dlogits;           // may be NULL
};

template <bool RES>
__global__ void __launch_bounds__(256) distill_rows_kernel(const DistillArgs a) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.B) return;
  const int D = a.D;
  const bool alias = a.logits == a.student;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  DlRow<RES> s, t;
  s.load(a.student + (int64_t)row * D, D, lane);
  t.load(a.teacher + (int64_t)row * D, D, lane);
  const double ms = (double)dl_row_max<RES>(s, D, lane), mt = (double)dl_row_max<RES>(t, D, lane);
  const double inv_T = a.inv_T;

  // sums of both softmaxes (and, for the alias, of softmax(student) at T = 1); KL: sum e_t (x_t - x_s) beside them, a
  // term with e_t == 0 is 0 (x_t - x_s is finite)
  double zs = 0.0, zt = 0.0, z1 = 0.0, kl = 0.0;
  dl_each<RES>(D, lane, [&](int j, int i) {
    const double xs = (s.at(j, i) - ms) * inv_T, xt = (t.at(j, i) - mt) * inv_T;
    const double et = exp(xt);
    zs += exp(xs);
    zt += et;
    if (a.mode == CSN_SOFT_KL) kl = fma(et, xt - xs, kl);
    if (alias) z1 += exp(s.at(j, i) - ms);
  });
  zs = dl_wave_sum(zs);
  zt = dl_wave_sum(zt);
  const double inv_zs = 1.0 / zs, inv_zt = 1.0 / zt;

  double soft, pmax = 0.0, log_zp = 0.0, qa = 0.0;
  if (a.mode == CSN_SOFT_KL) {
    // sum p_t (log p_t - log q) = sum p_t (x_t - x_s) - log Z_t + log Z_s
    soft = dl_wave_sum(kl) * inv_zt - log(zt) + log(zs);
  } else {
    // a = log_softmax(p_t): the largest p_t is exp(0) / Z_t
    pmax = inv_zt;
    double zp = 0.0;
    dl_each<RES>(D, lane, [&](int j, int i) {
      const double xs = (s.at(j, i) - ms) * inv_T, xt = (t.at(j, i) - mt) * inv_T;
      const double p = exp(xt) * inv_zt;
      zp += exp(p - pmax);
      qa = fma(exp(xs) * inv_zs, p - pmax, qa);
    });
    log_zp = log(dl_wave_sum(zp));
    qa = dl_wave_sum(qa) - log_zp;      // sum_o q_o a_o, sum q = 1
    soft = -qa;
  }

  // CE of the row's label: on the student row itself (alias) or on a logits row of its own, read where it lies
  double ce = 0.0, ml = ms, inv_zl = 0.0;
  bool bad = false;
  int64_t label = -1;
  const float* lrow = nullptr;
  if (a.logits != nullptr) {
    label = a.labels[row];
    bad = label < 0 || label >= (int64_t)a.K;
    lrow = a.logits + (int64_t)row * a.K;
    double zl;
    if (alias) {
      zl = dl_wave_sum(z1);
    } else {
      float m = -INFINITY;
      for (int i = lane; i < a.K; i += 64) m = fmaxf(m, lrow[i]);
      ml = (double)dl_wave_max(m);
      zl = 0.0;
      for (int i = lane; i < a.K; i += 64) zl += exp((double)lrow[i] - ml);
      zl = dl_wave_sum(zl);
    }
    inv_zl = 1.0 / zl;
    ce = bad ? nan : -(((double)lrow[bad ? 0 : label] - ml) - log(zl));
  }
  if (lane == 0) {
    a.soft_rows[row] = soft;
    a.ce_rows[row] = ce;
  }

  if (a.dstudent != nullptr) {
    float* out = a.dstudent + (int64_t)row * D;
    dl_each<RES>(D, lane, [&](int j, int i) {
      const double xs = (s.at(j, i) - ms) * inv_T, xt = (t.at(j, i) - mt) * inv_T;
      const double q = exp(xs) * inv_zs, p = exp(xt) * inv_zt;
      double g = a.mode == CSN_SOFT_KL ? a.g_soft * (q - p) : -a.g_soft * q * ((p - pmax - log_zp) - qa);
      if (alias) g += a.g_ce * (exp(s.at(j, i) - ms) * inv_zl - ((int64_t)i == label ? 1.0 : 0.0));
      out[i] = (float)((alias && bad) ? nan : g);
    });
  }
  if (a.dlogits != nullptr) {
    float* out = a.dlogits + (int64_t)row * a.K;
    for (int i = lane; i < a.K; i += 64) {
      const double g = a.g_ce * (exp((double)lrow[i] - ml) * inv_zl - ((int64_t)i == label ? 1.0 : 0.0));
      out[i] = (float)(bad ? nan : g);
    }
  }
}

// loss = fl32(ca * sum a_rows + cb * sum b_rows); b_rows may be NULL
__global__ void __launch_bounds__(64) dl_finish_kernel(const double* __restrict__ a_rows, const double* __restrict__ b_rows,
                                                      int B, double ca, double cb, float* __restrict__ loss) {
  double sa = 0.0, sb = 0.0;
  for (int i = threadIdx.x; i < B; i += 64) {
    sa += a_rows[i];
    if (b_rows != nullptr) sb += b_rows[i];
  }
  sa = dl_wave_sum(sa);
  sb = dl_wave_sum(sb);
  if (threadIdx.x == 0) loss[0] = (float)(b_rows != nullptr ? ca * sa + cb * sb : ca * sa);
}

struct DinoArgs {
  const float* student;     // [V,B,D]
  const float* teacher;     // [G,B,D]
  const float* center;      // [D] (stride 0) or [B,D] (stride D)
  int V, G, B, D, pairing;
  int64_t center_stride_b;
  double inv_tt, inv_st;
  double g_row;             // grad_scale / (G * B * (V - 1) * student_temp)
  double* rows;             // [B] sum over the pairs of q . log p
  double* qsum;             // [B,D] (only when the row is not register-resident)
  float* dstudent;          // may be NULL
};

// (teacher - center) of one teacher view as the wave sees it: both operands resident, or both read where they lie
template <bool RES>
struct DlTeacher {
  DlRow<RES> t;
  double m, inv_z;
  __device__ __forceinline__ double x(const DlRow<RES>& c, int j, int i, double inv_tt) const {
    return ((t.at(j, i) - c.at(j, i)) - m) * inv_tt;
  }
  __device__ __forceinline__ void load(const float* row, const DlRow<RES>& c, int D, int lane, double inv_tt) {
    t.load(row, D, lane);
    double mx = -INFINITY;      // the difference is exact in float64, not in float32
    dl_each<RES>(D, lane, [&](int j, int i) { mx = fmax(mx, t.at(j, i) - c.at(j, i)); });
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off, 64));
    m = mx;
    double z = 0.0;
    dl_each<RES>(D, lane, [&](int j, int i) { z += exp(x(c, j, i, inv_tt)); });
    inv_z = 1.0 / dl_wave_sum(z);
  }
};

template <bool RES>
__global__ void __launch_bounds__(256) dino_rows_kernel(const DinoArgs a) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= a.B) return;
  const int D = a.D, V = a.V, G = a.G;
  DlRow<RES> c;
  c.load(a.center + (int64_t)b * a.center_stride_b, D, lane);
  DlAcc<RES> qall;      // sum over all teacher views of q[g, b, :]
  qall.p = RES ? nullptr : a.qsum + (int64_t)b * D;
  dl_each<RES>(D, lane, [&](int j, int i) { qall.set(j, i, 0.0); });
  DlTeacher<RES> tv;
  for (int g = 0; g < G; ++g) {
    tv.load(a.teacher + ((int64_t)g * a.B + b) * D, c, D, lane, a.inv_tt);
    dl_each<RES>(D, lane, [&](int j, int i) { qall.set(j, i, qall.get(j, i) + exp(tv.x(c, j, i, a.inv_tt)) * tv.inv_z); });
  }
  double acc = 0.0;
  DlRow<RES> s;
  for (int v = 0; v < V; ++v) {
    // teacher views paired with student view v: all G of them, except view v itself (SKIP_SAME), none for v = 0 (SKIP_FIRST)
    const bool minus_own = a.pairing == CSN_DINO_SKIP_SAME && v < G;
    const int n_v = a.pairing == CSN_DINO_SKIP_FIRST ? (v >= 1 ? G : 0) : G - (minus_own ? 1 : 0);
    float* out = a.dstudent != nullptr ? a.dstudent + ((int64_t)v * a.B + b) * D : nullptr;
    if (n_v == 0) {
      if (out != nullptr)
        for (int i = lane; i < D; i += 64) out[i] = 0.0f;
      continue;
    }
    if (minus_own) tv.load(a.teacher + ((int64_t)v * a.B + b) * D, c, D, lane, a.inv_tt);
    s.load(a.student + ((int64_t)v * a.B + b) * D, D, lane);
    const double ms = (double)dl_row_max<RES>(s, D, lane);
    double z = 0.0;
    dl_each<RES>(D, lane, [&](int j, int i) { z += exp((s.at(j, i) - ms) * a.inv_st); });
    z = dl_wave_sum(z);
    const double inv_z = 1.0 / z, log_z = log(z);
    dl_each<RES>(D, lane, [&](int j, int i) {
      const double xs = (s.at(j, i) - ms) * a.inv_st;
      double q = qall.get(j, i);
      if (minus_own) q -= exp(tv.x(c, j, i, a.inv_tt)) * tv.inv_z;
      acc = fma(q, xs - log_z, acc);
      if (out != nullptr) out[i] = (float)(-a.g_row * (q - (double)n_v * exp(xs) * inv_z));
    });
  }
  acc = dl_wave_sum(acc);
  if (lane == 0) a.rows[b] = acc;
}

}  // namespace csn

using namespace csn;

extern "C" size_t csn_distill_loss_scratch_bytes(int B) { return B > 0 ? (size_t)B * 2 * sizeof(double) : 0; }

extern "C" int csn_distill_loss(const float* student, const float* teacher, int B, int D, const float* logits, int K,
                                const int64_t* labels, int soft_mode, double T, double w_soft, double w_ce, float* loss,
                                float* dstudent, float* dlogits, float grad_scale, void* scratch, csnStream_t stream) {
  CSN_REQUIRE(student && teacher && loss && scratch, "csn_distill_loss: null pointer");
  CSN_REQUIRE(B > 0 && D > 0, "csn_distill_loss: bad shape B=%d D=%d", B, D);
  CSN_REQUIRE(isfinite(T) && T > 0.0, "csn_distill_loss: temperature must be finite and positive, got %g", T);
  CSN_REQUIRE(soft_mode == CSN_SOFT_KL || soft_mode == CSN_SOFT_CE_OF_PROBS, "csn_distill_loss: unknown soft_mode %d", soft_mode);
  const bool alias = logits != nullptr && logits == student;
  if (logits != nullptr) {
    CSN_REQUIRE(labels != nullptr, "csn_distill_loss: logits without labels");
    CSN_REQUIRE(K > 0, "csn_distill_loss: logits with K=%d", K);
    CSN_REQUIRE(!alias || K == D, "csn_distill_loss: logits alias student but K=%d != D=%d", K, D);
    CSN_REQUIRE(!alias || dlogits == nullptr, "csn_distill_loss: dlogits with logits aliasing student (the CE gradient is added into dstudent)");
  } else {
    CSN_REQUIRE(dlogits == nullptr, "csn_distill_loss: dlogits without logits");
  }
  CSN_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 7) == 0, "csn_distill_loss: scratch must be 8-byte aligned");
  hipStream_t st = as_stream(stream);
  DistillArgs a;
  a.student = student; a.teacher = teacher; a.logits = logits; a.labels = labels;
  a.B = B; a.D = D; a.K = logits != nullptr ? K : 0; a.mode = soft_mode;
  a.inv_T = 1.0 / T;
  a.g_soft = (double)grad_scale * w_soft / ((double)B * T);
  a.g_ce = logits != nullptr ? (double)grad_scale * w_ce / (double)B : 0.0;
  a.soft_rows = (double*)scratch;
  a.ce_rows = a.soft_rows + B;
  a.dstudent = dstudent; a.dlogits = dlogits;
  const unsigned grid = (unsigned)((B + 3) / 4);
  if (D <= DL_RESIDENT_D) distill_rows_kernel<true><<<grid, 256, 0, st>>>(a);
  else distill_rows_kernel<false><<<grid, 256, 0, st>>>(a);
  CSN_LAUNCH_CHECK();
  dl_finish_kernel<<<1, 64, 0, st>>>(a.soft_rows, logits != nullptr ? a.ce_rows : nullptr, B, w_soft / (double)B,
                                     w_ce / (double)B, loss);
  CSN_LAUNCH_CHECK();
  return CSN_OK;
}

extern "C" size_t csn_dino_loss_scratch_bytes(int B, int D) {
  if (B <= 0 || D <= 0) return 0;
  return ((size_t)B + (D > DL_RESIDENT_D ? (size_t)B * (size_t)D : 0)) * sizeof(double);
}

extern "C" int csn_dino_loss(const float* student, const float* teacher, int V, int G, int B, int D, const float* center,
                             int64_t center_stride_b, double teacher_temp, double student_temp, int pairing, float* loss,
                             float* dstudent, float grad_scale, void* scratch, csnStream_t stream) {
  CSN_REQUIRE(student && teacher && center && loss && scratch, "csn_dino_loss: null pointer");
  CSN_REQUIRE(B > 0 && D > 0, "csn_dino_loss: bad shape B=%d D=%d", B, D);
  CSN_REQUIRE(V >= 2, "csn_dino_loss: needs at least two student views, got V=%d", V);
  CSN_REQUIRE(G >= 1 && G <= V, "csn_dino_loss: G=%d teacher views outside [1, V=%d]", G, V);
  CSN_REQUIRE(center_stride_b == 0 || center_stride_b == (int64_t)D,
              "csn_dino_loss: center_stride_b must be 0 (a [D] centre) or D (a [B,D] centre), got %lld", (long long)center_stride_b);
  CSN_REQUIRE(isfinite(teacher_temp) && teacher_temp > 0.0 && isfinite(student_temp) && student_temp > 0.0,
              "csn_dino_loss: temperatures must be finite and positive, got %g / %g", teacher_temp, student_temp);
  CSN_REQUIRE(pairing == CSN_DINO_SKIP_FIRST || pairing == CSN_DINO_SKIP_SAME, "csn_dino_loss: unknown pairing %d", pairing);
  CSN_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 7) == 0, "csn_dino_loss: scratch must be 8-byte aligned");
  hipStream_t st = as_stream(stream);
  const double cnorm = 1.0 / ((double)G * (double)B * (double)(V - 1));
  DinoArgs a;
  a.student = student; a.teacher = teacher; a.center = center;
  a.V = V; a.G = G; a.B = B; a.D = D; a.pairing = pairing;
  a.center_stride_b = center_stride_b;
  a.inv_tt = 1.0 / teacher_temp; a.inv_st = 1.0 / student_temp;
  a.g_row = (double)grad_scale * cnorm / student_temp;
  a.rows = (double*)scratch;
  a.qsum = a.rows + B;
  a.dstudent = dstudent;
  const unsigned grid = (unsigned)((B + 3) / 4);
  if (D <= DL_RESIDENT_D) dino_rows_kernel<true><<<grid, 256, 0, st>>>(a);
  else dino_rows_kernel<false><<<grid, 256, 0, st>>>(a);
  CSN_LAUNCH_CHECK();
  dl_finish_kernel<<<1, 64, 0, st>>>(a.rows, nullptr, B, -cnorm, 0.0, loss);
  CSN_LAUNCH_CHECK();
  return CSN_OK;
}
