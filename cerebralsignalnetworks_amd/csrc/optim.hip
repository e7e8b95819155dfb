// Optimiser tails of the hot loop on the flat float32 buffers of trainer.FlatGrads: per-tensor L2 norms, the DINO
// per-tensor clip, Adam / AdamW and LARS, each as ONE streaming pass over the whole model.
// Replaces: torch.optim.AdamW(...).step() at LstmDistillFromDinoV2TrainSpampinato.py:378 and
// LstmDistillation.py:150, torch.optim.Adam at LSTMDistill.py:322, LARS.step at EEG-BarlowNetworks/optim.py:17-44 and
// clip_gradients at utils/utils.py:132-141.
//
// A flat buffer of n elements is cut into nseg SEGMENTS (one per parameter tensor, packed back to back: a boundary is
// an arbitrary element offset) and, independently, into fixed CHUNKS of kChunk elements (a chunk starts 16-byte
// aligned).  One workgroup works on one chunk at a time.  A chunk that lies inside one segment (almost all of them)
// takes the vector path -- 16-byte accesses, per-segment coefficients in scalar registers; a chunk that holds a
// boundary takes the scalar path, one segment after the other.
//
// The segment table (caller-owned device memory, csn_flat_segments_scratch_bytes) holds
//   chunk_seg[nchunks]   segment of the chunk's first element
//   seg_end[nseg], seg_first[nseg + 1], seg_flags[nseg]
//   partials[2][cap]     one float64 per (quantity, segment x chunk intersection), cap = nchunks + nseg
//   sums[2][nseg]        float64 sum of squares per (quantity, segment)
// The intersection of segment s (elements [a, e)) with chunk c owns partial slot seg_first[s] + c - a / kChunk, so the
// slots of a segment are contiguous and stage two adds them in a fixed order: no floating-point atomics anywhere, two
// runs give the same bits.
//
// The GUARD (csn_grad_guard) is one more pass of that kind over the whole gradient buffer: it leaves
// the global L2 norm, clip_grad_norm_'s coefficient and a finiteness flag in a 16-byte device record.  Every step kernel
// and norm pass below is a template on GUARD: the guarded instantiation returns at once when the record says non-finite,
// and otherwise reads g' = fl32(scale g) wherever the unguarded one reads g; the unguarded instantiation is the kernel it
// was before.
#include "csn_common.h"

#include <math.h>

namespace csn {
namespace {

constexpr int kChunk = 2048;          // elements per chunk: 256 threads x 2 x float4
constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;      // 256 CUs x 8, grid-stride beyond (memory-bound streaming kernels)
constexpr int kUpload = 32;           // segments per upload launch (they travel as kernel arguments)
constexpr int kDecayed = 1, kScaled = 2;

struct Table {
  int32_t* chunk_seg;
  int64_t* seg_end;
  int32_t* seg_first;
  int32_t* seg_flags;
  double* partials;
  double* sums;
  int64_t cap;
  size_t bytes;
};

static inline int64_t num_chunks(int64_t n) { return (n + kChunk - 1) / kChunk; }

static Table table_layout(void* base, int nseg, int64_t n) {
  Table t{};
  char* p = static_cast<char*>(base);
  const int64_t nchunks = num_chunks(n);
  t.cap = nchunks + nseg;
  size_t off = 0;
  t.chunk_seg = reinterpret_cast<int32_t*>(p + off); off = align_up(off + (size_t)nchunks * 4, 16);
  t.seg_end = reinterpret_cast<int64_t*>(p + off);   off = align_up(off + (size_t)nseg * 8, 16);
  t.seg_first = reinterpret_cast<int32_t*>(p + off); off = align_up(off + (size_t)(nseg + 1) * 4, 16);
  t.seg_flags = reinterpret_cast<int32_t*>(p + off); off = align_up(off + (size_t)nseg * 4, 16);
  t.partials = reinterpret_cast<double*>(p + off);   off = align_up(off + (size_t)t.cap * 2 * 8, 16);
  t.sums = reinterpret_cast<double*>(p + off);       off = align_up(off + (size_t)nseg * 2 * 8, 16);
  t.bytes = off;
  return t;
}

static inline unsigned grid_for(int64_t n) {
  const int64_t c = num_chunks(n);
  return (unsigned)(c < kMaxBlocks ? c : kMaxBlocks);
}

// ---- table construction --------------------------------------------------------------------------------------------
struct UploadBatch {
  int64_t end[kUpload];
  int32_t first[kUpload];
  int32_t flags[kUpload];
};

__global__ void __launch_bounds__(64) flat_segments_upload_kernel(Table t, UploadBatch b, int s0, int count, int nseg, int total) {
  const int i = threadIdx.x;
  if (i < count) {
    t.seg_end[s0 + i] = b.end[i];
    t.seg_first[s0 + i] = b.first[i];
    t.seg_flags[s0 + i] = b.flags[i];
  }
  if (i == 0 && s0 + count == nseg) t.seg_first[nseg] = total;
}

__global__ void __launch_bounds__(kThreads) flat_chunk_seg_kernel(Table t, int nseg, int64_t nchunks) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nchunks) return;
  const int64_t pos = c * kChunk;
  int lo = 0, hi = nseg - 1;          // first segment whose end lies behind pos
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (t.seg_end[mid] > pos) hi = mid; else lo = mid + 1;
  }
  t.chunk_seg[c] = lo;
}

// ---- block reduction of float64 sums: wave shuffles, then LDS across the four waves -----------------------------------
template <int Q>
__device__ __forceinline__ void block_sum(double (&v)[Q], double (*lds)[kThreads / 64]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[q] += __shfl_down(v[q], off, 64);
    if (lane == 0) lds[q][wave] = v[q];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < Q; ++q) v[q] = ((lds[q][0] + lds[q][1]) + lds[q][2]) + lds[q][3];
  }
  __syncthreads();
}

// ---- the guard's view of a gradient element: g' = fl32(scale g), one rounding of its own (the product is the value of a
// call, so -ffp-contract=on cannot fuse it into the multiply-add that consumes it) ----------------------------------------
template <bool GUARD>
__device__ __forceinline__ float guarded(float g, float gs) {
  if constexpr (GUARD) return __fmul_rn(gs, g);
  else return g;
}

// false: the record says "non-finite", the kernel writes nothing.  (uniform: two scalar loads per workgroup)
template <bool GUARD>
__device__ __forceinline__ bool guard_open(const csnStepGuard* guard, float& gs) {
  gs = 1.0f;
  if constexpr (GUARD) {
    if (guard->finite == 0u) return false;
    gs = guard->scale;
  }
  return true;
}

// ---- stage one of the segment norms ------------------------------------------------------------------------------------
// PAIR = false: sum a^2.  PAIR = true: sum a^2 and sum d^2, d = b + wd a on decayed segments, b elsewhere (LARS: a = p, b = g).
template <bool PAIR>
__device__ __forceinline__ void sq_acc(double (&acc)[PAIR ? 2 : 1], float a, float b, float wd, bool decay) {
  acc[0] += (double)a * (double)a;
  if constexpr (PAIR) {
    const float d = decay ? fmaf(wd, a, b) : b;
    acc[1] += (double)d * (double)d;
  }
}

// GUARD: the gradient is b with PAIR (LARS), a without (Adam's per-tensor clip)
template <bool PAIR, bool GUARD>
__device__ __forceinline__ void sq_acc_g(double (&acc)[PAIR ? 2 : 1], float a, float b, float wd, bool decay, float gs) {
  if constexpr (PAIR) sq_acc<PAIR>(acc, a, guarded<GUARD>(b, gs), wd, decay);
  else sq_acc<PAIR>(acc, guarded<GUARD>(a, gs), b, wd, decay);
}

template <bool PAIR, bool GUARD>
__global__ void __launch_bounds__(kThreads) flat_sqsum_partial_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                     float wd, int64_t n, Table t,
                                                                     const csnStepGuard* __restrict__ guard) {
  constexpr int Q = PAIR ? 2 : 1;
  __shared__ double lds[Q][kThreads / 64];
  float gs;
  if (!guard_open<GUARD>(guard, gs)) return;
  const int64_t nchunks = (n + kChunk - 1) / kChunk;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int64_t cs = c * kChunk;
    const int64_t ce = cs + kChunk < n ? cs + kChunk : n;
    int s = t.chunk_seg[c];
    int64_t lo = cs;
    while (lo < ce) {                  // (uniform over the workgroup: one pass per segment the chunk holds)
      const int64_t e = t.seg_end[s];
      const int64_t hi = e < ce ? e : ce;
      const bool decay = PAIR && wd != 0.0f && (t.seg_flags[s] & kDecayed);
      double acc[Q] = {};
      if (lo == cs && hi == cs + kChunk) {      // a whole chunk inside one segment: two 16-byte loads per thread and buffer
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const int64_t i = cs / 4 + k * kThreads + threadIdx.x;
          const float4 av = reinterpret_cast<const float4*>(a)[i];
          float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
          if constexpr (PAIR) bv = reinterpret_cast<const float4*>(b)[i];
          sq_acc_g<PAIR, GUARD>(acc, av.x, bv.x, wd, decay, gs);
          sq_acc_g<PAIR, GUARD>(acc, av.y, bv.y, wd, decay, gs);
          sq_acc_g<PAIR, GUARD>(acc, av.z, bv.z, wd, decay, gs);
          sq_acc_g<PAIR, GUARD>(acc, av.w, bv.w, wd, decay, gs);
        }
      } else {
        for (int64_t i = lo + threadIdx.x; i < hi; i += kThreads) sq_acc_g<PAIR, GUARD>(acc, a[i], PAIR ? b[i] : 0.f, wd, decay, gs);
      }
      block_sum<Q>(acc, lds);
      if (threadIdx.x == 0) {
        const int64_t seg_start = s > 0 ? t.seg_end[s - 1] : 0;
        const int64_t slot = t.seg_first[s] + (c - seg_start / kChunk);
#pragma unroll
        for (int q = 0; q < Q; ++q) t.partials[q * t.cap + slot] = acc[q];
      }
      lo = hi;
      ++s;
    }
  }
}

// ---- stage two: one wave per (segment, quantity) adds that segment's partials, lane-strided, then across the lanes -----
template <bool GUARD>
__global__ void __launch_bounds__(64) flat_sqsum_final_kernel(Table t, int nseg, float* __restrict__ norms_out,
                                                              const csnStepGuard* __restrict__ guard) {
  float gs;
  if (!guard_open<GUARD>(guard, gs)) return;       // (stage one wrote no partials)
  const int s = blockIdx.x, q = blockIdx.y;
  const int first = t.seg_first[s], last = t.seg_first[s + 1];
  double acc = 0.0;
  for (int i = first + threadIdx.x; i < last; i += 64) acc += t.partials[q * t.cap + i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (threadIdx.x == 0) {
    t.sums[q * nseg + s] = acc;
    if (norms_out) norms_out[q * nseg + s] = (float)sqrt(acc);
  }
}

// ---- per-segment coefficients --------------------------------------------------------------------------------------------
// clip coefficient of utils/utils.py:132-141 on float32 norms: min(1, clip / (|g| + 1e-6))
__device__ __forceinline__ float clip_coef(const Table& t, int s, float clip) {
  const float norm = (float)sqrt(t.sums[s]);
  return fminf(__fdiv_rn(clip, __fadd_rn(norm, 1e-6f)), 1.0f);
}

// ---- standalone clip ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) flat_clip_kernel(float* __restrict__ g, int64_t n, Table t, float clip) {
  const int64_t nchunks = (n + kChunk - 1) / kChunk;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int64_t cs = c * kChunk;
    const int64_t ce = cs + kChunk < n ? cs + kChunk : n;
    int s = t.chunk_seg[c];
    if (t.seg_end[s] >= cs + kChunk) {
      const float coef = clip_coef(t, s, clip);
      if (coef == 1.0f) continue;       // (x * 1 == x: nothing to write)
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int64_t i = cs / 4 + k * kThreads + threadIdx.x;
        float4 gv = reinterpret_cast<float4*>(g)[i];
        gv.x *= coef; gv.y *= coef; gv.z *= coef; gv.w *= coef;
        reinterpret_cast<float4*>(g)[i] = gv;
      }
    } else {
      for (int64_t i = cs + threadIdx.x; i < ce; i += kThreads) {
        int si = s;
        while (i >= t.seg_end[si]) ++si;
        g[i] *= clip_coef(t, si, clip);
      }
    }
  }
}

// ---- Adam / AdamW ------------------------------------------------------------------------------------------------------
// The arithmetic of torch's single-tensor path (torch/optim/adam.py, adamw.py), one rounding per torch kernel:
//   g <- coef g                          (clip; DINO CLI)
//   p <- p (1 - lr wd)                   decoupled, decayed segments      | g <- g + wd p   not decoupled
//   m <- m + (1 - b1)(g - m)             lerp_ (b1 <= 0.5: m <- g - (g - m)(1 - (1 - b1)), as lerp_ does)
//   v <- v b2 ; v <- v + ((1 - b2) g) g  mul_, addcmul_
//   p <- p - (lr / bc1) (m / (sqrt(v) / sqrt(bc2) + eps))                addcdiv_
struct AdamArgs {
  float decay_mul;      // 1 - lr wd (decoupled)
  float wd;             // (not decoupled)
  float w1;             // 1 - beta1
  float beta2, w2;      // beta2, 1 - beta2
  float bc2_sqrt;       // sqrt(1 - beta2^t)
  float neg_step;       // -lr / (1 - beta1^t)
  float eps;
  float clip;           // <= 0: none
  int decoupled;
  int has_wd;
};

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const AdamArgs& a, float coef, bool clipped,
                                         bool decay) {
  if (clipped) g = __fmul_rn(g, coef);
  if (decay) {
    if (a.decoupled) p = __fmul_rn(p, a.decay_mul);
    else g = fmaf(a.wd, p, g);
  }
  const float diff = __fsub_rn(g, m);           // lerp_ has two forms (ATen/native/Lerp.h): weight < 0.5, i.e. beta1 > 0.5 ...
  m = a.w1 < 0.5f ? fmaf(a.w1, diff, m) : fmaf(-diff, __fsub_rn(1.0f, a.w1), g);        // ... or end - (end - m)(1 - weight)
  v = fmaf(__fmul_rn(a.w2, g), g, __fmul_rn(v, a.beta2));
  const float denom = __fadd_rn(__fdiv_rn(__fsqrt_rn(v), a.bc2_sqrt), a.eps);
  p = fmaf(a.neg_step, __fdiv_rn(m, denom), p);
}

template <bool GUARD>
__global__ void __launch_bounds__(kThreads) flat_adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                            float* __restrict__ v, int64_t n, Table t, AdamArgs a,
                                                            const csnStepGuard* __restrict__ guard) {
  float gs;
  if (!guard_open<GUARD>(guard, gs)) return;
  const int64_t nchunks = (n + kChunk - 1) / kChunk;
  const bool clip = a.clip > 0.0f;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int64_t cs = c * kChunk;
    const int64_t ce = cs + kChunk < n ? cs + kChunk : n;
    const int s = t.chunk_seg[c];
    if (t.seg_end[s] >= cs + kChunk) {
      const int flags = t.seg_flags[s];
      const bool clipped = clip && (flags & kScaled);
      const bool decay = a.has_wd && (flags & kDecayed);
      const float coef = clipped ? clip_coef(t, s, a.clip) : 1.0f;
      float4 pv[2], gv[2], mv[2], vv[2];
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int64_t i = cs / 4 + k * kThreads + threadIdx.x;
        pv[k] = reinterpret_cast<float4*>(p)[i];
        gv[k] = reinterpret_cast<const float4*>(g)[i];
        mv[k] = reinterpret_cast<float4*>(m)[i];
        vv[k] = reinterpret_cast<float4*>(v)[i];
      }
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int64_t i = cs / 4 + k * kThreads + threadIdx.x;
        adam_one(pv[k].x, guarded<GUARD>(gv[k].x, gs), mv[k].x, vv[k].x, a, coef, clipped, decay);
        adam_one(pv[k].y, guarded<GUARD>(gv[k].y, gs), mv[k].y, vv[k].y, a, coef, clipped, decay);
        adam_one(pv[k].z, guarded<GUARD>(gv[k].z, gs), mv[k].z, vv[k].z, a, coef, clipped, decay);
        adam_one(pv[k].w, guarded<GUARD>(gv[k].w, gs), mv[k].w, vv[k].w, a, coef, clipped, decay);
        reinterpret_cast<float4*>(m)[i] = mv[k];
        reinterpret_cast<float4*>(v)[i] = vv[k];
        reinterpret_cast<float4*>(p)[i] = pv[k];
      }
    } else {
      for (int64_t i = cs + threadIdx.x; i < ce; i += kThreads) {
        int si = s;
        while (i >= t.seg_end[si]) ++si;
        const int flags = t.seg_flags[si];
        const bool clipped = clip && (flags & kScaled);
        const bool decay = a.has_wd && (flags & kDecayed);
        const float coef = clipped ? clip_coef(t, si, a.clip) : 1.0f;
        float pi = p[i], mi = m[i], vi = v[i];
        adam_one(pi, guarded<GUARD>(g[i], gs), mi, vi, a, coef, clipped, decay);
        m[i] = mi;
        v[i] = vi;
        p[i] = pi;
      }
    }
  }
}

// ---- LARS ---------------------------------------------------------------------------------------------------------------
// losses.LARS (EEG-BarlowNetworks/optim.py:17-44), one rounding per torch kernel:
//   d <- g + wd p   (decayed segments) ;  d <- d trust,  trust = eta |p| / |d| when both > 0   (scaled segments)
//   mu <- momentum mu ; mu <- mu + d ;  p <- p - lr mu
struct LarsArgs {
  float wd, momentum, eta, neg_lr;
  int has_wd;
};

__device__ __forceinline__ float lars_trust(const Table& t, int s, int nseg, float eta) {
  const float pn = (float)sqrt(t.sums[s]), dn = (float)sqrt(t.sums[nseg + s]);
  return (pn > 0.0f && dn > 0.0f) ? __fdiv_rn(__fmul_rn(eta, pn), dn) : 1.0f;
}

__device__ __forceinline__ void lars_one(float& p, float g, float& mu, const LarsArgs& a, float trust, bool scaled, bool decay) {
  float d = decay ? fmaf(a.wd, p, g) : g;
  if (scaled) d = __fmul_rn(d, trust);
  mu = __fadd_rn(__fmul_rn(mu, a.momentum), d);
  p = fmaf(a.neg_lr, mu, p);
}

template <bool GUARD>
__global__ void __launch_bounds__(kThreads) flat_lars_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ mu,
                                                            int64_t n, int nseg, Table t, LarsArgs a,
                                                            const csnStepGuard* __restrict__ guard) {
  float gs;
  if (!guard_open<GUARD>(guard, gs)) return;
  const int64_t nchunks = (n + kChunk - 1) / kChunk;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int64_t cs = c * kChunk;
    const int64_t ce = cs + kChunk < n ? cs + kChunk : n;
    const int s = t.chunk_seg[c];
    if (t.seg_end[s] >= cs + kChunk) {
      const int flags = t.seg_flags[s];
      const bool scaled = flags & kScaled;
      const bool decay = a.has_wd && (flags & kDecayed);
      const float trust = scaled ? lars_trust(t, s, nseg, a.eta) : 1.0f;
      float4 pv[2], gv[2], mv[2];
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int64_t i = cs / 4 + k * kThreads + threadIdx.x;
        pv[k] = reinterpret_cast<float4*>(p)[i];
        gv[k] = reinterpret_cast<const float4*>(g)[i];
        mv[k] = reinterpret_cast<float4*>(mu)[i];
      }
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int64_t i = cs / 4 + k * kThreads + threadIdx.x;
        lars_one(pv[k].x, guarded<GUARD>(gv[k].x, gs), mv[k].x, a, trust, scaled, decay);
        lars_one(pv[k].y, guarded<GUARD>(gv[k].y, gs), mv[k].y, a, trust, scaled, decay);
        lars_one(pv[k].z, guarded<GUARD>(gv[k].z, gs), mv[k].z, a, trust, scaled, decay);
        lars_one(pv[k].w, guarded<GUARD>(gv[k].w, gs), mv[k].w, a, trust, scaled, decay);
        reinterpret_cast<float4*>(mu)[i] = mv[k];
        reinterpret_cast<float4*>(p)[i] = pv[k];
      }
    } else {
      for (int64_t i = cs + threadIdx.x; i < ce; i += kThreads) {
        int si = s;
        while (i >= t.seg_end[si]) ++si;
        const int flags = t.seg_flags[si];
        const bool scaled = flags & kScaled;
        const bool decay = a.has_wd && (flags & kDecayed);
        const float trust = scaled ? lars_trust(t, si, nseg, a.eta) : 1.0f;
        float pi = p[i], mi = mu[i];
        lars_one(pi, guarded<GUARD>(g[i], gs), mi, a, trust, scaled, decay);
        mu[i] = mi;
        p[i] = pi;
      }
    }
  }
}

// ---- the guard: global sum of squares, norm, clip coefficient, finiteness ------------------------------------------------
// Stage one: partials[c] = sum over chunk c of (double)g^2 -- exact products, so a partial is non-finite exactly when an
// element of its chunk is.  Whole chunks take two 16-byte loads per thread, the last (short) one the scalar loop.
__global__ void __launch_bounds__(kThreads) grad_guard_partial_kernel(const float* __restrict__ g, int64_t n, double* __restrict__ partials) {
  __shared__ double lds[1][kThreads / 64];
  const int64_t nchunks = (n + kChunk - 1) / kChunk;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int64_t cs = c * kChunk;
    const int64_t ce = cs + kChunk < n ? cs + kChunk : n;
    double acc[1] = {};
    if (ce == cs + kChunk) {
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const float4 gv = reinterpret_cast<const float4*>(g)[cs / 4 + k * kThreads + threadIdx.x];
        sq_acc<false>(acc, gv.x, 0.f, 0.f, false);
        sq_acc<false>(acc, gv.y, 0.f, 0.f, false);
        sq_acc<false>(acc, gv.z, 0.f, 0.f, false);
        sq_acc<false>(acc, gv.w, 0.f, 0.f, false);
      }
    } else {
      for (int64_t i = cs + threadIdx.x; i < ce; i += kThreads) sq_acc<false>(acc, g[i], 0.f, 0.f, false);
    }
    block_sum<1>(acc, lds);
    if (threadIdx.x == 0) partials[c] = acc[0];
  }
}

__device__ __forceinline__ double read_lane(double v, int lane) {      // (lane: a compile-time constant after unrolling)
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}

// Stage two, ONE wave: S = (((p_0 + p_1) + p_2) + ...) in ascending chunk order -- 64 partials per coalesced load, then a
// chain of 64 additions that every lane performs alike on values read lane by lane (a slot behind the last chunk holds
// +0, and x + 0 == x for the x >= 0 or NaN that a sum of squares is).  Lane 0 writes the record with ordinary stores.
__global__ void __launch_bounds__(64) grad_guard_final_kernel(const double* __restrict__ partials, int64_t nchunks, double max_norm,
                                                              csnStepGuard* __restrict__ guard) {
  double sum = 0.0;
  for (int64_t base = 0; base < nchunks; base += 64) {
    const int64_t i = base + threadIdx.x;
    const double v = i < nchunks ? partials[i] : 0.0;
#pragma unroll
    for (int j = 0; j < 64; ++j) sum += read_lane(v, j);
  }
  if (threadIdx.x == 0) {
    const bool finite = isfinite(sum);
    const double root = sqrt(sum);
    guard->norm = (float)root;
    guard->scale = finite ? (float)fmin(1.0, max_norm / (root + 1e-6)) : 0.0f;      // clip_grad_norm_'s clip_coef_clamped
    guard->finite = finite ? 1u : 0u;
    guard->skipped += finite ? 0u : 1u;
  }
}

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static inline bool unit_interval(double b) { return b >= 0.0 && b < 1.0; }      // (false for NaN)

}  // namespace
}  // namespace csn

using namespace csn;

// (name: a const char*, so that an entry point and its _guarded twin share one body and each speaks under its own name)
#define CSN_FLAT_COMMON(name, table)                                                                                 \
  CSN_REQUIRE(nseg >= 1, "%s: nseg must be >= 1, got %d", name, nseg);                                                \
  CSN_REQUIRE(n >= nseg && n <= ((int64_t)1 << 40), "%s: n = %lld elements for %d segments", name, (long long)n, nseg); \
  CSN_REQUIRE(table != nullptr, "%s: null segment table", name);                                                       \
  CSN_REQUIRE(aligned16(table), "%s: the segment table must be 16-byte aligned", name)
#define CSN_GUARD_RECORD(name, guard)                                                                                \
  CSN_REQUIRE(guard != nullptr, "%s: null guard record (the unguarded entry point exists for that)", name);            \
  CSN_REQUIRE(aligned16(guard), "%s: the guard record must be 16-byte aligned", name)

extern "C" size_t csn_flat_segments_scratch_bytes(int nseg, int64_t n) {
  if (nseg < 1 || n < nseg || n > ((int64_t)1 << 40)) {
    fail(CSN_ERR_INVALID_ARGUMENT, "csn_flat_segments_scratch_bytes: bad nseg=%d n=%lld", nseg, (long long)n);
    return 0;
  }
  return table_layout(nullptr, nseg, n).bytes;
}

extern "C" int csn_flat_segments_prepare(const int64_t* seg_end, const int32_t* flags, int nseg, int64_t n, void* table,
                                         csnStream_t stream) {
  CSN_FLAT_COMMON("csn_flat_segments_prepare", table);
  CSN_REQUIRE(seg_end != nullptr, "csn_flat_segments_prepare: null seg_end");
  int64_t prev = 0;
  for (int s = 0; s < nseg; ++s) {
    CSN_REQUIRE(seg_end[s] > prev, "csn_flat_segments_prepare: segment ends must ascend strictly from above 0 (seg_end[%d] = %lld after %lld)",
                s, (long long)seg_end[s], (long long)prev);
    CSN_REQUIRE(!flags || (flags[s] & ~3) == 0, "csn_flat_segments_prepare: flags[%d] = %d (bits 0-1 only)", s, (int)flags[s]);
    prev = seg_end[s];
  }
  CSN_REQUIRE(prev == n, "csn_flat_segments_prepare: the last segment ends at %lld, the buffer at n = %lld", (long long)prev, (long long)n);
  const Table t = table_layout(table, nseg, n);
  hipStream_t st = as_stream(stream);
  int64_t first = 0, start = 0;
  for (int s0 = 0; s0 < nseg; s0 += kUpload) {
    UploadBatch b{};
    const int count = nseg - s0 < kUpload ? nseg - s0 : kUpload;
    for (int i = 0; i < count; ++i) {
      const int64_t e = seg_end[s0 + i];
      b.end[i] = e;
      b.first[i] = (int32_t)first;
      b.flags[i] = flags ? flags[s0 + i] : (kDecayed | kScaled);
      first += (e - 1) / kChunk - start / kChunk + 1;      // chunks this segment intersects
      start = e;
    }
    flat_segments_upload_kernel<<<1, 64, 0, st>>>(t, b, s0, count, nseg, (int)first);
    CSN_LAUNCH_CHECK();
  }
  const int64_t nchunks = num_chunks(n);
  flat_chunk_seg_kernel<<<(unsigned)((nchunks + kThreads - 1) / kThreads), kThreads, 0, st>>>(t, nseg, nchunks);
  CSN_LAUNCH_CHECK();
  return CSN_OK;
}

// The bodies below serve an entry point (guard == nullptr) and its _guarded twin (the record checked by the twin).
template <bool PAIR, bool GUARD>
static int launch_segment_norms(const float* a, const float* b, float wd, int64_t n, int nseg, const Table& t, float* norms_out,
                                const csnStepGuard* guard, hipStream_t st) {
  flat_sqsum_partial_kernel<PAIR, GUARD><<<grid_for(n), kThreads, 0, st>>>(a, b, wd, n, t, guard);
  CSN_LAUNCH_CHECK();
  flat_sqsum_final_kernel<GUARD><<<dim3((unsigned)nseg, PAIR ? 2 : 1), 64, 0, st>>>(t, nseg, norms_out, guard);
  CSN_LAUNCH_CHECK();
  return CSN_OK;
}

static int segment_norms(const char* who, const float* a, const float* b, float weight_decay, int64_t n, int nseg, void* table,
                         float* norms_out, const csnStepGuard* guard, csnStream_t stream) {
  CSN_FLAT_COMMON(who, table);
  CSN_REQUIRE(a != nullptr, "%s: null buffer", who);
  CSN_REQUIRE(aligned16(a) && aligned16(b), "%s: buffers must be 16-byte aligned", who);
  const Table t = table_layout(table, nseg, n);
  hipStream_t st = as_stream(stream);
  if (b) {
    return guard ? launch_segment_norms<true, true>(a, b, weight_decay, n, nseg, t, norms_out, guard, st)
                 : launch_segment_norms<true, false>(a, b, weight_decay, n, nseg, t, norms_out, nullptr, st);
  }
  return guard ? launch_segment_norms<false, true>(a, nullptr, 0.0f, n, nseg, t, norms_out, guard, st)
               : launch_segment_norms<false, false>(a, nullptr, 0.0f, n, nseg, t, norms_out, nullptr, st);
}

extern "C" int csn_flat_segment_norms(const float* a, const float* b, float weight_decay, int64_t n, int nseg, void* table,
                                      float* norms_out, csnStream_t stream) {
  return segment_norms("csn_flat_segment_norms", a, b, weight_decay, n, nseg, table, norms_out, nullptr, stream);
}

extern "C" int csn_flat_clip(float* grads, int64_t n, int nseg, void* table, float clip, float* norms_out, csnStream_t stream) {
  CSN_FLAT_COMMON("csn_flat_clip", table);
  CSN_REQUIRE(grads != nullptr, "csn_flat_clip: null gradient buffer");
  CSN_REQUIRE(aligned16(grads), "csn_flat_clip: buffers must be 16-byte aligned");
  CSN_REQUIRE(clip > 0.0f, "csn_flat_clip: clip must be > 0, got %g", (double)clip);
  int rc = csn_flat_segment_norms(grads, nullptr, 0.0f, n, nseg, table, norms_out, stream);
  if (rc) return rc;
  flat_clip_kernel<<<grid_for(n), kThreads, 0, as_stream(stream)>>>(grads, n, table_layout(table, nseg, n), clip);
  CSN_LAUNCH_CHECK();
  return CSN_OK;
}

static int adam_step(const char* who, float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, int nseg,
                     void* table, int64_t t, double lr, double beta1, double beta2, double eps, double weight_decay,
                     int decoupled, double clip, float* norms_out, const csnStepGuard* guard, csnStream_t stream) {
  CSN_FLAT_COMMON(who, table);
  CSN_REQUIRE(params && grads && exp_avg && exp_avg_sq, "%s: null pointer", who);
  CSN_REQUIRE(aligned16(params) && aligned16(grads) && aligned16(exp_avg) && aligned16(exp_avg_sq),
              "%s: buffers must be 16-byte aligned", who);
  CSN_REQUIRE(t >= 1, "%s: step count t must be >= 1, got %lld", who, (long long)t);
  CSN_REQUIRE(unit_interval(beta1) && unit_interval(beta2), "%s: betas must lie in [0, 1), got (%g, %g)", who, beta1, beta2);
  CSN_REQUIRE(lr >= 0.0 && eps >= 0.0 && weight_decay >= 0.0, "%s: lr, eps and weight_decay must be >= 0 (%g, %g, %g)", who,
              lr, eps, weight_decay);
  if (clip > 0.0) {       // per-tensor norms of the gradient first; the step scales g on the fly and leaves the buffer alone
    int rc = segment_norms(who, grads, nullptr, 0.0f, n, nseg, table, norms_out, guard, stream);      // (guarded: norms of g')
    if (rc) return rc;
  }
  const double bc1 = 1.0 - pow(beta1, (double)t), bc2 = 1.0 - pow(beta2, (double)t);
  AdamArgs a{};
  a.decay_mul = (float)(1.0 - lr * weight_decay);
  a.wd = (float)weight_decay;
  a.w1 = (float)(1.0 - beta1);
  a.beta2 = (float)beta2;
  a.w2 = (float)(1.0 - beta2);
  a.bc2_sqrt = (float)sqrt(bc2);
  a.neg_step = (float)(-(lr / bc1));
  a.eps = (float)eps;
  a.clip = clip > 0.0 ? (float)clip : 0.0f;
  a.decoupled = decoupled != 0;
  a.has_wd = weight_decay != 0.0;
  const Table tb = table_layout(table, nseg, n);
  if (guard)
    flat_adam_kernel<true><<<grid_for(n), kThreads, 0, as_stream(stream)>>>(params, grads, exp_avg, exp_avg_sq, n, tb, a, guard);
  else
    flat_adam_kernel<false><<<grid_for(n), kThreads, 0, as_stream(stream)>>>(params, grads, exp_avg, exp_avg_sq, n, tb, a, nullptr);
  CSN_LAUNCH_CHECK();
  return CSN_OK;
}

extern "C" int csn_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, int nseg,
                             void* table, int64_t t, double lr, double beta1, double beta2, double eps, double weight_decay,
                             int decoupled, double clip, float* norms_out, csnStream_t stream) {
  return adam_step("csn_adam_step", params, grads, exp_avg, exp_avg_sq, n, nseg, table, t, lr, beta1, beta2, eps, weight_decay,
                   decoupled, clip, norms_out, nullptr, stream);
}

extern "C" int csn_adam_step_guarded(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, int nseg,
                                     void* table, int64_t t, double lr, double beta1, double beta2, double eps,
                                     double weight_decay, int decoupled, double clip, float* norms_out, const csnStepGuard* guard,
                                     csnStream_t stream) {
  CSN_GUARD_RECORD("csn_adam_step_guarded", guard);
  return adam_step("csn_adam_step_guarded", params, grads, exp_avg, exp_avg_sq, n, nseg, table, t, lr, beta1, beta2, eps,
                   weight_decay, decoupled, clip, norms_out, guard, stream);
}

static int lars_step(const char* who, float* params, const float* grads, float* mu, int64_t n, int nseg, void* table, double lr,
                     double weight_decay, double momentum, double eta, const csnStepGuard* guard, csnStream_t stream) {
  CSN_FLAT_COMMON(who, table);
  CSN_REQUIRE(params && grads && mu, "%s: null pointer", who);
  CSN_REQUIRE(aligned16(params) && aligned16(grads) && aligned16(mu), "%s: buffers must be 16-byte aligned", who);
  int rc = segment_norms(who, params, grads, (float)weight_decay, n, nseg, table, nullptr, guard, stream);
  if (rc) return rc;
  LarsArgs a{};
  a.wd = (float)weight_decay;
  a.momentum = (float)momentum;
  a.eta = (float)eta;
  a.neg_lr = (float)(-lr);
  a.has_wd = weight_decay != 0.0;
  const Table tb = table_layout(table, nseg, n);
  if (guard)
    flat_lars_kernel<true><<<grid_for(n), kThreads, 0, as_stream(stream)>>>(params, grads, mu, n, nseg, tb, a, guard);
  else
    flat_lars_kernel<false><<<grid_for(n), kThreads, 0, as_stream(stream)>>>(params, grads, mu, n, nseg, tb, a, nullptr);
  CSN_LAUNCH_CHECK();
  return CSN_OK;
}

extern "C" int csn_lars_step(float* params, const float* grads, float* mu, int64_t n, int nseg, void* table, double lr,
                             double weight_decay, double momentum, double eta, csnStream_t stream) {
  return lars_step("csn_lars_step", params, grads, mu, n, nseg, table, lr, weight_decay, momentum, eta, nullptr, stream);
}

extern "C" int csn_lars_step_guarded(float* params, const float* grads, float* mu, int64_t n, int nseg, void* table, double lr,
                                     double weight_decay, double momentum, double eta, const csnStepGuard* guard,
                                     csnStream_t stream) {
  CSN_GUARD_RECORD("csn_lars_step_guarded", guard);
  return lars_step("csn_lars_step_guarded", params, grads, mu, n, nseg, table, lr, weight_decay, momentum, eta, guard, stream);
}

// ---- the guard ------------------------------------------------------------------------------------------------------------
extern "C" size_t csn_grad_guard_scratch_bytes(int64_t n) {
  if (n <= 0 || n > ((int64_t)1 << 40)) {
    fail(CSN_ERR_INVALID_ARGUMENT, "csn_grad_guard_scratch_bytes: bad n=%lld", (long long)n);
    return 0;
  }
  return align_up((size_t)num_chunks(n) * 8, 16);
}

extern "C" int csn_grad_guard(const float* grads, int64_t n, double max_norm, void* scratch, csnStepGuard* guard,
                              csnStream_t stream) {
  CSN_REQUIRE(n > 0 && n <= ((int64_t)1 << 40), "csn_grad_guard: n = %lld elements", (long long)n);
  CSN_REQUIRE(grads != nullptr, "csn_grad_guard: null gradient buffer");
  CSN_REQUIRE(scratch != nullptr, "csn_grad_guard: null scratch");
  CSN_REQUIRE(aligned16(grads) && aligned16(scratch), "csn_grad_guard: the gradient buffer and the scratch must be 16-byte aligned");
  CSN_GUARD_RECORD("csn_grad_guard", guard);
  CSN_REQUIRE(max_norm > 0.0, "csn_grad_guard: max_norm must be > 0 (+INFINITY: measure and gate only), got %g", max_norm);      // (false for NaN)
  hipStream_t st = as_stream(stream);
  double* partials = static_cast<double*>(scratch);
  grad_guard_partial_kernel<<<grid_for(n), kThreads, 0, st>>>(grads, n, partials);
  CSN_LAUNCH_CHECK();
  grad_guard_final_kernel<<<1, 64, 0, st>>>(partials, num_chunks(n), max_norm, guard);
  CSN_LAUNCH_CHECK();
  return CSN_OK;
}
