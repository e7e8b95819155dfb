// K8, retrieval evaluation behind the search (csn_topk_merge / csn_topk_class_metrics).
//
// Kernel 1 (topk_merge_kernel), one workgroup per query: the exact merge of P candidate lists of k_in (float64 distance,
//   int64 index) pairs, the device form of retrieval.merge_topk.  The P * k_in candidates of the query are staged in LDS
//   when they fit (STAGED_MAX pairs, 32 KiB) and re-read from L2 when they do not, then k rounds of a block arg-min as in
//   chan_l2_select_kernel: round r takes the smallest key that is greater than round r-1's pick, so nothing is masked and
//   the inputs stay read-only.  The key is (distance, index, position in the concatenated list): the position makes every
//   key distinct, so the tie argument of DESIGN.md section 17 holds even where two parts carry the same pair, and it is
//   the order a stable sort on (index, distance) leaves equal pairs in.  A padding entry (index < 0) is no candidate at
//   all, whatever its distance; a real +inf is one.  When a round finds nothing, it and every later place get (+inf, -1).
// Kernel 2 (class_metrics_init_kernel): out_class rows = {0, 0, 0, -1}, out_top1_correct = 0.
// Kernel 3 (class_metrics_kernel), one wave per query: the lanes walk the k neighbours, look their classes up and count
//   the ones of the query's class with a wave reduction; lane 0 writes the per-query outputs and folds the query into its
//   class row with integer atomic adds and an atomic min.  The first-query column is kept as an unsigned minimum that
//   starts at all ones, which read as int64 is the -1 of a class without queries.  Integer sums and a minimum do not depend
//   on the order of their operands, so the result does not depend on grid, scheduling or stream.
// No workgroup waits on another; every loop is bounded by k, k_in * P or n_classes.
#include "csn_common.h"

namespace csn {

namespace tkm {
constexpr int MAX_K = 1024;
constexpr int MAX_PARTS = 64;
constexpr int STAGED_MAX = 2048;      // candidate pairs of a query the merge keeps in LDS (32 KiB); more stay in L2
constexpr int MAX_CLASSES = 65536;
}  // namespace tkm

using namespace tkm;

template <bool STAGED>
__global__ void __launch_bounds__(256)
topk_merge_kernel(const double* __restrict__ D_parts, const int64_t* __restrict__ I_parts, int P, int64_t Nq, int k_in,
                  int k, int64_t* __restrict__ out_idx, double* __restrict__ out_dist64, float* __restrict__ out_dist) {
  __shared__ double ds[STAGED ? STAGED_MAX : 1];
  __shared__ int64_t is[STAGED ? STAGED_MAX : 1];
  __shared__ double wd[2][4];
  __shared__ int64_t wi[2][4];
  __shared__ int wp[2][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t q = blockIdx.x;
  const int n = P * k_in;               // <= 64 * 1024
  // candidate c = (part c / k_in, place c % k_in): the position in merge_topk's concatenation along the second axis
  auto offset = [&](int c) -> int64_t { return ((int64_t)(c / k_in) * Nq + q) * k_in + c % k_in; };
  if (STAGED) {
    for (int c = tid; c < n; c += 256) {
      const int64_t o = offset(c);
      ds[c] = D_parts[o];
      is[c] = I_parts[o];
    }
    __syncthreads();
  }
  const double INF = __builtin_inf();
  double last_d = -INF;                 // the pick of the previous round: this round takes the smallest key after it
  int64_t last_i = -1;
  int last_p = -1;
  int r = 0;
  for (; r < k; ++r) {
    double best = INF;
    int64_t bi = INT64_MAX;
    int bp = INT32_MAX;                 // INT32_MAX: this thread has no candidate (a real one may be (+inf, INT64_MAX))
    for (int c = tid; c < n; c += 256) {           // ascending c: the first of equal pairs is the lowest position
      double v;
      int64_t i;
      if (STAGED) {
        v = ds[c];
        i = is[c];
      } else {
        const int64_t o = offset(c);
        v = D_parts[o];
        i = I_parts[o];
      }
      if (i < 0) continue;                         // padding
      const bool after = v > last_d || (v == last_d && (i > last_i || (i == last_i && c > last_p)));
      const bool less = bp == INT32_MAX ? v <= best : (v < best || (v == best && i < bi));
      if (after && less) { best = v; bi = i; bp = c; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double od = __shfl_down(best, off);
      const int64_t oi = __shfl_down(bi, off);
      const int op = __shfl_down(bp, off);
      if (op != INT32_MAX && (bp == INT32_MAX || od < best || (od == best && (oi < bi || (oi == bi && op < bp))))) {
        best = od; bi = oi; bp = op;
      }
    }
    const int s = r & 1;                // two slots: a wave may enter round r + 1 while another still reads round r's
    if (lane == 0) {
      wd[s][wave] = best;
      wi[s][wave] = bi;
      wp[s][wave] = bp;
    }
    __syncthreads();
    best = wd[s][0];
    bi = wi[s][0];
    bp = wp[s][0];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      const double od = wd[s][w];
      const int64_t oi = wi[s][w];
      const int op = wp[s][w];
      if (op != INT32_MAX && (bp == INT32_MAX || od < best || (od == best && (oi < bi || (oi == bi && op < bp))))) {
        best = od; bi = oi; bp = op;
      }
    }
    if (bp == INT32_MAX) break;         // no real candidate is left (the same for every thread): the rest is padding
    last_d = best;
    last_i = bi;
    last_p = bp;
    if (tid == 0) {
      out_idx[q * k + r] = bi;
      if (out_dist64) out_dist64[q * k + r] = best;
      if (out_dist) out_dist[q * k + r] = (float)best;
    }
  }
  for (int e = r + tid; e < k; e += 256) {
    out_idx[q * k + e] = -1;
    if (out_dist64) out_dist64[q * k + e] = INF;
    if (out_dist) out_dist[q * k + e] = (float)INF;
  }
}

__global__ void __launch_bounds__(256)
class_metrics_init_kernel(int64_t* __restrict__ out_class, int n_classes, int64_t* __restrict__ out_top1_correct) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (out_class && i < n_classes * 4) out_class[i] = (i & 3) == 3 ? -1 : 0;
  if (out_top1_correct && i == 0) out_top1_correct[0] = 0;
}

__global__ void __launch_bounds__(256)
class_metrics_kernel(const int64_t* __restrict__ idx, int64_t Nq, int k, const int* __restrict__ gallery_class, int64_t Ng,
                     const int* __restrict__ query_class, int n_classes, int* __restrict__ out_hits,
                     int* __restrict__ out_top1, int* __restrict__ out_pred, int64_t* __restrict__ out_class,
                     int64_t* __restrict__ out_top1_correct) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= Nq) return;                  // whole waves leave: no barrier follows
  const int qc = query_class[q];
  const int64_t* row = idx + q * k;
  int hits = 0;
  for (int r = lane; r < k; r += 64) {
    const int64_t g = row[r];
    if (g >= 0 && g < Ng) hits += gallery_class[g] == qc ? 1 : 0;      // a negative (or too large) index is a miss
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) hits += __shfl_down(hits, off);
  if (lane != 0) return;
  const int64_t g0 = row[0];
  const int top1 = (g0 >= 0 && g0 < Ng) ? gallery_class[g0] : -1;
  if (out_hits) out_hits[q] = hits;
  if (out_top1) out_top1[q] = top1;
  if (out_pred) out_pred[q] = hits > 0 ? qc : top1;
  if (out_class && qc >= 0 && qc < n_classes) {
    unsigned long long* c = reinterpret_cast<unsigned long long*>(out_class + (int64_t)qc * 4);
    atomicAdd(c + 0, 1ull);
    if (hits > 0) {
      atomicAdd(c + 1, 1ull);
      atomicAdd(c + 2, (unsigned long long)hits);
    }
    atomicMin(c + 3, (unsigned long long)q);       // starts at all ones = (int64) -1
  }
  if (out_top1_correct && top1 >= 0 && top1 == qc) atomicAdd(reinterpret_cast<unsigned long long*>(out_top1_correct), 1ull);
}

}  // namespace csn

using namespace csn;

extern "C" int csn_topk_merge_staged_max(void) { return STAGED_MAX; }

extern "C" int csn_topk_merge(const double* D_parts, const int64_t* I_parts, int P, int64_t Nq, int k_in, int k,
                              int64_t* out_idx, double* out_dist64, float* out_dist, csnStream_t stream) {
  CSN_REQUIRE(D_parts && I_parts && out_idx, "csn_topk_merge: null pointer");
  CSN_REQUIRE(P > 0 && Nq > 0 && k_in > 0 && k > 0, "csn_topk_merge: bad shape");
  CSN_REQUIRE(k <= MAX_K && k_in <= MAX_K && P <= MAX_PARTS,
              "csn_topk_merge: k=%d and k_in=%d must be at most 1024, P=%d at most 64", k, k_in, P);
  CSN_REQUIRE((int64_t)P * k_in >= k, "csn_topk_merge: P*k_in=%lld candidates are fewer than k=%d",
              (long long)P * k_in, k);
  CSN_REQUIRE(Nq <= 0x7fffffff, "csn_topk_merge: Nq too large for one grid");
  hipStream_t st = as_stream(stream);
  if (P * k_in <= STAGED_MAX)
    topk_merge_kernel<true><<<(unsigned)Nq, 256, 0, st>>>(D_parts, I_parts, P, Nq, k_in, k, out_idx, out_dist64, out_dist);
  else
    topk_merge_kernel<false><<<(unsigned)Nq, 256, 0, st>>>(D_parts, I_parts, P, Nq, k_in, k, out_idx, out_dist64, out_dist);
  CSN_LAUNCH_CHECK();
  return CSN_OK;
}

extern "C" int csn_topk_class_metrics(const int64_t* idx, int64_t Nq, int k, const int32_t* gallery_class, int64_t Ng,
                                      const int32_t* query_class, int n_classes, int32_t* out_hits, int32_t* out_top1,
                                      int32_t* out_pred, int64_t* out_class, int64_t* out_top1_correct,
                                      csnStream_t stream) {
  CSN_REQUIRE(idx && gallery_class && query_class, "csn_topk_class_metrics: null pointer");
  CSN_REQUIRE(out_hits || out_top1 || out_pred || out_class || out_top1_correct,
              "csn_topk_class_metrics: every output is null");
  CSN_REQUIRE(Nq > 0 && Ng > 0 && k > 0 && n_classes > 0, "csn_topk_class_metrics: bad shape");
  CSN_REQUIRE(k <= MAX_K, "csn_topk_class_metrics: k=%d must be at most 1024", k);
  CSN_REQUIRE(n_classes <= MAX_CLASSES, "csn_topk_class_metrics: n_classes=%d must be at most 65536", n_classes);
  CSN_REQUIRE((Nq + 3) / 4 <= 0x7fffffff, "csn_topk_class_metrics: Nq too large for one grid");
  hipStream_t st = as_stream(stream);
  if (out_class || out_top1_correct) {
    class_metrics_init_kernel<<<(unsigned)((n_classes * 4 + 255) / 256), 256, 0, st>>>(out_class, n_classes,
                                                                                      out_top1_correct);
    CSN_LAUNCH_CHECK();
  }
  class_metrics_kernel<<<(unsigned)((Nq + 3) / 4), 256, 0, st>>>(idx, Nq, k, gallery_class, Ng, query_class, n_classes,
                                                                out_hits, out_top1, out_pred, out_class, out_top1_correct);
  CSN_LAUNCH_CHECK();
  return CSN_OK;
}
