// K8, tiled form: exact squared-L2 top-k without the distance matrix (csn_l2_topk_tiled).
//
// Kernel 1 (l2_topk_tiled_kernel), grid = query tiles x gallery splits.  A workgroup of 256 threads owns 64 queries and
// one contiguous range of gallery rows, which it walks in ascending tiles of 64 rows.
//   distances: 4 x 4 pairs per thread (16 float64 accumulators); operand rows staged through LDS in 32-wide slices of d
//              as float32, transposed ([d][row], row stride 68 words so that the staging writes and the 16-byte reads are
//              conflict free), each element converted to float64 once per thread that reads it; the inner loop is
//              sub + fma on registers.  One chain per pair in ascending d: the bits of csn_l2_topk.
//   selection: the finished 64 x 64 tile goes to LDS (over the operand slices); each wave owns 16 of the queries.  Lane l
//              reads the distance to gallery row g0 + l, so the lanes of a wave ARE the tile in ascending index order.
//              A candidate passes only if d < tau (strictly), tau = the k-th best of the query's list once that holds k
//              entries, +inf before.  The passing lanes are ranked by (d, lane) in the wave and merged into the query's
//              sorted list by rank computation, list entries first on equal distance (they have lower indices).
//   The lists live in the caller's scratch, two buffers per (split, query): a merge reads one and writes the other.
// Kernel 2 (l2_topk_merge_splits_kernel), one workgroup per query: merges the splits' sorted lists pairwise (log2 S
// rounds of rank computation, the list of the lower index range first on equal distance) and writes the outputs.
// No workgroup waits on another; every loop is bounded by the shapes.
#include "l2_tile.h"

namespace csn {

namespace tk {
// (TQ, TG, DS, LDP and the distance-tile body: l2_tile.h, shared with channel_l2.hip)
constexpr int DTP = 66;       // float64 per row of the distance tile
constexpr int MAX_K = 1024, MAX_SPLITS = 64, TARGET_WGS = 512 /* 256 CUs about twice over */;

struct Lists {
  double* d[2];        // [splits][Nq][k] each
  int64_t* i[2];
  int* meta;           // [splits][Nq][2]: entries in the list, which buffer holds it
};

// the most splits a call may use (the scratch is sized for it): what the library would choose, or 8, within the gallery
static inline int splits_auto(int64_t Ng, int64_t Nq) {
  const int64_t qt = cdiv(Nq, TQ), gt = cdiv(Ng, TG);
  int64_t s = cdiv(TARGET_WGS, qt);
  if (s > MAX_SPLITS) s = MAX_SPLITS;
  if (s > gt) s = gt;
  return (int)(s < 1 ? 1 : s);
}
static inline int splits_cap(int64_t Ng, int64_t Nq) {
  const int64_t gt = cdiv(Ng, TG);
  int64_t s = splits_auto(Ng, Nq);
  if (s < 8) s = 8;
  if (s > gt) s = gt;
  return (int)s;
}
}  // namespace tk

using namespace tk;

// One wave merges the passing candidates of one query's tile row into the query's list.  Every lane of the wave calls it.
// d / pass / gidx: this lane's candidate; m: ballot of pass; n: entries in the source list; cs: 64 float64 of LDS of this wave.
__device__ __forceinline__ void merge_tile_row(double d, bool pass, uint64_t m, int lane, int64_t gidx, int k, int n,
                                               const double* sd, const int64_t* si, double* dd, int64_t* di,
                                               double* cs, double* tau_slot) {
  // the source list was written by other lanes of this wave in an earlier merge: workgroup scope orders that (one CU, one
  // vector L1) without the L2 write-back an agent-scope fence costs on this multi-die part
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  int crank = 0;        // rank of this candidate among the passing ones under (d, lane)
  for (uint64_t mm = m; mm; mm &= mm - 1) {
    const int j = __builtin_ctzll(mm);
    const double dj = __shfl(d, j);
    crank += (dj < d || (dj == d && j < lane)) ? 1 : 0;
  }
  const int nc = __builtin_popcountll(m);
  if (pass) cs[crank] = d;
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
  if (pass) {
    int lo = 0, hi = n;                     // list entries with distance <= d go first
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (sd[mid] <= d) lo = mid + 1; else hi = mid;
    }
    const int p = crank + lo;
    if (p < k) {
      dd[p] = d;
      di[p] = gidx;
      if (p == k - 1) *tau_slot = d;
    }
  }
  for (int i = lane; i < n; i += 64) {
    const double ld = sd[i];
    const int64_t li = si[i];
    int lo = 0, hi = nc;                    // candidates with distance < ld go first
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (cs[mid] < ld) lo = mid + 1; else hi = mid;
    }
    const int p = i + lo;
    if (p < k) {
      dd[p] = ld;
      di[p] = li;
      if (p == k - 1) *tau_slot = ld;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__global__ void __launch_bounds__(256)
l2_topk_tiled_kernel(const float* __restrict__ gallery, const float* __restrict__ query, int64_t Ng, int64_t Nq, int D,
                     int k, int64_t tiles_per_split, Lists L) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[TQ * DTP * sizeof(double)];
  __shared__ double tau[TQ];
  __shared__ double cs[4][64];
  __shared__ int cnt[TQ], cur[TQ];
  float* qs = reinterpret_cast<float*>(smem);          // [DS][LDP]
  float* gs = qs + DS * LDP;                           // [DS][LDP]; 2 * 32 * 68 * 4 = 17408 bytes of the 33792
  double* dt = reinterpret_cast<double*>(smem);        // [TQ][DTP], after the last slice of a tile

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tq = tid >> 4, tg = tid & 15;
  const int64_t q0 = (int64_t)blockIdx.x * TQ;
  const int split = blockIdx.y;
  const int64_t gtiles = (Ng + TG - 1) / TG;
  const int64_t t_begin = (int64_t)split * tiles_per_split;
  const int64_t t_end = (t_begin + tiles_per_split < gtiles) ? t_begin + tiles_per_split : gtiles;
  const int64_t g_end = (t_end * TG < Ng) ? t_end * TG : Ng;

  if (tid < TQ) {
    tau[tid] = __builtin_inf();
    cnt[tid] = 0;
    cur[tid] = 0;
  }
  for (int64_t t = t_begin; t < t_end; ++t) {
    const int64_t g0 = t * TG;
    double acc[4][4];
    l2_tile_distances(
        acc, qs, gs, tid, D,
        [&](int r, int c) { return (q0 + r < Nq && c < D) ? query[(q0 + r) * D + c] : 0.0f; },
        [&](int r, int c) { return (g0 + r < g_end && c < D) ? gallery[(g0 + r) * D + c] : 0.0f; });
    __syncthreads();            // every wave is done with the operand slices: the distance tile takes their place
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) dt[(tq * 4 + i) * DTP + tg * 4 + j] = acc[i][j];
    __syncthreads();

    const bool col_ok = g0 + lane < g_end;
    for (int qi = 0; qi < 16; ++qi) {
      const int ql = wave * 16 + qi;
      const int64_t qg = q0 + ql;
      if (qg >= Nq) break;
      const double d = dt[ql * DTP + lane];
      const bool pass = col_ok && d < tau[ql];
      const uint64_t m = __ballot(pass);
      if (m == 0) continue;
      const int n = cnt[ql], b = cur[ql];
      const int64_t base = ((int64_t)split * Nq + qg) * k;
      merge_tile_row(d, pass, m, lane, g0 + lane, k, n, L.d[b] + base, L.i[b] + base, L.d[b ^ 1] + base,
                     L.i[b ^ 1] + base, cs[wave], &tau[ql]);
      if (lane == 0) {
        const int nn = n + __builtin_popcountll(m);
        cnt[ql] = nn < k ? nn : k;
        cur[ql] = b ^ 1;
      }
    }
  }
  __syncthreads();
  if (tid < TQ && q0 + tid < Nq) {
    int* mt = L.meta + ((int64_t)split * Nq + q0 + tid) * 2;
    mt[0] = cnt[tid];
    mt[1] = cur[tid];
  }
}

// One workgroup per query: pairwise rounds over the splits' lists (list a absorbs list a + step into its other buffer).
__global__ void __launch_bounds__(256)
l2_topk_merge_splits_kernel(Lists L, int64_t Nq, int k, int S, int64_t* __restrict__ out_idx,
                            float* __restrict__ out_dist, double* __restrict__ out_dist64) {
  __shared__ int cnt[MAX_SPLITS], cur[MAX_SPLITS];
  const int tid = threadIdx.x;
  const int64_t q = blockIdx.x;
  if (tid < S) {
    const int* mt = L.meta + ((int64_t)tid * Nq + q) * 2;
    cnt[tid] = mt[0];
    cur[tid] = mt[1];
  }
  __syncthreads();
  for (int step = 1; step < S; step <<= 1) {
    for (int a = 0; a + step < S; a += 2 * step) {
      const int b = a + step;
      const int na = cnt[a], nb = cnt[b];
      const int64_t oa = ((int64_t)a * Nq + q) * k, ob = ((int64_t)b * Nq + q) * k;
      const double* ad = L.d[cur[a]] + oa;
      const int64_t* ai = L.i[cur[a]] + oa;
      const double* bd = L.d[cur[b]] + ob;
      const int64_t* bi = L.i[cur[b]] + ob;
      double* od = L.d[cur[a] ^ 1] + oa;
      int64_t* oi = L.i[cur[a] ^ 1] + oa;
      for (int e = tid; e < na + nb; e += 256) {
        double d;
        int64_t ix;
        int lo = 0, hi, own;
        if (e < na) {             // an entry of a: entries of b (higher indices) go first only if strictly smaller
          own = e; d = ad[e]; ix = ai[e]; hi = nb;
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (bd[mid] < d) lo = mid + 1; else hi = mid;
          }
        } else {                  // an entry of b: entries of a go first on equal distance too
          own = e - na; d = bd[own]; ix = bi[own]; hi = na;
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (ad[mid] <= d) lo = mid + 1; else hi = mid;
          }
        }
        const int p = own + lo;
        if (p < k) {
          od[p] = d;
          oi[p] = ix;
        }
      }
    }
    __syncthreads();            // (a workgroup-scope fence too: the next round reads what other waves of this CU wrote)
    if (tid < S && (tid % (2 * step)) == 0 && tid + step < S) {
      const int nn = cnt[tid] + cnt[tid + step];
      cnt[tid] = nn < k ? nn : k;
      cur[tid] ^= 1;
    }
    __syncthreads();
  }
  const int64_t o0 = q * k;      // list 0 holds min(k, Ng) = k entries now
  const double* rd = L.d[cur[0]] + o0;
  const int64_t* ri = L.i[cur[0]] + o0;
  for (int e = tid; e < k; e += 256) {
    const double d = rd[e];
    out_idx[o0 + e] = ri[e];
    out_dist[o0 + e] = (float)d;
    if (out_dist64) out_dist64[o0 + e] = d;
  }
}

}  // namespace csn

using namespace csn;

static bool tiled_args_ok(int64_t Ng, int64_t Nq, int k, const char* who) {
  if (Ng <= 0 || Nq <= 0) {
    fail(CSN_ERR_INVALID_ARGUMENT, "%s: bad shape", who);
    return false;
  }
  if (k <= 0 || k > MAX_K || k > Ng) {
    fail(CSN_ERR_INVALID_ARGUMENT, "%s: k=%d must be in 1..min(1024, Ng)", who, k);
    return false;
  }
  return true;
}

static size_t lists_bytes(int64_t Nq, int k, int S) { return align_up((size_t)S * (size_t)Nq * (size_t)k * 8, 256); }

extern "C" size_t csn_l2_topk_tiled_scratch_bytes(int64_t Ng, int64_t Nq, int k) {
  if (!tiled_args_ok(Ng, Nq, k, "csn_l2_topk_tiled_scratch_bytes")) return 0;
  const int S = splits_cap(Ng, Nq);
  return 4 * lists_bytes(Nq, k, S) + align_up((size_t)S * (size_t)Nq * 2 * sizeof(int), 256);
}

extern "C" int csn_l2_topk_tiled(const float* gallery, const float* query, int64_t Ng, int64_t Nq, int D, int k,
                                 int splits, int64_t* out_idx, float* out_dist, double* out_dist64, void* scratch,
                                 csnStream_t stream) {
  CSN_REQUIRE(gallery && query && out_idx && out_dist && scratch, "csn_l2_topk_tiled: null pointer");
  CSN_REQUIRE(D > 0, "csn_l2_topk_tiled: bad shape");
  if (!tiled_args_ok(Ng, Nq, k, "csn_l2_topk_tiled")) return CSN_ERR_INVALID_ARGUMENT;
  CSN_REQUIRE(splits >= 0, "csn_l2_topk_tiled: splits=%d must be >= 0 (0 = the library chooses)", splits);
  const int64_t gtiles = cdiv(Ng, TG), qtiles = cdiv(Nq, TQ);
  CSN_REQUIRE(qtiles <= 0x7fffffff, "csn_l2_topk_tiled: Nq too large");
  const int cap = splits_cap(Ng, Nq);
  int S = splits == 0 ? splits_auto(Ng, Nq) : (splits < cap ? splits : cap);
  const int64_t tps = cdiv(gtiles, S);
  S = (int)cdiv(gtiles, tps);              // no empty range
  Lists L;
  unsigned char* p = static_cast<unsigned char*>(scratch);
  const size_t lb = lists_bytes(Nq, k, cap);
  L.d[0] = reinterpret_cast<double*>(p);
  L.d[1] = reinterpret_cast<double*>(p + lb);
  L.i[0] = reinterpret_cast<int64_t*>(p + 2 * lb);
  L.i[1] = reinterpret_cast<int64_t*>(p + 3 * lb);
  L.meta = reinterpret_cast<int*>(p + 4 * lb);
  hipStream_t st = as_stream(stream);
  l2_topk_tiled_kernel<<<dim3((unsigned)qtiles, (unsigned)S), 256, 0, st>>>(gallery, query, Ng, Nq, D, k, tps, L);
  CSN_LAUNCH_CHECK();
  l2_topk_merge_splits_kernel<<<dim3((unsigned)Nq), 256, 0, st>>>(L, Nq, k, S, out_idx, out_dist, out_dist64);
  CSN_LAUNCH_CHECK();
  return CSN_OK;
}
