// K8, channel discovery: per-channel squared-L2 matrices and the batched selection of one greedy round
// (csn_chan_l2_dist / csn_chan_l2_select / csn_chan_l2_accumulate).
//
// The squared L2 distance over a channel subset is the sum of the per-channel distances, so the greedy forward selection
// of TestRetrieval_Perils_DiscoverChannels.py:125-351 needs the per-channel matrices once and, per round, one float64
// add and one selection per (candidate, query, gallery row).
//
// Kernel 1 (chan_l2_dist_kernel), grid = query tiles x gallery tiles x channels of the launch.  The distance tile of
//   csn_l2_topk_tiled (l2_tile.h) on the rows X[n, c_j, t0:t1] of the resident channel-first recordings, read in place
//   through (ld_n, ld_c); zeros are staged beyond the window and the rows.  The 64 x 64 tile goes straight to Dc with 64-bit
//   offsets.  The host passes the channel list by value, up to 64 channels per launch.
// Kernel 2 (chan_l2_select_kernel), one workgroup per (query, candidate) row: v[g] = base[q,g] + Dc[j,q,g] (one IEEE add;
//   Dc itself without base), staged in LDS when the row fits, then k rounds of a block arg-min under (value, index).
//   Round r takes the smallest pair that is greater than round r-1's pick, so nothing is masked and the inputs stay
//   read-only.  Thread 0 writes the outputs and counts the class hits.
// Kernel 3 (chan_l2_accumulate_kernel): base = first ? D_one : base + D_one, element-wise.
// No workgroup waits on another, there are no atomics, every loop is bounded by Ng, k or the window.
#include "l2_tile.h"

namespace csn {

namespace chl2 {
constexpr int MAX_CH_PER_LAUNCH = 64;
constexpr int MAX_K = 64;
constexpr int STAGE_ROWS = 2048;      // float64 values of a row the selection keeps in LDS (16 KiB); longer rows stay in L2
struct ChannelList { int ch[MAX_CH_PER_LAUNCH]; };
}  // namespace chl2

using namespace tk;
using namespace chl2;

__global__ void __launch_bounds__(256)
chan_l2_dist_kernel(const float* __restrict__ gallery, int64_t g_ld_n, int64_t g_ld_c, const float* __restrict__ query,
                    int64_t q_ld_n, int64_t q_ld_c, int64_t Ng, int64_t Nq, int t0, int Tw, ChannelList cl, int64_t j0,
                    double* __restrict__ Dc) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[TILE_LDS_BYTES];
  float* qs = reinterpret_cast<float*>(smem);          // [DS][LDP]
  float* gs = qs + DS * LDP;                           // [DS][LDP]
  const int tid = threadIdx.x;
  const int tq = tid >> 4, tg = tid & 15;
  const int64_t q0 = (int64_t)blockIdx.x * TQ, g0 = (int64_t)blockIdx.y * TG;
  const int c = cl.ch[blockIdx.z];
  const float* qb = query + (int64_t)c * q_ld_c + t0;
  const float* gb = gallery + (int64_t)c * g_ld_c + t0;

  double acc[4][4];
  l2_tile_distances(
      acc, qs, gs, tid, Tw,
      [&](int r, int t) { return (q0 + r < Nq && t < Tw) ? qb[(q0 + r) * q_ld_n + t] : 0.0f; },
      [&](int r, int t) { return (g0 + r < Ng && t < Tw) ? gb[(g0 + r) * g_ld_n + t] : 0.0f; });

  double* out = Dc + (j0 + blockIdx.z) * Nq * Ng;      // 64-bit: nch * Nq * Ng passes 2^31 at full size
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t q = q0 + tq * 4 + i;
    if (q >= Nq) break;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t g = g0 + tg * 4 + j;
      if (g < Ng) out[q * Ng + g] = acc[i][j];
    }
  }
}

template <bool STAGED>
__global__ void __launch_bounds__(256)
chan_l2_select_kernel(const double* __restrict__ base, const double* __restrict__ Dc, int64_t Nq, int64_t Ng, int k,
                      const int* __restrict__ gallery_class, const int* __restrict__ query_class,
                      int64_t* __restrict__ out_idx, double* __restrict__ out_dist, int* __restrict__ out_hits,
                      int* __restrict__ out_top1) {
  __shared__ double vs[STAGED ? STAGE_ROWS : 1];
  __shared__ double wd[2][4];
  __shared__ int64_t wi[2][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t q = blockIdx.x, row = (int64_t)blockIdx.y * Nq + q;
  const double* drow = Dc + row * Ng;
  const double* brow = base ? base + q * Ng : nullptr;
  auto value = [&](int64_t g) -> double {
    if (STAGED) return vs[g];
    return brow ? brow[g] + drow[g] : drow[g];
  };
  if (STAGED) {
    for (int64_t g = tid; g < Ng; g += 256) vs[g] = brow ? brow[g] + drow[g] : drow[g];
    __syncthreads();
  }
  const double INF = __builtin_inf();
  double last_d = -INF;           // the pick of the previous round: this round takes the smallest (v, g) after it
  int64_t last_i = -1;
  int hits = 0;
  const int qc = (tid == 0 && out_hits) ? query_class[q] : 0;
  for (int r = 0; r < k; ++r) {
    double best = INF;
    int64_t bi = INT64_MAX;
    for (int64_t g = tid; g < Ng; g += 256) {      // ascending g: the first of equal values is the lowest index
      const double v = value(g);
      const bool after = v > last_d || (v == last_d && g > last_i);
      if (after && v < best) { best = v; bi = g; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double od = __shfl_down(best, off);
      const int64_t oi = __shfl_down(bi, off);
      if (od < best || (od == best && oi < bi)) { best = od; bi = oi; }
    }
    const int p = r & 1;          // two slots: a wave may enter round r + 1 while another still reads round r's
    if (lane == 0) {
      wd[p][wave] = best;
      wi[p][wave] = bi;
    }
    __syncthreads();
    best = wd[p][0];
    bi = wi[p][0];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      const double od = wd[p][w];
      const int64_t oi = wi[p][w];
      if (od < best || (od == best && oi < bi)) { best = od; bi = oi; }
    }
    last_d = best;                // k <= Ng: every round finds a row
    last_i = bi;
    if (tid == 0) {
      if (out_idx) out_idx[row * k + r] = bi < Ng ? bi : -1;
      if (out_dist) out_dist[row * k + r] = best;
      if (out_hits || (out_top1 && r == 0)) {
        // bi >= Ng: no finite value was left (the inputs were not finite): idx -1, no hit, top-1 class -1
        const int gc = bi < Ng ? gallery_class[bi] : -1;
        if (out_hits) hits += (bi < Ng && gc == qc) ? 1 : 0;
        if (out_top1 && r == 0) out_top1[row] = gc;
      }
    }
  }
  if (tid == 0 && out_hits) out_hits[row] = hits;
}

__global__ void __launch_bounds__(256)
chan_l2_accumulate_kernel(double* __restrict__ base, const double* __restrict__ one, int64_t n, int first) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) base[i] = first ? one[i] : base[i] + one[i];
}

}  // namespace csn

using namespace csn;

static bool strides_ok(const char* what, int64_t ld_n, int64_t ld_c, int C, int T) {
  if (ld_c < T) {
    fail(CSN_ERR_INVALID_ARGUMENT, "csn_chan_l2_dist: %s ld_c=%lld must be >= T=%d", what, (long long)ld_c, T);
    return false;
  }
  if (ld_n < (int64_t)(C - 1) * ld_c + T) {
    fail(CSN_ERR_INVALID_ARGUMENT, "csn_chan_l2_dist: %s ld_n=%lld must be >= (C-1)*ld_c+T=%lld", what, (long long)ld_n,
         (long long)((int64_t)(C - 1) * ld_c + T));
    return false;
  }
  return true;
}

extern "C" int csn_chan_l2_dist(const float* gallery, int64_t g_ld_n, int64_t g_ld_c, const float* query, int64_t q_ld_n,
                                int64_t q_ld_c, int64_t Ng, int64_t Nq, int C, int T, int t0, int t1,
                                const int32_t* channels, int nch, double* Dc, csnStream_t stream) {
  CSN_REQUIRE(gallery && query && Dc, "csn_chan_l2_dist: null pointer");
  CSN_REQUIRE(Ng > 0 && Nq > 0 && C > 0 && T > 0, "csn_chan_l2_dist: bad shape");
  CSN_REQUIRE(t0 >= 0 && t1 <= T && t0 < t1, "csn_chan_l2_dist: window [%d, %d) must be non-empty and inside [0, T=%d]", t0,
              t1, T);
  if (!strides_ok("gallery", g_ld_n, g_ld_c, C, T) || !strides_ok("query", q_ld_n, q_ld_c, C, T))
    return CSN_ERR_INVALID_ARGUMENT;
  if (channels) {
    CSN_REQUIRE(nch > 0, "csn_chan_l2_dist: nch=%d must be > 0 with a channel list", nch);
    for (int j = 0; j < nch; ++j)
      CSN_REQUIRE(channels[j] >= 0 && channels[j] < C, "csn_chan_l2_dist: channel %d (entry %d) outside [0, C=%d)",
                  (int)channels[j], j, C);
  } else {
    nch = C;
  }
  const int64_t qtiles = cdiv(Nq, TQ), gtiles = cdiv(Ng, TG);
  CSN_REQUIRE(qtiles <= 0x7fffffff && gtiles <= 65535, "csn_chan_l2_dist: Nq or Ng too large for one grid");
  hipStream_t st = as_stream(stream);
  for (int j0 = 0; j0 < nch; j0 += MAX_CH_PER_LAUNCH) {
    const int n = nch - j0 < MAX_CH_PER_LAUNCH ? nch - j0 : MAX_CH_PER_LAUNCH;
    ChannelList cl;
    for (int j = 0; j < MAX_CH_PER_LAUNCH; ++j) cl.ch[j] = j < n ? (channels ? channels[j0 + j] : j0 + j) : 0;
    chan_l2_dist_kernel<<<dim3((unsigned)qtiles, (unsigned)gtiles, (unsigned)n), 256, 0, st>>>(
        gallery, g_ld_n, g_ld_c, query, q_ld_n, q_ld_c, Ng, Nq, t0, t1 - t0, cl, (int64_t)j0, Dc);
    CSN_LAUNCH_CHECK();
  }
  return CSN_OK;
}

extern "C" int csn_chan_l2_select(const double* base, const double* Dc, int nc, int64_t Nq, int64_t Ng,
                                  const int32_t* gallery_class, const int32_t* query_class, int k, int64_t* out_idx,
                                  double* out_dist, int32_t* out_hits, int32_t* out_top1, csnStream_t stream) {
  CSN_REQUIRE(Dc, "csn_chan_l2_select: null pointer (Dc)");
  CSN_REQUIRE(out_idx || out_dist || out_hits || out_top1, "csn_chan_l2_select: every output is null");
  CSN_REQUIRE(gallery_class || !(out_hits || out_top1), "csn_chan_l2_select: null pointer (gallery_class)");
  CSN_REQUIRE(query_class || !out_hits, "csn_chan_l2_select: null pointer (query_class)");
  CSN_REQUIRE(nc > 0 && Nq > 0 && Ng > 0, "csn_chan_l2_select: bad shape");
  CSN_REQUIRE(k > 0 && k <= MAX_K && k <= Ng, "csn_chan_l2_select: k=%d must be in 1..min(64, Ng)", k);
  CSN_REQUIRE(Nq <= 0x7fffffff && nc <= 65535, "csn_chan_l2_select: Nq or nc too large for one grid");
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)Nq, (unsigned)nc);
  if (Ng <= STAGE_ROWS)
    chan_l2_select_kernel<true><<<grid, 256, 0, st>>>(base, Dc, Nq, Ng, k, gallery_class, query_class, out_idx, out_dist,
                                                      out_hits, out_top1);
  else
    chan_l2_select_kernel<false><<<grid, 256, 0, st>>>(base, Dc, Nq, Ng, k, gallery_class, query_class, out_idx, out_dist,
                                                       out_hits, out_top1);
  CSN_LAUNCH_CHECK();
  return CSN_OK;
}

extern "C" int csn_chan_l2_accumulate(double* base, const double* D_one, int64_t n, int first, csnStream_t stream) {
  CSN_REQUIRE(base && D_one, "csn_chan_l2_accumulate: null pointer");
  CSN_REQUIRE(n > 0, "csn_chan_l2_accumulate: n=%lld must be > 0", (long long)n);
  int64_t blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  chan_l2_accumulate_kernel<<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(base, D_one, n, first ? 1 : 0);
  CSN_LAUNCH_CHECK();
  return CSN_OK;
}
