// Top-m search (include/eigenface.h ef_search_topk): the m best gallery rows
// per probe in fp64 order, from the top-1 search's own pieces — the scan kernels' per-chunk
// top-2 records, reduce_kernel's error bound (scan_delta), the COLLECT pass and score64.
//
// Launches of one piece, all stream-ordered with their counts on the device:
//   1. the scan kernel of (k, metric, split), unchanged, under a plan of >= m chunks;
//   2. topk_threshold_kernel: a cut per probe that provably keeps the m best rows;
//   3. the COLLECT pass over every probe (rows whose scan score is within the cut);
//   4. topk_resolve_kernel: fp64 re-score, rank 0 by the tie rule, the rest sorted;
//   5. for probes whose list overflowed: a tighter cut from the rows they did collect, one
//      more COLLECT + resolve over those probes only, and topk_sweep_kernel (two fp64 passes
//      over the whole gallery) for a probe that overflows again.
// The merge of several engines' records (ef_matches_merge_topk) is at the end.
#include "ef_search_common.hpp"

#include <cfloat>
#include <cmath>
#include <cstring>

namespace ef {

// where a probe whose candidate list overflowed is queued (thr / cnt null: the sweep's queue)
struct TopkNext {
  int* list;
  float* thr;
  int* cnt;
  int* count;
};

// fp32 ||q||^2 as reduce_kernel sums it (the bound's ||q||)
__device__ __forceinline__ float probe_norm2_f32(const float* __restrict__ q, int kpv, int lane) {
  float qq = 0.f;
  for (int c = lane; c < kpv; c += 64) qq = __builtin_fmaf(q[c], q[c], qq);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) qq += __shfl_xor(qq, off);
  return qq;
}
// fp64 ||q||^2 as reduce_kernel / resolve_kernel sum it (the tie window's scale)
__device__ __forceinline__ double probe_norm2_f64(const float* __restrict__ q, int kpv, int lane) {
  double qq = 0.0;
  for (int c = lane; c < kpv; c += 64) qq = fma((double)q[c], (double)q[c], qq);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) qq += __shfl_xor(qq, off);
  return qq;
}
// cut = tau + delta, delta = scan_delta at tau; the largest finite float when there is no
// finite tau, so that the +inf of a masked tail row never qualifies
template <int METRIC>
__device__ __forceinline__ float topk_cut(float tau, int s3, int kpv, float qn, float gmax2) {
  if (!(tau < __builtin_inff())) return FLT_MAX;
  const float delta = s3 ? scan_delta<METRIC, 1>(kpv, qn, gmax2, tau) : scan_delta<METRIC, 0>(kpv, qn, gmax2, tau);
  return fminf(tau + delta, FLT_MAX);
}

// The cut of every probe, one wave per probe.  The main pass left, per chunk, the scan scores
// of two DISTINCT rows: key_value(part_key) (the chunk's best) and part_b2 (its runner-up).
// tau = the m-th smallest of these 2 nchunks values (+inf when fewer than m are finite).
//
// Proof that the cut keeps every row the result can name.  Let s(g) be the scan score of row
// g, S(g) its exact score in scan units, |s(g) - S(g)| <= e (scan_delta returns delta = 4 e),
// and S(m) the exact m-th smallest score.  The 2 nchunks values belong to distinct rows, so
// at least m rows have s <= tau: tau is an upper bound of the m-th smallest scan score, and
// one of those m rows has S >= S(m), hence tau >= S(m) - e.  A row the result can name has
// an exact score <= S(m) + tol (tol the fp64 tie window, far below e), so its scan score is
// <= S(m) + tol + e <= tau + 2 e + tol <= tau + delta.  The bound's 4u |b1| term is taken at
// tau; a qualifying row's own |s| is covered by the (k + 4) u (2 |q| gm + gmax2) term, which
// dominates u |s| for every score, and the rounding of tau + delta (half an ulp of it) by the
// 2 e of slack.  With fewer than m finite values every row qualifies.
// Queue: slot p = probe p, cand_cnt = 0, amb_count = b (the COLLECT pass's contract).
template <int METRIC>
__global__ __launch_bounds__(256) void topk_threshold_kernel(const float* __restrict__ qpad, int64_t b, int64_t bpad,
                                                             int nchunks, int kpv, int m, int s3, float gmax2,
                                                             SearchWs ws) {
  const int lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= b) return;
  const float INF = __builtin_inff();
  const int nv = 2 * nchunks;
  auto value = [&](int i) -> float {
    const int64_t at = (int64_t)(i >> 1) * bpad + p;
    if (i & 1) return ws.part_b2[at];
    const long long k = ws.part_key[at];
    return k == LLONG_MAX ? INF : key_value(k);
  };
  // m rounds of "the least (value, position) after the previous one"
  float pv = -INF, tau = INF;
  int pi = -1;
  for (int r = 0; r < m; ++r) {
    float bv = INF;
    int bi = INT_MAX;
    for (int i = lane; i < nv; i += 64) {
      const float v = value(i);
      const bool after = v > pv || (v == pv && i > pi);
      const bool better = v < bv || (v == bv && i < bi);
      if (after && better) { bv = v; bi = i; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(bv, off);
      const int oi = __shfl_xor(bi, off);
      if (ov < bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    tau = bv;
    if (bi == INT_MAX || !(bv < INF)) { tau = INF; break; }  // fewer than m finite values
    pv = bv;
    pi = bi;
  }
  const float qq = probe_norm2_f32(qpad + p * kpv, kpv, lane);
  const double qq64 = probe_norm2_f64(qpad + p * kpv, kpv, lane);
  const float cut = topk_cut<METRIC>(tau, s3, kpv, sqrtf(qq), gmax2);
  // A probe outside the bound's domain (scan_regular, ef_search_common.hpp) takes nothing from
  // the scan: its list starts past the cap and the NaN cut collects nothing, so both rounds pass
  // it on and topk_sweep_kernel re-scores every row.  A probe with a NaN or an infinite component
  // (fp64 ||q||^2 not finite) collects nothing into an empty list: m empty slots.
  const bool finite = qq64 < __builtin_inf();
  const bool regular = scan_regular<METRIC>(qq, gmax2);
  if (lane == 0) {
    ws.thr[p] = finite && regular ? cut : __builtin_nanf("");
    ws.amb_list[p] = (int)p;
    ws.cand_cnt[p] = finite && !regular ? ws.cand_cap + 1 : 0;
    if (p == 0) *ws.amb_count = (int)b;
  }
}

// (v, row) lexicographic order
__device__ __forceinline__ bool pair_less(double av, int ar, double bv, int br) {
  return av < bv || (av == bv && ar < br);
}
// ascending bitonic sort of (sv, sr)[0, P) by (v, row), P a power of two, all threads of the
// workgroup; the caller has synchronised after filling the arrays
__device__ __forceinline__ void bitonic_sort_pairs(double* sv, int* sr, int P) {
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < P; i += blockDim.x) {
        const int l = i ^ j;
        if (l > i) {
          const double av = sv[i], bv = sv[l];
          const int ar = sr[i], br = sr[l];
          const bool up = (i & k) == 0;
          if (pair_less(bv, br, av, ar) == up) {
            sv[i] = bv; sr[i] = br;
            sv[l] = av; sr[l] = ar;
          }
        }
      }
      __syncthreads();
    }
  }
}
// The m slots of probe p from the sorted list (sv, sr)[0, nvalid): rank 0 = (v0, r0), the
// rest in list order without r0's entry (z = its position, INT_MAX when it is not listed).
__device__ __forceinline__ void topk_emit(const double* sv, const int* sr, int nvalid, double v0, int r0, int z, int m,
                                          double scale, int64_t g_offset, long long* __restrict__ keys,
                                          ef_match* __restrict__ match, int64_t p) {
  for (int j = threadIdx.x; j < m; j += blockDim.x) {
    const int at = j == 0 ? -1 : (j - 1 < z ? j - 1 : j);
    long long key = LLONG_MAX;
    ef_match rec = ef_match{__builtin_inf(), 0.0, LLONG_MAX};
    if (nvalid > 0 && at < nvalid) {
      const double v = j == 0 ? v0 : sv[at];
      const int row = j == 0 ? r0 : sr[at];
      key = pack_key((float)v, (unsigned)(row + g_offset));
      rec = ef_match{v, scale, key};
    }
    keys[p * m + j] = key;
    if (match) match[p * m + j] = rec;
  }
}

constexpr int kTopkCapMax = 4096;  // EF_OPT_SEARCH_TOPK_CAND's upper end: the resolve's LDS list

// fp64 resolution of one queued probe per workgroup.  Its cnt <= cap candidates are re-scored
// with score64 into LDS as (v, row) and sorted; rank 0 is the lowest row among those within
// the tie window of the minimum (resolve_kernel's rule, so rank 0 is ef_search's answer), the
// other ranks follow in (v, row) order.  cnt > cap: the list is incomplete, so the probe is
// not resolved; the m-th smallest fp64 score of the cap rows it did collect, taken back to
// scan units (L2: - ||q||^2; cosine: * ||q||) and rounded up to fp32, is a valid tau — any m
// distinct rows bound the m-th best from above — and the probe is queued in nx with it.
template <int METRIC>
__global__ __launch_bounds__(256) void topk_resolve_kernel(
    const float* __restrict__ qpad, const float* __restrict__ G, int64_t n, int64_t g_offset, float gmax2, int kpv,
    int m, int s3, const int* __restrict__ count, const int* __restrict__ list, const int* __restrict__ cnt_of,
    const int* __restrict__ cand, int cap, TopkNext nx, unsigned long long* __restrict__ counters, int first_round,
    long long* __restrict__ keys, ef_match* __restrict__ match) {
  __shared__ double sv[kTopkCapMax];
  __shared__ int sr[kTopkCapMax];
  __shared__ int s_r0, s_z;
  const int slot = blockIdx.x;
  if (slot >= *count) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t p = list[slot];
  const float* q = qpad + p * kpv;
  const int cnt = cnt_of[slot];
  const bool overflow = cnt > cap;
  const float qq32 = probe_norm2_f32(q, kpv, lane);
  const bool regular = scan_regular<METRIC>(qq32, gmax2);
  const int nc = overflow ? (regular ? cap : 0) : cnt;  // not regular: nothing was collected
  int P = 64;
  while (P < nc) P <<= 1;
  for (int j = wave; j < P; j += 4) {
    int row = INT_MAX;
    double v = INFINITY;
    if (j < nc) {
      row = cand[(int64_t)slot * cap + j];
      if (row >= 0 && row < n) v = score64<0, METRIC>(q, G + (int64_t)row * kpv, lane, kpv);
      else row = INT_MAX;
    }
    if (lane == 0) { sv[j] = v; sr[j] = row; }
  }
  if (threadIdx.x == 0) { s_r0 = INT_MAX; s_z = INT_MAX; }
  const double qq64 = probe_norm2_f64(q, kpv, lane);
  __syncthreads();
  bitonic_sort_pairs(sv, sr, P);
  if (overflow) {
    const float qn = sqrtf(qq32);
    if (threadIdx.x == 0) {
      const double t2 = sv[m - 1];  // cap >= m rows were scored
      const float tau = __double2float_ru(METRIC == EF_METRIC_L2 ? t2 - qq64 : t2 * sqrt(qq64));
      const int at = atomicAdd(nx.count, 1);
      nx.list[at] = (int)p;
      // not regular: past the cap again with a NaN cut, on to the sweep (topk_threshold_kernel)
      if (nx.thr) nx.thr[at] = regular ? topk_cut<METRIC>(tau, s3, kpv, qn, gmax2) : __builtin_nanf("");
      if (nx.cnt) nx.cnt[at] = regular ? 0 : cap + 1;
      if (first_round) atomicAdd(&counters[1], 1ull);
      atomicAdd(&counters[3], (unsigned long long)nc);
    }
    return;
  }
  const double vmin = sv[0];
  const double scale = METRIC == EF_METRIC_L2 ? qq64 + (double)fabsf(gmax2) : 1.0;  // negated: scan_regular
  const double tol = 1e-12 * (fabs(vmin) + scale);
  for (int i = threadIdx.x; i < nc; i += blockDim.x)
    if (sv[i] <= vmin + tol) atomicMin(&s_r0, sr[i]);
  __syncthreads();
  const int r0 = s_r0;
  for (int i = threadIdx.x; i < nc; i += blockDim.x)
    if (sr[i] == r0) s_z = i;
  __syncthreads();
  const int z = s_z;
  topk_emit(sv, sr, z == INT_MAX ? 0 : nc, z == INT_MAX ? 0.0 : sv[z], r0, z, m, scale, g_offset, keys, match, p);
  if (threadIdx.x == 0) atomicAdd(&counters[3], (unsigned long long)nc);
}

// The cold path: a probe whose second list overflowed too (e.g. thousands of equal rows).
// One workgroup per such probe, two fp64 passes over all n rows: the first finds vmin, the
// second the rank-0 row (lowest row within the tie window) and the 64 smallest (v, row) of
// each wave's rows, kept sorted across the wave's lanes (lane j = its j-th smallest); the
// four lists are sorted together.  Exact, not fast.
template <int METRIC>
__global__ __launch_bounds__(256) void topk_sweep_kernel(const float* __restrict__ qpad, const float* __restrict__ G,
                                                         int64_t n, int64_t g_offset, float gmax2, int kpv, int m,
                                                         const int* __restrict__ count, const int* __restrict__ list,
                                                         unsigned long long* __restrict__ counters,
                                                         long long* __restrict__ keys, ef_match* __restrict__ match) {
  __shared__ double sv[256];
  __shared__ int sr[256];
  __shared__ double w_v[4];
  __shared__ int w_r[4];
  __shared__ int s_z, s_nv;
  const int slot = blockIdx.x;
  if (slot >= *count) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t p = list[slot];
  const float* q = qpad + p * kpv;
  // a row with a NaN or an infinite component scores NaN or +inf: it is passed over
  double vm = INFINITY;
  for (int64_t row = wave; row < n; row += 4) {
    const double v = score64<0, METRIC>(q, G + row * kpv, lane, kpv);
    vm = v < vm ? v : vm;
  }
  if (lane == 0) w_v[wave] = vm;
  if (threadIdx.x == 0) { s_z = INT_MAX; s_nv = 0; }
  const double qq64 = probe_norm2_f64(q, kpv, lane);
  __syncthreads();
  const double vmin = fmin(fmin(w_v[0], w_v[1]), fmin(w_v[2], w_v[3]));
  const double scale = METRIC == EF_METRIC_L2 ? qq64 + (double)fabsf(gmax2) : 1.0;  // negated: scan_regular
  const double tol = 1e-12 * (fabs(vmin) + scale);
  __syncthreads();  // w_v is rewritten below
  double ev = INFINITY, v0 = INFINITY;  // this lane's entry of the wave's sorted list
  int er = INT_MAX, r0 = INT_MAX;
  for (int64_t row = wave; row < n; row += 4) {
    const double v = __shfl(score64<0, METRIC>(q, G + row * kpv, lane, kpv), 0);
    const int r = (int)row;
    const bool have = v < INFINITY;  // wave-uniform
    if (have && v <= vmin + tol && r < r0) { r0 = r; v0 = v; }
    // insert (v, r): entries below it stay, the first one not below takes it, the rest shift
    const double uv = __shfl_up(ev, 1);
    const int ur = __shfl_up(er, 1);
    if (have && !pair_less(ev, er, v, r)) {
      const bool first = lane == 0 || pair_less(uv, ur, v, r);
      ev = first ? v : uv;
      er = first ? r : ur;
    }
  }
  sv[threadIdx.x] = ev;
  sr[threadIdx.x] = er;
  if (lane == 0) { w_v[wave] = v0; w_r[wave] = r0; }
  __syncthreads();
  bitonic_sort_pairs(sv, sr, 256);
  r0 = INT_MAX;
  v0 = INFINITY;
  for (int w = 0; w < 4; ++w)
    if (w_r[w] < r0) { r0 = w_r[w]; v0 = w_v[w]; }
  if (sr[threadIdx.x] == r0) s_z = threadIdx.x;
  if (sr[threadIdx.x] != INT_MAX) atomicAdd(&s_nv, 1);  // the list's entries, sorted ahead of the empty ones
  __syncthreads();
  const int nvalid = s_nv;
  topk_emit(sv, sr, r0 == INT_MAX ? 0 : nvalid, v0, r0, s_z, m, scale, g_offset, keys, match, p);
  if (threadIdx.x == 0) {
    atomicAdd(&counters[2], 1ull);
    atomicAdd(&counters[3], (unsigned long long)n);
  }
}

template <int M>
static hipError_t topk_t(hipStream_t s, int kp, const SplitScan& sp, int m, const SearchPlan& pl, const float* qpad,
                         int64_t bpad, int64_t b, const float* G, const float* aux, int64_t n, int64_t g_offset,
                         float gmax2, const SearchWs& ws, const TopkWs& tw, int cap, unsigned long long* counters,
                         long long* keys, ef_match* match) {
  const int split = sp.variant, s3 = split ? 1 : 0;
  const float* Gs = split ? sp.G3 : G;
  const float* qs = nullptr;
  hipError_t e;
  if ((e = launch_scan_probes(s, sp, qpad, bpad, kp, &qs)) != hipSuccess) return e;
  SearchWs w1 = ws;
  w1.cand = tw.cand;
  w1.cand_cap = cap;
  w1.match = nullptr;
  if ((e = launch_search_scan(s, kp, M, false, split, false, pl, qs, Gs, aux, n, bpad, w1)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(tw.counts, 0, 4 * sizeof(int), s)) != hipSuccess) return e;
  const dim3 block(256), per_probe((unsigned)b);
  hipLaunchKernelGGL((topk_threshold_kernel<M>), dim3((unsigned)((b + 3) / 4)), block, 0, s, qpad, b, bpad, pl.nchunks,
                     kp, m, s3, gmax2, w1);
  if ((e = launch_search_scan(s, kp, M, true, split, false, pl, qs, Gs, aux, n, bpad, w1)) != hipSuccess) return e;
  hipLaunchKernelGGL((topk_resolve_kernel<M>), per_probe, block, 0, s, qpad, G, n, g_offset, gmax2, kp, m, s3,
                     w1.amb_count, w1.amb_list, w1.cand_cnt, tw.cand, cap,
                     TopkNext{tw.list2, tw.thr2, tw.cnt2, tw.counts}, counters, 1, keys, match);
  // second round over the probes queued by the first; it reuses the candidate array
  SearchWs w2 = w1;
  w2.amb_count = tw.counts;
  w2.amb_list = tw.list2;
  w2.thr = tw.thr2;
  w2.cand_cnt = tw.cnt2;
  if ((e = launch_search_scan(s, kp, M, true, split, false, pl, qs, Gs, aux, n, bpad, w2)) != hipSuccess) return e;
  hipLaunchKernelGGL((topk_resolve_kernel<M>), per_probe, block, 0, s, qpad, G, n, g_offset, gmax2, kp, m, s3,
                     tw.counts, tw.list2, tw.cnt2, tw.cand, cap, TopkNext{tw.list3, nullptr, nullptr, tw.counts + 1},
                     counters, 0, keys, match);
  hipLaunchKernelGGL((topk_sweep_kernel<M>), per_probe, block, 0, s, qpad, G, n, g_offset, gmax2, kp, m,
                     tw.counts + 1, tw.list3, counters, keys, match);
  return hipGetLastError();
}

hipError_t launch_search_topk(hipStream_t s, int kp, int metric, const SplitScan& sp, int m, const SearchPlan& pl,
                              const float* qpad, int64_t bpad, int64_t b, const float* G, const float* aux,
                              int64_t n, int64_t g_offset, float gmax2, const SearchWs& ws, const TopkWs& tw, int cap,
                              unsigned long long* counters, long long* keys, ef_match* match) {
  if (m < 1 || m > 64 || cap < m || cap > kTopkCapMax || b < 1 || n < 1 || n > INT_MAX || sp.variant == 3 ||
      (sp.variant && !sp.G3))
    return hipErrorInvalidValue;
  return metric == EF_METRIC_L2
             ? topk_t<EF_METRIC_L2>(s, kp, sp, m, pl, qpad, bpad, b, G, aux, n, g_offset, gmax2, ws, tw, cap, counters,
                                    keys, match)
             : topk_t<EF_METRIC_COSINE>(s, kp, sp, m, pl, qpad, bpad, b, G, aux, n, g_offset, gmax2, ws, tw, cap,
                                        counters, keys, match);
}

// ------------------------------------------------------------------------------- merge
// Top-m merge of one probe's nparts x m records (parts[r][p][j]): the rule of the single
// engine applied to the records.  Rank 0 = the lowest global index among the records within
// 1e-12 (|min| + max scale) of the minimum (merge_one's rule, ef_comm.hip); the others follow
// in (score, global index) order; EF_KEY_NONE records are skipped and missing ranks padded.
// Selection by rounds (the least record after the previous one) needs no storage, so the
// host and one device thread per probe run the same code; a row present in two parts is
// taken once.
__host__ __device__ inline long long merge_topk_key(double score, long long idx) {
  float v = (float)score;
  if (v == 0.0f) v = 0.0f;  // canonical +0 (ef_search_common.hpp pack_key)
  int bits;
  memcpy(&bits, &v, sizeof bits);
  const int s = bits >= 0 ? bits : (bits ^ 0x7FFFFFFF);
  return (long long)(((unsigned long long)(unsigned)s << 32) | (unsigned long long)(unsigned)idx);
}

__host__ __device__ inline void merge_topk_one(const ef_match* parts, int nparts, int64_t b, int m, int64_t p,
                                               long long* keys, ef_match* merged) {
  const ef_match none = ef_match{INFINITY, 0.0, LLONG_MAX};
  auto rec = [&](int r, int j) -> const ef_match& { return parts[((int64_t)r * b + p) * m + j]; };
  double vmin = INFINITY, sc = 0.0;
  bool any = false;
  for (int r = 0; r < nparts; ++r)
    for (int j = 0; j < m; ++j) {
      const ef_match& t = rec(r, j);
      if (t.key == LLONG_MAX) continue;
      any = true;
      vmin = t.score < vmin ? t.score : vmin;
      sc = t.scale > sc ? t.scale : sc;
    }
  int filled = 0;
  if (any) {
    const double tol = 1e-12 * (fabs(vmin) + sc);
    long long i0 = LLONG_MAX;
    double v0 = vmin;
    for (int r = 0; r < nparts; ++r)
      for (int j = 0; j < m; ++j) {
        const ef_match& t = rec(r, j);
        if (t.key == LLONG_MAX || !(t.score <= vmin + tol)) continue;
        const long long idx = t.key & 0xffffffffll;
        if (idx < i0) i0 = idx, v0 = t.score;
      }
    keys[0] = merge_topk_key(v0, i0);
    if (merged) merged[0] = ef_match{v0, sc, keys[0]};
    filled = 1;
    double pv = -INFINITY;
    long long pi = -1;
    for (; filled < m; ++filled) {
      double bv = INFINITY;
      long long bi = LLONG_MAX;
      for (int r = 0; r < nparts; ++r)
        for (int j = 0; j < m; ++j) {
          const ef_match& t = rec(r, j);
          if (t.key == LLONG_MAX || t.score != t.score) continue;
          const long long idx = t.key & 0xffffffffll;
          if (idx == i0) continue;
          const bool after = t.score > pv || (t.score == pv && idx > pi);
          const bool better = t.score < bv || (t.score == bv && idx < bi);
          if (after && better) bv = t.score, bi = idx;
        }
      if (bi == LLONG_MAX) break;
      keys[filled] = merge_topk_key(bv, bi);
      if (merged) merged[filled] = ef_match{bv, sc, keys[filled]};
      pv = bv;
      pi = bi;
    }
  }
  for (; filled < m; ++filled) {
    keys[filled] = LLONG_MAX;
    if (merged) merged[filled] = none;
  }
}

__global__ void matches_merge_topk_kernel(const ef_match* __restrict__ parts, int nparts, int64_t b, int m,
                                          long long* __restrict__ keys, ef_match* __restrict__ merged) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= b) return;
  merge_topk_one(parts, nparts, b, m, p, keys + p * m, merged ? merged + p * m : nullptr);
}

hipError_t launch_matches_merge_topk(hipStream_t s, const ef_match* parts, int nparts, int64_t b, int m,
                                     long long* keys, ef_match* merged) {
  if (b <= 0) return hipSuccess;
  hipLaunchKernelGGL(matches_merge_topk_kernel, dim3((unsigned)((b + 63) / 64)), dim3(64), 0, s, parts, nparts, b, m,
                     keys, merged);
  return hipGetLastError();
}

}  // namespace ef

using namespace ef;

extern "C" int ef_matches_merge_topk(ef_ctx* c, const ef_match* parts, int32_t nparts, int64_t b, int32_t m,
                                     int64_t* keys_out, ef_match* merged_out, uint32_t flags) {
  if (!parts || !keys_out || nparts < 1 || b < 0 || m < 1 || m > 64)
    return c ? set_err(c, EF_E_INVALID, "ef_matches_merge_topk: bad arguments (1 <= m <= 64)") : EF_E_INVALID;
  if (flags & EF_MEM_DEVICE) {
    if (!c) return EF_E_INVALID;
    (void)hipSetDevice(c->device);
    const hipError_t e = launch_matches_merge_topk(c->stream, parts, nparts, b, m,
                                                   reinterpret_cast<long long*>(keys_out), merged_out);
    return e == hipSuccess ? EF_OK : hip_err(c, e, "top-m matches merge");
  }
  for (int64_t p = 0; p < b; ++p)
    merge_topk_one(parts, nparts, b, m, p, reinterpret_cast<long long*>(keys_out) + p * m,
                   merged_out ? merged_out + p * m : nullptr);
  return EF_OK;
}
