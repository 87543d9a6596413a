// Range search (ef_search_range): for each probe, every resident gallery row
// within a threshold, as a CSR list (lims, rows, scores) in ascending row order.
//   * range_kernel (ef_range_tile.hpp, shared with ef_rank.hip) is census_kernel's distance GEMM (ef_census.hip: 128 rows x 128 probes per
//     tile, 16-k slices of both operands double-buffered in LDS by global_load_lds, XOR-swizzled
//     slice rows, four independent fp32 accumulator chains per wave) over the census's work items
//     (gallery chunk, probe tile), with cluster_kernel's epilogue (ef_cluster.hip): a pair is a
//     hit when its fp32 score s^ is on the accepting side of t, decided by s^ alone when
//     |s^ - t| > delta; the lanes inside the band are balloted and the whole wave settles them
//     one after another on score64.  delta is per probe (range_delta): a lane owns its probe.
//   * COUNT: each lane adds its hits in a register; at the end of the item the two lane halves
//     of a probe are added and half 0 stores cnt[chunk][probe] (a plain store, no atomics).
//   * range_tot_kernel turns a probe's counts into their exclusive prefix over the chunks (chunk
//     order is row order) and the probe's total; range_scan_kernel / range_lims_kernel are the
//     two-level exclusive scan of the totals: lims.
//   * FILL recomputes the same masks (same instructions, same fp64 settlements) and writes each
//     hit at lims[p] + prefix of its chunk + hits of the item's earlier tiles + its rank inside the
//     tile.  A lane of half h holds rows 32 rb + 8 q + 4 h + jj of a tile, so a probe's rows
//     alternate between lane c32 and lane c32 + 32 in groups of four: the rank is a popcount of
//     the lane's own mask below the bit plus one of the partner's mask below the nibble.  A
//     probe's segment is written only when it fits whole (lims[p + 1] <= cap).
// Every position is a function of exactly decided masks and every count an integer: the output
// does not depend on the order in which anything arrives.
#include "ef_range_tile.hpp"

namespace ef {

// ---- offsets -----------------------------------------------------------------------------
// cnt[c][p] <- hits of probe p in the chunks before c; tot[p] <- its hits; bsum[block] <- the
// block's hits
__global__ __launch_bounds__(256) void range_tot_kernel(int* __restrict__ cnt, int64_t n_chunks, int64_t stride,
                                                        int* __restrict__ tot, long long* __restrict__ bsum) {
  __shared__ long long wsum[4];
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;  // < stride: a multiple of 256
  int run = 0;
  for (int64_t c = 0; c < n_chunks; ++c) {
    const int v = cnt[c * stride + p];
    cnt[c * stride + p] = run;
    run += v;
  }
  tot[p] = run;
  long long s = run;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) bsum[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// second level: one workgroup turns the block sums into their exclusive scan, 256 at a time with
// the running total carried from round to round (cluster_scan_kernel's form); then info
__global__ __launch_bounds__(256) void range_scan_kernel(long long* __restrict__ bsum, int nblocks,
                                                         const unsigned long long* __restrict__ counters,
                                                         long long* __restrict__ info) {
  __shared__ long long s[256];
  __shared__ long long carry;
  const int tx = threadIdx.x;
  if (tx == 0) carry = 0;
  __syncthreads();
  for (int b0 = 0; b0 < nblocks; b0 += 256) {
    const long long v = b0 + tx < nblocks ? bsum[b0 + tx] : 0;
    s[tx] = v;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
      const long long add = tx >= d ? s[tx - d] : 0;
      __syncthreads();
      s[tx] += add;
      __syncthreads();
    }
    const long long base = carry;
    if (b0 + tx < nblocks) bsum[b0 + tx] = base + s[tx] - v;
    __syncthreads();
    if (tx == 255) carry = base + s[255];
    __syncthreads();
  }
  if (tx == 0) {
    info[0] = carry;
    info[1] = (long long)counters[kRcResolved];
    info[2] = 0;  // range_lims_kernel: the hits of the segments that do not fit
    info[3] = 0;
  }
}

// lims[p] = hits of the probes before p; lims[b] the total.  The segments that fit (lims[p + 1]
// <= cap) are a prefix of the probes: the one probe whose segment straddles cap reports the rest.
__global__ __launch_bounds__(256) void range_lims_kernel(const int* __restrict__ tot, const long long* __restrict__ bsum,
                                                         int64_t b, long long cap, long long* __restrict__ lims,
                                                         long long* __restrict__ info) {
  __shared__ long long s[256];
  const int tx = threadIdx.x;
  const int64_t p = (int64_t)blockIdx.x * 256 + tx;
  const long long v = p < b ? tot[p] : 0;
  s[tx] = v;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const long long add = tx >= d ? s[tx - d] : 0;
    __syncthreads();
    s[tx] += add;
    __syncthreads();
  }
  const long long hi = bsum[blockIdx.x] + s[tx], lo = hi - v;
  if (p < b) {
    lims[p] = lo;
    if (p == b - 1) lims[b] = hi;
    if (lo <= cap && hi > cap) info[2] = info[0] - lo;
  }
}

template <int METRIC, bool FILL>
static hipError_t launch_range_pass(hipStream_t s, const RangeArgs& a, int64_t n_chunks) {
  const dim3 grid((unsigned)(n_chunks * a.n_ptiles)), block(256);
  hipLaunchKernelGGL((range_kernel<METRIC, FILL>), grid, block, 0, s, a);
  return hipGetLastError();
}
template <bool FILL>
static hipError_t launch_range(hipStream_t s, int metric, const RangeArgs& a, int64_t n_chunks) {
  if (metric == EF_METRIC_L2) return launch_range_pass<EF_METRIC_L2, FILL>(s, a, n_chunks);
  return launch_range_pass<EF_METRIC_COSINE, FILL>(s, a, n_chunks);
}

}  // namespace ef

using namespace ef;

extern "C" int ef_search_range_plan(int64_t b, int64_t n, int32_t kp, int64_t* n_chunks, int64_t* tiles_per_item) {
  if (b < 0 || n < 0 || n > INT_MAX - RR || kp < RBK || kp % RBK != 0 || !n_chunks || !tiles_per_item)
    return EF_E_INVALID;
  range_plan(round_up(b, kSearchProbeTile), n, *n_chunks, *tiles_per_item);
  return EF_OK;
}

extern "C" int ef_search_range(ef_ctx* c, const float* Q, int64_t b, int32_t metric, double threshold,
                               const int64_t* exclude_rows, int64_t* lims, int64_t* rows, float* scores, int64_t cap,
                               int64_t* info, uint32_t flags) {
  if (!c) return EF_E_INVALID;
  if (c->gal.k == 0) return set_err(c, EF_E_STATE, "ef_search_range: no gallery (call ef_gallery_set)");
  if (!lims || !info || b < 0 || (b > 0 && !Q) || (metric != EF_METRIC_L2 && metric != EF_METRIC_COSINE) ||
      threshold != threshold || cap < 0 || (rows && !scores))
    return set_err(c, EF_E_INVALID, "ef_search_range: bad arguments (lims and info required, metric L2 or cosine, "
                                    "threshold not NaN, cap >= 0, scores with rows)");
  if (c->comm && c->comm_size > 1)
    return set_err(c, EF_E_STATE, "ef_search_range: no range search over a communicator; search each shard on a "
                                  "context without one and concatenate the segments");
  const Gallery& g = c->gal;
  if (g.n > INT_MAX - RR) return set_err(c, EF_E_INVALID, "ef_search_range: more than 2^31 - 129 rows");
  EF_HIP(c, hipSetDevice(c->device), "hipSetDevice");
  hipStream_t s = c->stream;
  const bool dev = (flags & EF_MEM_DEVICE) != 0;
  if (b == 0 || g.n == 0) {
    const size_t lb = (size_t)(b + 1) * sizeof(int64_t);
    if (dev) {
      EF_HIP(c, hipMemsetAsync(lims, 0, lb, s), "zero lims");
      EF_HIP(c, hipMemsetAsync(info, 0, 4 * sizeof(int64_t), s), "zero info");
    } else {
      std::memset(lims, 0, lb);
      std::memset(info, 0, 4 * sizeof(int64_t));
    }
    return EF_OK;
  }
  const bool fill = rows && cap > 0;
  const long long capv = fill ? cap : 0;  // the count-only form writes no segment
  const int64_t bpad = round_up(b, kSearchProbeTile);
  int64_t n_chunks, tpc;
  range_plan(bpad, g.n, n_chunks, tpc);
  const int nblocks = (int)(bpad / 256);
  if (bpad / 256 > INT_MAX || n_chunks * (bpad / RP) >= ((int64_t)1 << 31))
    return set_err(c, EF_E_INVALID, "ef_search_range: too many probes for one call");

  const auto carve = [&](Carve& cv, int*& plab, int*& pexcl, float*& qaux, int*& cnt, int*& tot, long long*& bsum,
                         unsigned long long*& counters, int64_t*& excl_st, long long*& lims_st, long long*& info_st,
                         long long*& rows_st, float*& scores_st) {
    plab = cv.take<int>((size_t)bpad);
    pexcl = cv.take<int>((size_t)bpad);
    qaux = cv.take<float>((size_t)bpad);
    cnt = cv.take<int>((size_t)(n_chunks * bpad));
    tot = cv.take<int>((size_t)bpad);
    bsum = cv.take<long long>((size_t)nblocks);
    counters = cv.take<unsigned long long>(kRcCount);
    excl_st = (!dev && exclude_rows) ? cv.take<int64_t>((size_t)b) : nullptr;
    lims_st = dev ? nullptr : cv.take<long long>((size_t)b + 1);
    info_st = dev ? nullptr : cv.take<long long>(4);
    rows_st = (dev || !fill) ? nullptr : cv.take<long long>((size_t)cap);
    scores_st = (dev || !fill) ? nullptr : cv.take<float>((size_t)cap);
  };
  int *plab, *pexcl, *cnt, *tot;
  float *qaux, *scores_st;
  long long *bsum, *lims_st, *info_st, *rows_st;
  unsigned long long* counters;
  int64_t* excl_st;
  Carve size, cv;
  carve(size, plab, pexcl, qaux, cnt, tot, bsum, counters, excl_st, lims_st, info_st, rows_st, scores_st);
  EF_TRY(ensure(c, c->range_ws, size.total));
  cv.base = c->range_ws.p;
  carve(cv, plab, pexcl, qaux, cnt, tot, bsum, counters, excl_st, lims_st, info_st, rows_st, scores_st);

  TimerEvt tm;
  timer_begin(c, EF_KERNEL_RANGE, &tm);
  EF_TRY(stage_queries(c, Q, b, dev, bpad));
  if (excl_st) {
    EF_HIP(c, hipMemcpyAsync(excl_st, exclude_rows, (size_t)b * sizeof(int64_t), hipMemcpyHostToDevice, s),
           "H2D excluded rows");
    exclude_rows = excl_st;
  }
  EF_HIP(c, hipMemsetAsync(counters, 0, kRcCount * sizeof(unsigned long long), s), "zero counters");
  EF_HIP(c, launch_label_prep(s, nullptr, exclude_rows, b, bpad, c->g_offset, g.n, plab, pexcl), "label prep");
  const float* qpad = static_cast<const float*>(c->q_pad.p);
  EF_HIP(c, launch_census_probe_aux(s, qpad, bpad, g.kp, metric, qaux), "range probe norms");

  long long* const lims_d = dev ? reinterpret_cast<long long*>(lims) : lims_st;
  long long* const info_d = dev ? reinterpret_cast<long long*>(info) : info_st;
  const bool outside = metric != EF_METRIC_L2 && (c->gal_rows_host & (kRowNotFinite | kRowTiny));
  RangeArgs a{};
  a.G = static_cast<const float*>(g.G.p);
  a.aux = static_cast<const float*>(metric == EF_METRIC_L2 ? g.gnorm2.p : g.ginv.p);
  a.n = g.n;
  a.kp = g.kp;
  a.tpc = (int)tpc;
  a.stride = bpad;
  a.t = (float)threshold;
  a.t64 = threshold;
  // an infinite threshold is itself in fp32; a finite one that overflows fp32 has an infinite error
  a.terr = (double)(float)threshold == threshold ? 0.0 : std::fabs((double)(float)threshold - threshold);
  a.gmax2 = outside ? -c->gmax2_host : c->gmax2_host;
  a.counters = counters;
  a.rows = dev ? reinterpret_cast<long long*>(rows) : rows_st;
  a.scores = dev ? scores : scores_st;
  a.cap = capv;
  a.g_offset = c->g_offset;
  const std::vector<SearchPiece> pieces = search_pieces(b, g.kp);  // a padded probe block stays below 2 GiB
  const auto pass = [&](bool do_fill) -> hipError_t {
    for (const SearchPiece& p : pieces) {
      a.qpad = qpad + p.off * g.kp;
      a.qaux = qaux + p.off;
      a.pexcl = pexcl + p.off;
      a.b = p.b;
      a.n_ptiles = (int)(p.bpad / RP);
      a.cnt = cnt + p.off;
      a.lims = lims_d + p.off;
      const hipError_t e = do_fill ? launch_range<true>(s, metric, a, n_chunks) : launch_range<false>(s, metric, a, n_chunks);
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  };
  EF_HIP(c, pass(false), "range count pass");
  hipLaunchKernelGGL(range_tot_kernel, dim3((unsigned)nblocks), dim3(256), 0, s, cnt, n_chunks, bpad, tot, bsum);
  hipLaunchKernelGGL(range_scan_kernel, dim3(1), dim3(256), 0, s, bsum, nblocks, counters, info_d);
  hipLaunchKernelGGL(range_lims_kernel, dim3((unsigned)nblocks), dim3(256), 0, s, tot, bsum, b, capv, lims_d, info_d);
  EF_HIP(c, hipGetLastError(), "range offset kernels");
  if (fill) EF_HIP(c, pass(true), "range fill pass");
  timer_end(c, &tm);
  if (dev) return EF_OK;

  EF_HIP(c, hipMemcpyAsync(lims, lims_st, (size_t)(b + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, s), "D2H lims");
  EF_HIP(c, hipMemcpyAsync(info, info_st, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, s), "D2H info");
  EF_HIP(c, hipStreamSynchronize(s), "sync");
  const int64_t written = fill ? info[0] - info[2] : 0;  // the segments that fit: a prefix of rows / scores
  if (written > 0) {
    EF_HIP(c, hipMemcpyAsync(rows, rows_st, (size_t)written * sizeof(int64_t), hipMemcpyDeviceToHost, s), "D2H rows");
    EF_HIP(c, hipMemcpyAsync(scores, scores_st, (size_t)written * sizeof(float), hipMemcpyDeviceToHost, s),
           "D2H scores");
    EF_HIP(c, hipStreamSynchronize(s), "sync");
  }
  return EF_OK;
}
