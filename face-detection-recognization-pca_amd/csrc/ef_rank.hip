// Identification rank (ef_search_rank): for each probe, the number of OTHER
// identities that have a resident row beating the probe's genuine row; the rank of the probe's
// identity is that number plus one.  No b x n array is written: the state is one bit per
// (probe, identity).
//   * the genuine rows come from the labelled SAME scan (ef_search_labelled, as it is), or from
//     the caller (EF_RANK_GENUINE_GIVEN: records merged over shards);
//   * rank_tau_kernel, one wave per probe, recomputes tau = score64 of (probe, genuine row) from
//     the stored features, so that bit-identical rows tie exactly, and forms the scan's fp32
//     threshold, its rounding error and the probe's dense class;
//   * range_kernel<METRIC, kRangeRank> (ef_range_tile.hpp) is the range search's COUNT pass over
//     range_plan's work items with the threshold per lane: a pair is a hit when it beats the
//     genuine row, decided by the fp32 score alone outside the probe's band and by the whole wave
//     on score64 inside it (lower score, or the same score at a lower global row).  A hit of
//     another class ORs that class's bit into bits[probe][class / 32];
//   * rank_count_kernel, one wave per probe, popcounts the bitmap row.
// The probes run in pieces of whole 256-probe blocks so that the bitmap stays inside a budget
// (EF_OPT_RANK_BITMAP_BYTES).  OR and popcount are order-free: the output is byte-identical on
// every run.  The dense class map (row label -> 0 .. C - 1) is built on the host by the first
// call after ef_gallery_labels and cached with the labels.
#include "ef_range_tile.hpp"

#include <vector>

namespace ef {

// uniq[C] ascending: the index of label v, or -1
__device__ __forceinline__ int rank_class_of(const int* __restrict__ uniq, int C, int v) {
  int lo = 0, hi = C;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (uniq[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return (lo < C && uniq[lo] == v) ? lo : -1;
}

struct RankTauArgs {
  const float* qpad;  // [bpad][kp] all probes of the call
  const float* G;     // [n][kp]
  const ef_match* gen;  // [b] genuine records
  const int* plab;      // [b] probe labels
  const int* uniq;      // [C] the labels that occur, ascending
  int64_t n, b, bpad;
  long long g_offset;
  int kp, n_classes;
  float* pt;
  double* pt64;
  double* pterr;
  long long* pgen;
  int* pcls;
};

// One wave per padded probe slot: what range_kernel<.., kRangeRank> reads of the probe.  A probe
// without a genuine row (no record, a record that is not finite, a slot past b) gets
// kRankNoGenuine.  The genuine row's score is recomputed when the row is resident here and
// taken from the record when it lies in another shard.
template <int METRIC>
__global__ __launch_bounds__(256) void rank_tau_kernel(const RankTauArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // wave-uniform
  if (p >= a.bpad) return;
  double tau = __builtin_nan("");
  long long row = -1;
  int cls = kRankNoGenuine;
  if (p < a.b) {
    const long long key = a.gen[p].key;
    if (key != EF_KEY_NONE) {
      row = (long long)((unsigned long long)key & 0xFFFFFFFFull);
      const long long loc = row - a.g_offset;
      if (loc >= 0 && loc < a.n) tau = score64<0, METRIC>(a.qpad + p * a.kp, a.G + loc * a.kp, lane, a.kp);
      else tau = a.gen[p].score;
      if (fabs(tau) < (double)__builtin_inff()) cls = rank_class_of(a.uniq, a.n_classes, a.plab[p]);  // false for NaN
    }
  }
  if (lane == 0) {
    const float t = (float)tau;
    a.pt[p] = METRIC == EF_METRIC_L2 ? t : -t;  // cosine: the scan scores the similarity itself
    a.pt64[p] = tau;
    a.pterr[p] = fabs((double)t - tau);  // +inf when fp32(tau) overflows: the probe's band is everything
    a.pgen[p] = row;
    a.pcls[p] = cls;
  }
}

// One wave per probe of a piece: better[p] <- the bits set in the probe's bitmap row, -1 without
// a genuine row
__global__ __launch_bounds__(256) void rank_count_kernel(const unsigned* __restrict__ bits, int words,
                                                         const int* __restrict__ pcls, int64_t b,
                                                         int* __restrict__ better) {
  const int lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= b) return;
  const unsigned* const row = bits + p * words;
  int s = 0;
  for (int w = lane; w < words; w += 64) s += __builtin_popcount(row[w]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if (lane == 0) better[p] = pcls[p] == kRankNoGenuine ? -1 : s;
}

__global__ void rank_info_kernel(const unsigned long long* __restrict__ counters, long long pieces, long long classes,
                                 long long* __restrict__ info) {
  info[0] = (long long)counters[kRcResolved];
  info[1] = pieces;
  info[2] = classes;
  info[3] = 0;
}

// The bitmap's shape for b probes and C classes under a budget: whole 256-probe blocks per piece,
// at least one.  Shared by the launches and ef_search_rank_plan.
inline void rank_plan(int64_t b, int64_t n, int64_t n_classes, int64_t budget, int64_t& words, int64_t& per_piece,
                      int64_t& n_pieces) {
  words = std::max<int64_t>(1, (n_classes + 31) / 32);
  const int64_t bpad = round_up(b, kSearchProbeTile);
  const int64_t block_bytes = words * 4 * kSearchProbeTile;
  per_piece = std::max<int64_t>(1, budget / block_bytes) * kSearchProbeTile;
  per_piece = std::min(per_piece, std::max<int64_t>(bpad, kSearchProbeTile));
  n_pieces = (b == 0 || n == 0) ? 0 : (bpad + per_piece - 1) / per_piece;
}

// The dense class map of the resident labels: cls[round_up(n, 128)] (-1 past n) and the sorted
// distinct labels.  Built on the host: one download of the labels, one upload of each array, and
// a wait, once per ef_gallery_labels.
static int rank_class_map(ef_ctx* c) {
  if (c->rank_map_valid) return EF_OK;
  const int64_t n = c->gal.n;
  hipStream_t s = c->stream;
  std::vector<int32_t> lab((size_t)n), uniq;
  EF_HIP(c, hipMemcpyAsync(lab.data(), c->glabels.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s),
         "D2H labels");
  EF_HIP(c, hipStreamSynchronize(s), "sync");
  uniq = lab;
  std::sort(uniq.begin(), uniq.end());
  uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
  const int64_t npad = round_up(n, RR);
  std::vector<int32_t> cls((size_t)npad, -1);
  for (int64_t i = 0; i < n; ++i)
    cls[(size_t)i] = (int32_t)(std::lower_bound(uniq.begin(), uniq.end(), lab[(size_t)i]) - uniq.begin());
  EF_TRY(ensure(c, c->rank_cls, (size_t)npad * sizeof(int32_t)));
  EF_TRY(ensure(c, c->rank_uniq, uniq.size() * sizeof(int32_t)));
  EF_HIP(c, hipMemcpyAsync(c->rank_cls.p, cls.data(), (size_t)npad * sizeof(int32_t), hipMemcpyHostToDevice, s),
         "H2D class ids");
  EF_HIP(c, hipMemcpyAsync(c->rank_uniq.p, uniq.data(), uniq.size() * sizeof(int32_t), hipMemcpyHostToDevice, s),
         "H2D class labels");
  EF_HIP(c, hipStreamSynchronize(s), "sync");  // the host arrays go away
  c->rank_classes = (int64_t)uniq.size();
  c->rank_map_valid = true;
  return EF_OK;
}

static hipError_t launch_rank_scan(hipStream_t s, int metric, const RangeArgs& a, int64_t n_chunks) {
  const dim3 grid((unsigned)(n_chunks * a.n_ptiles)), block(256);
  if (metric == EF_METRIC_L2) hipLaunchKernelGGL((range_kernel<EF_METRIC_L2, kRangeRank>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((range_kernel<EF_METRIC_COSINE, kRangeRank>), grid, block, 0, s, a);
  return hipGetLastError();
}

}  // namespace ef

using namespace ef;

extern "C" int ef_search_rank_plan(int64_t b, int64_t n, int64_t n_classes, int64_t bitmap_bytes,
                                   int64_t* words_per_probe, int64_t* probes_per_piece, int64_t* n_pieces) {
  if (b < 0 || n < 0 || n_classes < 0 || bitmap_bytes < 0 || !words_per_probe || !probes_per_piece || !n_pieces)
    return EF_E_INVALID;
  rank_plan(b, n, n_classes, bitmap_bytes, *words_per_probe, *probes_per_piece, *n_pieces);
  return EF_OK;
}

extern "C" int ef_search_rank(ef_ctx* c, const float* Q, int64_t b, int32_t metric, const int32_t* probe_labels,
                              const int64_t* exclude_rows, ef_match* genuine, int32_t* better, int64_t* info,
                              uint32_t flags) {
  if (!c) return EF_E_INVALID;
  if (c->gal.k == 0) return set_err(c, EF_E_STATE, "ef_search_rank: no gallery (call ef_gallery_set)");
  const bool given = (flags & EF_RANK_GENUINE_GIVEN) != 0;
  if (!info || b < 0 || (b > 0 && (!Q || !probe_labels || !better)) ||
      (metric != EF_METRIC_L2 && metric != EF_METRIC_COSINE) || (given && !genuine))
    return set_err(c, EF_E_INVALID, "ef_search_rank: bad arguments (probe_labels, better and info required, metric "
                                    "L2 or cosine, genuine with EF_RANK_GENUINE_GIVEN)");
  if (!c->has_labels)
    return set_err(c, EF_E_STATE, "ef_search_rank: the gallery has no labels (call ef_gallery_labels)");
  if (c->comm && c->comm_size > 1)
    return set_err(c, EF_E_STATE, "ef_search_rank: no rank search over a communicator; run each shard on a context "
                                  "without one with EF_RANK_GENUINE_GIVEN and add the counts");
  const Gallery& g = c->gal;
  if (g.n > INT_MAX - RR) return set_err(c, EF_E_INVALID, "ef_search_rank: more than 2^31 - 129 rows");
  EF_HIP(c, hipSetDevice(c->device), "hipSetDevice");
  hipStream_t s = c->stream;
  const bool dev = (flags & EF_MEM_DEVICE) != 0;
  const uint32_t mem = flags & EF_MEM_DEVICE;
  if (b == 0 || g.n == 0) {  // nobody has a genuine row
    if (dev) {
      EF_HIP(c, hipMemsetAsync(info, 0, 4 * sizeof(int64_t), s), "zero info");
      if (b > 0) EF_HIP(c, hipMemsetAsync(better, 0xFF, (size_t)b * sizeof(int32_t), s), "fill better");
    } else {
      std::memset(info, 0, 4 * sizeof(int64_t));
      std::fill(better, better + b, -1);
    }
    if (b > 0 && genuine && !given)
      EF_TRY(ef_search_labelled(c, Q, b, metric, EF_LABEL_SAME, probe_labels, exclude_rows, nullptr, genuine, mem));
    return EF_OK;
  }

  EF_TRY(rank_class_map(c));
  const int64_t C = c->rank_classes;
  const int64_t bpad = round_up(b, kSearchProbeTile);
  int64_t words, per_piece, n_pieces;
  rank_plan(b, g.n, C, c->opt_rank_bitmap_bytes, words, per_piece, n_pieces);
  if (words > INT_MAX) return set_err(c, EF_E_INVALID, "ef_search_rank: too many classes");

  struct Ws {
    float* qst;
    int32_t* lab_st;
    int64_t* excl_st;
    ef_match* gen;
    int *plabp, *pexcl, *pcls, *better_st;
    float *qaux, *pt;
    double *pt64, *pterr;
    long long *pgen, *info_st;
    unsigned long long* counters;
    unsigned* bits;
  };
  const bool own_gen = !dev || !genuine;  // the records live in the scratch
  const auto carve = [&](Carve& cv) {
    Ws w{};
    w.qst = dev ? nullptr : cv.take<float>((size_t)b * g.k);
    w.lab_st = dev ? nullptr : cv.take<int32_t>((size_t)b);
    w.excl_st = (!dev && exclude_rows) ? cv.take<int64_t>((size_t)b) : nullptr;
    w.gen = own_gen ? cv.take<ef_match>((size_t)b) : nullptr;
    w.plabp = cv.take<int>((size_t)bpad);
    w.pexcl = cv.take<int>((size_t)bpad);
    w.pcls = cv.take<int>((size_t)bpad);
    w.better_st = dev ? nullptr : cv.take<int>((size_t)b);
    w.qaux = cv.take<float>((size_t)bpad);
    w.pt = cv.take<float>((size_t)bpad);
    w.pt64 = cv.take<double>((size_t)bpad);
    w.pterr = cv.take<double>((size_t)bpad);
    w.pgen = cv.take<long long>((size_t)bpad);
    w.info_st = dev ? nullptr : cv.take<long long>(4);
    w.counters = cv.take<unsigned long long>(kRcCount);
    w.bits = cv.take<unsigned>((size_t)(per_piece * words));
    return w;
  };
  Carve size, cv;
  carve(size);
  EF_TRY(ensure(c, c->rank_ws, size.total));
  cv.base = c->rank_ws.p;
  const Ws w = carve(cv);

  TimerEvt tm;
  timer_begin(c, EF_KERNEL_RANK, &tm);
  ef_match* gen = own_gen ? w.gen : genuine;
  if (!dev) {
    EF_HIP(c, hipMemcpyAsync(w.qst, Q, (size_t)b * g.k * sizeof(float), hipMemcpyHostToDevice, s), "H2D queries");
    EF_HIP(c, hipMemcpyAsync(w.lab_st, probe_labels, (size_t)b * sizeof(int32_t), hipMemcpyHostToDevice, s),
           "H2D probe labels");
    Q = w.qst;
    probe_labels = w.lab_st;
    if (w.excl_st) {
      EF_HIP(c, hipMemcpyAsync(w.excl_st, exclude_rows, (size_t)b * sizeof(int64_t), hipMemcpyHostToDevice, s),
             "H2D excluded rows");
      exclude_rows = w.excl_st;
    }
    if (given)
      EF_HIP(c, hipMemcpyAsync(gen, genuine, (size_t)b * sizeof(ef_match), hipMemcpyHostToDevice, s),
             "H2D genuine records");
  }
  // the genuine rows: the labelled SAME scan on the device copies (it pads the probes into q_pad)
  if (given) EF_TRY(stage_queries(c, Q, b, true, bpad));
  else EF_TRY(ef_search_labelled(c, Q, b, metric, EF_LABEL_SAME, probe_labels, exclude_rows, nullptr, gen, EF_MEM_DEVICE));
  const float* qpad = static_cast<const float*>(c->q_pad.p);
  EF_HIP(c, hipMemsetAsync(w.counters, 0, kRcCount * sizeof(unsigned long long), s), "zero counters");
  EF_HIP(c, launch_label_prep(s, nullptr, exclude_rows, b, bpad, c->g_offset, g.n, w.plabp, w.pexcl), "label prep");
  EF_HIP(c, launch_census_probe_aux(s, qpad, bpad, g.kp, metric, w.qaux), "rank probe norms");

  RankTauArgs ta{};
  ta.qpad = qpad;
  ta.G = static_cast<const float*>(g.G.p);
  ta.gen = gen;
  ta.plab = probe_labels;
  ta.uniq = static_cast<const int*>(c->rank_uniq.p);
  ta.n = g.n;
  ta.b = b;
  ta.bpad = bpad;
  ta.g_offset = c->g_offset;
  ta.kp = g.kp;
  ta.n_classes = (int)C;
  ta.pt = w.pt;
  ta.pt64 = w.pt64;
  ta.pterr = w.pterr;
  ta.pgen = w.pgen;
  ta.pcls = w.pcls;
  if (metric == EF_METRIC_L2)
    hipLaunchKernelGGL(rank_tau_kernel<EF_METRIC_L2>, dim3((unsigned)(bpad / 4)), dim3(256), 0, s, ta);
  else
    hipLaunchKernelGGL(rank_tau_kernel<EF_METRIC_COSINE>, dim3((unsigned)(bpad / 4)), dim3(256), 0, s, ta);
  EF_HIP(c, hipGetLastError(), "rank thresholds");

  int* const better_d = dev ? better : w.better_st;
  long long* const info_d = dev ? reinterpret_cast<long long*>(info) : w.info_st;
  const bool outside = metric != EF_METRIC_L2 && (c->gal_rows_host & (kRowNotFinite | kRowTiny));
  RangeArgs a{};
  a.G = ta.G;
  a.aux = static_cast<const float*>(metric == EF_METRIC_L2 ? g.gnorm2.p : g.ginv.p);
  a.n = g.n;
  a.kp = g.kp;
  a.gmax2 = outside ? -c->gmax2_host : c->gmax2_host;
  a.counters = w.counters;
  a.g_offset = c->g_offset;
  a.cls = static_cast<const int*>(c->rank_cls.p);
  a.words = (int)words;
  a.n_classes = (int)C;
  for (int64_t off = 0; off < b; off += per_piece) {
    const int64_t pb = std::min(per_piece, b - off);  // the piece's probes; its bitmap rows are padded
    EF_HIP(c, hipMemsetAsync(w.bits, 0, (size_t)(round_up(pb, kSearchProbeTile) * words) * sizeof(unsigned), s),
           "zero bitmap");
    for (const SearchPiece& p : search_pieces(pb, g.kp)) {  // a padded probe block stays below 2 GiB
      const int64_t o = off + p.off;
      int64_t n_chunks, tpc;
      range_plan(p.bpad, g.n, n_chunks, tpc);
      if (n_chunks * (p.bpad / RP) >= ((int64_t)1 << 31))
        return set_err(c, EF_E_INVALID, "ef_search_rank: too many probes for one call");
      a.qpad = qpad + o * g.kp;
      a.qaux = w.qaux + o;
      a.pexcl = w.pexcl + o;
      a.pt = w.pt + o;
      a.pt64 = w.pt64 + o;
      a.pterr = w.pterr + o;
      a.pgen = w.pgen + o;
      a.pcls = w.pcls + o;
      a.bits = w.bits + p.off * words;
      a.b = p.b;
      a.n_ptiles = (int)(p.bpad / RP);
      a.tpc = (int)tpc;
      a.stride = p.bpad;
      EF_HIP(c, launch_rank_scan(s, metric, a, n_chunks), "rank scan");
    }
    hipLaunchKernelGGL(rank_count_kernel, dim3((unsigned)((pb + 3) / 4)), dim3(256), 0, s, w.bits, (int)words,
                       w.pcls + off, pb, better_d + off);
    EF_HIP(c, hipGetLastError(), "rank count");
  }
  hipLaunchKernelGGL(rank_info_kernel, dim3(1), dim3(1), 0, s, w.counters, (long long)n_pieces, (long long)C, info_d);
  EF_HIP(c, hipGetLastError(), "rank info");
  timer_end(c, &tm);
  if (dev) return EF_OK;

  EF_HIP(c, hipMemcpyAsync(better, w.better_st, (size_t)b * sizeof(int32_t), hipMemcpyDeviceToHost, s), "D2H better");
  EF_HIP(c, hipMemcpyAsync(info, w.info_st, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, s), "D2H info");
  if (genuine && !given)
    EF_HIP(c, hipMemcpyAsync(genuine, gen, (size_t)b * sizeof(ef_match), hipMemcpyDeviceToHost, s), "D2H genuine");
  EF_HIP(c, hipStreamSynchronize(s), "sync");
  return EF_OK;
}
