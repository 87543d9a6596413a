// C ABI: context, recognition model, gallery, search, timing (include/eigenface.h).
#include <climits>
#include <cmath>
#include <cstdio>
#include <algorithm>
#include <cstring>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <set>
#include <utility>
#include <vector>

#include "ef_internal.hpp"

#include <atomic>

namespace ef {

int set_err(ef_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}

int hip_err(ef_ctx* c, hipError_t e, const char* what) {
  return set_err(c, e == hipErrorOutOfMemory ? EF_E_NOMEM : EF_E_HIP,
                 std::string(what) + ": " + hipGetErrorString(e));
}

int ensure(ef_ctx* c, DevBuf& b, size_t bytes) {
  if (b.bytes >= bytes && b.p) return EF_OK;
  release(b);
  if (bytes == 0) bytes = 16;
  hipError_t e = hipMalloc(&b.p, bytes);
  if (e != hipSuccess) {
    b.p = nullptr;
    b.bytes = 0;
    return hip_err(c, e, "hipMalloc");
  }
  b.bytes = bytes;
  return EF_OK;
}

// ---- the owning handles (ef_internal.hpp): the only places that free ----------------
void free_device(void* p) { (void)hipFree(p); }
void free_pinned(void* p) { (void)hipHostFree(p); }
void free_event(hipEvent_t e) { (void)hipEventDestroy(e); }
void free_stream(hipStream_t s) { (void)hipStreamDestroy(s); }

hipError_t event_get(Event& e, hipStream_t record_on, unsigned flags) {
  if (e.p) return hipSuccess;
  hipError_t rc = hipEventCreateWithFlags(&e.p, flags);
  if (rc != hipSuccess) e.p = nullptr;
  else if (record_on) rc = hipEventRecord(e.p, record_on);
  return rc;
}

hipError_t stream_get(Stream& s) {
  if (s.p) return hipSuccess;
  const hipError_t rc = hipStreamCreateWithFlags(&s.p, hipStreamNonBlocking);
  if (rc != hipSuccess) s.p = nullptr;
  return rc;
}

hipError_t pinned_alloc(PinnedBuf& b, size_t bytes) {
  b.reset();
  const hipError_t rc = hipHostMalloc(&b.p, bytes, hipHostMallocDefault);
  if (rc != hipSuccess) b.p = nullptr;
  else b.bytes = bytes;
  return rc;
}

hipError_t SideJoin::fork() {
  hipError_t e = stream_get(side_.s);
  if (e == hipSuccess) e = event_get(side_.forked);
  if (e == hipSuccess) e = event_get(side_.done);
  if (e == hipSuccess) e = hipEventRecord(side_.forked, main_);
  if (e == hipSuccess) e = hipStreamWaitEvent(side_.s, side_.forked, 0);
  forked_ = e == hipSuccess;
  return e;
}

hipError_t SideJoin::done() {
  const hipError_t e = hipEventRecord(side_.done, side_.s);
  done_ = e == hipSuccess;
  return e;
}

hipError_t SideJoin::join() {
  if (!forked_) return hipSuccess;
  forked_ = false;
  // an exit between fork() and done(): whatever the side stream holds by now
  if (!done_ && hipEventRecord(side_.done, side_.s) != hipSuccess) return hipStreamSynchronize(side_.s);
  return hipStreamWaitEvent(main_, side_.done, 0);
}

// Timer events carry timestamps (the default flags).  A TimerEvt that is not queued frees
// its events when it goes out of scope.
static bool timer_events(ef_ctx* c, int kernel, TimerEvt* t) {
  t->kernel = -1;
  if (!c->timing) return false;
  if (event_get(t->a, nullptr, hipEventDefault) != hipSuccess) return false;
  if (event_get(t->b, nullptr, hipEventDefault) != hipSuccess) return false;
  t->kernel = kernel;
  return true;
}

void timer_begin(ef_ctx* c, int kernel, TimerEvt* t) {
  if (timer_events(c, kernel, t)) (void)hipEventRecord(t->a, c->stream);
}

void timer_arm(ef_ctx* c, int kernel, TimerEvt* t) { (void)timer_events(c, kernel, t); }

void timer_commit(ef_ctx* c, TimerEvt* t) {
  if (t->kernel >= 0) c->pending.push_back(std::move(*t));
  t->kernel = -1;
}

void timer_end(ef_ctx* c, TimerEvt* t) {
  if (t->kernel < 0) return;
  (void)hipEventRecord(t->b, c->stream);
  c->pending.push_back(std::move(*t));
  t->kernel = -1;
}

// The pieces a search launches for b probes of kp floats: whole 256-probe tiles, at
// most as many per piece as keep a probe row's byte offset below 2^31 (the kernels' 32-bit
// offsets).  Piece i covers probes [off, off + b) and is launched with bpad =
// round_up(b, 256) rows, and its plan is built from that same bpad — never from the
// caller's q_pad row count, which can be larger (the sharded projection pads
// R * ceil(b / R) rows): a plan whose probe-tile count differs from the launch's row count
// makes the kernels' part_key stride disagree between chunks.
std::vector<SearchPiece> search_pieces(int64_t b, int kp) {
  std::vector<SearchPiece> v;
  const int64_t row_bytes = (int64_t)kp * 4;
  const int64_t piece = std::max<int64_t>(kSearchProbeTile, ((int64_t)INT_MAX / row_bytes) / kSearchProbeTile * kSearchProbeTile);
  for (int64_t off = 0; off < b; off += piece) {
    const int64_t bi = std::min(piece, b - off);
    v.push_back(SearchPiece{off, bi, round_up(bi, kSearchProbeTile)});
  }
  return v;
}

SearchSchedule search_schedule(int64_t b, int64_t n, int kp, int variant, int k1, bool split1, int m, int cap) {
  SearchSchedule sc;
  sc.pieces = search_pieces(b, kp);
  for (const SearchPiece& p : sc.pieces) {
    sc.plans.push_back(search_plan(p.bpad, n, kp, variant != 0, 0, m));
    sc.bpad_max = std::max(sc.bpad_max, p.bpad);
    sc.parts = std::max(sc.parts, (size_t)sc.plans.back().nchunks * (size_t)p.bpad);
    if (k1 > 0) {
      sc.plans1.push_back(search_plan(p.bpad, n, k1, false, prefix_tile_rows(k1, split1)));
      sc.parts = std::max(sc.parts, (size_t)sc.plans1.back().nchunks * (size_t)p.bpad);
    }
  }
  Carve ws, pw;
  carve_search_ws(ws, sc.parts, (size_t)sc.bpad_max);
  if (m > 0) carve_topk_ws(ws, (size_t)sc.bpad_max, (size_t)cap);
  if (k1 > 0) carve_prefix_ws(pw, (size_t)sc.bpad_max, k1, kp);
  sc.ws_bytes = ws.total;
  sc.prefix_bytes = pw.total;
  return sc;
}

// EF_OPT_SEARCH_PREFIX auto: the prefix length and the smallest gallery it engages for at
// padded k = 128 (smaller galleries are launch-bound)
constexpr int kPrefixAutoK1 = 32;
constexpr int64_t kPrefixAutoMinRows = 65536;
constexpr int kPrefixGuardSkips = 16;  // searches kept off the prefix scan after a bad one

// The prefix length of this search, 0 = the plain full-k pipeline.  Also runs the guard: when
// the last prefix search whose counters have arrived (never waited for) sent more than half
// of its probe tiles to the full-k scan, this search and the next 15 skip the prefix scan —
// it would cost its own pass on top of most of a full one.  Results do not depend on it.
static int prefix_k1(ef_ctx* c, int metric, int variant) {
  const int kp = c->gal.kp;
  GalleryDerived& d = c->der;
  if (metric != EF_METRIC_L2 || variant != 0 || kp > 128 || c->opt_search_prefix == 0) return 0;
  int k1 = (int)c->opt_search_prefix;
  if (k1 == 1) k1 = kp == 128 && c->gal.n >= kPrefixAutoMinRows ? kPrefixAutoK1 : 0;
  if (k1 <= 0 || k1 >= kp) return 0;
  if (d.ev_pending) {
    const hipError_t q = hipEventQuery(c->prefix_ev);
    (void)hipGetLastError();  // hipErrorNotReady is an answer, not a failure of a later launch
    if (q == hipSuccess) {
      d.ev_pending = false;
      const int* host = static_cast<const int*>(c->prefix_host.p);
      const int64_t fb_tiles = round_up(host[0], kSearchProbeTile) / kSearchProbeTile;
      if (2 * fb_tiles > d.ev_tiles) d.skip_left = kPrefixGuardSkips;
      // the screen's own guard: it left more than half of the probe tiles' probes to the split
      // stage, which then costs most of a split scan on top of the screen
      const int64_t sc_tiles = d.ev_screen ? round_up(host[2], kSearchProbeTile) / kSearchProbeTile : 0;
      if (2 * sc_tiles > d.ev_tiles) d.screen_skip_left = kPrefixGuardSkips;
    }
  }
  if (d.skip_left > 0) {
    --d.skip_left;
    c->stats_skipped = true;
    return 0;
  }
  return k1;
}

// The derived copies a search of (variant, k1) reads, built on the first search that needs
// them and kept until GalleryDerived::reset(): G3 in the variant's layout with the scratch Q3
// of the probes' copy (wide k), the prefix copy (G1, gnorm1) in the arithmetic of split1, and
// beside it the screen's single-bf16 copy with its start values (G1h; screen).
// The only place that builds them and the only one that fills a SplitScan, so no launcher is
// handed a variant whose copy was not built.
static int search_copies(ef_ctx* c, int variant, int k1, bool split1, bool screen, int64_t bpad_max, SplitScan* sp) {
  const Gallery& g = c->gal;
  GalleryDerived& d = c->der;
  const float* G = static_cast<const float*>(g.G.p);
  *sp = SplitScan{};
  if (variant) {
    if (g.kp > 128) {
      EF_TRY(ensure(c, c->q3, (size_t)bpad_max * g.kp * sizeof(float)));
      sp->Q3 = static_cast<float*>(c->q3.p);
    }
    const int layout = split_layout(variant);
    if (d.g3_layout != layout) {
      d.g3_layout = 0;
      EF_TRY(ensure(c, d.G3, (size_t)g.n * g.kp * sizeof(float)));
      EF_HIP(c,
             layout == 3 ? launch_hi_rows(c->stream, G, g.n, g.kp, d.G3.p)
                         : launch_split_rows(c->stream, G, g.n, g.kp, d.G3.p),
             "split gallery");
      d.g3_layout = layout;
    }
    sp->variant = variant;
    sp->G3 = static_cast<const float*>(d.G3.p);
  }
  if (k1 > 0 && (d.g1_k1 != k1 || d.g1_split != split1)) {
    d.g1_k1 = 0;
    EF_TRY(ensure(c, d.G1, (size_t)g.n * k1 * sizeof(float)));
    EF_TRY(ensure(c, d.gnorm1, (size_t)g.n * 2 * sizeof(float)));
    EF_HIP(c,
           launch_prefix_gallery(c->stream, G, g.n, g.kp, k1, split1, static_cast<float*>(d.G1.p),
                                 static_cast<float*>(d.gnorm1.p)),
           "prefix gallery");
    d.g1_k1 = k1;
    d.g1_split = split1;
    d.g1h_k1 = 0;  // gnorm1's second half was rewritten
  }
  if (screen && d.g1h_k1 != k1) {
    d.g1h_k1 = 0;
    EF_TRY(ensure(c, d.G1h, (size_t)g.n * k1 * 2));
    EF_HIP(c, launch_prefix_screen_gallery(c->stream, G, g.n, g.kp, k1, d.G1h.p, static_cast<float*>(d.gnorm1.p)),
           "prefix screen gallery");
    d.g1h_k1 = k1;
  }
  return EF_OK;
}

// max ||g||^2 as the search kernels take it: negated when the gallery has a row outside the scans'
// error model for this metric (ef_search_common.hpp scan_regular), which sends every probe to the
// fp64 sweeps; the magnitude is the tie window's scale either way
static float scan_gmax2(const ef_ctx* c, int metric) {
  const unsigned bad = kRowNotFinite | (metric == EF_METRIC_L2 ? 0u : kRowTiny);
  return (c->gal_rows_host & bad) ? -c->gmax2_host : c->gmax2_host;
}

// Search the probes already in ctx->q_pad (at least round_up(b, 256) rows, kp = the gallery's)
// of this rank's gallery: keys_dev[b] and, when match_dev is non-null, the fp64 match
// records, piece by piece as search_schedule plans them.
static int search_run(ef_ctx* c, int64_t bpad, int64_t b, int metric, long long* keys_dev, ef_match* match_dev) {
  const Gallery& g = c->gal;
  c->stats_probes = b;
  c->stats_prefix = c->stats_skipped = false;
  c->stats_screen = c->stats_screen_skipped = false;
  if (g.n == 0) {
    EF_HIP(c, launch_keys_none(c->stream, keys_dev, b, match_dev), "keys");
    return EF_OK;
  }
  if (bpad < round_up(b, kSearchProbeTile))
    return set_err(c, EF_E_INVALID, "search: probe buffer shorter than the batch");
  const int variant = split_variant(c->opt_search_split_bf16, g.kp, false);
  const int k1 = prefix_k1(c, metric, variant);
  const bool split1 = c->opt_search_prefix_split != 0;  // the prefix scan's arithmetic
  // the screen engages where prefix64_kernel does, unless its guard keeps this search off it
  bool screen = k1 > 0 && k1 <= 32 && split1 && c->opt_search_prefix_screen != 0;
  if (screen && c->der.screen_skip_left > 0) {
    --c->der.screen_skip_left;
    c->stats_screen_skipped = true;
    screen = false;
  }
  const SearchSchedule sc = search_schedule(b, g.n, g.kp, variant, k1, split1, 0, 0);
  EF_TRY(ensure(c, c->search_ws, sc.ws_bytes));
  Carve cv{c->search_ws.p};
  SearchWs ws = carve_search_ws(cv, sc.parts, (size_t)sc.bpad_max);
  SplitScan sp;
  EF_TRY(search_copies(c, variant, k1, split1, screen, sc.bpad_max, &sp));
  PrefixWs pw{};
  if (k1 > 0) {
    if (!c->prefix_host.p) EF_HIP(c, pinned_alloc(c->prefix_host, 16), "pinned counters");
    EF_HIP(c, event_get(c->prefix_ev), "event");
    EF_TRY(ensure(c, c->prefix_ws, sc.prefix_bytes));
    Carve cvp{c->prefix_ws.p};
    pw = carve_prefix_ws(cvp, (size_t)sc.bpad_max, k1, g.kp);
    // [2] the search's total of probes sent to the full-k run; the screen's [3], [4] beside it
    EF_HIP(c, hipMemsetAsync(ws.amb_count + 2, 0, (screen ? 3 : 1) * sizeof(int), c->stream), "zero counters");
  }
  const float* G = static_cast<const float*>(g.G.p);
  const float* aux = static_cast<const float*>(metric == EF_METRIC_L2 ? g.gnorm2.p : g.ginv.p);
  int64_t tiles = 0;
  for (size_t i = 0; i < sc.pieces.size(); ++i) {
    const SearchPiece& p = sc.pieces[i];
    const float* q = static_cast<const float*>(c->q_pad.p) + p.off * g.kp;
    ws.match = match_dev ? match_dev + p.off : nullptr;
    tiles += p.bpad / kSearchProbeTile;
    if (screen && i > 0)  // the piece's own count of probes the screen leaves
      EF_HIP(c, hipMemsetAsync(ws.amb_count + kScreenCount, 0, sizeof(int), c->stream), "zero counters");
    if (k1 > 0)
      EF_HIP(c,
             launch_search_prefix(c->stream, g.kp, k1, sc.plans[i], sc.plans1[i], q, p.bpad, p.b, G, aux,
                                  static_cast<const float*>(c->der.G1.p), static_cast<const float*>(c->der.gnorm1.p),
                                  split1, screen ? static_cast<const float*>(c->der.G1h.p) : nullptr, g.n, c->g_offset,
                                  scan_gmax2(c, metric), ws, pw, keys_dev + p.off, c),
             "prefix search");
    else
      EF_HIP(c,
             launch_search(c->stream, g.kp, metric, sp, sc.plans[i], q, p.bpad, p.b, G, aux, g.n, c->g_offset,
                           scan_gmax2(c, metric), ws, keys_dev + p.off, c),
             "search");
  }
  if (k1 > 0) {
    // the counters follow the search to the host; nobody waits for them here
    EF_HIP(c,
           hipMemcpyAsync(c->prefix_host.p, ws.amb_count + 2, (screen ? 3 : 1) * sizeof(int), hipMemcpyDeviceToHost,
                          c->stream),
           "D2H prefix counters");
    EF_HIP(c, hipEventRecord(c->prefix_ev, c->stream), "event record");
    c->der.ev_pending = true;
    c->der.ev_tiles = tiles;
    c->der.ev_screen = screen;
    c->stats_prefix = true;
    c->stats_screen = screen;
  }
  return EF_OK;
}

// Search ctx->q_pad: this rank's shard, then (communicator attached) the exact merge of
// every rank's match records (ef_comm.hip).  match_dev (optional) receives the records
// of the (global) winners.
static int search_qpad(ef_ctx* c, int64_t bpad, int64_t b, int metric, long long* keys_dev, ef_match* match_dev) {
  if (!c->comm || c->comm_size == 1) return search_run(c, bpad, b, metric, keys_dev, match_dev);
  EF_TRY(ensure(c, c->match_local, (size_t)b * sizeof(ef_match)));
  EF_TRY(ensure(c, c->match_all, (size_t)b * c->comm_size * sizeof(ef_match)));
  ef_match* loc = static_cast<ef_match*>(c->match_local.p);
  ef_match* all = static_cast<ef_match*>(c->match_all.p);
  EF_TRY(search_run(c, bpad, b, metric, keys_dev, loc));
  EF_TRY(comm_allgather(c, loc, all, (size_t)b * sizeof(ef_match)));
  EF_HIP(c, launch_matches_merge(c->stream, all, c->comm_size, b, keys_dev, match_dev), "matches merge");
  return EF_OK;
}

// The split form of the fp32 model (EF_OPT_PROJECT_SPLIT_BF16): the three bf16 pieces of W,
// round(mean) as bytes and the correction row, built once per model by the first projection
// that can use them (ef_model_set resets split3_state); the device-side guard decides whether
// the form is exact for this model (split3_state 1) or the model keeps the fp32 kernel (-1).
static int split3_prepare(ef_ctx* c) {
  const int64_t d = c->d;
  const int ldw = c->kpw;
  EF_TRY(ensure(c, c->W3f, (size_t)3 * ldw * d * sizeof(unsigned short)));
  EF_TRY(ensure(c, c->corr, (size_t)ldw * sizeof(float)));
  const size_t off = align256((size_t)d);  // the two counters sit behind the bytes
  EF_TRY(ensure(c, c->mean_u8, off + 16));
  const int nchunk = 256;
  DevBuf cp;  // the kernels that use it are synchronised below, before it goes out of scope
  EF_TRY(ensure(c, cp, (size_t)nchunk * ldw * sizeof(double)));
  int bad[2] = {1, 1};
  int* bad_dev = reinterpret_cast<int*>(static_cast<char*>(c->mean_u8.p) + off);
  EF_HIP(c, hipMemsetAsync(bad_dev, 0, sizeof(bad), c->stream), "split model");
  EF_HIP(c,
         launch_split3_model(c->stream, static_cast<const float*>(c->W.p), static_cast<const float*>(c->mean.p), d,
                             ldw, c->W3f.p, static_cast<uint8_t*>(c->mean_u8.p), static_cast<float*>(c->corr.p),
                             static_cast<double*>(cp.p), nchunk, bad_dev),
         "split model");
  EF_HIP(c, hipMemcpyAsync(bad, bad_dev, sizeof(bad), hipMemcpyDeviceToHost, c->stream), "split model");
  EF_HIP(c, hipStreamSynchronize(c->stream), "split model");
  c->split3_state = (bad[0] == 0 && bad[1] == 0) ? 1 : -1;
  if (c->split3_state < 0) release(c->W3f);
  return EF_OK;
}

// Project b probes (device pointer P) into ctx->q_pad; optional feature output (device).
static int project_dev(ef_ctx* c, const void* P, int dtype, int64_t b, int64_t bpad, float* f_dev, DevBuf* dst) {
  EF_TRY(ensure(c, *dst, (size_t)bpad * c->kp * sizeof(float)));
  if (b == 0) {  // this rank's slice of a sharded projection can be empty
    EF_HIP(c, hipMemsetAsync(dst->p, 0, (size_t)bpad * c->kp * sizeof(float), c->stream), "zero features");
    return EF_OK;
  }
  int64_t pps = 0;
  // one selector for every caller: the split form wherever it is eligible, else the fp32 kernel
  bool split3 = !c->bf16 && c->opt_project_split_bf16 == 1 && c->split3_state >= 0 &&
                project_split3_ok(dtype, P, c->d, c->kpw);
  if (split3 && c->split3_state == 0) EF_TRY(split3_prepare(c));
  split3 = split3 && c->split3_state == 1;
  const uint8_t* mu8 = c->mean_u8_ok ? static_cast<const uint8_t*>(c->mean_u8.p) : nullptr;
  const void* wf = c->w16f_ok ? c->W16f.p : nullptr;
  const int ns = c->bf16  ? project_bf16_nsplit(dtype, P, mu8, wf, bpad, c->d, c->kpw, &pps)
                 : split3 ? project_split3_nsplit(bpad, c->d, c->kpw, &pps)
                          : project_nsplit(bpad, c->d, c->kpw, &pps);
  EF_TRY(ensure(c, c->proj_part, (size_t)ns * bpad * c->kpw * sizeof(float)));
  TimerEvt t;
  timer_begin(c, EF_KERNEL_PROJECT, &t);
  if (split3) {
    EF_HIP(c,
           launch_project_split3(c->stream, P, b, bpad, c->d, static_cast<const uint8_t*>(c->mean_u8.p), c->W3f.p,
                                 c->kpw, static_cast<float*>(c->proj_part.p), ns, pps),
           "project kernel (split bf16)");
  } else if (c->bf16) {
    EF_HIP(c,
           launch_project_bf16(c->stream, dtype, P, b, bpad, c->d, static_cast<const float*>(c->mean_r.p),
                               mu8, static_cast<const unsigned short*>(c->W16.p), wf,
                               c->kpw,
                               static_cast<float*>(c->proj_part.p), ns, pps),
           "project kernel (bf16)");
  } else {
    EF_HIP(c,
           launch_project(c->stream, c->kpw, dtype, P, b, bpad, c->d, static_cast<const float*>(c->mean.p),
                          static_cast<const float*>(c->W.p), static_cast<float*>(c->proj_part.p), ns, pps),
           "project kernel");
  }
  timer_end(c, &t);
  EF_HIP(c,
         launch_project_reduce(c->stream, static_cast<const float*>(c->proj_part.p), ns, b, bpad, c->kpw,
                               c->k, c->kp, c->bf16 || split3 ? static_cast<const float*>(c->corr.p) : nullptr,
                               static_cast<float*>(dst->p), f_dev),
         "project reduce");
  return EF_OK;
}

// Features of the whole batch in ctx->q_pad for the search.  With a communicator attached
// rank r projects probes [r*cs, (r+1)*cs), cs = ceil(b / ranks), and one all-gather of the
// (cs x kp) slices assembles the batch (rows past b are zero); otherwise the whole batch.
// Returns the padded row count of q_pad in *bpad_out.  f_dev (optional) gets this rank's
// rows only when sharded, so the fused path keeps the unsharded projection for it.
static int project_for_search(ef_ctx* c, const void* Pd, int dtype, int64_t b, float* f_dev, int64_t* bpad_out) {
  if (!c->comm || c->comm_size == 1 || f_dev) {
    const int64_t bpad = round_up(b, kSearchProbeTile);
    EF_TRY(project_dev(c, Pd, dtype, b, bpad, f_dev, &c->q_pad));
    *bpad_out = bpad;
    return EF_OK;
  }
  const int64_t R = c->comm_size, cs = (b + R - 1) / R;
  const int64_t lo = std::min<int64_t>(b, c->comm_rank * cs), hi = std::min<int64_t>(b, (c->comm_rank + 1) * cs);
  const size_t esz = dtype == EF_U8 ? 1 : 4;
  const void* Pl = static_cast<const char*>(Pd) + (size_t)lo * c->d * esz;
  EF_TRY(project_dev(c, Pl, dtype, hi - lo, round_up(cs, kSearchProbeTile), nullptr, &c->q_local));
  const int64_t rows = R * cs, bpad = round_up(rows, kSearchProbeTile);
  EF_TRY(ensure(c, c->q_pad, (size_t)bpad * c->kp * sizeof(float)));
  float* q = static_cast<float*>(c->q_pad.p);
  EF_TRY(comm_allgather(c, c->q_local.p, q, (size_t)cs * c->kp * sizeof(float)));
  if (bpad > rows)
    EF_HIP(c, hipMemsetAsync(q + rows * c->kp, 0, (size_t)(bpad - rows) * c->kp * sizeof(float), c->stream), "pad");
  *bpad_out = bpad;
  return EF_OK;
}

int stage_probes(ef_ctx* c, const void* P, int dtype, int64_t b, int64_t d, uint32_t flags, DevBuf& stage,
                 const void** Pd) {
  if (flags & EF_MEM_DEVICE) {
    *Pd = P;
    return EF_OK;
  }
  const size_t bytes = (size_t)b * d * (dtype == EF_U8 ? 1 : 4);
  EF_TRY(ensure(c, stage, bytes));
  EF_HIP(c, hipMemcpyAsync(stage.p, P, bytes, hipMemcpyHostToDevice, c->stream), "H2D probes");
  *Pd = stage.p;
  return EF_OK;
}

int Results::stage_feats(ef_ctx* c) {
  if (!feats) return EF_OK;
  fdev = feats;
  if (dev) return EF_OK;
  EF_TRY(ensure(c, c->feats_dev, (size_t)(b * fk) * sizeof(float)));
  fdev = static_cast<float*>(c->feats_dev.p);
  return EF_OK;
}

int Results::stage_keys(ef_ctx* c, int64_t bpad) {
  const size_t kbytes = (size_t)bpad * rec * sizeof(long long);
  EF_TRY(ensure(c, c->keys, kbytes + (size_t)b * rec * sizeof(ef_match)));
  kdev = (dev && keys) ? reinterpret_cast<long long*>(keys) : static_cast<long long*>(c->keys.p);
  if (match) mdev = dev ? match : reinterpret_cast<ef_match*>(static_cast<char*>(c->keys.p) + kbytes);
  return EF_OK;
}

int Results::fetch(ef_ctx* c) const {
  if (dev) return EF_OK;  // stream-ordered; the caller synchronises
  auto d2h = [&](void* dst, const void* src, size_t bytes) {
    return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
  };
  EF_HIP(c, d2h(keys, kdev, (size_t)b * rec * sizeof(long long)), "D2H keys");
  EF_HIP(c, d2h(match, mdev, (size_t)b * rec * sizeof(ef_match)), "D2H matches");
  EF_HIP(c, d2h(feats, fdev, (size_t)(b * fk) * sizeof(float)), "D2H features");
  EF_HIP(c, hipStreamSynchronize(c->stream), "sync");
  return EF_OK;
}

// b probe features Q[b][k of the gallery] (host, or device with dev) into ctx->q_pad, padded
// to bpad rows of the gallery's kp
int stage_queries(ef_ctx* c, const float* Q, int64_t b, bool dev, int64_t bpad) {
  const Gallery& g = c->gal;
  EF_TRY(ensure(c, c->q_pad, (size_t)bpad * g.kp * sizeof(float)));
  if (!dev) {
    const size_t bytes = (size_t)b * g.k * sizeof(float);
    EF_TRY(ensure(c, c->p_stage, bytes));
    EF_HIP(c, hipMemcpyAsync(c->p_stage.p, Q, bytes, hipMemcpyHostToDevice, c->stream), "H2D queries");
    Q = static_cast<const float*>(c->p_stage.p);
  }
  EF_HIP(c, launch_pad_rows(c->stream, Q, b, g.k, bpad, static_cast<float*>(c->q_pad.p), g.kp), "pad queries");
  return EF_OK;
}

namespace {
class HostPool {
 public:
  explicit HostPool(int workers) {
    for (int i = 0; i < workers; ++i) threads_.emplace_back([this] { loop(); });
  }
  void run(int n, const std::function<void(int)>& fn) {
    std::lock_guard<std::mutex> job(job_mu_);  // one job at a time
    {
      std::lock_guard<std::mutex> lk(mu_);
      fn_ = &fn;
      n_ = n;
      next_ = 0;
      done_ = 0;
    }
    cv_.notify_all();
    std::unique_lock<std::mutex> lk(mu_);
    while (next_ < n_) {  // the caller takes tasks too (and finishes the job alone if
      const int i = next_++;  // the workers are gone, e.g. in a forked child)
      lk.unlock();
      fn(i);
      lk.lock();
      ++done_;
    }
    done_cv_.wait(lk, [&] { return done_ == n_; });
    fn_ = nullptr;
    n_ = 0;
  }

 private:
  void loop() {
    std::unique_lock<std::mutex> lk(mu_);
    for (;;) {
      cv_.wait(lk, [&] { return fn_ && next_ < n_; });
      const int i = next_++;
      const std::function<void(int)>* f = fn_;
      lk.unlock();
      (*f)(i);  // the job cannot end before this task is counted
      lk.lock();
      if (++done_ == n_) done_cv_.notify_all();
    }
  }
  std::mutex job_mu_, mu_;
  std::condition_variable cv_, done_cv_;
  const std::function<void(int)>* fn_ = nullptr;
  int n_ = 0, next_ = 0, done_ = 0;
  std::vector<std::thread> threads_;
};
}  // namespace

// Host worker count (EF_OPT_HOST_THREADS, process-wide): the job's CPU share.  The machine's
// hardware_concurrency() is the wrong size on a shared host (256 on the GPU pool's boxes,
// whose one-GPU jobs get 16 CPUs), so the default is min(16, hardware threads) and the
// Python layer sets the share it sees (OMP_NUM_THREADS, else the affinity mask).
static std::atomic<int> g_host_threads{0};
int host_threads() {
  const int v = g_host_threads.load(std::memory_order_relaxed);
  if (v > 0) return v;
  return (int)std::min<unsigned>(16u, std::max(1u, std::thread::hardware_concurrency()));
}

void host_parallel(int n, const std::function<void(int)>& fn) {
  if (n <= 1) {
    if (n == 1) fn(0);
    return;
  }
  // never destroyed: the workers block on the condition variable until the process exits
  // (sized on first use; the caller takes tasks too, so n tasks always finish)
  static HostPool* pool = new HostPool(std::max(0, std::min(host_threads(), 64) - 1));
  pool->run(n, fn);
}

// dst[rows][kp] <- src[rows][k] (host, or device with EF_MEM_DEVICE) on c->stream.  A host
// source that needs padding is staged unpadded in `staging`: the caller keeps it alive until
// it has synchronised.  direct: rows that need no padding (k == kp) are copied without the
// kernel, as the gallery's always were; W always goes through it.
static int load_padded(ef_ctx* c, const float* src, int64_t rows, int k, int kp, uint32_t flags, bool direct,
                       DevBuf& dst, DevBuf& staging, const char* what, const char* what_pad) {
  const bool dev = flags & EF_MEM_DEVICE;
  const size_t bytes = (size_t)rows * k * sizeof(float);
  EF_TRY(ensure(c, dst, (size_t)rows * kp * sizeof(float)));
  if (direct && k == kp) {
    EF_HIP(c, hipMemcpyAsync(dst.p, src, bytes, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream), what);
    return EF_OK;
  }
  if (!dev) {
    EF_TRY(ensure(c, staging, bytes));
    EF_HIP(c, hipMemcpyAsync(staging.p, src, bytes, hipMemcpyHostToDevice, c->stream), what);
    src = static_cast<const float*>(staging.p);
  }
  EF_HIP(c, launch_pad_rows(c->stream, src, rows, k, rows, static_cast<float*>(dst.p), kp), what_pad);
  return EF_OK;
}

int weights_load(ef_ctx* c, DevBuf& mean_dst, DevBuf& W_dst, const float* mean, const float* W, int64_t d, int k,
                 int kpw, uint32_t flags, DevBuf& staging) {
  EF_TRY(ensure(c, mean_dst, (size_t)d * sizeof(float)));
  EF_HIP(c,
         hipMemcpyAsync(mean_dst.p, mean, (size_t)d * sizeof(float),
                        (flags & EF_MEM_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream),
         "copy mean");
  return load_padded(c, W, d, k, kpw, flags, false, W_dst, staging, "copy W", "pad W");
}

int gallery_load(ef_ctx* c, Gallery& g, const float* G, int64_t n, int k, uint32_t flags, DevBuf& staging,
                 float* gmax2_host, unsigned* rows_host) {
  const int kp = feature_pad(k);
  if (rows_host) *rows_host = 0;
  g.n = 0;  // empty until the last step has succeeded
  if (n > 0) {
    EF_TRY(ensure(c, g.gnorm2, (size_t)n * sizeof(float)));
    EF_TRY(ensure(c, g.ginv, (size_t)n * sizeof(float)));
    EF_TRY(ensure(c, g.gmax2, 16));
    EF_TRY(load_padded(c, G, n, k, kp, flags, true, g.G, staging, "copy gallery", "pad gallery"));
    if (gmax2_host && k != kp) {
      EF_HIP(c, hipStreamSynchronize(c->stream), "pad gallery");
      release(staging);  // as large as the gallery itself
    }
    EF_HIP(c,
           launch_gallery_aux(c->stream, static_cast<const float*>(g.G.p), n, kp, static_cast<float*>(g.gnorm2.p),
                              static_cast<float*>(g.ginv.p), static_cast<unsigned*>(g.gmax2.p)),
           "gallery norms");
    if (gmax2_host) {
      EF_HIP(c, hipMemcpyAsync(gmax2_host, g.gmax2.p, sizeof(float), hipMemcpyDeviceToHost, c->stream), "D2H gmax2");
      if (rows_host)
        EF_HIP(c,
               hipMemcpyAsync(rows_host, static_cast<const unsigned*>(g.gmax2.p) + 1, sizeof(unsigned),
                              hipMemcpyDeviceToHost, c->stream),
               "D2H gallery row bits");
      EF_HIP(c, hipStreamSynchronize(c->stream), "sync");
    }
  }
  g.n = n;
  g.k = k;
  g.kp = kp;
  return EF_OK;
}

hipError_t allow_dynamic_lds(const void* fn, int bytes) {
  static std::mutex mu;
  static std::set<std::pair<const void*, int>> done;  // (kernel, device)
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lk(mu);
  if (done.count({fn, dev})) return hipSuccess;
  e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) done.insert({fn, dev});
  return e;
}

}  // namespace ef

using namespace ef;

ef_ctx::~ef_ctx() {
  comm_release(this);
  tm_release(this);
  haar_release(this);
}

extern "C" {

int ef_api_version(void) { return EF_API_VERSION; }

int ef_search_schedule(int64_t b, int32_t k, int64_t n, int32_t split_bf16, int64_t* pieces_out, int32_t max_pieces,
                       int32_t* n_pieces) {
  if (b < 0 || k < 1 || k > 65536 || n < 1 || !n_pieces || max_pieces < 0 || (max_pieces > 0 && !pieces_out))
    return EF_E_INVALID;
  const int kp = feature_pad(k);
  const SearchSchedule sc = search_schedule(b, n, kp, split_bf16 != 0, 0, false, 0, 0);  // what search_run launches
  const std::vector<SearchPiece>& pieces = sc.pieces;
  *n_pieces = (int32_t)pieces.size();
  for (size_t i = 0; i < pieces.size() && (int64_t)i < max_pieces; ++i) {
    const SearchPlan& pl = sc.plans[i];
    int64_t* o = pieces_out + 6 * i;
    o[0] = pieces[i].off;
    o[1] = pieces[i].b;
    o[2] = pieces[i].bpad;
    o[3] = pl.n_ptiles;
    o[4] = pl.nchunks;
    o[5] = (int64_t)pl.tiles_per_chunk;
  }
  return EF_OK;
}

int ef_device_count(int* out) {
  if (!out) return EF_E_INVALID;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
  *out = n;
  return EF_OK;
}

int ef_create(int device, ef_ctx** out) {
  if (!out) return EF_E_INVALID;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return EF_E_HIP;
  if (device < 0 || device >= n) return EF_E_INVALID;
  if (hipSetDevice(device) != hipSuccess) return EF_E_HIP;
  ef_ctx* c = new ef_ctx();
  c->device = device;
  if (stream_get(c->own_stream) != hipSuccess) {
    delete c;
    return EF_E_HIP;
  }
  c->stream = c->own_stream;
  *out = c;
  return EF_OK;
}

void ef_destroy(ef_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  (void)jpeg_quiesce(c);
  for (const SideStream* side : {&c->fit_side, &c->tm_side})
    if (side->s.p) (void)hipStreamSynchronize(side->s);
  delete c;
}

const char* ef_last_error(const ef_ctx* c) { return c ? c->err.c_str() : "null context"; }

int ef_set_stream(ef_ctx* c, void* s) {
  if (!c) return EF_E_INVALID;
  c->stream = static_cast<hipStream_t>(s);  // NULL = the default stream
  return EF_OK;
}

int ef_get_stream(const ef_ctx* c, void** out) {
  if (!c || !out) return EF_E_INVALID;
  *out = static_cast<void*>(c->stream);
  return EF_OK;
}

int ef_use_own_stream(ef_ctx* c) {
  if (!c) return EF_E_INVALID;
  c->stream = c->own_stream;
  return EF_OK;
}

int ef_synchronize(ef_ctx* c) {
  if (!c) return EF_E_INVALID;
  EF_HIP(c, hipStreamSynchronize(c->stream), "hipStreamSynchronize");
  return EF_OK;
}

int ef_trim(ef_ctx* c) {
  if (!c) return EF_E_INVALID;
  EF_HIP(c, hipSetDevice(c->device), "hipSetDevice");
  EF_HIP(c, hipStreamSynchronize(c->stream), "hipStreamSynchronize");
  EF_HIP(c, jpeg_quiesce(c), "jpeg quiesce");
  c->fit_pool.clear();
  for (DevBuf* b : {&c->jpeg_ws, &c->jpeg_out, &c->jpeg_rows, &c->jpeg_up[0], &c->jpeg_up[1]}) release(*b);
  for (PinnedBuf& b : c->jpeg_pinned) b.reset();
  return EF_OK;
}

// no reconstruction state: the flag first, then the resident operands (the frees wait for the device)
static void recon_drop(ef_ctx* c) {
  c->recon = false;
  release(c->recon_R);
  release(c->recon_w);
}

int ef_model_set(ef_ctx* c, const float* mean, const float* W, int64_t d, int32_t k, uint32_t flags) {
  if (!c) return EF_E_INVALID;
  if (!mean || !W || d < 1 || k < 1) return set_err(c, EF_E_INVALID, "ef_model_set: bad arguments");
  const int kp = feature_pad(k);
  if (kp < 0) return set_err(c, EF_E_INVALID, "ef_model_set: k > 65536 is not supported");
  (void)hipSetDevice(c->device);
  const bool bf16 = (flags & EF_MODEL_BF16) != 0;
  const int kpw = bf16 ? (kp + 127) / 128 * 128 : proj_pad(kp);  // bf16 kernel: 128-column tiles
  c->d = 0;  // no model until the last step has succeeded (never old dimensions over new buffers)
  recon_drop(c);  // its R belonged to the old W
  {
    DevBuf staging;  // freed at the end of this block, after the synchronise (or by a hipFree that waits)
    EF_TRY(weights_load(c, c->mean, c->W, mean, W, d, k, kpw, flags, staging));
    EF_HIP(c, hipStreamSynchronize(c->stream), "pad W");
  }
  c->mean_u8_ok = c->w16f_ok = false;
  c->split3_state = 0;  // the pieces belonged to the old W
  if (bf16) {
    const int ldw = kpw;
    EF_TRY(ensure(c, c->W16, (size_t)ldw * d * sizeof(unsigned short)));
    EF_TRY(ensure(c, c->mean_r, (size_t)d * sizeof(float)));
    EF_TRY(ensure(c, c->corr, (size_t)ldw * sizeof(float)));
    const size_t off = align256((size_t)d);  // the counter sits behind the bytes
    EF_TRY(ensure(c, c->mean_u8, off + 16));
    const int nchunk = 256;
    DevBuf cp;  // the kernels that use it are synchronised below, before it goes out of scope
    EF_TRY(ensure(c, cp, (size_t)nchunk * ldw * sizeof(double)));
    int bad = 1;
    int* bad_dev = reinterpret_cast<int*>(static_cast<char*>(c->mean_u8.p) + off);
    EF_HIP(c,
           launch_bf16_model(c->stream, static_cast<const float*>(c->W.p), static_cast<const float*>(c->mean.p), d, ldw,
                             static_cast<unsigned short*>(c->W16.p), static_cast<float*>(c->mean_r.p),
                             static_cast<float*>(c->corr.p), static_cast<double*>(cp.p), nchunk),
           "bf16 model");
    EF_HIP(c, hipMemsetAsync(bad_dev, 0, sizeof(int), c->stream), "bf16 model");
    EF_HIP(c,
           launch_mean_u8(c->stream, static_cast<const float*>(c->mean_r.p), d, static_cast<uint8_t*>(c->mean_u8.p),
                          bad_dev),
           "bf16 model");
    EF_HIP(c, hipMemcpyAsync(&bad, bad_dev, sizeof(int), hipMemcpyDeviceToHost, c->stream), "bf16 model");
    EF_HIP(c, hipStreamSynchronize(c->stream), "bf16 model");
    c->mean_u8_ok = bad == 0;
    if (bf16_frag_supported(d, ldw)) {
      EF_TRY(ensure(c, c->W16f, (size_t)ldw * d * sizeof(unsigned short)));
      EF_HIP(c, launch_bf16_frag(c->stream, static_cast<const unsigned short*>(c->W16.p), d, ldw, c->W16f.p),
             "bf16 fragment model");
      EF_HIP(c, hipStreamSynchronize(c->stream), "sync");
      c->w16f_ok = true;
    }
  }
  c->bf16 = bf16;
  c->d = d;
  c->k = k;
  c->kp = kp;
  c->kpw = kpw;
  return EF_OK;
}

int ef_project(ef_ctx* c, const void* P, int32_t dtype, int64_t b, float* F, uint32_t flags) {
  if (!c) return EF_E_INVALID;
  if (c->d == 0) return set_err(c, EF_E_STATE, "ef_project: no model (call ef_model_set)");
  if (!P || !F || b < 0 || (dtype != EF_U8 && dtype != EF_F32))
    return set_err(c, EF_E_INVALID, "ef_project: bad arguments");
  if (b == 0) return EF_OK;
  (void)hipSetDevice(c->device);
  const int64_t bpad = round_up(b, kSearchProbeTile);
  const void* Pd = nullptr;
  EF_TRY(stage_probes(c, P, dtype, b, c->d, flags, c->p_stage, &Pd));
  Results r{(flags & EF_MEM_DEVICE) != 0, b, 1, c->k, nullptr, nullptr, F};
  EF_TRY(r.stage_feats(c));
  EF_TRY(project_dev(c, Pd, dtype, b, bpad, r.fdev, &c->q_pad));
  return r.fetch(c);
}

int ef_recon_set(ef_ctx* c, const float* R, const float* weight, int64_t d, int32_t k, uint32_t flags) {
  if (!c) return EF_E_INVALID;
  if (c->d == 0) return set_err(c, EF_E_STATE, "ef_recon_set: no model (call ef_model_set)");
  (void)hipSetDevice(c->device);
  recon_drop(c);  // a failed call leaves none
  if (!R || d != c->d || k != c->k) return set_err(c, EF_E_INVALID, "ef_recon_set: R must be the model's k x d");
  if (d > (int64_t)INT_MAX - 128) return set_err(c, EF_E_INVALID, "ef_recon_set: d >= 2^31 - 128 is not supported");
  const int64_t dp = recon_dpad(d);
  const bool dev = (flags & EF_MEM_DEVICE) != 0;
  std::vector<float> ones;
  DevBuf staging;  // freed after the synchronise below
  EF_TRY(ensure(c, c->recon_R, (size_t)c->kp * dp * sizeof(float)));
  EF_TRY(ensure(c, c->recon_w, (size_t)d * sizeof(float)));
  if (!dev) {
    EF_TRY(ensure(c, staging, (size_t)k * d * sizeof(float)));
    EF_HIP(c, hipMemcpyAsync(staging.p, R, (size_t)k * d * sizeof(float), hipMemcpyHostToDevice, c->stream), "copy R");
    R = static_cast<const float*>(staging.p);
  }
  EF_HIP(c, launch_pad_rows(c->stream, R, k, (int)d, c->kp, static_cast<float*>(c->recon_R.p), (int)dp), "pad R");
  if (!weight) {
    ones.assign((size_t)d, 1.f);
    weight = ones.data();
  }
  EF_HIP(c,
         hipMemcpyAsync(c->recon_w.p, weight, (size_t)d * sizeof(float),
                        dev && ones.empty() ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream),
         "copy weight");
  EF_HIP(c, hipStreamSynchronize(c->stream), "pad R");
  c->recon = true;
  return EF_OK;
}

int ef_reconstruct(ef_ctx* c, const float* F, int64_t b, int32_t out_dtype, void* out, uint32_t flags) {
  if (!c) return EF_E_INVALID;
  if (!c->recon) return set_err(c, EF_E_STATE, "ef_reconstruct: no reconstruction state (call ef_recon_set)");
  if (b < 0 || (out_dtype != EF_U8 && out_dtype != EF_F32) || (b > 0 && (!F || !out)))
    return set_err(c, EF_E_INVALID, "ef_reconstruct: bad arguments");
  if (b == 0) return EF_OK;  // (an empty batch may come with null pointers)
  (void)hipSetDevice(c->device);
  const bool dev = (flags & EF_MEM_DEVICE) != 0;
  const int64_t bpad = round_up(b, kProjRowTile);
  const size_t obytes = (size_t)b * c->d * (out_dtype == EF_U8 ? 1 : 4);
  EF_TRY(ensure(c, c->q_pad, (size_t)bpad * c->kp * sizeof(float)));
  if (!dev) {
    const size_t fbytes = (size_t)b * c->k * sizeof(float);
    EF_TRY(ensure(c, c->p_stage, fbytes));
    EF_TRY(ensure(c, c->recon_out, obytes));
    EF_HIP(c, hipMemcpyAsync(c->p_stage.p, F, fbytes, hipMemcpyHostToDevice, c->stream), "H2D features");
    F = static_cast<const float*>(c->p_stage.p);
  }
  void* odev = dev ? out : c->recon_out.p;
  EF_HIP(c, launch_pad_rows(c->stream, F, b, c->k, bpad, static_cast<float*>(c->q_pad.p), c->kp), "pad features");
  int tps = 0;
  const int ns = recon_nsplit(b, c->d, &tps);
  TimerEvt t;
  timer_begin(c, EF_KERNEL_RECON, &t);
  EF_HIP(c,
         launch_recon(c->stream, out_dtype == EF_U8 ? 1 : 0, EF_F32, static_cast<const float*>(c->q_pad.p), c->kp,
                      static_cast<const float*>(c->recon_R.p), static_cast<const float*>(c->mean.p),
                      static_cast<const float*>(c->recon_w.p), nullptr, b, c->d, odev, nullptr, ns, tps),
         "reconstruct kernel");
  timer_end(c, &t);
  if (dev) return EF_OK;
  EF_HIP(c, hipMemcpyAsync(out, odev, obytes, hipMemcpyDeviceToHost, c->stream), "D2H reconstruction");
  EF_HIP(c, hipStreamSynchronize(c->stream), "sync");
  return EF_OK;
}

int ef_face_distance(ef_ctx* c, const void* P, int32_t p_dtype, int64_t b, float* dffs2, float* energy, float* F_out,
                     uint32_t flags) {
  if (!c) return EF_E_INVALID;
  if (!c->recon) return set_err(c, EF_E_STATE, "ef_face_distance: no reconstruction state (call ef_recon_set)");
  if (b < 0 || (p_dtype != EF_U8 && p_dtype != EF_F32) || (b > 0 && (!P || !dffs2)))
    return set_err(c, EF_E_INVALID, "ef_face_distance: bad arguments");
  if (b == 0) return EF_OK;  // (an empty batch may come with null pointers)
  (void)hipSetDevice(c->device);
  const int64_t bpad = round_up(b, kSearchProbeTile);  // ef_project's padding: the same features, bit for bit
  const void* Pd = nullptr;
  EF_TRY(stage_probes(c, P, p_dtype, b, c->d, flags, c->p_stage, &Pd));
  Results r{(flags & EF_MEM_DEVICE) != 0, b, 1, c->k, nullptr, nullptr, F_out};
  EF_TRY(r.stage_feats(c));
  EF_TRY(project_dev(c, Pd, p_dtype, b, bpad, r.fdev, &c->q_pad));
  int tps = 0;
  const int ns = recon_nsplit(b, c->d, &tps);
  const int64_t bp = round_up(b, kProjRowTile);
  EF_TRY(ensure(c, c->recon_part, (size_t)2 * ns * bp * sizeof(float)));
  float* ddev = dffs2;
  float* edev = energy;
  if (!r.dev) {
    EF_TRY(ensure(c, c->recon_out, (size_t)2 * b * sizeof(float)));
    ddev = static_cast<float*>(c->recon_out.p);
    edev = energy ? ddev + b : nullptr;
  }
  TimerEvt t;
  timer_begin(c, EF_KERNEL_RECON, &t);
  EF_HIP(c,
         launch_recon(c->stream, 2, p_dtype, static_cast<const float*>(c->q_pad.p), c->kp,
                      static_cast<const float*>(c->recon_R.p), static_cast<const float*>(c->mean.p),
                      static_cast<const float*>(c->recon_w.p), Pd, b, c->d, nullptr,
                      static_cast<float*>(c->recon_part.p), ns, tps),
         "residual kernel");
  timer_end(c, &t);
  timer_begin(c, EF_KERNEL_RECON_REDUCE, &t);
  EF_HIP(c, launch_recon_reduce(c->stream, static_cast<const float*>(c->recon_part.p), ns, b, ddev, edev),
         "residual reduce");
  timer_end(c, &t);
  if (!r.dev) {
    EF_HIP(c, hipMemcpyAsync(dffs2, ddev, (size_t)b * sizeof(float), hipMemcpyDeviceToHost, c->stream), "D2H distances");
    if (energy)
      EF_HIP(c, hipMemcpyAsync(energy, edev, (size_t)b * sizeof(float), hipMemcpyDeviceToHost, c->stream), "D2H energy");
  }
  return r.fetch(c);
}

int ef_gallery_set(ef_ctx* c, const float* G, int64_t n, int32_t k, int64_t offset, uint32_t flags) {
  if (!c) return EF_E_INVALID;
  if ((!G && n > 0) || n < 0 || k < 1 || offset < 0 || n + offset > (int64_t)UINT_MAX)
    return set_err(c, EF_E_INVALID, "ef_gallery_set: bad arguments");
  const int kp = feature_pad(k);
  if (kp < 0) return set_err(c, EF_E_INVALID, "ef_gallery_set: k > 65536 is not supported");
  (void)hipSetDevice(c->device);
  c->der.reset();  // the copies and the guard's history belong to the gallery they were made from
  c->has_labels = false;  // and so do the row labels (ef_gallery_labels)
  c->rank_map_valid = false;  // and their dense class map (ef_search_rank)
  release(c->glabels);
  DevBuf staging;
  EF_TRY(gallery_load(c, c->gal, G, n, k, flags, staging, &c->gmax2_host, &c->gal_rows_host));
  c->g_offset = offset;
  return EF_OK;
}

int ef_gallery_labels(ef_ctx* c, const int32_t* labels, int64_t n, uint32_t flags) {
  if (!c) return EF_E_INVALID;
  if (c->gal.k == 0) return set_err(c, EF_E_STATE, "ef_gallery_labels: no gallery (call ef_gallery_set)");
  (void)hipSetDevice(c->device);
  if (!labels) {  // drop them, once no queued search reads them any more
    EF_HIP(c, hipStreamSynchronize(c->stream), "sync");
    c->has_labels = false;
    c->rank_map_valid = false;
    release(c->glabels);
    return EF_OK;
  }
  if (n != c->gal.n)
    return set_err(c, EF_E_INVALID, "ef_gallery_labels: n differs from the resident gallery's row count");
  // the new state is built completely, then published: a failure leaves the previous labels
  DevBuf nb;
  EF_TRY(ensure(c, nb, (size_t)n * sizeof(int32_t)));
  if (n > 0)
    EF_HIP(c,
           hipMemcpyAsync(nb.p, labels, (size_t)n * sizeof(int32_t),
                          (flags & EF_MEM_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream),
           "copy labels");
  EF_HIP(c, hipStreamSynchronize(c->stream), "copy labels");  // also: nothing queued reads the old ones
  c->glabels = std::move(nb);
  c->has_labels = true;
  c->rank_map_valid = false;  // ef_search_rank rebuilds its class map from the new labels
  return EF_OK;
}

// The labelled top-1 search of the probes in ctx->q_pad (search_run's contract): always the fp32
// scan (no split copy, no prefix scan), piece by piece; the probes' labels and exclusions
// (plab, pexcl: launch_label_prep's output for all round_up(b, 256) rows) and the outputs advance
// with the piece's offset.
static int search_labelled_run(ef_ctx* c, int64_t bpad, int64_t b, int metric, int relation, const int* plab,
                               const int* pexcl, long long* keys_dev, ef_match* match_dev) {
  const Gallery& g = c->gal;
  if (g.n == 0) {
    EF_HIP(c, launch_keys_none(c->stream, keys_dev, b, match_dev), "keys");
    return EF_OK;
  }
  if (bpad < round_up(b, kSearchProbeTile))
    return set_err(c, EF_E_INVALID, "labelled search: probe buffer shorter than the batch");
  const SearchSchedule sc = search_schedule(b, g.n, g.kp, 0, 0, false, 0, 0);
  EF_TRY(ensure(c, c->search_ws, sc.ws_bytes));
  Carve cv{c->search_ws.p};
  SearchWs ws = carve_search_ws(cv, sc.parts, (size_t)sc.bpad_max);
  ws.lbl = relation + 1;
  ws.glab = relation == EF_LABEL_ANY ? nullptr : static_cast<const int*>(c->glabels.p);
  const float* G = static_cast<const float*>(g.G.p);
  const float* aux = static_cast<const float*>(metric == EF_METRIC_L2 ? g.gnorm2.p : g.ginv.p);
  for (size_t i = 0; i < sc.pieces.size(); ++i) {
    const SearchPiece& p = sc.pieces[i];
    ws.match = match_dev ? match_dev + p.off : nullptr;
    ws.plab = plab + p.off;
    ws.pexcl = pexcl + p.off;
    EF_HIP(c,
           launch_search(c->stream, g.kp, metric, SplitScan{}, sc.plans[i],
                         static_cast<const float*>(c->q_pad.p) + p.off * g.kp, p.bpad, p.b, G, aux, g.n, c->g_offset,
                         scan_gmax2(c, metric), ws, keys_dev + p.off, c),
           "labelled search");
  }
  return EF_OK;
}

int ef_search_labelled(ef_ctx* c, const float* Q, int64_t b, int32_t metric, int32_t relation,
                       const int32_t* probe_labels, const int64_t* exclude_rows, int64_t* keys, ef_match* matches,
                       uint32_t flags) {
  if (!c) return EF_E_INVALID;
  if (c->gal.k == 0) return set_err(c, EF_E_STATE, "ef_search_labelled: no gallery (call ef_gallery_set)");
  const bool any = relation == EF_LABEL_ANY;
  if ((!keys && !matches) || b < 0 || (b > 0 && !Q) || (metric != EF_METRIC_L2 && metric != EF_METRIC_COSINE) ||
      (relation != EF_LABEL_SAME && relation != EF_LABEL_OTHER && !any) || (!any && b > 0 && !probe_labels))
    return set_err(c, EF_E_INVALID, "ef_search_labelled: bad arguments");
  if (!any && !c->has_labels)
    return set_err(c, EF_E_STATE, "ef_search_labelled: the gallery has no labels (call ef_gallery_labels)");
  if (c->comm && c->comm_size > 1)
    return set_err(c, EF_E_STATE, "ef_search_labelled: no labelled search over a communicator; search each shard "
                                  "for its records on a context without one and merge them with ef_matches_merge");
  if (b == 0) return EF_OK;
  (void)hipSetDevice(c->device);
  Results r{(flags & EF_MEM_DEVICE) != 0, b, 1, c->k, keys, matches, nullptr};
  const int64_t bpad = round_up(b, kSearchProbeTile);
  EF_TRY(stage_queries(c, Q, b, r.dev, bpad));
  EF_TRY(r.stage_keys(c, bpad));
  // scratch: plab[bpad], pexcl[bpad], then a host call's labels and exclusions
  const size_t lab_off = align256((size_t)2 * bpad * sizeof(int));
  const size_t exc_off = lab_off + align256((size_t)b * sizeof(int32_t));
  EF_TRY(ensure(c, c->label_ws, exc_off + (size_t)b * sizeof(int64_t)));
  char* base = static_cast<char*>(c->label_ws.p);
  int* plab = reinterpret_cast<int*>(base);
  int* pexcl = plab + bpad;
  if (!r.dev) {
    if (probe_labels) {
      EF_HIP(c, hipMemcpyAsync(base + lab_off, probe_labels, (size_t)b * sizeof(int32_t), hipMemcpyHostToDevice, c->stream),
             "H2D probe labels");
      probe_labels = reinterpret_cast<const int32_t*>(base + lab_off);
    }
    if (exclude_rows) {
      EF_HIP(c, hipMemcpyAsync(base + exc_off, exclude_rows, (size_t)b * sizeof(int64_t), hipMemcpyHostToDevice, c->stream),
             "H2D excluded rows");
      exclude_rows = reinterpret_cast<const int64_t*>(base + exc_off);
    }
  }
  EF_HIP(c,
         launch_label_prep(c->stream, any ? nullptr : probe_labels, exclude_rows, b, bpad, c->g_offset, c->gal.n, plab,
                           pexcl),
         "label prep");
  EF_TRY(search_labelled_run(c, bpad, b, metric, relation, plab, pexcl, r.kdev, r.mdev));
  return r.fetch(c);
}

int ef_score_census(ef_ctx* c, const float* Q, int64_t b, int32_t metric, const int32_t* probe_labels,
                    const int64_t* exclude_rows, float lo, float hi, int32_t nbins, int64_t* counts, uint32_t flags) {
  if (!c) return EF_E_INVALID;
  if (c->gal.k == 0) return set_err(c, EF_E_STATE, "ef_score_census: no gallery (call ef_gallery_set)");
  // NaN bounds fail lo < hi; infinite ones the differences
  if (!counts || !probe_labels || b < 0 || (b > 0 && !Q) || (metric != EF_METRIC_L2 && metric != EF_METRIC_COSINE) ||
      nbins < 1 || nbins > kCensusMaxBins || !(lo < hi) || !(hi - lo < __builtin_inff()) || !(lo - lo == 0.f))
    return set_err(c, EF_E_INVALID, "ef_score_census: bad arguments (1 <= nbins <= 2048, finite lo < hi, "
                                    "probe_labels and counts required)");
  if (!c->has_labels)
    return set_err(c, EF_E_STATE, "ef_score_census: the gallery has no labels (call ef_gallery_labels)");
  if (c->comm && c->comm_size > 1)
    return set_err(c, EF_E_STATE, "ef_score_census: no census over a communicator; run each shard on a context "
                                  "without one and add the counts");
  (void)hipSetDevice(c->device);
  const bool dev = (flags & EF_MEM_DEVICE) != 0;
  const Gallery& g = c->gal;
  const size_t cnt_bytes = (size_t)2 * (nbins + 3) * sizeof(int64_t);
  if (b == 0 || g.n == 0) {
    if (dev) EF_HIP(c, hipMemsetAsync(counts, 0, cnt_bytes, c->stream), "zero counts");
    else std::memset(counts, 0, cnt_bytes);
    return EF_OK;
  }
  const int64_t bpad = round_up(b, kSearchProbeTile);
  EF_TRY(stage_queries(c, Q, b, dev, bpad));
  // scratch: plab[bpad], pexcl[bpad], qaux[bpad], then a host call's labels, exclusions and counts
  const size_t lab_off = align256((size_t)3 * bpad * sizeof(int));
  const size_t exc_off = lab_off + align256((size_t)b * sizeof(int32_t));
  const size_t cnt_off = exc_off + align256((size_t)b * sizeof(int64_t));
  EF_TRY(ensure(c, c->label_ws, cnt_off + cnt_bytes));
  char* base = static_cast<char*>(c->label_ws.p);
  int* plab = reinterpret_cast<int*>(base);
  int* pexcl = plab + bpad;
  float* qaux = reinterpret_cast<float*>(pexcl + bpad);
  unsigned long long* cdev = reinterpret_cast<unsigned long long*>(counts);
  if (!dev) {
    EF_HIP(c, hipMemcpyAsync(base + lab_off, probe_labels, (size_t)b * sizeof(int32_t), hipMemcpyHostToDevice, c->stream),
           "H2D probe labels");
    probe_labels = reinterpret_cast<const int32_t*>(base + lab_off);
    if (exclude_rows) {
      EF_HIP(c, hipMemcpyAsync(base + exc_off, exclude_rows, (size_t)b * sizeof(int64_t), hipMemcpyHostToDevice, c->stream),
             "H2D excluded rows");
      exclude_rows = reinterpret_cast<const int64_t*>(base + exc_off);
    }
    cdev = reinterpret_cast<unsigned long long*>(base + cnt_off);
  }
  EF_HIP(c, hipMemsetAsync(cdev, 0, cnt_bytes, c->stream), "zero counts");
  EF_HIP(c, launch_label_prep(c->stream, probe_labels, exclude_rows, b, bpad, c->g_offset, g.n, plab, pexcl),
         "label prep");
  const float* qpad = static_cast<const float*>(c->q_pad.p);
  EF_HIP(c, launch_census_probe_aux(c->stream, qpad, bpad, g.kp, metric, qaux), "census probe norms");
  const float* aux = static_cast<const float*>(metric == EF_METRIC_L2 ? g.gnorm2.p : g.ginv.p);
  for (const SearchPiece& p : search_pieces(b, g.kp))  // a padded probe block stays below 2 GiB
    EF_HIP(c,
           launch_census(c->stream, g.kp, metric, qpad + p.off * g.kp, p.bpad, p.b, static_cast<const float*>(g.G.p),
                         aux, static_cast<const int*>(c->glabels.p), g.n, qaux + p.off, plab + p.off, pexcl + p.off, lo,
                         hi, nbins, cdev),
           "score census");
  if (!dev) {
    EF_HIP(c, hipMemcpyAsync(counts, cdev, cnt_bytes, hipMemcpyDeviceToHost, c->stream), "D2H counts");
    EF_HIP(c, hipStreamSynchronize(c->stream), "sync");
  }
  return EF_OK;
}

// Top-m search of the probes in ctx->q_pad (search_run's contract): keys_dev[b][m] and,
// when match_dev is non-null, match_dev[b][m].  The split scans of EF_OPT_SEARCH_SPLIT_BF16
// apply (3, the single-bf16 screen, counts as 1); the prefix scan never does.
static int search_topk_run(ef_ctx* c, int64_t bpad, int64_t b, int m, int metric, long long* keys_dev,
                           ef_match* match_dev) {
  const Gallery& g = c->gal;
  const int cap = (int)c->opt_search_topk_cand;
  if (cap < m) return set_err(c, EF_E_INVALID, "top-m search: EF_OPT_SEARCH_TOPK_CAND is below m");
  EF_TRY(ensure(c, c->topk_counters, 4 * sizeof(unsigned long long)));
  unsigned long long* counters = static_cast<unsigned long long*>(c->topk_counters.p);
  EF_HIP(c, hipMemsetAsync(counters, 0, 4 * sizeof(unsigned long long), c->stream), "zero counters");
  c->topk_probes = b;
  if (g.n == 0) {
    EF_HIP(c, launch_keys_none(c->stream, keys_dev, b * m, match_dev), "keys");
    return EF_OK;
  }
  if (bpad < round_up(b, kSearchProbeTile))
    return set_err(c, EF_E_INVALID, "top-m search: probe buffer shorter than the batch");
  const int variant = split_variant(c->opt_search_split_bf16, g.kp, true);
  const SearchSchedule sc = search_schedule(b, g.n, g.kp, variant, 0, false, m, cap);
  EF_TRY(ensure(c, c->search_ws, sc.ws_bytes));
  Carve cv{c->search_ws.p};
  const SearchWs ws = carve_search_ws(cv, sc.parts, (size_t)sc.bpad_max);
  const TopkWs tw = carve_topk_ws(cv, (size_t)sc.bpad_max, (size_t)cap);
  SplitScan sp;
  EF_TRY(search_copies(c, variant, 0, false, false, sc.bpad_max, &sp));
  const float* aux = static_cast<const float*>(metric == EF_METRIC_L2 ? g.gnorm2.p : g.ginv.p);
  for (size_t i = 0; i < sc.pieces.size(); ++i) {
    const SearchPiece& p = sc.pieces[i];
    EF_HIP(c,
           launch_search_topk(c->stream, g.kp, metric, sp, m, sc.plans[i],
                              static_cast<const float*>(c->q_pad.p) + p.off * g.kp, p.bpad, p.b,
                              static_cast<const float*>(g.G.p), aux, g.n, c->g_offset, scan_gmax2(c, metric), ws, tw, cap,
                              counters, keys_dev + p.off * m, match_dev ? match_dev + p.off * m : nullptr),
           "top-m search");
  }
  return EF_OK;
}

// Every search entry point: keys and / or match records (and, pixels, the features) of b
// probes.  X is the probe features, or (pixels) the probe pixels to project first; m = 0 is the
// top-1 search (one key per probe, across the communicator when one is attached), m >= 1 the
// top-m search.
static int query_impl(ef_ctx* c, const void* X, bool pixels, int32_t dtype, int64_t b, int32_t m, bool topm,
                      int32_t metric, int64_t* keys, ef_match* match, float* feats, uint32_t flags, const char* fn) {
  if (!c) return EF_E_INVALID;
  const std::string f(fn);
  if (pixels && c->d == 0) return set_err(c, EF_E_STATE, f + ": no model (call ef_model_set)");
  if (c->gal.k == 0) return set_err(c, EF_E_STATE, f + ": no gallery (call ef_gallery_set)");
  if (pixels && c->gal.k != c->k) return set_err(c, EF_E_INVALID, f + ": gallery k != model k");
  if (topm && (m < 1 || m > 64)) return set_err(c, EF_E_INVALID, f + ": m must be 1 .. 64");
  if (!X || (!keys && !match) || b < 0 || (pixels && dtype != EF_U8 && dtype != EF_F32) ||
      (metric != EF_METRIC_L2 && metric != EF_METRIC_COSINE))
    return set_err(c, EF_E_INVALID, f + ": bad arguments");
  if (topm && c->opt_search_topk_cand < m) return set_err(c, EF_E_INVALID, f + ": EF_OPT_SEARCH_TOPK_CAND is below m");
  if (topm && c->comm && c->comm_size > 1)
    return set_err(c, EF_E_STATE, f + ": no top-m search over a communicator; search each shard for its records "
                                      "(ef_search_topk_matches on a context without one) and merge them with "
                                      "ef_matches_merge_topk");
  if (b == 0) return EF_OK;
  (void)hipSetDevice(c->device);
  Results r{(flags & EF_MEM_DEVICE) != 0, b, topm ? m : 1, c->k, keys, match, feats};
  int64_t bpad = round_up(b, kSearchProbeTile);
  if (pixels) {
    const void* Pd = nullptr;
    EF_TRY(stage_probes(c, X, dtype, b, c->d, flags, c->p_stage, &Pd));
    EF_TRY(r.stage_feats(c));
    EF_TRY(project_for_search(c, Pd, dtype, b, r.fdev, &bpad));
  } else {
    EF_TRY(stage_queries(c, static_cast<const float*>(X), b, r.dev, bpad));
  }
  EF_TRY(r.stage_keys(c, bpad));
  EF_TRY(topm ? search_topk_run(c, bpad, b, m, metric, r.kdev, r.mdev) : search_qpad(c, bpad, b, metric, r.kdev, r.mdev));
  return r.fetch(c);
}

int ef_search_topk(ef_ctx* c, const float* Q, int64_t b, int32_t m, int32_t metric, int64_t* keys, uint32_t flags) {
  if (c && !keys) return set_err(c, EF_E_INVALID, "ef_search_topk: bad arguments");
  return query_impl(c, Q, false, EF_F32, b, m, true, metric, keys, nullptr, nullptr, flags, "ef_search_topk");
}

int ef_search_topk_matches(ef_ctx* c, const float* Q, int64_t b, int32_t m, int32_t metric, ef_match* out,
                           uint32_t flags) {
  if (c && !out) return set_err(c, EF_E_INVALID, "ef_search_topk_matches: bad arguments");
  return query_impl(c, Q, false, EF_F32, b, m, true, metric, nullptr, out, nullptr, flags, "ef_search_topk_matches");
}

int ef_recognize_topk(ef_ctx* c, const void* P, int32_t dtype, int64_t b, int32_t m, int32_t metric, int64_t* keys,
                      float* feats, uint32_t flags) {
  if (c && !keys) return set_err(c, EF_E_INVALID, "ef_recognize_topk: bad arguments");
  return query_impl(c, P, true, dtype, b, m, true, metric, keys, nullptr, feats, flags, "ef_recognize_topk");
}

int ef_search_topk_stats(ef_ctx* c, int64_t out[4]) {
  if (!c || !out) return EF_E_INVALID;
  (void)hipSetDevice(c->device);
  EF_HIP(c, hipStreamSynchronize(c->stream), "sync");
  unsigned long long dev[4] = {0, 0, 0, 0};
  if (c->topk_counters.p)
    EF_HIP(c, hipMemcpy(dev, c->topk_counters.p, sizeof dev, hipMemcpyDeviceToHost), "D2H top-m counters");
  out[0] = c->topk_counters.p ? c->topk_probes : 0;
  for (int i = 1; i < 4; ++i) out[i] = (int64_t)dev[i];
  return EF_OK;
}

int ef_search(ef_ctx* c, const float* Q, int64_t b, int32_t metric, int64_t* keys, uint32_t flags) {
  if (c && !keys) return set_err(c, EF_E_INVALID, "ef_search: bad arguments");
  return query_impl(c, Q, false, EF_F32, b, 0, false, metric, keys, nullptr, nullptr, flags, "ef_search");
}

int ef_search_matches(ef_ctx* c, const float* Q, int64_t b, int32_t metric, ef_match* out, uint32_t flags) {
  if (c && !out) return set_err(c, EF_E_INVALID, "ef_search_matches: bad arguments");
  return query_impl(c, Q, false, EF_F32, b, 0, false, metric, nullptr, out, nullptr, flags, "ef_search_matches");
}

int ef_recognize(ef_ctx* c, const void* P, int32_t dtype, int64_t b, int32_t metric, int64_t* keys, float* feats,
                 uint32_t flags) {
  if (c && !keys) return set_err(c, EF_E_INVALID, "ef_recognize: bad arguments");
  return query_impl(c, P, true, dtype, b, 0, false, metric, keys, nullptr, feats, flags, "ef_recognize");
}

int ef_recognize_matches(ef_ctx* c, const void* P, int32_t dtype, int64_t b, int32_t metric, ef_match* out,
                         float* feats, uint32_t flags) {
  if (c && !out) return set_err(c, EF_E_INVALID, "ef_recognize_matches: bad arguments");
  return query_impl(c, P, true, dtype, b, 0, false, metric, nullptr, out, feats, flags, "ef_recognize_matches");
}

int ef_set_option(ef_ctx* c, int32_t option, int64_t value) {
  if (!c) return EF_E_INVALID;
  switch (option) {
    case EF_OPT_FIT_MAX_ITERS:
      if (value < 1) return set_err(c, EF_E_INVALID, "EF_OPT_FIT_MAX_ITERS must be >= 1");
      c->opt_fit_max_iters = value;
      return EF_OK;
    case EF_OPT_FIT_FP32_COARSE:
      if (value < 0 || value > 2) return set_err(c, EF_E_INVALID, "EF_OPT_FIT_FP32_COARSE must be 0, 1 or 2");
      c->opt_fit_fp32_coarse = value;
      return EF_OK;
    case EF_OPT_COV_SLAB_BYTES:
      if (value < 1) return set_err(c, EF_E_INVALID, "EF_OPT_COV_SLAB_BYTES must be >= 1");
      c->opt_cov_slab_bytes = value;
      return EF_OK;
    case EF_OPT_TM_INT64_SUMS:
      c->opt_tm_int64 = value != 0;
      return EF_OK;
    case EF_OPT_HAAR_ORDERED:
      c->opt_haar_ordered = value != 0;
      return EF_OK;
    case EF_OPT_JPEG_CHUNK_BITS:
      if (value < 0 || value > (1 << 24) || value % 32)
        return set_err(c, EF_E_INVALID, "EF_OPT_JPEG_CHUNK_BITS must be 0 or a multiple of 32 up to 2^24");
      c->opt_jpeg_chunk_bits = value;
      return EF_OK;
    case EF_OPT_JPEG_PART_FILES:
      if (value < 1) return set_err(c, EF_E_INVALID, "EF_OPT_JPEG_PART_FILES must be >= 1");
      c->opt_jpeg_part_files = value;
      return EF_OK;
    case EF_OPT_FIT_CHEBYSHEV:
      c->opt_fit_chebyshev = value != 0;
      return EF_OK;
    case EF_OPT_SEARCH_SPLIT_BF16:
      if (value < 0 || value > 3) return set_err(c, EF_E_INVALID, "EF_OPT_SEARCH_SPLIT_BF16 must be 0, 1, 2 or 3");
      c->opt_search_split_bf16 = value;
      return EF_OK;
    case EF_OPT_SEARCH_PREFIX:
      if (value != 0 && value != 1 && value != 16 && value != 32 && value != 64)
        return set_err(c, EF_E_INVALID, "EF_OPT_SEARCH_PREFIX must be 0, 1, 16, 32 or 64");
      if (value >= 16 && c->gal.kp > 0 && value >= c->gal.kp)
        return set_err(c, EF_E_INVALID, "EF_OPT_SEARCH_PREFIX: the prefix must be shorter than the gallery's padded k");
      c->opt_search_prefix = value;
      c->der.reset();  // a new setting starts with a clean guard
      return EF_OK;
    case EF_OPT_SEARCH_PREFIX_SPLIT:
      if (value != 0 && value != 1) return set_err(c, EF_E_INVALID, "EF_OPT_SEARCH_PREFIX_SPLIT must be 0 or 1");
      c->opt_search_prefix_split = value;
      c->der.reset();  // a clean guard; the compact copy is rebuilt in the new arithmetic's layout
      return EF_OK;
    case EF_OPT_SEARCH_PREFIX_SCREEN:
      if (value != 0 && value != 1) return set_err(c, EF_E_INVALID, "EF_OPT_SEARCH_PREFIX_SCREEN must be 0 or 1");
      c->opt_search_prefix_screen = value;
      c->der.reset();  // clean guards
      return EF_OK;
    case EF_OPT_PROJECT_SPLIT_BF16:
      if (value != 0 && value != 1) return set_err(c, EF_E_INVALID, "EF_OPT_PROJECT_SPLIT_BF16 must be 0 or 1");
      c->opt_project_split_bf16 = value;  // read by the next projection; the pieces stay with the model
      return EF_OK;
    case EF_OPT_SEARCH_TOPK_CAND:
      if (value < 16 || value > 4096) return set_err(c, EF_E_INVALID, "EF_OPT_SEARCH_TOPK_CAND must be 16 .. 4096");
      c->opt_search_topk_cand = value;
      return EF_OK;
    case EF_OPT_RANK_BITMAP_BYTES:
      if (value < 1) return set_err(c, EF_E_INVALID, "EF_OPT_RANK_BITMAP_BYTES must be >= 1");
      c->opt_rank_bitmap_bytes = value;
      return EF_OK;
    case EF_OPT_HOST_THREADS:
      if (value < 0 || value > 256) return set_err(c, EF_E_INVALID, "EF_OPT_HOST_THREADS must be 0..256");
      g_host_threads.store((int)value, std::memory_order_relaxed);
      return EF_OK;
    default:
      return set_err(c, EF_E_INVALID, "ef_set_option: unknown option " + std::to_string(option));
  }
}

int ef_get_option(const ef_ctx* c, int32_t option, int64_t* value) {
  if (!c || !value) return EF_E_INVALID;
  switch (option) {
    case EF_OPT_FIT_MAX_ITERS: *value = c->opt_fit_max_iters; return EF_OK;
    case EF_OPT_FIT_FP32_COARSE: *value = c->opt_fit_fp32_coarse; return EF_OK;
    case EF_OPT_COV_SLAB_BYTES: *value = c->opt_cov_slab_bytes; return EF_OK;
    case EF_OPT_TM_INT64_SUMS: *value = c->opt_tm_int64; return EF_OK;
    case EF_OPT_HAAR_ORDERED: *value = c->opt_haar_ordered; return EF_OK;
    case EF_OPT_JPEG_CHUNK_BITS: *value = c->opt_jpeg_chunk_bits; return EF_OK;
    case EF_OPT_SEARCH_SPLIT_BF16: *value = c->opt_search_split_bf16; return EF_OK;
    case EF_OPT_JPEG_PART_FILES: *value = c->opt_jpeg_part_files; return EF_OK;
    case EF_OPT_FIT_CHEBYSHEV: *value = c->opt_fit_chebyshev; return EF_OK;
    case EF_OPT_HOST_THREADS: *value = host_threads(); return EF_OK;
    case EF_OPT_SEARCH_PREFIX: *value = c->opt_search_prefix; return EF_OK;
    case EF_OPT_SEARCH_TOPK_CAND: *value = c->opt_search_topk_cand; return EF_OK;
    case EF_OPT_SEARCH_PREFIX_SPLIT: *value = c->opt_search_prefix_split; return EF_OK;
    case EF_OPT_PROJECT_SPLIT_BF16: *value = c->opt_project_split_bf16; return EF_OK;
    case EF_OPT_SEARCH_PREFIX_SCREEN: *value = c->opt_search_prefix_screen; return EF_OK;
    case EF_OPT_RANK_BITMAP_BYTES: *value = c->opt_rank_bitmap_bytes; return EF_OK;
    default: return EF_E_INVALID;
  }
}

void ef_keys_decode(const int64_t* keys, int64_t b, int32_t metric, float* best, int64_t* idx) {
  for (int64_t i = 0; i < b; ++i) {
    const int64_t key = keys[i];
    if (key == EF_KEY_NONE) {
      if (best) best[i] = NAN;
      if (idx) idx[i] = -1;
      continue;
    }
    const int32_t s = (int32_t)(key >> 32);
    const int32_t bits = s >= 0 ? s : (s ^ 0x7FFFFFFF);
    float v;
    std::memcpy(&v, &bits, sizeof(v));
    if (best) best[i] = metric == EF_METRIC_COSINE ? -v : v;
    if (idx) idx[i] = (int64_t)(uint32_t)(key & 0xffffffffll);
  }
}

int ef_search_stats(ef_ctx* c, int64_t out[4]) {
  if (!c || !out) return EF_E_INVALID;
  (void)hipSetDevice(c->device);
  EF_HIP(c, hipStreamSynchronize(c->stream), "hipStreamSynchronize");
  const int64_t fb = c->stats_prefix ? (int64_t)*static_cast<const int*>(c->prefix_host.p) : 0;
  out[0] = c->stats_probes;
  out[1] = c->stats_prefix ? c->stats_probes - fb : 0;
  out[2] = fb;
  out[3] = c->stats_skipped ? 1 : 0;
  return EF_OK;
}

int ef_prefix_screen_stats(ef_ctx* c, int64_t out[3]) {
  if (!c || !out) return EF_E_INVALID;
  (void)hipSetDevice(c->device);
  EF_HIP(c, hipStreamSynchronize(c->stream), "hipStreamSynchronize");
  const int64_t left = c->stats_screen ? (int64_t) static_cast<const int*>(c->prefix_host.p)[2] : 0;
  out[0] = c->stats_screen ? c->stats_probes : 0;
  out[1] = c->stats_screen ? c->stats_probes - left : 0;
  out[2] = c->stats_screen_skipped ? 1 : 0;
  return EF_OK;
}

int ef_timing_enable(ef_ctx* c, int on) {
  if (!c) return EF_E_INVALID;
  c->timing = on != 0;
  return EF_OK;
}

static int timing_drain(ef_ctx* c) {
  if (c->pending.empty()) return EF_OK;
  EF_HIP(c, hipStreamSynchronize(c->stream), "sync");
  for (auto& t : c->pending) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, t.a, t.b) == hipSuccess && t.kernel >= 0 && t.kernel < kTimers) {
      c->t_ms[t.kernel] += ms;
      c->t_n[t.kernel] += 1;
    }
  }
  c->pending.clear();
  return EF_OK;
}

int ef_timing_get(ef_ctx* c, int32_t kernel, double* total_ms, int64_t* launches) {
  if (!c || kernel < 0 || kernel >= kTimers) return EF_E_INVALID;
  EF_TRY(timing_drain(c));
  if (total_ms) *total_ms = c->t_ms[kernel];
  if (launches) *launches = c->t_n[kernel];
  return EF_OK;
}

int ef_timing_reset(ef_ctx* c) {
  if (!c) return EF_E_INVALID;
  EF_TRY(timing_drain(c));
  for (int i = 0; i < kTimers; ++i) {
    c->t_ms[i] = 0;
    c->t_n[i] = 0;
  }
  return EF_OK;
}

}  // extern "C"
