// Host-only unit checks of the library's internal host layer, linked against the sanitized
// objects (Makefile target `asan`, run by tests/test_host_sanitizers.py).  No HIP call
// reaches the runtime: the four free / destroy entry points the owning handles use are
// defined here (they take precedence over the shared library's) and only count.
//   * Carve / carve_search_ws / carve_prefix_ws against the workspace arithmetic of the
//     search written out by hand;
//   * carve_frame_out, the frame scans' result block behind either route's front, against its
//     layout written out by hand, and frame_route over every form of a call's outputs;
//   * search_schedule, the plan every search runs and ef_search_schedule reports: pieces,
//     per-piece plans, their maxima and the carved totals against the same arithmetic;
//   * DevBuf, PinnedBuf, Event, Stream: default-empty, move-construct and move-assign leave
//     the source empty, an empty or moved-from handle frees nothing, a full one frees once;
//   * std::vector<DevBuf> resize / clear on empty buffers;
//   * SideJoin never forked, ef_tm_sums_bits at the int32 limits;
//   * RitzPolicy, the fit's Rayleigh-Ritz schedule and acceptance rules, on hand-made Ritz
//     sequences.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "../../face-detection-recognization-pca_amd/csrc/ef_fit_policy.hpp"
#include "../../face-detection-recognization-pca_amd/csrc/ef_internal.hpp"

static int g_frees = 0;
static void* g_last = nullptr;
extern "C" {
hipError_t hipFree(void* p) { ++g_frees; g_last = p; return hipSuccess; }
hipError_t hipHostFree(void* p) { ++g_frees; g_last = p; return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) { ++g_frees; g_last = e; return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t s) { ++g_frees; g_last = s; return hipSuccess; }
}

static int g_fail = 0;
#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                                        \
    }                                                                  \
  } while (0)

using namespace ef;

static size_t al(size_t x) { return (x + 255) & ~size_t(255); }

// the workspaces' sizes written out by hand, as the search laid them out before the helpers
static size_t search_ws_bytes(size_t parts, size_t bpad) {
  return al(parts * 8) + al(parts * 4) + al(16) + al(bpad * 4) + al(bpad * 4) + al(bpad * kCandMax * 4) + al(bpad * 4);
}
static size_t prefix_ws_bytes(size_t bpad, int k1, int kp) {
  return al(bpad * k1 * 4) + al(bpad * (size_t)kp * 4) + al(bpad * 4) + al(bpad * 8) + al(bpad * sizeof(ef_match));
}
static size_t topk_ws_bytes(size_t bpad, size_t cap) { return al(bpad * cap * 4) + 4 * al(bpad * 4) + al(16); }

static void check_carve(size_t parts, size_t bpad, int k1, int kp) {
  const size_t nkb = al(parts * 8), nb2 = al(parts * 4), ncnt = al(16), nlist = al(bpad * 4), nthr = al(bpad * 4);
  const size_t ncand = al(bpad * kCandMax * 4), ncc = al(bpad * 4);
  Carve size;
  const SearchWs none = carve_search_ws(size, parts, bpad);
  CHECK(size.total == nkb + nb2 + ncnt + nlist + nthr + ncand + ncc);
  CHECK(size.total == search_ws_bytes(parts, bpad));
  CHECK(!none.part_key && !none.part_b2 && !none.amb_count && !none.amb_list && !none.thr && !none.cand &&
        !none.cand_cnt && !none.match);
  std::vector<char> mem(size.total + 256);
  char* base = reinterpret_cast<char*>(al(reinterpret_cast<size_t>(mem.data())));
  Carve cv{base};
  const SearchWs ws = carve_search_ws(cv, parts, bpad);
  CHECK(cv.total == size.total);
  size_t off = 0;
  CHECK(reinterpret_cast<char*>(ws.part_key) == base + off); off += nkb;
  CHECK(reinterpret_cast<char*>(ws.part_b2) == base + off); off += nb2;
  CHECK(reinterpret_cast<char*>(ws.amb_count) == base + off); off += ncnt;
  CHECK(reinterpret_cast<char*>(ws.amb_list) == base + off); off += nlist;
  CHECK(reinterpret_cast<char*>(ws.thr) == base + off); off += nthr;
  CHECK(reinterpret_cast<char*>(ws.cand) == base + off); off += ncand;
  CHECK(reinterpret_cast<char*>(ws.cand_cnt) == base + off);
  CHECK(ws.match == nullptr);
  // the last piece lies inside the allocation (written, so the sanitizer sees it)
  ws.cand_cnt[bpad - 1] = 1;
  ws.part_key[parts - 1] = 1;
  if (k1 <= 0) return;
  const size_t nq1 = al(bpad * k1 * 4), nq2 = al(bpad * (size_t)kp * 4), nk2 = al(bpad * 8);
  const size_t nm2 = al(bpad * sizeof(ef_match));
  Carve psize;
  carve_prefix_ws(psize, bpad, k1, kp);
  CHECK(psize.total == nq1 + nq2 + nlist + nk2 + nm2);
  CHECK(psize.total == prefix_ws_bytes(bpad, k1, kp));
  std::vector<char> pmem(psize.total + 256);
  char* pb = reinterpret_cast<char*>(al(reinterpret_cast<size_t>(pmem.data())));
  Carve pcv{pb};
  const PrefixWs pw = carve_prefix_ws(pcv, bpad, k1, kp);
  CHECK(pcv.total == psize.total);
  off = 0;
  CHECK(reinterpret_cast<char*>(pw.q1) == pb + off); off += nq1;
  CHECK(reinterpret_cast<char*>(pw.qpad2) == pb + off); off += nq2;
  CHECK(reinterpret_cast<char*>(pw.list) == pb + off); off += nlist;
  CHECK(reinterpret_cast<char*>(pw.keys2) == pb + off); off += nk2;
  CHECK(reinterpret_cast<char*>(pw.match2) == pb + off);
  pw.match2[bpad - 1].key = 1;
}

// ---- the frame scans' result block (carve_frame_out) and output routing (frame_route) ----
// the block's size written out by hand: a front of dets[g] (32-byte records) or of head[1]
// (16 bytes) and rects[g][4], then keys[g][M], best[g], rows[g][d] and, gated, dffs2 and energy
static size_t frame_out_bytes(bool haar, size_t g, size_t M, size_t d, bool gated) {
  const size_t front = haar ? al(16) + al(g * 16) : al(g * 32);
  return front + al(g * M * 8) + al(g * 4) + al(g * d) + (gated ? 2 * al(g * M * 4) : 0);
}

static void check_frame_out(bool haar, size_t g, size_t M, size_t d) {
  static_assert(sizeof(ef_scan_det) == 32 && sizeof(ef_haar_scan_head) == 16, "front records");
  const FrameFront fr = haar ? FrameFront{2, {sizeof(ef_haar_scan_head), g * 4 * sizeof(int)}}
                             : FrameFront{1, {g * sizeof(ef_scan_det)}};
  std::vector<char> mem(frame_out_bytes(haar, g, M, d, true) + 256);
  char* base = reinterpret_cast<char*>(al(reinterpret_cast<size_t>(mem.data())));
  FrameOut both[2];
  for (int gated = 0; gated <= 1; ++gated) {
    Carve size;
    const FrameOut none = carve_frame_out(size, fr, g, M, d, gated != 0);
    CHECK(size.total == frame_out_bytes(haar, g, M, d, gated != 0));
    CHECK(!none.front[0] && !none.front[1] && !none.keys && !none.best && !none.rows && !none.dffs2 && !none.energy);
    Carve cv{base};
    const FrameOut o = both[gated] = carve_frame_out(cv, fr, g, M, d, gated != 0);
    CHECK(cv.total == size.total);  // the size pass and the pointer pass agree
    // the pieces in order, each 256-byte aligned
    size_t off = 0;
    CHECK(static_cast<char*>(o.front[0]) == base + off); off += al(haar ? 16 : g * 32);
    if (haar) { CHECK(static_cast<char*>(o.front[1]) == base + off); off += al(g * 16); }
    else CHECK(o.front[1] == nullptr);
    CHECK(reinterpret_cast<char*>(o.keys) == base + off); off += al(g * M * 8);
    CHECK(reinterpret_cast<char*>(o.best) == base + off); off += al(g * 4);
    CHECK(reinterpret_cast<char*>(o.rows) == base + off); off += al(g * d);
    if (gated) {
      CHECK(reinterpret_cast<char*>(o.dffs2) == base + off); off += al(g * M * 4);
      CHECK(reinterpret_cast<char*>(o.energy) == base + off); off += al(g * M * 4);
      o.energy[g * M - 1] = 1.f;  // the last piece lies inside the allocation
    } else {
      CHECK(!o.dffs2 && !o.energy);
      o.rows[g * d - 1] = 1;
    }
    CHECK(off == size.total && off % 256 == 0);
  }
  // the ungated block is a byte prefix of the gated one
  CHECK(both[0].front[0] == both[1].front[0] && both[0].front[1] == both[1].front[1] && both[0].keys == both[1].keys &&
        both[0].best == both[1].best && both[0].rows == both[1].rows);
  CHECK(frame_out_bytes(haar, g, M, d, false) + 2 * al(g * M * 4) == frame_out_bytes(haar, g, M, d, true));
}

static void check_frame_route() {
  // distinct fake addresses: nothing is dereferenced
  auto at = [](size_t v) { return reinterpret_cast<char*>(v); };
  const FrameOut blk{{at(0x1000), at(0x1100)}, reinterpret_cast<long long*>(at(0x1200)),
                     reinterpret_cast<int*>(at(0x1300)), reinterpret_cast<uint8_t*>(at(0x1400)),
                     reinterpret_cast<float*>(at(0x1500)), reinterpret_cast<float*>(at(0x1600))};
  for (int dev = 0; dev <= 1; ++dev)
    for (int has_rows = 0; has_rows <= 1; ++has_rows)
      for (int has_energy = 0; has_energy <= 1; ++has_energy)
        for (int gated = 0; gated <= 1; ++gated) {
          const FrameOut caller{{at(0x2000), at(0x2100)}, reinterpret_cast<long long*>(at(0x2200)),
                                reinterpret_cast<int*>(at(0x2300)),
                                has_rows ? reinterpret_cast<uint8_t*>(at(0x2400)) : nullptr,
                                reinterpret_cast<float*>(at(0x2500)),
                                has_energy ? reinterpret_cast<float*>(at(0x2600)) : nullptr};
          const FrameRoute r = frame_route(caller, dev != 0, gated != 0, blk);
          const FrameOut& o = r.o;
          if (!dev) {  // the host form writes everything into the block
            CHECK(r.need);
            CHECK(o.front[0] == blk.front[0] && o.front[1] == blk.front[1] && o.keys == blk.keys && o.best == blk.best &&
                  o.rows == blk.rows && o.dffs2 == blk.dffs2 && o.energy == blk.energy);
            continue;
          }
          // the device form writes to the caller's arrays ...
          CHECK(o.front[0] == caller.front[0] && o.front[1] == caller.front[1] && o.keys == caller.keys &&
                o.best == caller.best && o.dffs2 == caller.dffs2);
          // ... except the rows and (gated) the energy, which fall back to the block exactly when null
          CHECK(o.rows == (has_rows ? caller.rows : blk.rows));
          CHECK(o.energy == (has_energy ? caller.energy : gated ? blk.energy : nullptr));
          // and the block is asked for exactly when something falls back to it
          CHECK(r.need == (o.rows == blk.rows || o.energy == blk.energy));
          CHECK(r.need == (!has_rows || (gated && !has_energy)));
        }
}

static bool same_plan(const SearchPlan& a, const SearchPlan& b) {
  return a.n_ptiles == b.n_ptiles && a.nchunks == b.nchunks && a.tiles_per_chunk == b.tiles_per_chunk &&
         a.pblk == b.pblk && a.cblk == b.cblk && a.c_chunks == b.c_chunks && a.c_tpc == b.c_tpc && a.c_grid == b.c_grid;
}

// search_schedule at one shape: scan variants 0 and 1, every prefix length k1 < kp <= 128 in
// both prefix arithmetics, and the top-m plans of m = 1 and 64 (never with a prefix scan)
static void check_schedule(int64_t b, int64_t n, int kp, size_t want_pieces) {
  const int cap = 1024;
  for (int variant = 0; variant <= 1; ++variant)
    for (int k1 : {0, 16, 32})
      for (int split1 = 0; split1 <= (k1 ? 1 : 0); ++split1)
        for (int m : {0, 1, 64}) {
          if (k1 && (k1 >= kp || kp > 128 || m)) continue;
          const SearchSchedule sc = search_schedule(b, n, kp, variant, k1, split1 != 0, m, cap);
          CHECK(sc.pieces.size() == want_pieces && sc.plans.size() == want_pieces);
          CHECK(sc.plans1.size() == (k1 ? want_pieces : 0));
          int64_t off = 0, bpad_max = 0;
          size_t parts = 0;
          for (size_t i = 0; i < sc.pieces.size(); ++i) {
            const SearchPiece& p = sc.pieces[i];
            CHECK(p.off == off && p.b >= 1 && p.bpad == round_up(p.b, kSearchProbeTile));
            off += p.b;
            // every piece is planned from its own bpad
            const SearchPlan& pl = sc.plans[i];
            CHECK(same_plan(pl, search_plan(p.bpad, n, kp, variant != 0, 0, m)));
            CHECK(pl.n_ptiles >= 1 && p.bpad % pl.n_ptiles == 0);
            // min_chunks raises nchunks to a multiple of 8 that is at least m
            CHECK(pl.nchunks % 8 == 0 && pl.nchunks >= 8 && pl.nchunks >= m);
            bpad_max = std::max(bpad_max, p.bpad);
            parts = std::max(parts, (size_t)pl.nchunks * (size_t)p.bpad);
            if (k1) {
              CHECK(same_plan(sc.plans1[i], search_plan(p.bpad, n, k1, false, prefix_tile_rows(k1, split1 != 0))));
              parts = std::max(parts, (size_t)sc.plans1[i].nchunks * (size_t)p.bpad);
            }
          }
          CHECK(off == b);
          CHECK(sc.bpad_max == bpad_max && sc.parts == parts);  // the maxima over the pieces
          CHECK(sc.ws_bytes == search_ws_bytes(parts, (size_t)bpad_max) + (m ? topk_ws_bytes((size_t)bpad_max, cap) : 0));
          CHECK(sc.prefix_bytes == (k1 ? prefix_ws_bytes((size_t)bpad_max, k1, kp) : 0));
        }
}

// H: an owning handle; set / get write and read its handle field (fake values: nothing is freed for real)
template <class H, class Set, class Get>
static void check_owner(Set set, Get get) {
  void* const fake = reinterpret_cast<void*>(0x1000);
  g_frees = 0;
  {
    H empty;
    CHECK(get(empty) == nullptr);
  }
  CHECK(g_frees == 0);  // destroying an empty handle frees nothing
  {
    H a;
    set(a, fake);
    H b(std::move(a));  // move-construct
    CHECK(get(a) == nullptr && get(b) == fake);
    H c;
    c = std::move(b);  // move-assign into an empty handle
    CHECK(get(b) == nullptr && get(c) == fake && g_frees == 0);
    H d;
    set(d, reinterpret_cast<void*>(0x2000));
    d = std::move(c);  // move-assign over a full handle frees what it held, once
    CHECK(g_frees == 1 && g_last == reinterpret_cast<void*>(0x2000));
    CHECK(get(c) == nullptr && get(d) == fake);
    d.reset();         // early free leaves the handle empty
    CHECK(g_frees == 2 && g_last == fake && get(d) == nullptr);
    d.reset();
    CHECK(g_frees == 2);
  }
  CHECK(g_frees == 2);  // a, b, c (moved from) and d (reset) freed nothing more
  {
    H e;
    set(e, fake);
  }
  CHECK(g_frees == 3 && g_last == fake);  // the destructor of a full handle frees once
}

// ---- RitzPolicy (csrc/ef_fit_policy.hpp): the fit's Rayleigh-Ritz rules on hand-made Ritz
// sequences, each expectation written out from the rule's own comment.  kk = 2 kept pairs in
// a block of m = 4, Chebyshev and shift on, order 2048 (period 16, early steps) unless said.
static RitzPolicy policy(int64_t dim = 2048, int max_iters = 100, bool cheb = true, bool shift = true,
                         bool coarse = false) {
  return RitzPolicy(dim, 2, 4, max_iters, cheb, shift, coarse);
}
// One step on the Ritz values th of C: the solver hands over those of C - sigma I
static RitzStep step_at(RitzPolicy& p, int it, const double (&th)[4], const double* rnorm) {
  double raw[4];
  for (int i = 0; i < 4; ++i) raw[i] = th[i] - p.sigma;
  return p.step(it, raw, rnorm);
}

static void check_policy_schedule() {
  {  // 1: before any step, order 2048: the early steps 1, 2, 4 and the first scheduled one, 8
    const RitzPolicy p = policy();
    for (int it = 1; it <= 8; ++it) CHECK(p.rr_due(it) == (it == 1 || it == 2 || it == 4 || it == 8));
    const RitzPolicy big = policy(16384);  // no early steps from order 12288 on
    for (int it = 1; it <= 8; ++it) CHECK(big.rr_due(it) == (it == 8));
    const RitzPolicy capped = policy(16384, 5);  // the last iteration always takes a step
    CHECK(capped.rr_due(5) && !capped.rr_due(3) && capped.rr_due(8));
    CHECK(policy(2048, 3).rr_due(3));
  }
  {  // 2: Jacobi tolerance: 1e-2 first coarse step, 1e-4 later coarse steps, 1e-12 when fine
    const double th[4] = {1.0, 0.9, 0.8, 0.7}, moved[4] = {1.5, 1.2, 0.9, 0.7};
    RitzPolicy p = policy(4096, 100, false, true, true);  // (no rate: only the 1e-4 rule ends the phase)
    CHECK(!p.fine() && p.jacobi_tol() == 1e-2);
    CHECK(!step_at(p, 8, th, nullptr).accepted);
    CHECK(!p.fine() && p.jacobi_tol() == 1e-4);  // (the first step has nothing to compare with: still coarse)
    step_at(p, 16, moved, nullptr);
    CHECK(!p.fine() && p.jacobi_tol() == 1e-4);
    RitzPolicy f = policy();
    CHECK(f.fine() && f.jacobi_tol() == 1e-12);  // fine, first step or not
    step_at(f, 1, th, nullptr);
    CHECK(f.jacobi_tol() == 1e-12);
  }
  {  // 9: the medium int8 form: it >= 5, and no step reads this product (it + 1 < next_rr) or
     // the last one (it + 1 < max_iters); next_rr is 8 before any step
    const RitzPolicy p = policy();
    CHECK(!p.medium(4) && p.medium(5) && p.medium(6) && !p.medium(7) && !p.medium(8));
    const RitzPolicy capped = policy(2048, 7);
    CHECK(capped.medium(5) && !capped.medium(6));
    RitzPolicy late = policy();
    late.next_rr = 32;
    CHECK(!late.medium(4) && late.medium(5) && late.medium(30) && !late.medium(31));
  }
}

static void check_policy_acceptance() {
  const double th[4] = {1.0, 0.9, 0.8, 0.7};  // all gaps 0.1 theta_1
  {  // 3: the value rule needs two consecutive fine steps.  Residuals up to 1e-8 theta_1 (the
     // larger in pair 2): above resid_tol (1e-9), within the gap rule (1e-8 <= 1e-5 x 0.1)
    const double r[2] = {0.5e-8, 1e-8};
    RitzPolicy p = policy(2048, 100, true, true, true);
    CHECK(!step_at(p, 1, th, nullptr).accepted);  // coarse step
    p.coarse = false;                             // the products are fp64 from here on
    CHECK(p.wants_resid());
    CHECK(!step_at(p, 2, th, r).accepted);  // fine, but the step before was not
    const RitzStep s = step_at(p, 4, th, r);
    CHECK(s.accepted && s.worst == 0.0 && std::fabs(s.resid_max - 1e-8) < 1e-20);
    // "unchanged" is 1e-13 relative: theta_2 moving by 1e-12 is not, by 5e-14 is
    const double moved[4] = {1.0, 0.9 * (1.0 + 1e-12), 0.8, 0.7};
    const double settled[4] = {1.0, moved[1] * (1.0 + 5e-14), 0.8, 0.7};
    const RitzStep t = step_at(p, 8, moved, r);
    CHECK(!t.accepted && t.worst_i == 1 && t.worst > 0.9e-12 && t.worst < 1.1e-12);
    CHECK(step_at(p, 9, settled, r).accepted);
  }
  {  // 4: the residual rule accepts from one fine step when every kept pair's residual is
     // <= 1e-9 theta_1: pair 2 at 0.9e-9 passes, at 2e-9 it does not
    for (int pass = 0; pass <= 1; ++pass) {
      const double r[2] = {1e-10, pass ? 0.9e-9 : 2e-9};
      RitzPolicy p = policy(2048, 100, true, true, true);
      CHECK(!p.wants_resid());
      CHECK(!step_at(p, 1, th, nullptr).accepted);
      p.coarse = false;
      const RitzStep s = step_at(p, 2, th, r);
      CHECK(s.accepted == (pass == 1) && std::fabs(s.resid_max - r[1]) < 1e-20);
    }
  }
  {  // 5: the gap rule vetoes, and places the next step.  theta_2 - theta_3 = 1e-4 theta_1:
     // pair 2's bound is max(1e-5 x 1e-4, 1e-12) theta_1 = 1e-9 theta_1, its residual 1e-8
     // theta_1, need = 10.  theta_m = 0.45: sigma = 0.225, x = theta_k / sigma - 1 = 1.22, so
     // the rule asks for ceil(acosh(2 need) / acosh(x)) = ceil(3.69 / 0.655) = 6 more products
    const double tg[4] = {1.0, 0.5, 0.5 - 1e-4, 0.45};
    const double r[2] = {1e-8, 1e-8};
    const double bound = std::fmax(1e-5 * (tg[1] - tg[2]), 1e-12 * tg[0]);
    const double x = tg[1] / (0.5 * tg[3]) - 1.0;
    const int p1 = (int)std::ceil(std::acosh(2.0 * (r[1] / bound)) / std::acosh(x));
    CHECK(p1 == 6);
    for (int stalls = 0; stalls <= 1; ++stalls) {
      RitzPolicy p = policy();
      const RitzStep a = step_at(p, 4, tg, r);  // first step: neither the rate nor the value rule places
      CHECK(!a.accepted && a.gap_i == 1 && a.gap_worst > 0.99e-4 && a.gap_worst < 1.01e-4);
      CHECK(p.next_rr == 4 + p1);  // 10, past the 8 every earlier step falls back to
      CHECK(!p.rr_due(8) && p.rr_due(10));
      if (stalls) {  // values converged and the residuals no longer shrinking: the arithmetic's floor
        CHECK(step_at(p, 10, tg, r).accepted);
      } else {  // residuals still shrinking (0.4 x, need = 4): not yet.  The value and rate rules
                // ask for the very next iteration (unchanged values), the gap rule for
                // ceil(acosh(8) / acosh(x)) = ceil(2.77 / 0.655) = 5 more products
        const double r2[2] = {0.4e-8, 0.4e-8};
        const int p2 = (int)std::ceil(std::acosh(2.0 * (r2[1] / bound)) / std::acosh(x));
        CHECK(p2 == 5);
        CHECK(!step_at(p, 10, tg, r2).accepted);
        CHECK(p.next_rr == 10 + p2);
      }
    }
  }
  {  // 6: an exactly degenerate kept pair (gap 0) with residual 5e-13 theta_1 <= kResidFloor
    const double td[4] = {1.0, 1.0, 0.8, 0.7};
    const double r[2] = {5e-13, 5e-13};
    RitzPolicy p = policy();
    CHECK(step_at(p, 1, td, r).accepted);
    const double r2[2] = {5e-12, 5e-12};  // above the floor: the gap rule holds it back
    RitzPolicy q = policy();
    CHECK(!step_at(q, 1, td, r2).accepted);
  }
  {  // 10: a non-finite theta_1 reports divergence and changes no state
    RitzPolicy p = policy(2048, 100, true, true, true);
    step_at(p, 1, th, nullptr);
    const RitzPolicy before = p;
    const double bad[4] = {NAN, 0.9, 0.8, 0.7}, r[2] = {1.0, 1.0};
    const RitzStep s = p.step(2, bad, r);
    CHECK(s.diverged && !s.accepted);
    CHECK(p.coarse == before.coarse && p.sigma == before.sigma && p.prev == before.prev);
    CHECK(p.have_prev == before.have_prev && p.prev_fine == before.prev_fine && p.last_worst == before.last_worst);
    CHECK(p.prev_resid_max == before.prev_resid_max && p.rate_prev == before.rate_prev);
    CHECK(p.last_rr_it == before.last_rr_it && p.next_rr == before.next_rr);
    const double inf[4] = {INFINITY, 0.9, 0.8, 0.7};
    CHECK(p.step(2, inf, nullptr).diverged && p.last_rr_it == before.last_rr_it);
  }
}

static void check_policy_phase_and_shift() {
  {  // 7: the coarse phase ends when the kept values moved by < 1e-4 since the previous step
    const double a[4] = {1.0, 0.9, 0.8, 0.7}, b[4] = {1.0 + 0.5e-4, 0.9, 0.8, 0.7};
    RitzPolicy p = policy(4096, 100, true, true, true);
    step_at(p, 8, a, nullptr);
    CHECK(p.coarse);
    const RitzStep s = step_at(p, 16, b, nullptr);
    CHECK(s.worst > 0.4e-4 && s.worst < 0.6e-4 && s.worst_i == 0 && !p.coarse);
    // ... not at 1e-3 when no rate predicts the error (Chebyshev off: rate_prev = 0)
    const double c[4] = {1.0 + 1e-3, 0.9, 0.8, 0.7};
    RitzPolicy q = policy(4096, 100, false, true, true);
    step_at(q, 8, a, nullptr);
    CHECK(q.rate_prev == 0.0);
    const RitzStep t = step_at(q, 16, c, nullptr);
    CHECK(t.worst > 0.9e-3 && t.worst < 1.1e-3 && q.coarse);
    // with the rate (x = 0.9 / 0.35 - 1, rho^2 = 7.7 per product) the 8 products since the
    // last step predict 1e-3 / 7.7^8 < 1e-6: the phase ends
    RitzPolicy u = policy(4096, 100, true, true, true);
    step_at(u, 8, a, nullptr);
    CHECK(u.rate_prev > 0.12 && u.rate_prev < 0.14);
    step_at(u, 16, c, nullptr);
    CHECK(!u.coarse);
  }
  {  // 8: the next shift is theta_m / 2 when theta_m > 0, else 0; 0 with the shift off
    const double a[4] = {1.0, 0.9, 0.8, 0.5}, z[4] = {1.0, 0.9, 0.8, 0.0}, n[4] = {1.0, 0.9, 0.8, -0.125};
    RitzPolicy p = policy();
    CHECK(step_at(p, 1, a, nullptr).sigma_next == 0.25 && p.sigma == 0.25);
    CHECK(p.theta()[3] == 0.5 && p.theta()[0] == 1.0);  // reported unshifted
    CHECK(step_at(p, 2, a, nullptr).sigma_next == 0.25);  // (handed over shifted by 0.25)
    CHECK(step_at(p, 4, z, nullptr).sigma_next == 0.0);
    CHECK(step_at(p, 8, n, nullptr).sigma_next == 0.0 && p.sigma == 0.0 && p.rate_prev == 0.0);
    RitzPolicy off = policy(2048, 100, true, false);
    CHECK(step_at(off, 1, a, nullptr).sigma_next == 0.0 && off.rate_prev == 0.0);
    // Chebyshev on: rate = 1 / rho^2, rho = x + sqrt(x^2 - 1), x = theta_k / sigma - 1 = 2.6
    RitzPolicy on = policy();
    step_at(on, 1, a, nullptr);
    const double rho = 2.6 + std::sqrt(2.6 * 2.6 - 1.0);
    CHECK(std::fabs(on.rate_prev - 1.0 / (rho * rho)) < 1e-15);
    // Chebyshev off: the rate is 0, and next_rr follows the period (16 below order 12288, 8
    // from there; 8 before iteration 8) and the one-step-later rule only
    RitzPolicy q = policy(2048, 100, false);
    step_at(q, 1, a, nullptr);
    CHECK(q.rate_prev == 0.0 && q.sigma == 0.25 && q.next_rr == 8);
    const double a6[4] = {1.0 + 1e-6, 0.9, 0.8, 0.5}, a10[4] = {1.0 + 1e-6 + 1e-10, 0.9, 0.8, 0.5};
    step_at(q, 8, a6, nullptr);  // worst 1e-6 after 1: predicted 1e-12 > 3e-14
    CHECK(q.next_rr == 16);
    step_at(q, 16, a10, nullptr);  // worst 1e-10 after 1e-6: predicted 1e-14 <= 3e-14
    CHECK(q.rate_prev == 0.0 && q.next_rr == 17);
    step_at(q, 17, a, nullptr);  // moving again: back to the period
    CHECK(q.next_rr == 32);
    RitzPolicy big = policy(16384, 100, false);
    step_at(big, 8, a, nullptr);
    CHECK(big.next_rr == 16);
    step_at(big, 16, a6, nullptr);
    CHECK(big.next_rr == 24);
  }
}

// Where the next step goes when the Chebyshev rate is known.  theta_k = 0.9, theta_m = 0.5:
// sigma = 0.25, x = 2.6, rho = x + sqrt(x^2 - 1) = 5, so each product shrinks the error 25 x
static void check_policy_placement() {
  const double a[4] = {1.0, 0.9, 0.8, 0.5};
  const double rate = 1.0 / 25.0;
  {  // fine steps at 1 and 4, theta_1 moved by 1e-6: the three products since step 1 leave
     // e = 1e-6 / 25^3 = 6.4e-11, which reaches 3e-14 after ceil(log(e / 3e-14) / log 25) =
     // ceil(7.67 / 3.22) = 3 more: the step goes to 7, before the fallback 8
    const double a6[4] = {1.0 + 1e-6, 0.9, 0.8, 0.5};
    RitzPolicy p = policy();
    step_at(p, 1, a, nullptr);
    CHECK(std::fabs(p.rate_prev - rate) < 1e-15 && p.next_rr == 8);
    const RitzStep s = step_at(p, 4, a6, nullptr);
    const double e = (a6[0] - a[0]) / a6[0] * std::pow(rate, 4 - 1);
    const int want = (int)std::ceil(std::log(e / 3e-14) / std::log(1.0 / rate));
    CHECK(want == 3 && !s.accepted && p.next_rr == 4 + want);
  }
  {  // the step that ends the coarse phase (values moved by 5e-5 < 1e-4): its Ritz values carry
     // the reduced-precision products' error, so the prediction starts from 3e-7, not from
     // 5e-5 / 25^8: ceil(log(1e7) / log 25) = ceil(16.1 / 3.22) = 6 products, 16 + 6 = 22
    const double b[4] = {1.0 + 5e-5, 0.9, 0.8, 0.5};
    RitzPolicy p = policy(4096, 100, true, true, true);
    step_at(p, 8, a, nullptr);
    CHECK(p.coarse && p.next_rr == 16);
    step_at(p, 16, b, nullptr);
    const int want = (int)std::ceil(std::log(3e-7 / 3e-14) / std::log(1.0 / rate));
    CHECK(want == 6 && !p.coarse && p.next_rr == 16 + want);
  }
  {  // exactly unchanged values (binary fractions, so the shift adds no rounding): nothing is
     // left to predict, log 0 = -inf, and the step count takes its floor of 1.  At 16 the
     // value rule asks for 17 as well; at 17 the change before was 0 too, so only the rate
     // rule places the step
    const double e[4] = {1.0, 0.875, 0.75, 0.5};
    RitzPolicy p = policy();
    step_at(p, 8, e, nullptr);
    CHECK(p.next_rr == 16);
    CHECK(step_at(p, 16, e, nullptr).worst == 0.0 && p.next_rr == 17);
    CHECK(step_at(p, 17, e, nullptr).worst == 0.0 && p.last_worst == 0.0 && p.next_rr == 18);
  }
}

int main() {
  check_policy_schedule();
  check_policy_acceptance();
  check_policy_phase_and_shift();
  check_policy_placement();

  // (parts, bpad_max, k1, kp): parts = nchunks x bpad of the largest piece
  check_carve(256, 256, 0, 16);
  check_carve(256 * 7, 256, 16, 32);
  check_carve(256 * 3, 256, 32, 128);
  check_carve(768 * 41, 768, 0, 512);
  check_carve(1024 * 5, 1024, 64, 128);
  check_carve(4096 * 13, 4096, 16, 64);
  check_carve(33 * 1280, 1280, 32, 128);

  // (template or Haar front, g, M, d)
  for (int haar = 0; haar <= 1; ++haar) {
    check_frame_out(haar != 0, 1, 1, 1);
    check_frame_out(haar != 0, 3, 3, 4096);
    check_frame_out(haar != 0, 8, 3, 1024);
    check_frame_out(haar != 0, 64, 64, 4096);
  }
  check_frame_route();

  // (b, n, kp, pieces): planning only, nothing is allocated
  check_schedule(1, 1, 16, 1);
  check_schedule(256, 64, 128, 1);
  check_schedule(257, 65, 128, 1);
  check_schedule(4096, 1000000, 128, 1);
  check_schedule(300, 193, 256, 1);
  check_schedule(300, 193, 640, 1);
  {
    // search_pieces' rule: whole 256-probe tiles whose rows' byte offsets stay below 2^31;
    // one probe more than a piece holds is the smallest batch of two pieces
    const int kp = 65536;
    const int64_t piece = std::max<int64_t>(kSearchProbeTile, ((int64_t)INT_MAX / ((int64_t)kp * 4)) / kSearchProbeTile * kSearchProbeTile);
    CHECK(piece == 7936);
    check_schedule(piece, 1000, kp, 1);
    check_schedule(piece + 1, 1000, kp, 2);
    // the resolved variants: 3 only for wide k in the top-1 search
    CHECK(split_variant(0, 128, false) == 0 && split_variant(1, 640, false) == 1 && split_variant(2, 128, true) == 2);
    CHECK(split_variant(3, 128, false) == 1 && split_variant(3, 256, false) == 3 && split_variant(3, 256, true) == 1);
    CHECK(split_layout(1) == 1 && split_layout(2) == 1 && split_layout(3) == 3);
  }

  check_owner<DevBuf>([](DevBuf& b, void* p) { b.p = p; b.bytes = 64; }, [](const DevBuf& b) { return b.p; });
  check_owner<PinnedBuf>([](PinnedBuf& b, void* p) { b.p = p; b.bytes = 64; }, [](const PinnedBuf& b) { return b.p; });
  check_owner<Event>([](Event& e, void* p) { e.p = static_cast<hipEvent_t>(p); },
                     [](const Event& e) { return static_cast<void*>(e.p); });
  check_owner<Stream>([](Stream& s, void* p) { s.p = static_cast<hipStream_t>(p); },
                      [](const Stream& s) { return static_cast<void*>(s.p); });
  {
    DevBuf a;
    a.p = reinterpret_cast<void*>(0x1000);
    a.bytes = 64;
    DevBuf b(std::move(a));
    CHECK(a.bytes == 0 && b.bytes == 64);  // the size moves with the pointer
  }

  g_frees = 0;
  {
    std::vector<DevBuf> pool;  // the fit's pool: grown slot by slot, emptied by ef_trim
    for (size_t n = 1; n <= 40; ++n) pool.resize(n);
    CHECK(pool.size() == 40 && pool[39].p == nullptr && pool[0].bytes == 0);
    pool.resize(3);
    pool.clear();
    CHECK(pool.empty());
    std::vector<TimerEvt> pending;
    TimerEvt t;
    pending.push_back(std::move(t));
    pending.clear();
    SideStream side;
    SideJoin join(side, nullptr);  // never forked: join() and the destructor do nothing
    CHECK(join.join() == hipSuccess);
  }
  CHECK(g_frees == 0);

  CHECK(ef_tm_sums_bits(INT32_MAX, INT32_MAX, 1) == 64);
  CHECK(ef_tm_sums_bits(1, 1, 0) == 32);

  if (g_fail) return 1;
  std::printf("host_units: clean\n");
  return 0;
}
