// Host-only unit checks of the library's internal host layer, linked against the sanitized
// objects (Makefile target `asan`, run by tests/test_host_sanitizers.py).  No HIP call
// reaches the runtime: the four free / destroy entry points the owning handles use are
// defined here (they take precedence over the shared library's) and only count.
//   * Carve / carve_search_ws / carve_prefix_ws against the workspace arithmetic of the
//     search written out by hand;
//   * search_schedule, the plan every search runs and ef_search_schedule reports: pieces,
//     per-piece plans, their maxima and the carved totals against the same arithmetic;
//   * DevBuf, PinnedBuf, Event, Stream: default-empty, move-construct and move-assign leave
//     the source empty, an empty or moved-from handle frees nothing, a full one frees once;
//   * std::vector<DevBuf> resize / clear on empty buffers;
//   * SideJoin never forked, ef_tm_sums_bits at the int32 limits.
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

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

int main() {
  // (parts, bpad_max, k1, kp): parts = nchunks x bpad of the largest piece
  check_carve(256, 256, 0, 16);
  check_carve(256 * 7, 256, 16, 32);
  check_carve(256 * 3, 256, 32, 128);
  check_carve(768 * 41, 768, 0, 512);
  check_carve(1024 * 5, 1024, 64, 128);
  check_carve(4096 * 13, 4096, 16, 64);
  check_carve(33 * 1280, 1280, 32, 128);

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
