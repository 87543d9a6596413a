// Host-only unit checks of the library's internal host layer, linked against the sanitized
// objects (Makefile target `asan`, run by tests/test_host_sanitizers.py).  No HIP call
// reaches the runtime: the four free / destroy entry points the owning handles use are
// defined here (they take precedence over the shared library's) and only count.
//   * Carve / carve_search_ws / carve_prefix_ws against the workspace arithmetic of the
//     search written out by hand;
//   * DevBuf, PinnedBuf, Event, Stream: default-empty, move-construct and move-assign leave
//     the source empty, an empty or moved-from handle frees nothing, a full one frees once;
//   * std::vector<DevBuf> resize / clear on empty buffers;
//   * SideJoin never forked, ef_tm_sums_bits at the int32 limits.
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

static void check_carve(size_t parts, size_t bpad, int k1, int kp) {
  // the search workspace as search_local laid it out before the helper
  const size_t nkb = al(parts * 8), nb2 = al(parts * 4), ncnt = al(16), nlist = al(bpad * 4), nthr = al(bpad * 4);
  const size_t ncand = al(bpad * kCandMax * 4), ncc = al(bpad * 4);
  Carve size;
  const SearchWs none = carve_search_ws(size, parts, bpad);
  CHECK(size.total == nkb + nb2 + ncnt + nlist + nthr + ncand + ncc);
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
