// Internal declarations shared by the libeigenface translation units.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "../../include/eigenface.h"

struct ef_ctx;

namespace ef {

int set_err(ef_ctx* c, int code, const std::string& msg);
int hip_err(ef_ctx* c, hipError_t e, const char* what);

// ---- padded widths ------------------------------------------------------------------
// Gallery / probe features are stored with k zero-padded to KP in {16,32,64,128,256,512},
// beyond 512 to a multiple of 128 (zero padding is exact for dot products and distances).
// k > 512 arises from full-rank per-person models (train-v5.py:539-545 sets
// n_components = face count).  The search kernels address a probe row with a 32-bit byte
// offset, so a launch covers at most 2^31 / (4 KP) probes (longer batches run in pieces).
constexpr int kMaxFeatureK = 1 << 16;
inline int feature_pad(int k) {
  if (k <= 16) return 16;
  if (k <= 32) return 32;
  if (k <= 64) return 64;
  if (k <= 128) return 128;
  if (k <= 256) return 256;
  if (k <= 512) return 512;
  if (k <= kMaxFeatureK) return (k + 127) / 128 * 128;
  return -1;
}
// The projection GEMM writes KPW = 64 or a multiple of 128 columns (128-column tiles).
inline int proj_pad(int kp) { return kp <= 64 ? 64 : (kp + 127) / 128 * 128; }

constexpr int kSearchProbeTile = 256;   // probes per search workgroup (4 waves x 64)
constexpr int kProjRowTile = 128;       // probes per projection workgroup
constexpr int kJacobiMax = 88;          // largest (even) order the LDS Jacobi handles
constexpr int kTimers = 15;             // EF_KERNEL_* ids (include/eigenface.h)
constexpr int kCandMax = 32;            // fp64 re-rank candidates kept per ambiguous probe (top-1 search)
// What gallery_aux_kernel reports of a gallery's rows (ef_search_common.hpp scan_regular)
constexpr unsigned kRowNotFinite = 1;   // a row whose fp32 ||g||^2 is +inf or NaN
constexpr unsigned kRowTiny = 2;        // a row, not all zeros, whose fp32 ||g||^2 is below 2^-80

// Workspace of one search call (device pointers).
struct SearchWs {
  long long* part_key;  // [nchunks][bpad] best (score, row) per chunk
  float* part_b2;       // [nchunks][bpad] runner-up score per chunk
  int* amb_count;       // probes queued for fp64 resolution
  int* amb_list;        // [bpad] probe of each queued slot
  float* thr;           // [bpad] fp32 score threshold of each slot
  int* cand;            // [bpad][kCandMax] candidate rows
  int* cand_cnt;        // [bpad]
  ef_match* match;      // [b] exact merge records (fp64 winner score), may be null
  int cand_cap;         // rows kept per slot in cand (kCandMax; the top-m search sets its own), read on a hit
  // labelled search (ef_search_labelled): read by the labelled instantiations of
  // the scan kernels and of resolve_kernel alone, which launch_search_scan / top1_t pick when
  // lbl != 0.  lbl = 0: a plain search; else EF_LABEL_* + 1.
  const int* glab;      // [n] label of each gallery row; null for EF_LABEL_ANY
  const int* plab;      // [bpad] label of each probe of the piece
  const int* pexcl;     // [bpad] the probe's excluded local row, -1 for none (label_prep_kernel)
  int lbl;
};

struct SearchPlan {
  int n_ptiles = 0, nchunks = 0, tiles_per_chunk = 0;
  // wide kernel: (chunk, probe tile) pairs are dealt to XCDs in blocks of cblk chunks x
  // pblk probe tiles, so one XCD's L2 holds pblk probe tiles instead of all of them
  int pblk = 0, cblk = 1;
  // collect pass (queued probes only): c_grid workgroups stride over (c_chunks chunks of
  // c_tpc tiles) x (queued probe tiles) items
  int c_chunks = 1, c_tpc = 1, c_grid = 8;
};

// Scratch of one prefix search (EF_OPT_SEARCH_PREFIX; device pointers).  The counters of the
// path live beside SearchWs::amb_count: amb_count[1] = probes of this piece sent to the
// full-k scan (the device count of the second run), amb_count[2] = their total over the
// search's pieces.  The cascade (EF_OPT_SEARCH_PREFIX_SCREEN) adds amb_count[kScreenCount] = probes
// of this piece the screen left unproven (the device count of the split stage) and
// amb_count[kScreenTotal] = their total over the pieces.
constexpr int kScreenCount = 3, kScreenTotal = 4;
struct PrefixWs {
  float* q1;         // [bpad][K1] the probes' first K1 components (the search_kernel forms; prefix64_kernel reads qpad,
                     // and the cascade, which runs only where it does, keeps the screen's list of bpad ints here)
  float* qpad2;      // [bpad][KP] the unproven probes' rows, in list order
  int* list;         // [bpad] probe of each unproven slot
  long long* keys2;  // [bpad] keys of the second run, by slot
  ef_match* match2;  // [bpad] match records of the second run, by slot
};

// one launch of a (possibly piecewise) search: probes [off, off + b), launched and planned
// with bpad = round_up(b, 256) rows (ef_api.hip search_pieces)
struct SearchPiece {
  int64_t off, b, bpad;
};

// ---- the scan's arithmetic ----------------------------------------------------------
// The one numbering of the scan variants, as every launcher takes it:
//   0  fp32 kernels on the gallery itself
//   1  split bf16 (hi + lo rows), the 16x16x32 kernels
//   2  split bf16, the 32x32x16 kernels (at padded k < 128 the same kernel as 1)
//   3  single-bf16 screen: wide k (kp > 128) only, counts as 1 below that and in the top-m search
// split_variant resolves EF_OPT_SEARCH_SPLIT_BF16 to it once per search, on the host; the copy
// of the gallery a variant reads has layout 3 (single-bf16 rows) for 3 and 1 (split rows) else.
inline int split_variant(int64_t opt, int kp, bool topm) {
  if (opt == 3) return kp > 128 && !topm ? 3 : 1;
  return (int)opt;
}
inline int split_layout(int variant) { return variant == 3 ? 3 : 1; }
// A resolved variant with the copies that match it: G3 the gallery copy in split_layout(variant)
// (null for 0), Q3 the scratch [bpad][kp] for the probes' copy (variant != 0 at kp > 128 only).
struct SplitScan {
  int variant = 0;
  const float* G3 = nullptr;
  float* Q3 = nullptr;
};

// ---- error propagation --------------------------------------------------------------
#define EF_TRY(expr)              \
  do {                            \
    int _rc = (expr);             \
    if (_rc != EF_OK) return _rc; \
  } while (0)
#define EF_HIP(ctx, expr, what)                              \
  do {                                                       \
    hipError_t _e = (expr);                                  \
    if (_e != hipSuccess) return ef::hip_err(ctx, _e, what); \
  } while (0)

inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }
inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

// ---- owning handles -----------------------------------------------------------------
// Move-only owner of one HIP handle (p; bytes for memory).  The destructor and reset() free
// through Free, the only caller of the HIP free / destroy functions (ef_api.hip); an empty
// handle makes no HIP call, and a move leaves its source empty.
template <class H, void (*Free)(H)>
struct Owned {
  H p = nullptr;
  size_t bytes = 0;
  Owned() = default;
  Owned(Owned&& o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
  Owned& operator=(Owned&& o) noexcept {
    if (this != &o) { reset(); p = std::exchange(o.p, nullptr); bytes = std::exchange(o.bytes, 0); }
    return *this;
  }
  ~Owned() { reset(); }
  void reset() {
    if (p) Free(p);
    p = nullptr;
    bytes = 0;
  }
  operator H() const { return p; }
};
void free_device(void* p);
void free_pinned(void* p);
void free_event(hipEvent_t e);
void free_stream(hipStream_t s);
using DevBuf = Owned<void*, free_device>;      // grown with ensure(), freed early with release()
using PinnedBuf = Owned<void*, free_pinned>;   // pinned_alloc()
using Event = Owned<hipEvent_t, free_event>;   // created on first use: event_get()
using Stream = Owned<hipStream_t, free_stream>;  // created on first use: stream_get()

// An existing handle is kept.  A new event has timing disabled unless flags says otherwise
// and, with record_on, is recorded there at once (waits on it pass until it is re-recorded).
hipError_t event_get(Event& e, hipStream_t record_on = nullptr, unsigned flags = hipEventDisableTiming);
hipError_t stream_get(Stream& s);                     // non-blocking
hipError_t pinned_alloc(PinnedBuf& b, size_t bytes);  // frees what b held first

// A side stream with the two events that order it against a main stream.
struct SideStream {
  Stream s;
  Event forked, done;
};
// Fork / join of one call's side work.  fork() makes the side stream wait for what the main
// stream has queued so far, done() marks the end of the side work, join() makes the main
// stream wait for it.  Once forked, the destructor joins on every exit that did not, so
// nothing queued on the main stream later (or a free after a synchronise) overtakes it.
class SideJoin {
 public:
  SideJoin(SideStream& side, hipStream_t main) : side_(side), main_(main) {}
  SideJoin(const SideJoin&) = delete;
  ~SideJoin() { (void)join(); }
  hipError_t fork();
  hipError_t done();
  hipError_t join();

 private:
  SideStream& side_;
  hipStream_t main_;
  bool forked_ = false, done_ = false;
};

struct TimerEvt {
  Event a, b;
  int kernel = -1;
};

// ---- workspace carve-out ------------------------------------------------------------
// Hands out consecutive 256-byte-aligned typed pieces of one allocation.  The same carve
// function runs twice — on a null base for the total, then on the allocation — so the sizes
// and the pointers cannot disagree.
struct Carve {
  void* base = nullptr;
  size_t total = 0;
  template <class T>
  T* take(size_t count) {
    T* p = base ? reinterpret_cast<T*>(static_cast<char*>(base) + total) : nullptr;
    total += align256(count * sizeof(T));
    return p;
  }
};
// parts: the largest nchunks x bpad of the call's pieces; bpad: its largest piece (the
// braces evaluate left to right, in member order; match stays null)
inline SearchWs carve_search_ws(Carve& cv, size_t parts, size_t bpad) {
  return SearchWs{cv.take<long long>(parts), cv.take<float>(parts), cv.take<int>(8), cv.take<int>(bpad),
                  cv.take<float>(bpad), cv.take<int>(bpad * kCandMax), cv.take<int>(bpad), nullptr, kCandMax};
}
// Scratch of one top-m search beside its SearchWs (ef_search_topk.hip; device pointers).  The
// first collect / resolve round runs on the SearchWs queue (amb_count, amb_list, thr,
// cand_cnt), the second on queue 2; cand replaces the SearchWs's 32-row lists.
struct TopkWs {
  int* cand;       // [bpad][cap] candidate rows of either round
  int* list2;      // [bpad] probes whose first list overflowed
  float* thr2;     // [bpad] their refined thresholds
  int* cnt2;       // [bpad] their second candidate counts
  int* list3;      // [bpad] probes whose second list overflowed too (full fp64 sweep)
  int* counts;     // [0] probes in queue 2, [1] probes in queue 3
};
inline TopkWs carve_topk_ws(Carve& cv, size_t bpad, size_t cap) {
  return TopkWs{cv.take<int>(bpad * cap), cv.take<int>(bpad), cv.take<float>(bpad), cv.take<int>(bpad),
                cv.take<int>(bpad), cv.take<int>(4)};
}
inline PrefixWs carve_prefix_ws(Carve& cv, size_t bpad, int k1, int kp) {
  return PrefixWs{cv.take<float>(bpad * k1), cv.take<float>(bpad * kp), cv.take<int>(bpad),
                  cv.take<long long>(bpad), cv.take<ef_match>(bpad)};
}

// ---- one frame of a scan: what the template and the Haar route share (frame_call below) ----
// A plan's buffers for a frame's way in and out.  The result block of one frame is one device
// allocation with a pinned mirror, so a host call downloads it with one copy.
struct FrameIo {
  DevBuf frame_in;  // a host call's frame, H rows of W * channels bytes
  DevBuf gray;      // the grey plane of a colour frame (Haar: or of a strided grey one), round_up(H * W, 4) bytes
  DevBuf out;       // the result block
  PinnedBuf host;   // its pinned mirror
  // a gated host call's gate stays resident and is uploaded again only when its values change,
  // so a frame still costs one upload
  DevBuf gate;
  std::vector<float> gate_host;
};
// The front of a result block is the route's own, one or two pieces of so many bytes: the
// template route's ef_scan_det[g]; the Haar route's ef_haar_scan_head[1], then int[g * 4].
constexpr int kFrameFrontMax = 2;
struct FrameFront {
  int n;
  size_t bytes[kFrameFrontMax];
};
// The pieces of a result block for g rectangles, M bank slots and d face pixels: the front and,
// behind it, what every route returns.  gated: the distances from face space and the energies
// too, last, so the ungated block is a prefix of the gated one.  Also how a call's own output
// arrays are passed around (front[i]: the caller's array for piece i).
struct FrameOut {
  void* front[kFrameFrontMax];
  long long* keys;  // [g][M]
  int* best;        // [g]
  uint8_t* rows;    // [g][d]
  float* dffs2;     // [g][M]
  float* energy;    // [g][M]
};
inline FrameOut carve_frame_out(Carve& cv, const FrameFront& fr, size_t g, size_t M, size_t d, bool gated) {
  FrameOut o{};
  for (int i = 0; i < fr.n; ++i) o.front[i] = cv.take<char>(fr.bytes[i]);
  o.keys = cv.take<long long>(g * M);
  o.best = cv.take<int>(g);
  o.rows = cv.take<uint8_t>(g * d);
  if (gated) {
    o.dffs2 = cv.take<float>(g * M);
    o.energy = cv.take<float>(g * M);
  }
  return o;
}
// Where a frame's kernels write.  The host form: everything into the block.  The device form:
// the caller's arrays, except that the rows (the bank reads them) and, gated, the energy (the
// gate's kernels write it) fall back to the block when the caller passes none.  need: the block
// is used at all; a size pass's null block answers that before anything is allocated.
struct FrameRoute {
  FrameOut o;
  bool need;
};
inline FrameRoute frame_route(const FrameOut& caller, bool dev, bool gated, const FrameOut& blk) {
  if (!dev) return FrameRoute{blk, true};
  FrameRoute r{caller, false};
  if (!caller.rows) r.o.rows = blk.rows, r.need = true;
  if (gated && !caller.energy) r.o.energy = blk.energy, r.need = true;
  return r;
}

// ---- the plan of one search (host only: no HIP call) --------------------------------
// What a search of b probes against n rows of padded width kp launches: the pieces
// (search_pieces), every piece's plan built from that piece's own bpad (a shorter last piece's
// plan may have more chunks), the prefix scan's plans when k1 > 0 (split1: its split-bf16
// arithmetic), and the workspace they share, sized for the largest piece.  m > 0 plans the
// top-m search (at least m chunks, and cap candidate rows per probe in the TopkWs).
// ef_search_schedule reports it, search_run and search_topk_run launch it.
struct SearchSchedule {
  std::vector<SearchPiece> pieces;
  std::vector<SearchPlan> plans, plans1;  // per piece; plans1 empty unless k1 > 0
  size_t parts = 0;                        // largest nchunks x bpad over the pieces and both plans
  int64_t bpad_max = 0;
  size_t ws_bytes = 0;      // carve_search_ws(parts, bpad_max) and, m > 0, carve_topk_ws(bpad_max, cap)
  size_t prefix_bytes = 0;  // carve_prefix_ws(bpad_max, k1, kp), k1 > 0
};
SearchSchedule search_schedule(int64_t b, int64_t n, int kp, int variant, int k1, bool split1, int m, int cap);

// ---- resident gallery -----------------------------------------------------------------
// Rows padded to kp = feature_pad(k) with their norms; the context holds one, a bank slot one.
struct Gallery {
  int64_t n = 0;
  int k = 0, kp = 0;
  DevBuf G;       // float[n][kp]
  DevBuf gnorm2;  // float[n]  ||g||^2
  DevBuf ginv;    // float[n]  1/||g|| (0 for a zero row)
  DevBuf gmax2;   // uint[2]: (float bits) max ||g||^2 over the rows whose norm is finite, the kRow* bits
};
// What the context derives from its gallery on the first search that needs it, and the prefix
// guard's history, which belongs to the gallery and settings it was seen on.  reset() forgets
// all of it (the buffers stay allocated for the next build).  ef_gallery_set calls it, and so do
// the setters of EF_OPT_SEARCH_PREFIX and EF_OPT_SEARCH_PREFIX_SPLIT: after either the next search
// rebuilds the copies it reads (one pass over the gallery each), not only a clean guard.
struct GalleryDerived {
  DevBuf G3;          // copy of G for the split scans (same bytes)
  int g3_layout = 0;  // what G3 holds: 0 nothing, 1 split (hi + lo) rows, 3 single-bf16 rows
  // prefix scan (EF_OPT_SEARCH_PREFIX): compact copy of the first g1_k1 components of every row
  DevBuf G1;      // float[n][g1_k1], or the same bytes as split-bf16 rows (g1_split)
  DevBuf gnorm1;  // float[2][n]: fp32 ||g[:K1]||^2, then the aux kernel's unused 1/||.|| output
  int g1_k1 = 0;  // 0: no copy
  bool g1_split = false;  // only the copy the chosen arithmetic reads is kept
  // the screen (EF_OPT_SEARCH_PREFIX_SCREEN): single-bf16 copy of the same prefix; its start
  // values take gnorm1's second half, so it is rebuilt whenever G1 is
  DevBuf G1h;      // bf16[n][g1h_k1]
  int g1h_k1 = 0;  // 0: no copy
  // the guard: counters of the last prefix search arrive in pinned memory behind ev
  bool ev_pending = false;
  int64_t ev_tiles = 0;  // probe tiles of the search ev belongs to
  int skip_left = 0;     // searches the guard still keeps off the prefix scan
  bool ev_screen = false;    // the search ev belongs to ran the screen
  int screen_skip_left = 0;  // searches the screen's guard still sends straight to the split stage
  void reset() {
    g3_layout = g1_k1 = g1h_k1 = 0;
    ev_pending = ev_screen = false;
    skip_left = screen_skip_left = 0;
  }
};

// ---- model bank (ef_bank.hip) ---------------------------------------------------------
// One resident (mean, W, gallery) triple.  W is padded to kpw = round_up(kp, 128) columns (the
// grouped projection works in 128-column tiles), the gallery to kp as ef_gallery_set pads it.
struct BankSlot {
  int kpw = 0;
  DevBuf mean;  // float[d]
  DevBuf W;     // float[d][kpw]
  Gallery g;    // k, kp and the rows; gmax2 is read on the device
  // the way back (ef_bank_recon_set): published together, once completely built
  bool recon = false;
  DevBuf recon_R;  // float[kp][recon_dpad(d)], zero past k and past d
  DevBuf recon_w;  // float[d] per-pixel weight (ones when the caller gave none)
};
// One slot's operands of the grouped residual (ef_bank_recon.hip); R null: the slot has none.
struct BankReconDev {
  const float* R;
  const float* mean;
  const float* wgt;
  int kp;
  int64_t kp_off;  // the slot's feature block is q + bpad * kp_off, [bpad][kp]
};
// The face gate of one gated call: device pointers.
struct BankGate {
  const float* gate;  // [slots]
  bool relative;      // bound = gate[m] * energy[p][m]
  float* dffs2;       // [b][slots]
  float* energy;      // [b][slots]: required here (the scratch of a call that does not return it)
};
// The slots, their device tables (rebuilt on the first recognize after a change) and the
// per-call scratch.  A slot is built completely before it is appended.
struct Bank {
  int64_t d = 0;
  std::vector<BankSlot> slots;
  int64_t total_k = 0, total_kp = 0, total_kpw = 0, total_rows = 0, total_slices = 0;
  int kp_max = 0, search_lds = 0;  // widest slot; dynamic LDS bytes of the search launch
  bool tables_valid = false;
  DevBuf proj_items;  // BankProjItem[column tiles]
  DevBuf slot_tab;    // BankSlotDev[slots]
  DevBuf recon_tab;   // BankReconDev[slots]
  int recon_rk = 32;       // stage depth of the grouped residual: 16 when any slot has kp = 16
  DevBuf recon_part;  // float[2][nsplit][slots][bpad] partial eps^2 and E
  DevBuf recon_out;   // dffs2, energy (and the gate) of a host call; the energy of a call that has no use for it
  DevBuf part;        // float[nsplit][bpad][total_kpw] partial slabs
  DevBuf q;           // per slot float[bpad][kp], slot m at bpad * sum_{j<m} kp_j
  DevBuf ws;          // search scratch (per row slice and probe)
  DevBuf out;         // staging of a host call's best slots (the rest: ef::Results)
  DevBuf p_stage;     // probe pixels staged from host
};

// ef_bank_recognize on device pointers (ef_bank.hip), shared with ef_scan_frame: b probes
// Pd[b][bank.d] -> kdev[b][slots] and, each optional, mdev[b][slots], sdev[b] (best slot) and
// fdev[b][sum k].  Everything is queued on c->stream; only the table upload after the bank
// changed waits.  The caller has checked the bank's state and the arguments.
// gate non-null: the grouped residual and its reduce are queued between the projection's reduce
// and the search (-> gate->dffs2, gate->energy, from the same features), and the walk over models
// skips the slots the gate rejects; null: exactly the launches described above.
int bank_recognize_dev(ef_ctx* c, const void* Pd, int p_dtype, int64_t b, int metric, long long* kdev, ef_match* mdev,
                       int* sdev, float* fdev, const BankGate* gate = nullptr);
// EF_OK when every slot has reconstruction state, else EF_E_STATE naming the first without (ef_bank.hip)
int bank_recon_complete(ef_ctx* c, const char* who);
// The grouped residual's plan (ef_bank_recon.hip): what ef_bank_recon_schedule reports and
// launch_bank_recon launches.
struct BankReconPlan {
  int nsplit = 1, tiles_per_split = 1;
  int64_t n_workgroups = 0, scratch_bytes = 0;
};
BankReconPlan bank_recon_plan(int64_t b, int64_t d, int64_t n_slots);
// q: the bank's feature blocks (slot m at q + bpad * kp_off_m, [bpad][kp_m], zero past b and past
// k_m); P[b][d] pixels; part[2][nsplit][n_slots][bpad] -> launch_bank_recon_reduce ->
// dffs2[b][n_slots], energy[b][n_slots] (optional).  rk: 16 | 32, dividing every slot's kp.
hipError_t launch_bank_recon(hipStream_t s, const BankReconDev* tab, int n_slots, int rk, int p_dtype, const float* q,
                             const void* P, int64_t b, int64_t bpad, int64_t d, float* part, const BankReconPlan& pl);
hipError_t launch_bank_recon_reduce(hipStream_t s, const float* part, int nsplit, int n_slots, int64_t b, int64_t bpad,
                                    float* dffs2, float* energy);

struct TmState;    // template-localiser state (ef_image.hip)
struct HaarState;  // Haar cascade state (ef_haar.hip)

}  // namespace ef

// Every buffer, pinned block, event and stream below is an owning handle: `delete ctx` frees
// all of it.  Members go in reverse declaration order, and the streams and events are declared
// last, after every buffer whose work they order, so they go first: a stream destroyed with
// work queued drains on its own, and the hipFree of a buffer waits for the device.
struct ef_ctx {
  ef_ctx() = default;
  ~ef_ctx();  // the localiser, cascade and communicator first, then the members
  int device = 0;
  // tunables set with ef_set_option (include/eigenface.h EF_OPT_*)
  int64_t opt_fit_max_iters = 500;
  int64_t opt_fit_fp32_coarse = 1;
  int64_t opt_cov_slab_bytes = (int64_t)8 << 30;
  int64_t opt_tm_int64 = 0;
  int64_t opt_haar_ordered = 0;
  int64_t opt_jpeg_chunk_bits = 0;
  int64_t opt_search_split_bf16 = 0;  // resolved per search by ef::split_variant
  int64_t opt_jpeg_part_files = 8192;
  int64_t opt_fit_chebyshev = 1;
  hipStream_t stream = nullptr;  // own_stream or the caller's (ef_set_stream): not owned
  std::string err;

  // recognition model (p - mean) . W
  int64_t d = 0;
  int k = 0, kp = 0, kpw = 0;
  ef::DevBuf mean;  // float[d]
  ef::DevBuf W;     // float[d][kpw]
  bool bf16 = false;   // EF_MODEL_BF16: project with W16 on bf16 MFMA
  ef::DevBuf W16;      // bf16[kpw][d]
  ef::DevBuf W16f;     // W16 in MFMA-fragment order (frag-form projection), when supported
  bool w16f_ok = false;
  ef::DevBuf mean_r;   // float[d] round(mean)
  ef::DevBuf mean_u8;  // uint8[d] round(mean) (wide bf16 kernel) + int counter
  bool mean_u8_ok = false;  // every round(mean) in 0..255
  ef::DevBuf corr;     // float[kpw] (mean - round(mean)).W
  // split form of an fp32 model (EF_OPT_PROJECT_SPLIT_BF16): built by the first projection that
  // can use it (split3_prepare, ef_api.hip), dropped by ef_model_set; mean_u8 and corr above
  // are then this model's
  int64_t opt_project_split_bf16 = 1;
  int split3_state = 0;  // 0 not built yet, 1 usable, -1 the guard ruled this model out
  ef::DevBuf W3f;        // the hi, mid, lo bf16 pieces of W in MFMA-fragment order

  // gallery
  ef::Gallery gal;       // gal.k == 0: none set yet
  int64_t g_offset = 0;  // global index of row 0
  float gmax2_host = 0.f;
  unsigned gal_rows_host = 0;  // the gallery's kRow* bits (scan_gmax2, ef_api.hip)
  // one label per gallery row (ef_gallery_labels); ef_gallery_set drops them
  bool has_labels = false;
  ef::DevBuf glabels;   // int32[gal.n]
  ef::DevBuf label_ws;  // per-call scratch of ef_search_labelled: int[2][bpad], then the host call's staging
                        // (ef_score_census: int[2][bpad], float[bpad] probe norms, the staging, the counts)
  ef::DevBuf cluster_ws;  // per-call scratch of ef_gallery_cluster (ef_cluster.hip): O(n)
  ef::DevBuf range_ws;    // per-call scratch of ef_search_range (ef_range.hip): O(b chunks), then a host call's staging
  // ef_search_rank (ef_rank.hip): the dense class map of the row labels, built by the first rank
  // call after ef_gallery_labels and dropped with the labels or the gallery; the per-call scratch
  // (O(b), a host call's staging, and the bitmap up to opt_rank_bitmap_bytes)
  bool rank_map_valid = false;
  int64_t rank_classes = 0;
  ef::DevBuf rank_cls;   // int32[round_up(gal.n, 128)] class of each row, -1 past the end
  ef::DevBuf rank_uniq;  // int32[rank_classes] the distinct labels, ascending
  ef::DevBuf rank_ws;
  int64_t opt_rank_bitmap_bytes = (int64_t)256 << 20;
  ef::GalleryDerived der;  // the split and prefix copies and the prefix guard (search_copies)
  int64_t opt_search_prefix = 1;
  int64_t opt_search_prefix_split = 1;  // the prefix scan's arithmetic: 1 split bf16, 0 fp32
  int64_t opt_search_prefix_screen = 1;  // 1: a single-bf16 screen ahead of the split scan at K1 <= 32
  ef::DevBuf prefix_ws;  // per-call scratch of the prefix path (ef::PrefixWs carve-out)
  // counters of the last prefix search, copied to pinned host memory behind the search
  // ([0] probes sent to the full-k scan, [2] probes the screen left unproven); the next search
  // reads them once prefix_ev has passed
  ef::PinnedBuf prefix_host;  // int[4]
  // what ef_search_stats reports: {probes, used the prefix scan, guard skipped}
  int64_t stats_probes = 0;
  bool stats_prefix = false, stats_skipped = false;
  bool stats_screen = false, stats_screen_skipped = false;  // ef_prefix_screen_stats

  // per-call scratch (grown on demand, never shrunk)
  ef::DevBuf q_pad;     // float[bpad][kp]
  ef::DevBuf q3;        // split-bf16 probes [bpad][kp] (wide split-bf16 scans)
  ef::DevBuf keys;      // int64[bpad]
  ef::DevBuf search_ws; // SearchWs carve-out
  // top-m search (ef_search_topk.hip): candidate rows kept per probe, and the counters of the
  // most recent top-m search ({-, overflowed, swept, re-scored} on the device; probes here)
  int64_t opt_search_topk_cand = 1024;
  ef::DevBuf topk_counters;  // unsigned long long[4]
  int64_t topk_probes = 0;
  ef::DevBuf p_stage;   // probe pixels staged from host
  ef::DevBuf proj_part; // float[nsplit][bpad][kpw]
  ef::DevBuf feats_dev; // float[b][k] staging for host output

  // reconstruction x^ = mean + f . R of the model above (ef_recon_set; ef_model_set drops it)
  bool recon = false;
  ef::DevBuf recon_R;     // float[kp][recon_dpad(d)], zero past k and past d
  ef::DevBuf recon_w;     // float[d] per-pixel weight (ones when the caller gave none)
  ef::DevBuf recon_part;  // float[2][nsplit][round_up(b, 128)] partial eps^2 and E
  ef::DevBuf recon_out;   // staging of a host call's outputs (pixels, or eps^2 and E)

  ef::Bank bank;  // model bank (ef_bank_*): independent of the model and gallery above

  std::vector<ef::DevBuf> fit_pool;  // ef_fit workspaces, reused across calls (ef_trim frees)

  // JPEG decode (ef_jpeg.hip): device workspace, host-output staging, and two upload slots
  // (a pinned host buffer + its device copy each): the host stages batch i + 1 into one slot
  // — the next part of a call, or the next call — while the device decodes batch i from
  // the other.  up_done[s]: the upload that last read pinned slot s (copy stream);
  // ws_free[s]: the last kernel that read device slot s (compute stream); done: the last
  // decode's kernels (a call on another stream, or a reallocation, waits for it).
  ef::DevBuf jpeg_ws, jpeg_out, jpeg_rows;
  ef::DevBuf jpeg_up[2];
  ef::PinnedBuf jpeg_pinned[2];
  int jpeg_slot = 0;                // slot of the next staged batch

  // published only once completely built (ef_tm_prepare, ef_haar_set_cascade); null otherwise
  ef::TmState* tm = nullptr;
  ef::HaarState* haar = nullptr;
  ef::DevBuf haar_group_ws;  // ef_haar_group's scratch (ef::HaarGroupWs carve-out, header, staged results)

  // multi-GPU: RCCL communicator (ef_comm_init), null when single-rank
  void* comm = nullptr;
  int comm_size = 1, comm_rank = 0;
  ef::DevBuf match_local;  // ef_match[b] this rank's records
  ef::DevBuf match_all;    // ef_match[comm_size][b] gathered records
  ef::DevBuf q_local;      // float[cpad][kp] this rank's slice of the projected probes

  bool timing = false;
  double t_ms[ef::kTimers] = {};
  int64_t t_n[ef::kTimers] = {};

  // streams and events, all created on first use except own_stream (ef_create)
  ef::Stream own_stream;
  ef::Stream jpeg_copy;  // upload stream
  ef::Event jpeg_up_done[2], jpeg_ws_free[2], jpeg_done;
  ef::Event prefix_ev;
  // the fit's side stream: work off the critical path of the subspace iteration, e.g. the
  // int8 digit planes of C during the coarse phase
  ef::SideStream fit_side;
  // the template localiser's side stream: the integral images' column pass runs beside the
  // correlation kernel
  ef::SideStream tm_side;
  std::vector<ef::TimerEvt> pending;  // timed kernels not yet read by ef_timing_get
};

namespace ef {

// delete the context's localiser / cascade state, if any
void tm_release(ef_ctx* c);
void haar_release(ef_ctx* c);
int ensure(ef_ctx* c, DevBuf& b, size_t bytes);
inline void release(DevBuf& b) { b.reset(); }
void timer_begin(ef_ctx* c, int kernel, TimerEvt* t);
void timer_end(ef_ctx* c, TimerEvt* t);
// events created but not recorded: the launcher records them itself around the kernels
// (t->kernel < 0 when timing is off); timer_commit queues them for ef_timing_get
void timer_arm(ef_ctx* c, int kernel, TimerEvt* t);
void timer_commit(ef_ctx* c, TimerEvt* t);

// ---- launchers (defined in the .hip files) -------------------------------------------
// tile_rows: gallery rows per tile when not the kernel family's own (the prefix scan); the
// 256-row plans are the split-bf16 prefix scan's at k1 <= 32, whose workgroups take 512 probes:
// n_ptiles counts those, rounding up (bpad is a multiple of 256)
// min_chunks (the top-m search): at least round_up(min_chunks, 8) gallery chunks
SearchPlan search_plan(int64_t bpad, int64_t n, int kp, bool s3, int tile_rows = 0, int min_chunks = 0);
// rows per tile of the prefix scan at prefix length k1 (split: the split-bf16 scan)
int prefix_tile_rows(int k1, bool split);
std::vector<SearchPiece> search_pieces(int64_t b, int kp);
// b probe features Q[b][k of the gallery] (host, or device with dev) into ctx->q_pad, padded to
// bpad rows of the gallery's kp
int stage_queries(ef_ctx* c, const float* Q, int64_t b, bool dev, int64_t bpad);
// Top-1 search of one piece.  sp: the scan's variant (0 fp32; 1 split 16x16x32; 2 split 32x32x16;
// 3 single-bf16 screen, wide k only — split_variant above) with the copies that match it.  The
// sequence: the probes' copy into sp.Q3 (variant != 0 at kp > 128), then the timed main scan,
// the queue counter's memset, reduce_kernel, the COLLECT scan over the queue, resolve_kernel.
// timer: the context whose EF_KERNEL_SEARCH timer brackets the main scan; nothing else is read
// from it.
hipError_t launch_search(hipStream_t s, int kp, int metric, const SplitScan& sp, const SearchPlan& pl,
                         const float* qpad, int64_t bpad, int64_t b, const float* G, const float* aux, int64_t n,
                         int64_t g_offset, float gmax2, const SearchWs& ws, long long* keys, ef_ctx* timer);
// Prefix search (EF_OPT_SEARCH_PREFIX; L2, fp32 scan, k1 < kp <= 128): the scan over the
// compact prefix copy (G1, gnorm1), the proof per probe, and the full-k pipeline of
// launch_search on the unproven probes.  Same keys / match records as launch_search.
// split (EF_OPT_SEARCH_PREFIX_SPLIT): G1 holds split-bf16 rows and the scan runs the split
// chain; pl1 is planned with prefix_tile_rows(k1, split).
// G1h (EF_OPT_SEARCH_PREFIX_SCREEN; split and k1 <= 32 only, else null): the single-bf16 copy
// of the prefix, its start values at gnorm1 + n.  The scan then runs as a cascade: the screen
// over G1h, the split scan for the probes the screen could not prove, the full-k pipeline for
// the rest.  The caller zeroes ws.amb_count[kScreenCount] ahead of every piece.
hipError_t launch_search_prefix(hipStream_t s, int kp, int k1, const SearchPlan& pl, const SearchPlan& pl1,
                                const float* qpad, int64_t bpad,
                                int64_t b, const float* G, const float* gnorm2, const float* G1, const float* gnorm1,
                                bool split, const float* G1h, int64_t n, int64_t g_offset, float gmax2,
                                const SearchWs& ws, const PrefixWs& pw, long long* keys, ef_ctx* c);
// G1[n][k1] <- G[n][kp][:k1], gnorm1[n] = ||G1 row||^2 in fp32 (gnorm1 holds 2 n floats);
// split: G1's rows are then rewritten as split-bf16 rows (launch_split_rows, same bytes)
hipError_t launch_prefix_gallery(hipStream_t s, const float* G, int64_t n, int kp, int k1, bool split, float* G1,
                                 float* gnorm1);
// G1h[n][k1] <- bf16(G[n][kp][:k1]) and the screen's start values gnorm1[n + r] from gnorm1[r]
// (after launch_prefix_gallery, whose aux kernel writes that half too)
hipError_t launch_prefix_screen_gallery(hipStream_t s, const float* G, int64_t n, int kp, int k1, void* G1h,
                                        float* gnorm1);
hipError_t launch_split_rows(hipStream_t s, const float* G, int64_t n, int kp, void* out);
// single-bf16 copy for the bf16 screen (EF_OPT_SEARCH_SPLIT_BF16 = 3), kp % 64 == 0
hipError_t launch_hi_rows(hipStream_t s, const float* G, int64_t n, int kp, void* out);
hipError_t launch_keys_none(hipStream_t s, long long* keys, int64_t b, ef_match* match);
// Labelled search (ef_search_labelled): plab[rows] / pexcl[rows] <- the probes' labels (0 when
// plabels is null) and their excluded rows as local row indices, -1 for "none" (excl null, a
// negative entry, one outside [g_offset, g_offset + n), and the rows past b)
hipError_t launch_label_prep(hipStream_t s, const int32_t* plabels, const int64_t* excl, int64_t b, int64_t rows,
                             int64_t g_offset, int64_t n, int* plab, int* pexcl);
// Score census (ef_score_census; ef_census.hip).  launch_census_probe_aux:
// qaux[rows] <- what the census epilogue needs of each probe row of qpad[rows][kp], from the fp64
// sum of squares rounded once: ||q||^2 (L2), or 1/||q|| (cosine; 0 for a zero probe, NaN for one
// with a NaN or infinite component).  launch_census: the pairs of probes [0, b) of qpad (bpad
// rows, a multiple of 128) with the n gallery rows are added to counts[2][nbins + 3], which the
// caller has zeroed; aux as the scans take it (||g||^2 for L2, 1/||g|| for cosine), plab / pexcl
// launch_label_prep's output.
constexpr int kCensusMaxBins = EF_CENSUS_MAX_BINS;
hipError_t launch_census_probe_aux(hipStream_t s, const float* qpad, int64_t rows, int kp, int metric, float* qaux);
hipError_t launch_census(hipStream_t s, int kp, int metric, const float* qpad, int64_t bpad, int64_t b, const float* G,
                         const float* aux, const int* glab, int64_t n, const float* qaux, const int* plab,
                         const int* pexcl, float lo, float hi, int nbins, unsigned long long* counts);
// One scan launch, the only map from (kp, metric, variant, main or COLLECT, cnt, labelled) to a scan
// kernel: search_kernel, search16_kernel (kp == 128 under variant 1) and, kp > 128, the wide
// kernels; variant 3 counts as 1 at kp <= 128.  ws.lbl != 0 picks the labelled instantiations
// (fp32 scan only: variant 0, no cnt).  The main pass writes per-chunk top-2 records
// into ws, the COLLECT pass sweeps ws's queue.  q / G: what the variant reads (the fp32 probes
// and gallery for 0, else the copies; at kp <= 128 the kernels split the fp32 probes themselves).
// cnt: the main pass over a device-side probe count (the prefix path's second run: fp32, L2,
// 32 <= kp <= 128 only).
hipError_t launch_search_scan(hipStream_t s, int kp, int metric, bool collect, int variant, bool cnt,
                              const SearchPlan& pl, const float* q, const float* G, const float* aux, int64_t n,
                              int64_t bpad, const SearchWs& ws);
// *qs <- the probes a scan of sp reads: qpad itself, or (variant != 0 at kp > 128) their copy in
// sp.Q3, launched here, in the layout of the gallery copy
hipError_t launch_scan_probes(hipStream_t s, const SplitScan& sp, const float* qpad, int64_t bpad, int kp,
                              const float** qs);
// Top-m search of one piece (ef_search_topk.hip): keys[b][m] and, when match is non-null,
// match[b][m].  sp as launch_search (never variant 3); cap = rows of tw.cand per probe;
// counters[1..3] accumulate what ef_search_topk_stats reports.
hipError_t launch_search_topk(hipStream_t s, int kp, int metric, const SplitScan& sp, int m, const SearchPlan& pl,
                              const float* qpad, int64_t bpad, int64_t b, const float* G, const float* aux,
                              int64_t n, int64_t g_offset, float gmax2, const SearchWs& ws, const TopkWs& tw, int cap,
                              unsigned long long* counters, long long* keys, ef_match* match);
// keys[b][m] (+ merged[b][m]) <- the top-m merge of parts x b x m records (ef_search_topk.hip)
hipError_t launch_matches_merge_topk(hipStream_t s, const ef_match* parts, int nparts, int64_t b, int m,
                                     long long* keys, ef_match* merged);
// keys[b] (+ merged[b]) <- exact arg-best over parts x b match records (ef_comm.hip)
hipError_t launch_matches_merge(hipStream_t s, const ef_match* parts, int nparts, int64_t b, long long* keys,
                                ef_match* merged);
void comm_release(ef_ctx* c);
// ragged resize (ef_image.hip) from device descriptors written by img_desc_fill: the Haar
// pyramid and the JPEG ingest (BGR order for 3-channel sources)
hipError_t launch_resize_gray(hipStream_t s, const uint8_t* src, const void* desc_dev, int count, int64_t max_out,
                              uint8_t* dst);
size_t img_desc_size();
// grey plane of an H x W x c (3, 4) frame, rows ld bytes apart -> dst, round_up(H * W, 4) bytes,
// 4-byte aligned (ef_image.hip frame_gray_kernel): ef_scan_frame and ef_haar_scan_frame
hipError_t launch_frame_gray(hipStream_t s, const uint8_t* src, int64_t ld, int H, int W, int c, bool rgb, void* dst);
// ef_preprocess_rois on device pointers (ef_image.hip roi_resize_kernel): rectangle i is the four
// ints at rects + i * rect_stride, clipped to the frame by the kernel
hipError_t launch_roi_resize(hipStream_t s, const uint8_t* frame, int64_t ld, int fh, int fw, int c, const int* rects,
                             int rect_stride, int64_t n, int oh, int ow, bool rgb, uint8_t* dst);
void img_desc_fill(void* d, int64_t src_off, int64_t dst_off, int h, int w, int c, int oh, int ow);
// One frame through grey, a route's own kernels, the ROI rows and the model bank (ef_image.hip):
// the body of ef_scan_frame, ef_scan_frame_gated and ef_haar_scan_frame behind their "no plan"
// checks.  It checks the bank's state and the arguments (messages prefixed with `who`), routes
// the outputs (frame_route), keeps a host call's gate resident, and queues on c->stream: the
// host form's upload, then between timer_begin(timer) and timer_end the grey plane, `middle`,
// the ROI rows and the bank; the host form then downloads the block once, synchronises once and
// copies the pieces out.
struct FrameShape {
  int H, W, face_h, face_w;
  int n;  // rectangles recognised per frame: the template route's groups, the Haar route's max_faces
};
struct FrameArgs {  // as the entry point got them; out.front[i]: the caller's array for front piece i
  const uint8_t* frame;
  int64_t frame_ld;
  int32_t channels, metric;
  const float* gate;  // null: ungated
  FrameOut out;
  uint32_t flags;
};
struct FrameRects {  // what launch_roi_resize reads
  const int* p;
  int stride;
};
// The route's step: f is the grey plane on the device, rows ld bytes apart (packed for a colour
// frame; a route that needs packed rows packs a strided grey frame itself and updates f and ld).
// It queues the route's kernels, which write the front pieces at front[i], and names the
// rectangles they leave.
using FrameMiddle = std::function<int(const uint8_t*& f, int64_t& ld, void* const* front, FrameRects& rects)>;
int frame_call(ef_ctx* c, const char* who, int timer, const FrameShape& fs, FrameIo& io, const FrameFront& front,
               const FrameArgs& a, const FrameMiddle& middle);
// wait for every queued JPEG upload and decode of the context (ef_jpeg.hip)
hipError_t jpeg_quiesce(ef_ctx* c);
// hipFuncSetAttribute(fn, MaxDynamicSharedMemorySize, bytes) once per (kernel, device),
// thread-safe (several contexts may launch the same kernel on different devices)
hipError_t allow_dynamic_lds(const void* fn, int bytes);

// Runs fn(0) .. fn(n - 1) on a process-wide pool of host worker threads (created once, at
// most 15, plus the calling thread, which takes tasks too) and returns when all are done.
// Jobs from concurrent callers run one at a time.  Spawning threads per call cost ~1-2 ms
// per 16 threads in the sandboxed containers, as much as the host work it split.
void host_parallel(int n, const std::function<void(int)>& fn);
int host_threads();  // EF_OPT_HOST_THREADS (the job's CPU share)
// all-gather over the attached communicator on ctx->stream (bytes per rank)
int comm_allgather(ef_ctx* c, const void* send, void* recv, size_t bytes_per_rank);
// ---- one call's inputs and outputs (ef_api.hip) ----------------------------------------
// Where one call's keys, match records and features (each optional) are written: the caller's
// own pointers with EF_MEM_DEVICE, else the context's staging buffers (ctx->keys: bpad x rec
// keys, then the records; ctx->feats_dev), which fetch() copies to the caller's host pointers
// before it synchronises.  rec: keys / records per probe (1, the m of a top-m search, the
// bank's slots); fk: feature floats per probe.
struct Results {
  bool dev;
  int64_t b;
  int rec;
  int64_t fk;
  int64_t* keys;  // as the caller gave them
  ef_match* match;
  float* feats;
  long long* kdev = nullptr;  // where the kernels write
  ef_match* mdev = nullptr;
  float* fdev = nullptr;
  int stage_feats(ef_ctx* c);
  int stage_keys(ef_ctx* c, int64_t bpad);  // keys are always produced
  int fetch(ef_ctx* c) const;
};
// *Pd <- b probes of d pixels on the device: P itself with EF_MEM_DEVICE, else its copy in stage
int stage_probes(ef_ctx* c, const void* P, int dtype, int64_t b, int64_t d, uint32_t flags, DevBuf& stage,
                 const void** Pd);

// The two loaders of resident data (ef_api.hip), for the context and the bank alike.  Sources are
// host pointers, or device ones with EF_MEM_DEVICE; a host source that needs padding is staged
// unpadded in `staging`, which the caller keeps alive until it has synchronised c->stream.
// weights_load: mean[d] and W[d][k] into mean_dst and W_dst[d][kpw]; queued, not synchronised.
// gallery_load: G[n][k] into g's buffers, grown in place (never a second copy of the rows), with
// the norms; g is empty (n == 0) until the last step has succeeded.  gmax2_host non-null (the
// context): the load is synchronised and max ||g||^2 is on the host on return, with the kRow* bits
// in *rows_host; null (a bank slot): everything stays queued and both stay on the device.
int weights_load(ef_ctx* c, DevBuf& mean_dst, DevBuf& W_dst, const float* mean, const float* W, int64_t d, int k,
                 int kpw, uint32_t flags, DevBuf& staging);
int gallery_load(ef_ctx* c, Gallery& g, const float* G, int64_t n, int k, uint32_t flags, DevBuf& staging,
                 float* gmax2_host, unsigned* rows_host = nullptr);
hipError_t launch_pad_rows(hipStream_t s, const float* src, int64_t rows, int k, int64_t rows_pad,
                           float* dst, int kp);
hipError_t launch_gallery_aux(hipStream_t s, const float* G, int64_t n, int kp, float* gnorm2,
                              float* ginv, unsigned* gmax2_bits);

hipError_t launch_project(hipStream_t s, int kpw, int p_dtype, const void* P, int64_t b,
                          int64_t bpad, int64_t d, const float* mean, const float* W,
                          float* part, int nsplit, int64_t pix_per_split);
int project_nsplit(int64_t bpad, int64_t d, int kpw, int64_t* pix_per_split);
hipError_t launch_project_reduce(hipStream_t s, const float* part, int nsplit, int64_t b,
                                 int64_t bpad, int kpw, int k, int kp, const float* corr, float* qpad,
                                 float* f_out);
// bf16 model (EF_MODEL_BF16): W16 [kpw][d] bf16, round(mean), fp64-derived correction row
hipError_t launch_bf16_model(hipStream_t s, const float* W, const float* mean, int64_t d, int ldw,
                             unsigned short* Wt16, float* mean_r, float* corr, double* corr_part, int nchunk);
int project_bf16_nsplit(int p_dtype, const void* P, const uint8_t* mean_u8, const void* Wf, int64_t bpad, int64_t d,
                        int ldw, int64_t* pix_per_split);
hipError_t launch_project_bf16(hipStream_t s, int p_dtype, const void* P, int64_t b, int64_t bpad, int64_t d,
                               const float* mean_r, const uint8_t* mean_u8, const unsigned short* Wt16,
                               const void* Wf, int ldw, float* part, int nsplit, int64_t pps);
// fragment-native copy of W16 for the frag-form projection (d % 64 == 0, ldw % 128 == 0)
bool bf16_frag_supported(int64_t d, int ldw);
hipError_t launch_bf16_frag(hipStream_t s, const unsigned short* Wt16, int64_t d, int ldw, void* Wf);
hipError_t launch_mean_u8(hipStream_t s, const float* mean_r, int64_t d, uint8_t* out, int* bad);
// split form of an fp32 model (EF_OPT_PROJECT_SPLIT_BF16; d % 64 == 0, ldw % 128 == 0): the three
// bf16 pieces of W in fragment order (3 x 2 bytes per element), round(mean) as bytes, the correction
// row; bad[0] / bad[1] count the W elements / mean entries for which the form is not exact
bool split3_supported(int64_t d, int ldw);
hipError_t launch_split3_model(hipStream_t s, const float* W, const float* mean, int64_t d, int ldw, void* Wf3,
                               uint8_t* mean_u8, float* corr, double* corr_part, int nchunk, int* bad);
bool project_split3_ok(int p_dtype, const void* P, int64_t d, int ldw);
int project_split3_nsplit(int64_t bpad, int64_t d, int ldw, int64_t* pix_per_split);
hipError_t launch_project_split3(hipStream_t s, const void* P, int64_t b, int64_t bpad, int64_t d,
                                 const uint8_t* mean_u8, const void* Wf3, int ldw, float* part, int nsplit,
                                 int64_t pps);

// ---- back-projection (ef_recon.hip) ---------------------------------------------------
// R is kept as [kp][recon_dpad(d)] (zero past k and past d).  recon_nsplit: pixel-axis splits of
// a launch over b probes and the 128-pixel tiles each split walks.  launch_recon: qpad holds at
// least round_up(b, 128) rows of kp (zero past b and past k); epi 0 stores mean + f . R as fp32
// into out[b][d], 1 as uint8 (clamped, round half to even), 2 reads the pixels P (p_dtype) and
// writes part[2][nsplit][round_up(b, 128)]: the partial eps^2, then the partial energy, which
// launch_recon_reduce adds in split order into dffs2[b] and (optional) energy[b].
int64_t recon_dpad(int64_t d);
int recon_nsplit(int64_t b, int64_t d, int* tiles_per_split);
hipError_t launch_recon(hipStream_t s, int epi, int p_dtype, const float* qpad, int kp, const float* R, const float* mean,
                        const float* wgt, const void* P, int64_t b, int64_t d, void* out, float* part, int nsplit,
                        int tiles_per_split);
hipError_t launch_recon_reduce(hipStream_t s, const float* part, int nsplit, int64_t b, float* dffs2, float* energy);

}  // namespace ef
