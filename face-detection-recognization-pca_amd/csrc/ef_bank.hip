// Model bank (include/eigenface.h ef_bank_*): any number of (mean, W, gallery) triples resident
// on one context, recognised against in one call whose launch count does not depend on the
// number of models.  Replaces the per-model loop of recognize_face_all_models
// (scan-template-v4.py:289-319): scaler + PCA folded into (mean, W) per person, a gallery of a
// few hundred rows per person, the best similarity kept under a strict '>'.
//
//   bank_project_kernel   one launch over (slot, 128-column tile, K-split, probe tile) items;
//                         the tile body is project_kernel's (ef_project_tile.hpp)
//   bank_reduce_kernel    sums the K-split slabs in fixed order into per-slot padded feature
//                         blocks [bpad][kp_m] (and the caller's feats)
//   bank_search_kernel    every gallery row scored in fp64 with score64, two passes: the minimum
//                         per (probe, slot), then the lowest row inside the tie window
//   bank_merge_kernel     the row slices' answers -> keys and match records
//   bank_best_kernel      the reference's best-over-models walk per probe; with a face gate it
//                         skips the slots whose distance from face space exceeds the bound
// The distance from face space per slot (ef_bank_face_distance, the gated calls) is the grouped
// residual of ef_bank_recon.hip on the feature blocks bank_reduce_kernel leaves.
#include <algorithm>
#include <climits>
#include <cmath>
#include <string>
#include <vector>

#include "ef_project_tile.hpp"
#include "ef_search_common.hpp"

namespace ef {

// A slot's gallery is searched in row slices of a multiple of 32 rows: at most 64 slices per
// slot and about 4096 over the bank, which bounds the per-(slice, probe) scratch.
constexpr int kBankSliceMin = 32;
constexpr int kBankSlotSlices = 64;
constexpr int kBankSlicesTotal = 4096;
constexpr int64_t kBankSearchWgs = 1024;  // the probe tile shrinks (to 8) until the search has this many items
constexpr int kBankPtMax = 128;      // most probes per search work item
// dynamic LDS of a search workgroup: its probes' feature rows + one gallery row per wave.  56 KiB
// beside the 8 KiB of static arrays keeps two workgroups on a CU (160 KiB): the fp64 chains
// are latency-bound and want the waves more than a taller probe tile.
constexpr int kBankLdsBytes = 56 * 1024;
constexpr int kBankPtGlobal = 32;    // probes per item when a feature row does not fit in LDS
constexpr int64_t kBankTargetWgs = 768;  // ~3 projection workgroups per CU (256 CUs)

struct BankProjItem {
  const float* mean;
  const float* W;
  int ldw;        // columns of W
  int col0;       // first column of the tile in W
  int64_t pcol0;  // first column of the tile in the partial slabs
};

struct BankSlotDev {
  const float* G;
  const float* gmax2;
  int64_t n;
  int k, kp;
  int64_t kp_off;     // sum of kp over earlier slots: the slot's feature block is q + bpad * kp_off
  int64_t k_off;      // sum of k over earlier slots: the slot's columns in feats
  int64_t pcol0;      // first column in the partial slabs
  int pt;             // probes per search item
  int lds;            // 1: feature rows and gallery rows go through LDS
  int slice_rows;     // gallery rows per slice
  int nslices;        // row slices
  int64_t slice_off;  // slices of earlier slots
};

// The bank's own K-split: one split count for every item, chosen so that the launch has about
// kBankTargetWgs workgroups, capped at 64 and at the number of 32-pixel stages.
static void bank_split(int64_t b, int64_t d, int64_t coltiles, int* nsplit, int64_t* pps, int64_t* nwg) {
  const int64_t ptiles = (b + BM - 1) / BM;
  const int64_t items = std::max<int64_t>(1, ptiles * coltiles);
  const int64_t steps = (d + BK - 1) / BK;
  int64_t ns = (kBankTargetWgs + items - 1) / items;
  ns = std::min<int64_t>(ns, std::min<int64_t>(64, steps));
  ns = std::max<int64_t>(ns, 1);
  const int64_t steps_per = (steps + ns - 1) / ns;
  *pps = steps_per * BK;
  *nsplit = (int)((d + *pps - 1) / *pps);
  *nwg = ptiles * coltiles * *nsplit;
}

// rows per slice of an n-row gallery in a bank of n_slots slots
static int64_t bank_slice_rows(int64_t n, int64_t n_slots) {
  const int64_t per_slot = std::min<int64_t>(kBankSlotSlices, std::max<int64_t>(1, kBankSlicesTotal / n_slots));
  return round_up(std::max<int64_t>(kBankSliceMin, (n + per_slot - 1) / per_slot), kBankSliceMin);
}

static int bank_search_pt(int kp, int* lds) {
  const int rows = kBankLdsBytes / (kp * 4) - 4;  // 4: one gallery row per wave
  *lds = rows >= 1;
  return rows >= 1 ? std::min(rows, kBankPtMax) : kBankPtGlobal;
}

template <int PDT, bool VEC, bool FAST>
__global__ __launch_bounds__(256, 2) void bank_project_kernel(const BankProjItem* __restrict__ items,
                                                              const void* __restrict__ Pv, int64_t b, int64_t d,
                                                              float* __restrict__ part, int64_t bpad, int64_t ldp,
                                                              int nsplit, int n_ptiles, int64_t pix_per_split) {
  // probe tiles of one (item, split) are neighbours: they read the same piece of W
  const int pt = blockIdx.x % n_ptiles;
  const int rest = blockIdx.x / n_ptiles;
  const int split = rest % nsplit;
  const BankProjItem it = items[rest / nsplit];
  const int64_t k_beg = (int64_t)split * pix_per_split;
  int64_t k_end = k_beg + pix_per_split;
  if (k_end > d) k_end = d;
  project_tile<128, PDT, VEC, FAST>(Pv, b, d, it.mean, it.W, it.ldw, it.col0, (int64_t)pt * BM, k_beg, k_end,
                                    part + (int64_t)split * bpad * ldp + it.pcol0, ldp);
}

// q_m[row][c] = sum_z part[z][row][pcol0_m + c] (fixed z order; 0 for rows >= b and c >= k_m);
// feats[row][k_off_m + c] when requested.  gridDim.y = slots.
__global__ void bank_reduce_kernel(const BankSlotDev* __restrict__ tab, const float* __restrict__ part, int nsplit,
                                   int64_t b, int64_t bpad, int64_t ldp, int64_t total_k, float* __restrict__ q,
                                   float* __restrict__ feats) {
  const BankSlotDev T = tab[blockIdx.y];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= bpad * T.kp) return;
  const int64_t row = i / T.kp;
  const int c = (int)(i - row * T.kp);
  float s = 0.f;
  if (row < b && c < T.k) {
    for (int z = 0; z < nsplit; ++z) s += part[((int64_t)z * bpad + row) * ldp + T.pcol0 + c];
    if (feats) feats[row * total_k + T.k_off + c] = s;
  }
  q[bpad * T.kp_off + i] = s;
}

// Search scratch, one entry per (row slice, probe): entry (slice_off_m + s) * b + p.
struct BankWs {
  double* smin;    // pass 1: the slice's minimum score
  double* sval;    // pass 2: score of the slice's lowest row inside the tie window
  int* srow;       // pass 2: that row, INT_MAX when the slice has none
  double* sscale;  // [slots][b] tie-tolerance scale of the match record
};

// One item = (slot, probe tile, row slice); blockIdx.y = slot, blockIdx.x = tile * slices + slice
// (slots with fewer items leave early).  Each wave takes every fourth row of the slice, stages it
// in LDS and scores it against every probe of the tile with score64 — the call the search's
// reduce and resolve kernels make, so the bits are theirs.
// PASS 1: the minimum per probe.  PASS 2: the minimum over the slot's slices gives the tie window
// of resolve_kernel, and the slice reports its lowest row inside it.
template <int METRIC, int PASS>
__global__ __launch_bounds__(256) void bank_search_kernel(const BankSlotDev* __restrict__ tab,
                                                          const float* __restrict__ q, int64_t b, int64_t bpad,
                                                          int pt_cap, BankWs ws) {
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  __shared__ double swv[4][kBankPtMax];
  __shared__ int swr[4][kBankPtMax];
  __shared__ double sthr[kBankPtMax];
  const BankSlotDev T = tab[blockIdx.y];
  const int nsl = T.nslices;
  const int pt = T.pt < pt_cap ? T.pt : pt_cap;  // probes per item of this launch
  const int64_t npt = (b + pt - 1) / pt;
  if ((int64_t)blockIdx.x >= npt * nsl) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sl = (int)(blockIdx.x % nsl);
  const int64_t p0 = (int64_t)(blockIdx.x / nsl) * pt;
  const int np = (int)(b - p0 < pt ? b - p0 : pt);
  const int kp = T.kp;
  const float* qg = q + bpad * T.kp_off + p0 * kp;
  if (T.lds) {
    const int n4 = np * (kp / 4);
    for (int i = tid; i < n4; i += 256)
      reinterpret_cast<float4*>(dyn)[i] = reinterpret_cast<const float4*>(qg)[i];
  }
  for (int p = tid; p < np; p += 256)
    for (int w = 0; w < 4; ++w) {
      swv[w][p] = INFINITY;
      swr[w][p] = INT_MAX;
    }
  if constexpr (PASS == 2) {
    for (int p = wave; p < np; p += 4) {
      double vmin = INFINITY;
      for (int s = lane; s < nsl; s += 64) {
        const double v = ws.smin[(T.slice_off + s) * b + p0 + p];
        vmin = v < vmin ? v : vmin;
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(vmin, off);
        vmin = o < vmin ? o : vmin;
      }
      double qq = 0.0;  // as reduce_kernel forms the record's scale
      if constexpr (METRIC == EF_METRIC_L2) {
        const float* qp = qg + (int64_t)p * kp;
        for (int c = lane; c < kp; c += 64) qq = fma((double)qp[c], (double)qp[c], qq);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) qq += __shfl_xor(qq, off);
      }
      const double scale = METRIC == EF_METRIC_L2 ? qq + (double)*T.gmax2 : 1.0;
      const double tol = 1e-12 * (fabs(vmin) + scale);
      if (lane == 0) {
        sthr[p] = vmin + tol;
        if (sl == 0) ws.sscale[(int64_t)blockIdx.y * b + p0 + p] = scale;
      }
    }
  }
  __syncthreads();

  const int64_t r0 = (int64_t)sl * T.slice_rows;
  const int64_t r1 = r0 + T.slice_rows < T.n ? r0 + T.slice_rows : T.n;
  auto keep = [&](int p, double v, int64_t row) {
    if (lane != 0) return;
    if constexpr (PASS == 1) {
      if (v < swv[wave][p]) swv[wave][p] = v;
    } else {
      // the wave's rows ascend: its first hit is its lowest
      if (v <= sthr[p] && swr[wave][p] == INT_MAX) {
        swr[wave][p] = (int)row;
        swv[wave][p] = v;
      }
    }
  };
  if (T.lds) {
    float* sg = dyn + (size_t)pt * kp + (size_t)wave * kp;
    for (int64_t row = r0 + wave; row < r1; row += 4) {
      const float* g = T.G + row * kp;
      // the wave's own row buffer: its LDS operations execute in order, the barriers keep the
      // compiler from moving the reads of the previous row below these writes or above them
      __builtin_amdgcn_wave_barrier();
      for (int c = lane * 4; c < kp; c += 256)
        *reinterpret_cast<float4*>(sg + c) = *reinterpret_cast<const float4*>(g + c);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      for (int p = 0; p < np; ++p) keep(p, score64<0, METRIC>(dyn + (size_t)p * kp, sg, lane, kp), row);
    }
  } else {
    for (int64_t row = r0 + wave; row < r1; row += 4) {
      const float* g = T.G + row * kp;
      for (int p = 0; p < np; ++p) keep(p, score64<0, METRIC>(qg + (int64_t)p * kp, g, lane, kp), row);
    }
  }
  __syncthreads();
  for (int p = tid; p < np; p += 256) {
    const int64_t at = (T.slice_off + sl) * b + p0 + p;
    if constexpr (PASS == 1) {
      double vm = INFINITY;
      for (int w = 0; w < 4; ++w) vm = swv[w][p] < vm ? swv[w][p] : vm;
      ws.smin[at] = vm;
    } else {
      int r = INT_MAX;
      double v = INFINITY;
      for (int w = 0; w < 4; ++w)
        if (swr[w][p] < r) {
          r = swr[w][p];
          v = swv[w][p];
        }
      ws.srow[at] = r;
      ws.sval[at] = v;
    }
  }
}

// keys[p][m] (+ match[p][m]): the first slice with a row inside the window holds the lowest one.
__global__ void bank_merge_kernel(const BankSlotDev* __restrict__ tab, int n_slots, int64_t b, BankWs ws,
                                  long long* __restrict__ keys, ef_match* __restrict__ match) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b * n_slots) return;
  const int64_t p = i / n_slots;
  const int m = (int)(i - p * n_slots);
  const BankSlotDev T = tab[m];
  int r = INT_MAX;
  double v = INFINITY;
  for (int s = 0; s < T.nslices && r == INT_MAX; ++s) {
    const int64_t at = (T.slice_off + s) * b + p;
    r = ws.srow[at];
    v = ws.sval[at];
  }
  if (r == INT_MAX) {  // an empty gallery
    keys[i] = LLONG_MAX;
    if (match) match[i] = ef_match{__builtin_inf(), 0.0, LLONG_MAX};
    return;
  }
  const long long key = pack_key((float)v, (unsigned)r);
  keys[i] = key;
  if (match) match[i] = ef_match{v, ws.sscale[(int64_t)m * b + p], key};
}

// scan-template-v4.py:293-309 on the decoded fp32 scores: start from 0.0 (cosine similarity) or
// -inf (negated L2 distance), slots in order, a slot wins only with a strictly greater value.
// GATED: slot m is skipped for probe p when dffs2[p][m] > bound is true (false for NaN), bound =
// gate[m], or fl(gate[m] * energy[p][m]) when relative.
template <bool GATED>
__global__ void bank_best_kernel(const long long* __restrict__ keys, int n_slots, int64_t b, int metric,
                                 const float* __restrict__ gate, int relative, const float* __restrict__ dffs2,
                                 const float* __restrict__ energy, int* __restrict__ best_slot) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= b) return;
  float best = metric == EF_METRIC_L2 ? -__builtin_inff() : 0.0f;
  int slot = -1;
  for (int m = 0; m < n_slots; ++m) {
    const long long key = keys[p * n_slots + m];
    if (key == LLONG_MAX) continue;
    if constexpr (GATED) {
      const float bound = relative ? __fmul_rn(gate[m], energy[p * n_slots + m]) : gate[m];
      if (dffs2[p * n_slots + m] > bound) continue;
    }
    const float val = -key_value(key);  // the key holds the distance, or minus the similarity
    if (val > best) {
      best = val;
      slot = m;
    }
  }
  best_slot[p] = slot;
}

static int bank_tables(ef_ctx* c) {
  Bank& bk = c->bank;
  if (bk.tables_valid) return EF_OK;
  std::vector<BankProjItem> items;
  std::vector<BankSlotDev> tab;
  std::vector<BankReconDev> rtab;
  int64_t kp_off = 0, k_off = 0, pcol = 0, slice_off = 0;
  int lds_bytes = 0, kp_max = 0, recon_rk = 32;
  for (const BankSlot& slot : bk.slots) {
    const Gallery& s = slot.g;
    BankSlotDev t{};
    t.G = static_cast<const float*>(s.G.p);
    t.gmax2 = static_cast<const float*>(s.gmax2.p);
    t.n = s.n;
    t.k = s.k;
    t.kp = s.kp;
    t.kp_off = kp_off;
    t.k_off = k_off;
    t.pcol0 = pcol;
    t.pt = bank_search_pt(s.kp, &t.lds);
    t.slice_rows = (int)bank_slice_rows(s.n, (int64_t)bk.slots.size());
    t.nslices = (int)((s.n + t.slice_rows - 1) / t.slice_rows);
    t.slice_off = slice_off;
    if (t.lds) lds_bytes = std::max(lds_bytes, (t.pt + 4) * s.kp * 4);
    kp_max = std::max(kp_max, s.kp);
    for (int col = 0; col < slot.kpw; col += 128)
      items.push_back(BankProjItem{static_cast<const float*>(slot.mean.p), static_cast<const float*>(slot.W.p), slot.kpw, col,
                                   pcol + col});
    tab.push_back(t);
    rtab.push_back(BankReconDev{slot.recon ? static_cast<const float*>(slot.recon_R.p) : nullptr,
                                static_cast<const float*>(slot.mean.p), static_cast<const float*>(slot.recon_w.p), s.kp,
                                kp_off});
    if (s.kp == 16) recon_rk = 16;
    kp_off += s.kp;
    k_off += s.k;
    pcol += slot.kpw;
    slice_off += t.nslices;
  }
  EF_TRY(ensure(c, bk.proj_items, items.size() * sizeof(BankProjItem)));
  EF_TRY(ensure(c, bk.slot_tab, tab.size() * sizeof(BankSlotDev)));
  EF_TRY(ensure(c, bk.recon_tab, rtab.size() * sizeof(BankReconDev)));
  // the stream may still read the old tables: the copies are ordered on it, and waited for
  // because they read these host vectors
  EF_HIP(c, hipMemcpyAsync(bk.proj_items.p, items.data(), items.size() * sizeof(BankProjItem), hipMemcpyHostToDevice,
                           c->stream), "bank tables");
  EF_HIP(c, hipMemcpyAsync(bk.slot_tab.p, tab.data(), tab.size() * sizeof(BankSlotDev), hipMemcpyHostToDevice,
                           c->stream), "bank tables");
  EF_HIP(c, hipMemcpyAsync(bk.recon_tab.p, rtab.data(), rtab.size() * sizeof(BankReconDev), hipMemcpyHostToDevice,
                           c->stream), "bank tables");
  EF_HIP(c, hipStreamSynchronize(c->stream), "bank tables");
  bk.recon_rk = recon_rk;
  bk.total_slices = slice_off;
  bk.search_lds = lds_bytes;
  bk.kp_max = kp_max;
  bk.tables_valid = true;
  return EF_OK;
}

template <int PDT>
static hipError_t bank_project_t(hipStream_t s, const BankProjItem* items, int64_t n_items, const void* P, int64_t b,
                                 int64_t bpad, int64_t d, float* part, int64_t ldp, int nsplit, int64_t pps) {
  const int n_ptiles = (int)(bpad / BM);
  const int64_t wgs = n_items * nsplit * n_ptiles;
  if (wgs > INT_MAX) return hipErrorInvalidValue;
  const dim3 grid((unsigned)wgs);
  const bool vec = (d % 16 == 0) && ((reinterpret_cast<uintptr_t>(P) & 15) == 0) && (pps % 16 == 0);
  const bool fast = PDT == EF_U8 && vec && d % BK == 0 && pps % BK == 0 && b >= 1;
  if (fast)
    hipLaunchKernelGGL((bank_project_kernel<PDT, true, true>), grid, dim3(256), 0, s, items, P, b, d, part, bpad, ldp,
                       nsplit, n_ptiles, pps);
  else if (vec)
    hipLaunchKernelGGL((bank_project_kernel<PDT, true, false>), grid, dim3(256), 0, s, items, P, b, d, part, bpad, ldp,
                       nsplit, n_ptiles, pps);
  else
    hipLaunchKernelGGL((bank_project_kernel<PDT, false, false>), grid, dim3(256), 0, s, items, P, b, d, part, bpad,
                       ldp, nsplit, n_ptiles, pps);
  return hipGetLastError();
}

template <int METRIC>
static hipError_t bank_search_t(hipStream_t s, const BankSlotDev* tab, int n_slots, int64_t items_max, int lds,
                                const float* q, int64_t b, int64_t bpad, int pt_cap, const BankWs& ws) {
  const dim3 grid((unsigned)items_max, (unsigned)n_slots);
  hipLaunchKernelGGL((bank_search_kernel<METRIC, 1>), grid, dim3(256), lds, s, tab, q, b, bpad, pt_cap, ws);
  hipLaunchKernelGGL((bank_search_kernel<METRIC, 2>), grid, dim3(256), lds, s, tab, q, b, bpad, pt_cap, ws);
  return hipGetLastError();
}

static BankWs carve_bank_ws(Carve& cv, size_t entries, size_t scales) {
  return BankWs{cv.take<double>(entries), cv.take<double>(entries), cv.take<int>(entries), cv.take<double>(scales)};
}

// The grouped projection and its reduce: the bank's feature blocks bk.q (and fdev) of b probes.
static int bank_project_dev(ef_ctx* c, const void* Pd, int p_dtype, int64_t b, float* fdev) {
  Bank& bk = c->bank;
  const int64_t M = (int64_t)bk.slots.size();
  const int64_t bpad = round_up(b, BM);
  const int64_t coltiles = bk.total_kpw / 128;
  int ns = 0;
  int64_t pps = 0, nwg = 0;
  bank_split(b, bk.d, coltiles, &ns, &pps, &nwg);
  EF_TRY(ensure(c, bk.part, (size_t)ns * bpad * bk.total_kpw * sizeof(float)));
  EF_TRY(ensure(c, bk.q, (size_t)bpad * bk.total_kp * sizeof(float)));
  const BankProjItem* items = static_cast<const BankProjItem*>(bk.proj_items.p);
  const BankSlotDev* tab = static_cast<const BankSlotDev*>(bk.slot_tab.p);
  float* part = static_cast<float*>(bk.part.p);
  float* q = static_cast<float*>(bk.q.p);
  TimerEvt t;
  timer_begin(c, EF_KERNEL_PROJECT, &t);
  EF_HIP(c,
         p_dtype == EF_U8 ? bank_project_t<EF_U8>(c->stream, items, coltiles, Pd, b, bpad, bk.d, part, bk.total_kpw, ns, pps)
                          : bank_project_t<EF_F32>(c->stream, items, coltiles, Pd, b, bpad, bk.d, part, bk.total_kpw, ns, pps),
         "bank projection");
  timer_end(c, &t);
  {
    const int64_t tot = bpad * bk.kp_max;
    hipLaunchKernelGGL(bank_reduce_kernel, dim3((unsigned)((tot + 255) / 256), (unsigned)M), dim3(256), 0, c->stream, tab,
                       part, ns, b, bpad, bk.total_kpw, bk.total_k, q, fdev);
    EF_HIP(c, hipGetLastError(), "bank reduce");
  }
  return EF_OK;
}

// The grouped residual and its reduce on the feature blocks bank_project_dev left: dffs2[b][M]
// and (optional) energy[b][M].  The caller has checked that every slot has its R.
static int bank_residual_dev(ef_ctx* c, const void* Pd, int p_dtype, int64_t b, float* dffs2, float* energy) {
  Bank& bk = c->bank;
  const int M = (int)bk.slots.size();
  const int64_t bpad = round_up(b, BM);
  const BankReconPlan pl = bank_recon_plan(b, bk.d, M);
  EF_TRY(ensure(c, bk.recon_part, (size_t)pl.scratch_bytes));
  float* part = static_cast<float*>(bk.recon_part.p);
  TimerEvt t;
  timer_begin(c, EF_KERNEL_RECON, &t);
  EF_HIP(c,
         launch_bank_recon(c->stream, static_cast<const BankReconDev*>(bk.recon_tab.p), M, bk.recon_rk, p_dtype,
                           static_cast<const float*>(bk.q.p), Pd, b, bpad, bk.d, part, pl),
         "bank residual kernel");
  timer_end(c, &t);
  timer_begin(c, EF_KERNEL_RECON_REDUCE, &t);
  EF_HIP(c, launch_bank_recon_reduce(c->stream, part, pl.nsplit, M, b, bpad, dffs2, energy), "bank residual reduce");
  timer_end(c, &t);
  return EF_OK;
}

// The launches of one recognise call on device pointers (ef_internal.hpp).
int bank_recognize_dev(ef_ctx* c, const void* Pd, int p_dtype, int64_t b, int metric, long long* kdev, ef_match* mdev,
                       int* sdev, float* fdev, const BankGate* gate) {
  Bank& bk = c->bank;
  EF_TRY(bank_tables(c));
  const int64_t M = (int64_t)bk.slots.size();
  const int64_t bpad = round_up(b, BM);
  EF_TRY(bank_project_dev(c, Pd, p_dtype, b, fdev));
  if (gate) EF_TRY(bank_residual_dev(c, Pd, p_dtype, b, gate->dffs2, gate->energy));
  const BankSlotDev* tab = static_cast<const BankSlotDev*>(bk.slot_tab.p);
  const float* q = static_cast<const float*>(bk.q.p);
  TimerEvt t;

  // search: at least one entry per slot, so an empty slot's entry reads "no row"
  // the probe tile of this call: the largest of 128 .. 8 that gives the launch kBankSearchWgs items
  // (small banks and batches get small tiles: the fp64 chains need the waves, and the gallery
  // rows a smaller tile re-reads come from L2)
  int64_t items_max = 1;
  int pt_cap = kBankPtMax;
  for (;; pt_cap /= 2) {
    int64_t items = 0;
    items_max = 1;
    for (const BankSlot& slot : bk.slots) {
      const Gallery& s = slot.g;
      int lds = 0;
      const int pt = std::min(bank_search_pt(s.kp, &lds), pt_cap);
      const int64_t rows = bank_slice_rows(s.n, M);
      const int64_t it = (b + pt - 1) / pt * ((s.n + rows - 1) / rows);
      items += it;
      items_max = std::max(items_max, it);
    }
    if (items >= kBankSearchWgs || pt_cap <= 8) break;
  }
  const size_t entries = (size_t)std::max<int64_t>(bk.total_slices, 1) * (size_t)b;
  Carve size_ws, cvw;
  carve_bank_ws(size_ws, entries, (size_t)(M * b));
  EF_TRY(ensure(c, bk.ws, size_ws.total));
  cvw.base = bk.ws.p;
  const BankWs ws = carve_bank_ws(cvw, entries, (size_t)(M * b));
  timer_begin(c, EF_KERNEL_SEARCH, &t);
  if (bk.total_slices > 0)
    EF_HIP(c,
           metric == EF_METRIC_L2
               ? bank_search_t<EF_METRIC_L2>(c->stream, tab, (int)M, items_max, bk.search_lds, q, b, bpad, pt_cap, ws)
               : bank_search_t<EF_METRIC_COSINE>(c->stream, tab, (int)M, items_max, bk.search_lds, q, b, bpad, pt_cap,
                                                 ws),
           "bank search");
  hipLaunchKernelGGL(bank_merge_kernel, dim3((unsigned)((b * M + 255) / 256)), dim3(256), 0, c->stream, tab, (int)M, b, ws,
                     kdev, mdev);
  if (sdev && gate)
    hipLaunchKernelGGL(bank_best_kernel<true>, dim3((unsigned)((b + 255) / 256)), dim3(256), 0, c->stream, kdev, (int)M,
                       b, metric, gate->gate, gate->relative ? 1 : 0, gate->dffs2, gate->energy, sdev);
  else if (sdev)
    hipLaunchKernelGGL(bank_best_kernel<false>, dim3((unsigned)((b + 255) / 256)), dim3(256), 0, c->stream, kdev, (int)M,
                       b, metric, nullptr, 0, nullptr, nullptr, sdev);
  EF_HIP(c, hipGetLastError(), "bank merge");
  timer_end(c, &t);
  return EF_OK;
}

// EF_E_STATE naming the first slot without reconstruction state (ef_internal.hpp)
int bank_recon_complete(ef_ctx* c, const char* who) {
  const std::vector<BankSlot>& slots = c->bank.slots;
  for (size_t m = 0; m < slots.size(); ++m)
    if (!slots[m].recon)
      return set_err(c, EF_E_STATE, std::string(who) + ": slot " + std::to_string(m) +
                                        " has no reconstruction state (call ef_bank_recon_set)");
  return EF_OK;
}

}  // namespace ef

using namespace ef;

extern "C" {

int ef_bank_schedule(int64_t b, int64_t d, const int32_t* k, int32_t n_models, int32_t* nsplit,
                     int64_t* pix_per_split, int64_t* n_workgroups, int64_t* scratch_bytes) {
  if (b < 1 || b > EF_BANK_MAX_PROBES || d < 1 || !k || n_models < 1 || n_models > EF_BANK_MAX_MODELS)
    return EF_E_INVALID;
  int64_t coltiles = 0, total_kp = 0;
  for (int i = 0; i < n_models; ++i) {
    if (k[i] < 1) return EF_E_INVALID;
    const int kp = feature_pad(k[i]);
    if (kp < 0) return EF_E_INVALID;
    coltiles += (kp + 127) / 128;
    total_kp += kp;
  }
  int ns = 0;
  int64_t pps = 0, nwg = 0;
  bank_split(b, d, coltiles, &ns, &pps, &nwg);
  const int64_t bpad = round_up(b, BM);
  if (nsplit) *nsplit = ns;
  if (pix_per_split) *pix_per_split = pps;
  if (n_workgroups) *n_workgroups = nwg;
  if (scratch_bytes) *scratch_bytes = ((int64_t)ns * coltiles * 128 + total_kp) * bpad * (int64_t)sizeof(float);
  return EF_OK;
}

int ef_bank_clear(ef_ctx* c) {
  if (!c) return EF_E_INVALID;
  (void)hipSetDevice(c->device);
  EF_HIP(c, hipStreamSynchronize(c->stream), "hipStreamSynchronize");
  c->bank = Bank{};
  return EF_OK;
}

int ef_bank_info(const ef_ctx* c, int32_t* n_models, int64_t* d, int64_t* total_k, int64_t* total_rows) {
  if (!c) return EF_E_INVALID;
  if (n_models) *n_models = (int32_t)c->bank.slots.size();
  if (d) *d = c->bank.d;
  if (total_k) *total_k = c->bank.total_k;
  if (total_rows) *total_rows = c->bank.total_rows;
  return EF_OK;
}

int ef_bank_add(ef_ctx* c, const float* mean, const float* W, int64_t d, int32_t k, const float* G, int64_t n,
                uint32_t flags, int32_t* slot_out) {
  if (!c) return EF_E_INVALID;
  if (!mean || !W || d < 1 || k < 1 || n < 0 || (!G && n > 0) || n >= (int64_t)INT_MAX)
    return set_err(c, EF_E_INVALID, "ef_bank_add: bad arguments");
  const int kp = feature_pad(k);
  if (kp < 0) return set_err(c, EF_E_INVALID, "ef_bank_add: k > 65536 is not supported");
  if (flags & EF_MODEL_BF16) return set_err(c, EF_E_INVALID, "ef_bank_add: the bank projects in fp32 only");
  Bank& bk = c->bank;
  if (!bk.slots.empty() && d != bk.d) return set_err(c, EF_E_INVALID, "ef_bank_add: d differs from the bank's");
  if (bk.slots.size() >= EF_BANK_MAX_MODELS) return set_err(c, EF_E_INVALID, "ef_bank_add: the bank is full");
  (void)hipSetDevice(c->device);
  BankSlot s;  // built here, appended only when complete: a failure below frees it and changes nothing
  s.kpw = (kp + 127) / 128 * 128;
  DevBuf tmp_w, tmp_g;  // host sources staged unpadded; freed after the synchronise below
  EF_TRY(weights_load(c, s.mean, s.W, mean, W, d, k, s.kpw, flags, tmp_w));
  EF_TRY(gallery_load(c, s.g, G, n, k, flags, tmp_g, nullptr));
  EF_HIP(c, hipStreamSynchronize(c->stream), "ef_bank_add");
  try {
    bk.slots.push_back(std::move(s));
  } catch (const std::bad_alloc&) {
    return set_err(c, EF_E_NOMEM, "ef_bank_add: host allocation failed");
  }
  bk.d = d;
  bk.total_k += k;
  bk.total_kp += kp;
  bk.total_kpw += bk.slots.back().kpw;
  bk.total_rows += n;
  bk.tables_valid = false;
  if (slot_out) *slot_out = (int32_t)bk.slots.size() - 1;
  return EF_OK;
}

// ef_bank_recognize and ef_bank_recognize_gated: gate null is the former, with exactly its launches
static int bank_recognize_call(ef_ctx* c, const char* who, const void* P, int32_t p_dtype, int64_t b, int32_t metric,
                               const float* gate, int64_t* keys, ef_match* matches, int32_t* best_slot, float* dffs2,
                               float* energy, float* feats, uint32_t flags) {
  if (!c) return EF_E_INVALID;
  Bank& bk = c->bank;
  const std::string w(who);
  if (bk.slots.empty()) return set_err(c, EF_E_STATE, w + ": the bank is empty (call ef_bank_add)");
  if (c->comm && c->comm_size > 1) return set_err(c, EF_E_STATE, w + ": not available with a communicator attached");
  if (gate) EF_TRY(bank_recon_complete(c, who));
  if (!P || !keys || b < 0 || b > EF_BANK_MAX_PROBES || (p_dtype != EF_U8 && p_dtype != EF_F32) ||
      (metric != EF_METRIC_L2 && metric != EF_METRIC_COSINE) || (gate && !dffs2))
    return set_err(c, EF_E_INVALID, w + ": bad arguments");
  if (b == 0) return EF_OK;
  (void)hipSetDevice(c->device);
  EF_TRY(bank_tables(c));
  const bool dev = flags & EF_MEM_DEVICE;
  const int64_t M = (int64_t)bk.slots.size();

  const void* Pd = nullptr;
  EF_TRY(stage_probes(c, P, p_dtype, b, bk.d, flags, bk.p_stage, &Pd));
  // where the kernels write: the caller's device pointers, or the staging of a host call; the
  // best slots are this call's own extension of it
  Results r{dev, b, (int)M, bk.total_k, keys, matches, feats};
  EF_TRY(r.stage_feats(c));
  EF_TRY(r.stage_keys(c, b));
  int* sdev = best_slot;
  if (!dev && best_slot) {
    EF_TRY(ensure(c, bk.out, (size_t)b * sizeof(int)));
    sdev = static_cast<int*>(bk.out.p);
  }
  BankGate g{gate, (flags & EF_BANK_GATE_RELATIVE) != 0, dffs2, energy};
  const size_t bm = (size_t)(b * M);
  if (gate && (!dev || !energy)) {
    // [eps^2 | E | gate]: the host call's staging; a device call with no energy output only needs E's
    EF_TRY(ensure(c, bk.recon_out, (2 * bm + (size_t)M) * sizeof(float)));
    float* o = static_cast<float*>(bk.recon_out.p);
    if (!dev) {
      EF_HIP(c, hipMemcpyAsync(o + 2 * bm, gate, (size_t)M * sizeof(float), hipMemcpyHostToDevice, c->stream), "H2D gate");
      g.gate = o + 2 * bm;
      g.dffs2 = o;
    }
    if (!dev || !energy) g.energy = o + bm;
  }
  EF_TRY(bank_recognize_dev(c, Pd, p_dtype, b, metric, r.kdev, r.mdev, sdev, r.fdev, gate ? &g : nullptr));
  if (!dev && best_slot)
    EF_HIP(c, hipMemcpyAsync(best_slot, sdev, (size_t)b * sizeof(int), hipMemcpyDeviceToHost, c->stream), "D2H best slot");
  if (!dev && gate) {
    EF_HIP(c, hipMemcpyAsync(dffs2, g.dffs2, bm * sizeof(float), hipMemcpyDeviceToHost, c->stream), "D2H distances");
    if (energy) EF_HIP(c, hipMemcpyAsync(energy, g.energy, bm * sizeof(float), hipMemcpyDeviceToHost, c->stream), "D2H energy");
  }
  return r.fetch(c);
}

int ef_bank_recognize(ef_ctx* c, const void* P, int32_t p_dtype, int64_t b, int32_t metric, int64_t* keys,
                      ef_match* matches, int32_t* best_slot, float* feats, uint32_t flags) {
  return bank_recognize_call(c, "ef_bank_recognize", P, p_dtype, b, metric, nullptr, keys, matches, best_slot, nullptr,
                             nullptr, feats, flags);
}

int ef_bank_recognize_gated(ef_ctx* c, const void* P, int32_t p_dtype, int64_t b, int32_t metric, const float* gate,
                            int64_t* keys, ef_match* matches, int32_t* best_slot, float* dffs2, float* energy,
                            float* feats, uint32_t flags) {
  if (!c) return EF_E_INVALID;
  if (!gate) return set_err(c, EF_E_INVALID, "ef_bank_recognize_gated: bad arguments");
  return bank_recognize_call(c, "ef_bank_recognize_gated", P, p_dtype, b, metric, gate, keys, matches, best_slot, dffs2,
                             energy, feats, flags);
}

int ef_bank_recon_set(ef_ctx* c, int32_t slot, const float* R, const float* weight, uint32_t flags) {
  if (!c) return EF_E_INVALID;
  Bank& bk = c->bank;
  if (slot < 0 || (size_t)slot >= bk.slots.size())
    return set_err(c, EF_E_INVALID, "ef_bank_recon_set: slot " + std::to_string(slot) + " is outside the bank");
  if (!R) return set_err(c, EF_E_INVALID, "ef_bank_recon_set: bad arguments");
  if (bk.d > (int64_t)INT_MAX - 128) return set_err(c, EF_E_INVALID, "ef_bank_recon_set: d >= 2^31 - 128 is not supported");
  (void)hipSetDevice(c->device);
  BankSlot& s = bk.slots[(size_t)slot];
  const int64_t d = bk.d, dp = recon_dpad(d);
  const int k = s.g.k, kp = s.g.kp;
  const bool dev = (flags & EF_MEM_DEVICE) != 0;
  std::vector<float> ones;
  DevBuf Rn, wn, staging;  // built here, published only when complete: a failure below changes nothing
  EF_TRY(ensure(c, Rn, (size_t)kp * dp * sizeof(float)));
  EF_TRY(ensure(c, wn, (size_t)d * sizeof(float)));
  if (!dev) {
    EF_TRY(ensure(c, staging, (size_t)k * d * sizeof(float)));
    EF_HIP(c, hipMemcpyAsync(staging.p, R, (size_t)k * d * sizeof(float), hipMemcpyHostToDevice, c->stream), "copy R");
    R = static_cast<const float*>(staging.p);
  }
  EF_HIP(c, launch_pad_rows(c->stream, R, k, (int)d, kp, static_cast<float*>(Rn.p), (int)dp), "pad R");
  if (!weight) {
    try {
      ones.assign((size_t)d, 1.f);
    } catch (const std::bad_alloc&) {
      return set_err(c, EF_E_NOMEM, "ef_bank_recon_set: host allocation failed");
    }
    weight = ones.data();
  }
  EF_HIP(c,
         hipMemcpyAsync(wn.p, weight, (size_t)d * sizeof(float),
                        dev && ones.empty() ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream),
         "copy weight");
  // also behind every queued kernel that reads the slot's previous R
  EF_HIP(c, hipStreamSynchronize(c->stream), "ef_bank_recon_set");
  s.recon_R = std::move(Rn);
  s.recon_w = std::move(wn);
  s.recon = true;
  bk.tables_valid = false;
  return EF_OK;
}

int ef_bank_face_distance(ef_ctx* c, const void* P, int32_t p_dtype, int64_t b, float* dffs2, float* energy, float* feats,
                          uint32_t flags) {
  if (!c) return EF_E_INVALID;
  Bank& bk = c->bank;
  if (bk.slots.empty()) return set_err(c, EF_E_STATE, "ef_bank_face_distance: the bank is empty (call ef_bank_add)");
  if (c->comm && c->comm_size > 1)
    return set_err(c, EF_E_STATE, "ef_bank_face_distance: not available with a communicator attached");
  EF_TRY(bank_recon_complete(c, "ef_bank_face_distance"));
  if (b < 0 || b > EF_BANK_MAX_PROBES || (p_dtype != EF_U8 && p_dtype != EF_F32) || (b > 0 && (!P || !dffs2)))
    return set_err(c, EF_E_INVALID, "ef_bank_face_distance: bad arguments");
  if (b == 0) return EF_OK;
  (void)hipSetDevice(c->device);
  EF_TRY(bank_tables(c));
  const bool dev = flags & EF_MEM_DEVICE;
  const int64_t M = (int64_t)bk.slots.size();
  const void* Pd = nullptr;
  EF_TRY(stage_probes(c, P, p_dtype, b, bk.d, flags, bk.p_stage, &Pd));
  Results r{dev, b, (int)M, bk.total_k, nullptr, nullptr, feats};
  EF_TRY(r.stage_feats(c));
  const size_t bm = (size_t)(b * M);
  float* ddev = dffs2;
  float* edev = energy;
  if (!dev) {
    EF_TRY(ensure(c, bk.recon_out, 2 * bm * sizeof(float)));
    ddev = static_cast<float*>(bk.recon_out.p);
    edev = energy ? ddev + bm : nullptr;
  }
  EF_TRY(bank_project_dev(c, Pd, p_dtype, b, r.fdev));
  EF_TRY(bank_residual_dev(c, Pd, p_dtype, b, ddev, edev));
  if (!dev) {
    EF_HIP(c, hipMemcpyAsync(dffs2, ddev, bm * sizeof(float), hipMemcpyDeviceToHost, c->stream), "D2H distances");
    if (energy) EF_HIP(c, hipMemcpyAsync(energy, edev, bm * sizeof(float), hipMemcpyDeviceToHost, c->stream), "D2H energy");
  }
  return r.fetch(c);
}

}  // extern "C"
