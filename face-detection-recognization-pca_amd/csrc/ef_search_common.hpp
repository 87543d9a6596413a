// Device and host helpers shared by the search kernels (ef_search.hip, ef_search_wide.hip,
// and the diagnostic-only ef_search_screen.hip): the arg-best contract (top-2 merge, tie
// rule, per-chunk partial records, COLLECT), the XCD block deal, and the wide kernels'
// common chunk / DMA geometry.
#pragma once

#include <climits>

#include "ef_dma.hpp"
#include "ef_internal.hpp"

namespace ef {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));

// min / max of three floats as one v_min3_f32 / v_max3_f32, without the compiler's IEEE-mode
// canonicalisation of each input (scores are finite or +-inf, never NaN)
__device__ __forceinline__ float min3_raw(float a, float b, float c) {
  float r;
  asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
__device__ __forceinline__ float max3_raw(float a, float b, float c) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
// 16 bytes (a float4 from LDS, a register quad) as a bf16x8 MFMA operand
template <typename T>
__device__ __forceinline__ bf16x8 as_bf16x8(const T& v) {
  static_assert(sizeof(T) == 16, "one 16-byte fragment");
  bf16x8 r;
  __builtin_memcpy(&r, &v, 16);
  return r;
}

__device__ __forceinline__ long long pack_key(float v, unsigned idx) {
  if (v == 0.0f) v = 0.0f;  // canonical +0 so that -0 and +0 tie on index
  int b = __float_as_int(v);
  int s = b >= 0 ? b : (b ^ 0x7FFFFFFF);
  return (long long)(((unsigned long long)(unsigned)s << 32) | (unsigned long long)idx);
}
__device__ __forceinline__ float key_value(long long key) {
  const int s = (int)(key >> 32);
  return __int_as_float(s >= 0 ? s : (s ^ 0x7FFFFFFF));
}

// ---- the arg-best contract ------------------------------------------------------------
// A running record is (b1 best score, b2 runner-up score, i1 row of the best; i1 = INT_MAX
// while empty).  Merge another record of the same probe over disjoint rows into it: the
// lower score wins, equal scores go to the lower row (np.argmin / np.argmax order).
__device__ __forceinline__ void top2_merge(float& b1, float& b2, int& i1, float ob1, float ob2, int oi1) {
  const bool other = ob1 < b1 || (ob1 == b1 && oi1 < i1);
  const float lose = other ? b1 : ob1;
  b2 = fminf(fminf(b2, ob2), lose);
  // selects, not `if (other) { b1 = ob1; i1 = oi1; }`: through the references that form
  // becomes exec-masked branches (+23 instructions in search_kernel's epilogue, 3 more
  // spilled VGPRs in search_kernel<128, cosine>)
  b1 = other ? ob1 : b1;
  i1 = other ? oi1 : i1;
}
// Publish a chunk's record for one probe at chunk_base + slot, chunk_base = chunk * bpad
// (reduce_kernel takes the min key over chunks and the min runner-up); an empty chunk
// publishes no candidate.  Base and slot are separate arguments, added once per store as the
// kernels always wrote it: with the sum passed in, the compiler shares the two helpers'
// stores and the kernels' prologues and epilogues change.
__device__ __forceinline__ void top2_store(const SearchWs& ws, int64_t chunk_base, int64_t slot, float b1, float b2,
                                           int i1) {
  ws.part_key[chunk_base + slot] = i1 == INT_MAX ? LLONG_MAX : pack_key(b1, (unsigned)i1);
  ws.part_b2[chunk_base + slot] = b2;
}
__device__ __forceinline__ void top2_store_empty(const SearchWs& ws, int64_t chunk_base, int64_t slot) {
  ws.part_key[chunk_base + slot] = LLONG_MAX;
  ws.part_b2[chunk_base + slot] = __builtin_inff();
}
// COLLECT pass: queue row row_base + row_off for the fp64 resolution of queued probe `slot`
// when its fp32 score is within the slot's threshold (at most ws.cand_cap rows are kept:
// kCandMax for the top-1 search, whose resolve_kernel re-scans the gallery past it).  The row comes in two parts so that it is formed only on a hit: passed as
// one value, the 16 rows of an unrolled block are computed ahead of the compares and cost up
// to 10 VGPRs (search_kernel<64, .., COLLECT>: 96 -> 106).
__device__ __forceinline__ void collect_hit(const SearchWs& ws, int64_t slot, float thr, float score, int row_base,
                                            int row_off) {
  if (score <= thr) {
    const int pos = atomicAdd(&ws.cand_cnt[slot], 1);
    if (pos < ws.cand_cap) ws.cand[slot * ws.cand_cap + pos] = row_base + row_off;
  }
}
// the slot's COLLECT threshold (main pass, or a slot past the queue: nothing qualifies)
template <bool COLLECT>
__device__ __forceinline__ float collect_threshold(const SearchWs& ws, int64_t slot, int n_amb) {
  float thr = -__builtin_inff();
  if constexpr (COLLECT) {
    if (slot < n_amb) thr = ws.thr[slot];
  }
  return thr;
}

// ---- labelled scan (ef_search_labelled) ----------------------------------
// What a lane keeps of its probe for the whole sweep: the probe's label and its excluded
// local row, less the lane half's row offset 4 h (so a block's row base plus a constant is
// compared against it).  other / any are wave-uniform: the relation.
struct LabelLane {
  int plab, excl_h;
  bool other, any;
};
__device__ __forceinline__ LabelLane label_lane(const SearchWs& ws, int64_t probe, int h) {
  return LabelLane{ws.plab[probe], ws.pexcl[probe] - 4 * h, ws.lbl == EF_LABEL_OTHER + 1, ws.lbl == EF_LABEL_ANY + 1};
}
// Scores of one finished 32-row block (register r <-> row rowbase + (r & 3) + 8 (r >> 2) + 4 h)
// whose row does not qualify become +inf, as the rows past the gallery's end do: the arg-best
// epilogue and COLLECT then see the sub-gallery of qualifying rows.  labs: the block's 32 row
// labels staged in LDS (not read for EF_LABEL_ANY, which has none).
__device__ __forceinline__ void label_mask(f32x16& v, const float* labs, int rowbase, int h, const LabelLane& L) {
  // the label reads stay behind the block's MFMAs: hoisted above them by the scheduler, their 16
  // registers per block would be live across the chain (search_kernel then spills at every KP)
  __builtin_amdgcn_sched_barrier(0);
  // the excluded row relative to the block, compared against the 16 constants 8 q + j.  Opaque:
  // left to itself the compiler hoists 32 loop-invariant 64-bit values excl_h - (8 q + j) out of
  // the sweep (64 VGPRs; search_kernel<16> went from 76 VGPRs to 128 and spilled)
  int d = L.excl_h - rowbase;
  asm volatile("" : "+v"(d));
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (q == 2) __builtin_amdgcn_sched_barrier(0);  // two reads in flight at a time: 8 registers, not 16
    const float4 x = *reinterpret_cast<const float4*>(labs + 8 * q + 4 * h);
    const int l[4] = {__float_as_int(x.x), __float_as_int(x.y), __float_as_int(x.z), __float_as_int(x.w)};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool keep = (((l[j] == L.plab) != L.other) || L.any) && (d != 8 * q + j);
      v[4 * q + j] = keep ? v[4 * q + j] : __builtin_inff();
    }
  }
}
// the same rule for one row, all lanes of a wave alike (resolve_kernel's sweep)
__device__ __forceinline__ bool label_row_ok(const SearchWs& ws, int64_t probe, int64_t row) {
  if (row == ws.pexcl[probe]) return false;
  if (ws.lbl == EF_LABEL_ANY + 1) return true;
  return (ws.glab[row] == ws.plab[probe]) != (ws.lbl == EF_LABEL_OTHER + 1);
}

// Rigorous bound on |scan score - exact score| (fp32 FMA chain of kpv terms, fp32 ||g||^2 /
// 1/||g||, final rounding), doubled for two compared scores and doubled again as a safety
// factor: delta = 4 e.  S3 is the scan's arithmetic (0 fp32, 1 split bf16, 2 single bf16),
// qn = fp32 ||q||, b1 the score the bound is taken at.  reduce_kernel queues a probe whose
// runner-up is within delta of the winner; topk_threshold_kernel widens its cut by it.
template <int METRIC, int S3>
__device__ __forceinline__ float scan_delta(int kpv, float qn, float gmax2, float b1) {
  const float u = 5.9604645e-08f;  // 2^-24
  float delta;
  if constexpr (S3 == 2) {
    // single-bf16 chain: |x - bf16(x)| <= 2^-8 |x| for both operands, so each product is
    // within (2 + 2^-8) 2^-8 |q||g| of the exact one (2.01 2^-8 taken); KP exact products +
    // the start value summed in fp32 (2u per add allowed), ||g||^2 itself to KP u
    const float es = 2.01f * 3.90625e-03f;  // 2.01 * 2^-8
    if constexpr (METRIC == EF_METRIC_L2) {
      const float gm = sqrtf(gmax2);
      delta = 2.f * (2.f * es * qn * gm + (kpv + 4) * 2.f * u * 1.01f * (2.02f * qn * gm + gmax2) +
                     kpv * u * gmax2 + 4.f * u * fabsf(b1)) + 1e-30f;
    } else {
      delta = 2.f * ((es + (kpv + 8) * 2.f * u) * 1.01f * qn) + 1e-30f;
    }
  } else if constexpr (S3 == 1) {
    // split-bf16 chain: dropped terms (lo.lo', hi.e', lo.e', e.q) <= 3.02 * 2^-16 |q||g| per
    // element, 3 KP exact products + the start value summed in fp32 (2u per add allowed, in
    // case the matrix core's adds do not round to nearest), ||g||^2 itself to KP u
    const float es = 3.05f * 1.5258789e-05f;  // 3.05 * 2^-16
    if constexpr (METRIC == EF_METRIC_L2) {
      const float gm = sqrtf(gmax2);
      delta = 2.f * (2.f * es * qn * gm + (3 * kpv + 4) * 2.f * u * 1.01f * (2.02f * qn * gm + gmax2) +
                     kpv * u * gmax2 + 4.f * u * fabsf(b1)) + 1e-30f;
    } else {
      delta = 2.f * ((es + (3 * kpv + 8) * 2.f * u) * 1.01f * qn) + 1e-30f;
    }
  } else if constexpr (METRIC == EF_METRIC_L2) {
    const float gm = sqrtf(gmax2);
    delta = 2.f * ((kpv + 4) * u * 1.01f * (2.f * qn * gm + gmax2) + 4.f * u * fabsf(b1));
  } else {
    delta = 2.f * ((kpv + 8) * u * 1.01f * qn) + 1e-30f;
  }
  return delta * 2.f;  // safety factor
}

// Where scan_delta's error model holds.  The bound counts roundings relative to the values
// (u per operation), so it needs every partial sum of a chain below fp32's overflow and the
// absolute error of underflow (at most 2^-126 per operand or operation, whether the unit
// flushes subnormals or rounds them gradually) far below delta.
//   above: every element product, norm and partial sum of a chain is at most
//     mag = gmax2 + 2.02 ||q|| gm in magnitude (1 % more for the split chains' hi parts);
//     mag <= 2^126 keeps them finite.  An overflowed fp32 ||q||^2 makes mag +inf.
//   below: L2's delta is at least 4 (k + 4) u gmax2 and (4 k + 8) underflows cost at most
//     (4 k + 8) 2^-126, which is below 2^-20 of it for gmax2 >= 2^-80; a flushed operand
//     costs 2^-126 times the other one, covered alike since gm >= 2^-40.  Cosine's delta is
//     proportional to ||q|| and its score carries 1/||g|| <= 2^40, so ||q||^2 >= 2^-80 as well.
// gmax2 arrives NEGATED (scan_gmax2, ef_api.hip) when a gallery row is outside the model:
// a row whose fp32 ||g||^2 is not finite, or for cosine a non-zero row whose ||g||^2 is below
// 2^-80 (its 1/||g|| is inexact or 0).  |gmax2| is then the maximum over the other rows.  A
// NaN anywhere makes the answer false.  A probe that is not regular is never decided from scan
// scores: every row is re-scored in fp64 (resolve_kernel's sweep, topk_sweep_kernel).
constexpr float kScanNormFloor = 8.2718061e-25f;  // 2^-80
constexpr float kScanMagMax = 8.5070592e+37f;     // 2^126
template <int METRIC>
__device__ __forceinline__ bool scan_regular(float qq, float gmax2) {
  const float mag = gmax2 + 2.02f * sqrtf(qq) * sqrtf(gmax2);  // NaN for a negated gmax2
  bool ok = gmax2 >= kScanNormFloor && mag <= kScanMagMax;
  if constexpr (METRIC != EF_METRIC_L2) ok = ok && qq >= kScanNormFloor;
  return ok;
}

// ---- work items -----------------------------------------------------------------------
// Tiles [t0, t1) of gallery chunk gc (ROWS rows per tile); t0 >= t1 for an empty chunk.
template <int ROWS>
__device__ __forceinline__ void chunk_range(int64_t n, int gc, int tiles_per_chunk, int64_t& t0, int64_t& t1) {
  const int64_t tiles_total = (n + ROWS - 1) / ROWS;
  t0 = (int64_t)gc * tiles_per_chunk;
  t1 = t0 + tiles_per_chunk < tiles_total ? t0 + tiles_per_chunk : tiles_total;
}
// Collect pass: n_chunks is the collect plan's chunk count; the grid strides over the
// (chunk, queued probe tile) items, so a handful of queued probes still spread over the
// whole grid instead of one workgroup per main-pass chunk.  body(chunk, probe tile, n_amb).
template <int PROBE_TILE, typename Body>
__device__ __forceinline__ void collect_items(const SearchWs& ws, int n_chunks, const Body& body) {
  const int n_amb = *ws.amb_count;
  const int items = ((n_amb + PROBE_TILE - 1) / PROBE_TILE) * n_chunks;
  for (int item = blockIdx.x; item < items; item += gridDim.x) body(item % n_chunks, item / n_chunks, n_amb);
}
// Wide kernels' main pass: (chunk, probe tile) blocks of cblk x pblk, one block per XCD run
// of xcd_lin() (see search_plan); block_deal_ok is the host's check that this is a bijection.
__device__ __forceinline__ void xcd_block_deal(int lin, int n_ptiles, int pblk, int cblk, int& gc, int& pt) {
  const int bsz = cblk * pblk;
  const int blk = lin / bsz, r = lin - blk * bsz;
  const int nbp = n_ptiles / pblk;
  gc = (blk / nbp) * cblk + r / pblk;
  pt = (blk % nbp) * pblk + r % pblk;
}
inline bool block_deal_ok(const SearchPlan& pl, int probe_tile, int64_t bpad) {
  const int items = pl.nchunks * pl.n_ptiles;
  return pl.n_ptiles % pl.pblk == 0 && pl.nchunks % pl.cblk == 0 && items % 8 == 0 &&
         (items / 8) % (pl.cblk * pl.pblk) == 0 && bpad % probe_tile == 0;
}

// ---- wide kernels: DMA geometry of a 32-k slice -----------------------------------------
// A slice row is 128 B = eight 16-B chunks; a slice is pieces of 1 KiB (8 rows); wave w
// issues pieces 4w .. 4w + 3 of the gallery slice and of the probe slice.  Lane l of piece
// j carries row 8j + (l >> 3), physical chunk l & 7, which holds logical chunk
// (l & 7) ^ ((row >> 1) & SWZ) = (l & 7) ^ ((4 jj + (l >> 4)) & SWZ).  The per-lane byte
// offsets are fixed for the whole sweep (SGPR-base DMA: the slice's base address is
// wave-uniform), so a slice's DMAs cost no per-lane address arithmetic.  COLLECT: the probe
// rows are those of the queued slots.
// Also written out, with SWZ = 5, in search_wide16_kernel (ef_search_wide.hip; the reason is
// given there): keep the two in step.
template <int SWZ, int PROBE_TILE, bool COLLECT>
__device__ __forceinline__ void wide_dma_offsets(const SearchWs& ws, int pt, int wave, int lane, int n_amb,
                                                 int row_bytes, unsigned (&goff)[4], unsigned (&qoff)[4]) {
  const int prow = lane >> 3;
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    const int slot = pt * PROBE_TILE + (wave * 4 + jj) * 8 + prow;
    int qrow = slot;
    if constexpr (COLLECT) qrow = slot < n_amb ? ws.amb_list[slot] : 0;
    const unsigned lch16 = (unsigned)(((lane & 7) ^ ((4 * jj + (lane >> 4)) & SWZ)) * 16);
    goff[jj] = (unsigned)((wave * 4 + jj) * 8 + prow) * row_bytes + lch16;
    qoff[jj] = (unsigned)qrow * row_bytes + lch16;
  }
}
// rows of tile t that exist (ROWS except in the tail tile)
template <int ROWS>
__device__ __forceinline__ int tile_rows(int64_t n, int64_t t) {
  return (int)((n - t * ROWS) < ROWS ? (n - t * ROWS) : ROWS);
}
// Tail tile: a gallery piece's rows past the end re-read the last row (masked later).
// go = row * row_bytes + byte offset inside the row; nrem = tile_rows().
template <int ROWS>
__device__ __forceinline__ unsigned wide_tail_clamp(unsigned go, int nrem, int row_bytes) {
  if (nrem < ROWS) {
    const unsigned row = go / row_bytes;
    go = (row < (unsigned)nrem ? row : (unsigned)(nrem - 1)) * row_bytes + go % row_bytes;
  }
  return go;
}


// fp64 score of gallery row `row` for probe q (L2: squared distance in difference form;
// cosine: -q.g/(|q||g|), 0 for a zero vector — sklearn normalize semantics; NaN when a norm is
// NaN or infinite, +inf or NaN for L2 with such a component: the sweeps pass such rows over).
// KP = 0: the row length is kp_rt (k > 512, any multiple of 128).
template <int KP, int METRIC>
__device__ __forceinline__ double score64(const float* __restrict__ q, const float* __restrict__ g, int lane,
                                          int kp_rt = KP) {
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  auto term = [&](int c) {
    const double qv = q[c], gv = g[c];
    if constexpr (METRIC == EF_METRIC_L2) {
      const double dv = qv - gv;
      s0 = fma(dv, dv, s0);
    } else {
      s0 = fma(qv, gv, s0);
      s1 = fma(qv, qv, s1);
      s2 = fma(gv, gv, s2);
    }
  };
  if constexpr (KP > 0) {
#pragma unroll
    for (int c = lane; c < KP; c += 64) term(c);
  } else {
    for (int c = lane; c < kp_rt; c += 64) term(c);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s0 += __shfl_xor(s0, off);
    if constexpr (METRIC != EF_METRIC_L2) {
      s1 += __shfl_xor(s1, off);
      s2 += __shfl_xor(s2, off);
    }
  }
  if constexpr (METRIC == EF_METRIC_L2) {
    return s0;
  } else {
    if (s1 > 0.0 && s2 > 0.0) return -(s0 / (sqrt(s1) * sqrt(s2)));  // NaN for an infinite norm
    // 0 is for a true zero vector alone: a NaN norm (a NaN component) scores NaN, so that the
    // sweeps pass the row over instead of ranking it at cosine 0
    return (s1 != s1 || s2 != s2) ? __builtin_nan("") : 0.0;
  }
}

// Wide search (KP in {256, 512}, or KP = 0 with a run-time row length kp > 512, a
// multiple of 128): probes streamed through LDS with the gallery.
constexpr int kWideRowTile = 128;    // gallery rows per tile
constexpr int kWideProbeTile = 128;  // probes per workgroup
constexpr int kWide3RowTile = 256;    // split-bf16 wide kernel: gallery rows per tile
constexpr int kWide3ProbeTile = 256;  // split-bf16 wide kernel: probes per workgroup
// Called by launch_search_scan alone.  s3: the scan variant in ef_internal.hpp's numbering (0 the
// fp32 scan; 1 split 16x16x32; 2 split 32x32x16; 3 the single-bf16 screen); for 1 .. 3 qpad and
// G are the copies in the variant's layout
hipError_t launch_search_wide(hipStream_t s, int kp, int metric, bool collect, int s3, const SearchPlan& pl,
                              const float* qpad, const float* G, const float* aux, int64_t n, int64_t bpad,
                              const SearchWs& ws);
#ifdef EF_DIAGNOSTICS
// Diagnostic builds only (ef_search_screen.hip is not part of the product library): the
// single-bf16 screen's main pass with the gallery operand in VGPRs (kh = k / 2 in
// {128, 256}); screen_vg_enabled: the EF_SCREEN_VG=1 A/B knob
bool screen_vg_enabled();
hipError_t launch_search_screen(hipStream_t s, int kh, int metric, const SearchPlan& pl, const float* q1,
                                const float* G1, const float* aux, int64_t n, int64_t bpad, const SearchWs& ws);
#endif

}  // namespace ef
