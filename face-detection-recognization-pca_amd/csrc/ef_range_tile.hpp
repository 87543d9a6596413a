// The threshold scan that ef_search_range (ef_range.hip) and ef_search_rank
// (ef_rank.hip) share: the plan, the arguments, the per-probe band and
// range_kernel, one kernel template with three epilogues.
//   kRangeCount, kRangeFill: the range search's two passes over one threshold for all probes.
//   kRangeRank: the threshold is per probe (a lane owns its probe: tau of its genuine row), a
//     tile also stages the dense class id of its 128 rows in LDS, and every decided hit of
//     another class sets that class's bit in the probe's bitmap row.
#pragma once
#include "ef_search_common.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

namespace ef {

constexpr int RR = 128;        // gallery rows per tile
constexpr int RP = 128;        // probes per workgroup
constexpr int RBK = 16;        // k per slice
constexpr int RSL = RR * RBK;  // floats per slice of one operand
// LDS map in floats: [stage 0: rows | probes][stage 1: rows | probes][aux of even | odd tiles]
// and, kRangeRank alone, [class ids of even | odd tiles]
constexpr int kRangeAux0 = 4 * RSL;
constexpr int kRangeLdsFloats = kRangeAux0 + 2 * RR;
constexpr int kRangeCls0 = kRangeLdsFloats;
constexpr int64_t kRangeTargetItems = 2048;  // work items aimed for: 256 CUs x 2 workgroups x 4
// range_kernel's epilogues
enum { kRangeCount = 0, kRangeFill = 1, kRangeRank = 2 };
// kRangeRank: pcls of a probe that has no genuine row (its lane scans nothing); -1 is a probe
// whose class no row of this gallery carries (it differs from every row's)
constexpr int kRankNoGenuine = -2;

// counters of one call (device)
enum { kRcResolved = 0, kRcCount = 2 };

// The plan of one call: the gallery's row tiles are cut into n_chunks chunks of tiles_per_item
// tiles (the last one shorter); a work item is (chunk, probe tile), about kRangeTargetItems of
// them.  bpad: the padded probe count, a multiple of 256.  Shared by the launches and
// ef_search_range_plan.
inline void range_plan(int64_t bpad, int64_t n, int64_t& n_chunks, int64_t& tiles_per_item) {
  const int64_t n_ptiles = bpad / RP;
  const int64_t tiles = (n + RR - 1) / RR;
  if (n_ptiles <= 0 || tiles <= 0) {
    n_chunks = tiles_per_item = 0;
    return;
  }
  const int64_t want = std::max<int64_t>(1, (kRangeTargetItems + n_ptiles - 1) / n_ptiles);
  const int64_t parts = std::min(want, tiles);
  tiles_per_item = (tiles + parts - 1) / parts;
  n_chunks = (tiles + tiles_per_item - 1) / tiles_per_item;
}

struct RangeArgs {
  const float* qpad;  // [bpad][kp] the piece's probes
  const float* G;     // [n][kp]
  const float* aux;   // [n] ||g||^2 (L2) or 1/||g|| (cosine)
  const float* qaux;  // [bpad] ||q||^2 (L2) or 1/||q|| (cosine), rounded once from fp64
  const int* pexcl;   // [bpad] excluded local row, -1 for none
  int64_t n, b;       // rows; probes of the piece
  int kp, n_ptiles, tpc;
  int64_t stride;  // probes of the whole call, padded: the row length of cnt
  float t;         // fp32 threshold
  double t64, terr;  // the threshold; |fp32(t) - t|
  float gmax2;       // max |g|^2, negated when the gallery is outside the scan's domain
  int* cnt;          // [chunks][stride] at the piece's first probe: COUNT writes the hits of
                     // (chunk, probe); FILL reads their exclusive prefix over the chunks
  unsigned long long* counters;
  const long long* lims;  // FILL: [b + 1] at the piece's first probe
  long long* rows;        // FILL: [cap]
  float* scores;          // FILL: [cap]
  long long cap, g_offset;
  // kRangeRank: t, t64 and terr above are not read; everything per probe is at the piece's first
  const float* pt;         // [bpad] fp32(tau) (L2) or fp32(-tau) (cosine): the scan score's orientation
  const double* pt64;      // [bpad] tau, as score64 carries it
  const double* pterr;     // [bpad] |fp32(tau) - tau|
  const long long* pgen;   // [bpad] global index of the genuine row
  const int* pcls;         // [bpad] the probe's dense class, -1, or kRankNoGenuine
  const int* cls;          // [round_up(n, 128)] dense class of each row, -1 past n
  unsigned* bits;          // [bpad][words] one bit per (probe, class)
  int words, n_classes;
};

// row offset inside a tile (less 4 h) of accumulator element e = 16 rb + 4 q + j
__device__ __forceinline__ int range_elem_off(int e) { return (e >> 4) * 32 + ((e >> 2) & 3) * 8 + (e & 3); }
// bits [0, i) of a 64-bit mask, i = 0 .. 64
__device__ __forceinline__ unsigned long long range_below(int i) { return i >= 64 ? ~0ull : (1ull << i) - 1ull; }

// Half-width of the band that is settled in fp64, for this lane's probe (include/eigenface.h,
// ef_search_range).  qa: the probe's fp32 ||q||^2 (L2) or 1/||q|| (cosine).  +inf
// outside the scan's domain: every pair with a finite scan score is then settled in fp64.  The
// factor 1.001 covers the roundings of qa, gmax2 and of the result to fp32.
template <int METRIC>
__device__ __forceinline__ float range_delta(float qa, float gmax2, int kp, double terr) {
  const float INF = __builtin_inff();
  const double u = 5.9604644775390625e-08;  // 2^-24
  if (!(gmax2 >= kScanNormFloor)) return INF;  // also a negated or NaN gmax2
  const double gm2 = gmax2, gm = sqrt(gm2);
  double d;
  if constexpr (METRIC == EF_METRIC_L2) {
    if (!(qa < INF)) return INF;
    const double qn = sqrt((double)qa);
    if (!(gm2 + 2.02 * qn * gm <= (double)kScanMagMax)) return INF;
    d = 2.0 * ((kp + 4) * u * 1.01 * (2.0 * qn * gm + gm2) + 4.0 * u * (qn + gm) * (qn + gm));
  } else {
    if (qa != 0.f) {  // a zero probe scores exactly 0 against every row, in fp32 as in fp64
      if (!(qa <= 1.0995116e12f)) return INF;  // |q|^2 < 2^-80, or not finite
      if (!(gm2 + 2.02 * gm / (double)qa <= (double)kScanMagMax)) return INF;
    }
    d = 2.0 * (kp + 12) * u * 1.01;
  }
  d = (d + terr) * 1.001;
  return d < 1e38 ? (float)d : INF;
}

template <int METRIC, int MODE>
__global__ __launch_bounds__(256, 2) void range_kernel(const RangeArgs a) {
  constexpr bool FILL = MODE == kRangeFill;
  constexpr bool RANK = MODE == kRangeRank;
  __shared__ __attribute__((aligned(16))) float smem[kRangeLdsFloats + (RANK ? 2 * RR : 0)];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5;
  const int c32 = lane & 31;

  // one (gallery chunk gc, probe tile pt) work item per workgroup; the probe tiles of a chunk
  // are neighbours in the grid, so they stream the chunk's rows through the L2s together
  const int pt = (int)(blockIdx.x % (unsigned)a.n_ptiles);
  const int gc = (int)(blockIdx.x / (unsigned)a.n_ptiles);
  int64_t t0, t1;
  chunk_range<RR>(a.n, gc, a.tpc, t0, t1);
  if (t0 >= t1) return;  // never: every chunk of range_plan holds a tile

  const int ns = a.kp / RBK;  // slices per tile
  const int row_bytes = a.kp * 4;
  const int64_t slot = (int64_t)pt * RP + wave * 32 + c32;  // this lane's probe (< bpad)
  bool valid = slot < a.b;
  const float qa = a.qaux[slot];
  const int pexcl = a.pexcl[slot];
  // the fp32 threshold and its rounding error: the call's, or (RANK) this lane's probe's
  float tl = a.t;
  double terr = a.terr;
  int pcls = 0;
  if constexpr (RANK) {
    tl = a.pt[slot];
    terr = a.pterr[slot];
    pcls = a.pcls[slot];
    valid = valid && pcls != kRankNoGenuine;
  }
  const float delta = range_delta<METRIC>(qa, a.gmax2, a.kp, terr);
  int* const cnt = a.cnt + (int64_t)gc * a.stride + slot;
  long long run = 0;  // FILL: where this probe's next hit goes
  bool fits = false;  // FILL: the probe's segment fits whole
  if constexpr (FILL) {
    if (valid) {
      fits = a.lims[slot + 1] <= a.cap;
      run = a.lims[slot] + *cnt;
    }
  }

  // DMA geometry (census_kernel's): a slice row is 64 B = four 16-B chunks, a piece is 1 KiB =
  // 16 rows, wave w issues pieces 2w, 2w + 1 of each operand; lane l of piece p carries row
  // 16 p + (l >> 2), physical chunk l & 3 = logical chunk (l & 3) ^ ((l >> 4) & 3).
  unsigned goff[2], qoff[2];
#pragma unroll
  for (int jj = 0; jj < 2; ++jj) {
    const int row = (wave * 2 + jj) * 16 + (lane >> 2);
    const unsigned lch16 = (unsigned)(((lane & 3) ^ ((lane >> 4) & 3)) * 16);
    goff[jj] = (unsigned)row * row_bytes + lch16;
    qoff[jj] = (unsigned)(pt * RP + row) * row_bytes + lch16;
  }
  // settle these loads before the loop (a loop-merged wait would drain the LDS-DMA)
  asm volatile("" ::"v"(qa), "v"(pexcl), "v"(delta), "v"(run), "v"((int)fits));
  if constexpr (RANK) asm volatile("" ::"v"(tl), "v"(pcls), "v"((int)valid));

  const unsigned lds_base = lds_addr(smem);
  const unsigned aoff = (unsigned)lane * 4;
  auto issue = [&](int64_t t, int sl, int buf) {
    const int nrem = tile_rows<RR>(a.n, t);
    const unsigned long long gb = (unsigned long long)(size_t)(a.G + t * RR * a.kp + sl * RBK);
    const unsigned long long qb = (unsigned long long)(size_t)(a.qpad + sl * RBK);
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const int p = wave * 2 + jj;
      glds16s(wide_tail_clamp<RR>(goff[jj], nrem, row_bytes), gb, lds_base + (unsigned)((buf * 2 * RSL + p * 256) * 4));
      glds16s(qoff[jj], qb, lds_base + (unsigned)((buf * 2 * RSL + RSL + p * 256) * 4));
    }
    if (sl == 0 && wave == 0) {  // the tile's aux values; rows past the end re-read the last row's
      const int par = (int)((t - t0) & 1);
      const unsigned long long ab = (unsigned long long)(size_t)(a.aux + t * RR);
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int rr = 64 * q + lane;
        const unsigned ao = rr < nrem ? aoff + 256u * q : (unsigned)(nrem - 1) * 4;
        glds4s(ao, ab, lds_base + (unsigned)((kRangeAux0 + par * RR + 64 * q) * 4));
      }
    }
    if constexpr (RANK) {
      if (sl == 0 && wave == 1) {  // the tile's class ids; cls is padded to whole tiles with -1
        const int par = (int)((t - t0) & 1);
        const unsigned long long cb = (unsigned long long)(size_t)(a.cls + t * RR);
#pragma unroll
        for (int q = 0; q < 2; ++q)
          glds4s(aoff + 256u * q, cb, lds_base + (unsigned)((kRangeCls0 + par * RR + 64 * q) * 4));
      }
    }
  };

  const float INF = __builtin_inff();
  unsigned nhits = 0u;  // COUNT: this lane's hits
  unsigned nres = 0u;   // pairs this wave settled in fp64 (wave-uniform)

  issue(t0, 0, 0);
  dma_wait_all();
  __syncthreads();

  const int swk = (c32 >> 2) & 3;  // swizzle key of rows c32 + 32 rb and of probe 32 w + c32
  f32x16 acc[4];
  int64_t t = t0;
  int sl = 0, buf = 0;
  for (;;) {
    int sl_n = sl + 1;
    int64_t t_n = t;
    if (sl_n == ns) {
      sl_n = 0;
      ++t_n;
    }
    const bool more = t_n < t1;
    if (more) issue(t_n, sl_n, buf ^ 1);  // lands under this slice's MFMAs
    const int par = (int)((t - t0) & 1);
    const float* const sAux = smem + kRangeAux0 + par * RR;
    if (sl == 0) {
      // L2: start from -||g||^2 / 2 and accumulate q.g, so that ||q||^2 - 2 acc is the squared
      // distance with the chain's rounding scaled exactly by -2.  Cosine: start from 0.
#pragma unroll
      for (int rb = 0; rb < 4; ++rb) {
        acc[rb] = f32x16{};
        if constexpr (METRIC == EF_METRIC_L2) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float4 x = *reinterpret_cast<const float4*>(sAux + rb * 32 + 8 * q + 4 * h);
            acc[rb][4 * q] = -0.5f * x.x;
            acc[rb][4 * q + 1] = -0.5f * x.y;
            acc[rb][4 * q + 2] = -0.5f * x.z;
            acc[rb][4 * q + 3] = -0.5f * x.w;
          }
        }
      }
    }
    const float* sg = smem + buf * 2 * RSL;
    const float* sq = sg + RSL;
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const int pch = ((h * 2 + jj) ^ swk) * 4;  // lane half h owns k in [8h, 8h + 8) of the slice
      const float4 bq = *reinterpret_cast<const float4*>(sq + (wave * 32 + c32) * RBK + pch);
      float4 av[4];
#pragma unroll
      for (int rb = 0; rb < 4; ++rb) av[rb] = *reinterpret_cast<const float4*>(sg + (rb * 32 + c32) * RBK + pch);
#pragma unroll
      for (int rb = 0; rb < 4; ++rb) acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[rb].x, bq.x, acc[rb], 0, 0, 0);
#pragma unroll
      for (int rb = 0; rb < 4; ++rb) acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[rb].y, bq.y, acc[rb], 0, 0, 0);
#pragma unroll
      for (int rb = 0; rb < 4; ++rb) acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[rb].z, bq.z, acc[rb], 0, 0, 0);
#pragma unroll
      for (int rb = 0; rb < 4; ++rb) acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[rb].w, bq.w, acc[rb], 0, 0, 0);
    }
    if (sl == ns - 1) {
      // register r of block rb is row tb + off, off = 32 rb + (r & 3) + 8 (r >> 2)
      const int64_t tb = t * RR + 4 * h;
      const int64_t rem = a.n - tb;  // rows at off >= rem do not exist; a probe past b has none
      const int nrel = !valid ? 0 : rem > RR ? RR : (int)rem;
      const int64_t er = (int64_t)pexcl - tb;  // the excluded row as an off (negative: none)
      const int erel = (er >= 0 && er < RR) ? (int)er : -1;
      unsigned long long lm = 0ull, nm = 0ull;  // hit by s^; inside the band
#pragma unroll
      for (int rb = 0; rb < 4; ++rb) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float x[4] = {0.f, 0.f, 0.f, 0.f};
          if constexpr (METRIC != EF_METRIC_L2) {
            const float4 xa = *reinterpret_cast<const float4*>(sAux + rb * 32 + 8 * q + 4 * h);
            x[0] = xa.x, x[1] = xa.y, x[2] = xa.z, x[3] = xa.w;
          }
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) {
            const int off = rb * 32 + 8 * q + jj;
            const unsigned long long bit = 1ull << (rb * 16 + q * 4 + jj);
            const float v = acc[rb][4 * q + jj];
            float sc;
            if constexpr (METRIC == EF_METRIC_L2) sc = __builtin_fmaf(-2.f, v, qa);
            else sc = (v * x[jj]) * qa;
            const bool ok = off < nrel && off != erel && fabsf(sc) < INF;  // false for NaN
            const bool lk = METRIC == EF_METRIC_L2 ? sc <= tl : sc >= tl;
            lm |= (ok && lk) ? bit : 0ull;
            nm |= (ok && fabsf(sc - tl) <= delta) ? bit : 0ull;
          }
        }
      }
      // the band: the whole wave settles one pair at a time on its fp64 score
      unsigned long long sm = 0ull;  // FILL: hits settled here, whose reported score is the fp64 one
      unsigned long long pend = __ballot(nm != 0ull);
      while (pend) {
        const int l = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(pend));
        const unsigned mlo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)nm, l);
        const unsigned mhi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(nm >> 32), l);
        const int e = mlo ? __builtin_ctz(mlo) : 32 + __builtin_ctz(mhi);
        const int64_t rj = (int64_t)pt * RP + wave * 32 + (l & 31);
        const int64_t ri = t * RR + 4 * (l >> 5) + range_elem_off(e);
        const double s = score64<0, METRIC>(a.qpad + rj * a.kp, a.G + ri * a.kp, lane, a.kp);
        // score64's cosine is the negated similarity; a NaN score is no hit
        bool d;
        if constexpr (RANK) {
          // beats the genuine row: a lower score, or the same score at a lower global index (the
          // settling probe's tau and genuine row: wave-uniform reads)
          const double tau = a.pt64[rj];
          d = s < tau || (s == tau && a.g_offset + ri < a.pgen[rj]);
        } else {
          d = METRIC == EF_METRIC_L2 ? s <= a.t64 : -s >= a.t64;
        }
        if (lane == l) {
          const unsigned long long bit = 1ull << e;
          nm &= ~bit;
          lm = d ? (lm | bit) : (lm & ~bit);
          if constexpr (FILL) sm |= d ? bit : 0ull;
        }
        ++nres;
        pend = __ballot(nm != 0ull);
      }
      if constexpr (RANK) {
        // every hit of another class marks that class in the probe's bitmap row.  The word is
        // read first and the atomic skipped when the bit is there (OR is idempotent, so a stale
        // read costs a redundant atomic at most); a hit of the previous hit's class is skipped
        // unread.  A class outside [0, n_classes) never comes out of the library's own map; the
        // compare keeps every store inside the row whatever cls holds.
        const int* const sCls = reinterpret_cast<const int*>(smem) + kRangeCls0 + par * RR + 4 * h;
        unsigned* const brow = a.bits + slot * a.words;
        int prev = pcls;
        while (lm) {
          const int e = __builtin_ctzll(lm);
          lm &= lm - 1ull;
          const int cl = sCls[range_elem_off(e)];
          if (cl != prev && cl != pcls && (unsigned)cl < (unsigned)a.n_classes) {
            prev = cl;
            const unsigned bit = 1u << (cl & 31);
            unsigned* const w = brow + (cl >> 5);
            if (!(*w & bit)) atomicOr(w, bit);
          }
        }
      } else if constexpr (!FILL) {
        nhits += (unsigned)__builtin_popcountll(lm);
      } else {
        // the probe's other half: rows 8 N + 4 (1 - h) + jj of the tile, N = 4 rb + q
        const unsigned long long pm = __shfl_xor(lm, 32);
        if (!fits) sm = 0ull;
        if (lm != 0ull && fits) {
#pragma unroll
          for (int rb = 0; rb < 4; ++rb) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const int N = rb * 4 + q;
              const unsigned nib = (unsigned)(lm >> (4 * N)) & 15u;
              if (nib) {
                // hits of the tile in front of this nibble: the lane's own lower nibbles and the
                // partner's, whose nibble N comes first when this lane is half 1
                const long long pb = run + __builtin_popcountll(lm & range_below(4 * N)) +
                                     __builtin_popcountll(pm & (h ? range_below(4 * N + 4) : range_below(4 * N)));
                const unsigned own = nib & ~((unsigned)(sm >> (4 * N)) & 15u);  // settled hits are written below
                float x[4] = {0.f, 0.f, 0.f, 0.f};
                if constexpr (METRIC != EF_METRIC_L2) {
                  const float4 xa = *reinterpret_cast<const float4*>(sAux + rb * 32 + 8 * q + 4 * h);
                  x[0] = xa.x, x[1] = xa.y, x[2] = xa.z, x[3] = xa.w;
                }
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                  if (own & (1u << jj)) {
                    const long long pos = pb + __builtin_popcount(nib & ((1u << jj) - 1u));
                    const float v = acc[rb][4 * q + jj];
                    float sc;
                    if constexpr (METRIC == EF_METRIC_L2) sc = __builtin_fmaf(-2.f, v, qa);
                    else sc = (v * x[jj]) * qa;
                    if (pos < a.cap) {  // always (pos < lims[p + 1] <= cap): no store leaves the arrays
                      a.rows[pos] = a.g_offset + tb + (rb * 32 + 8 * q + jj);
                      a.scores[pos] = sc;
                    }
                  }
                }
              }
            }
          }
        }
        // the hits settled in the band report (float) of their fp64 score
        pend = __ballot(sm != 0ull);
        while (pend) {
          const int l = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(pend));
          const unsigned mlo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)sm, l);
          const unsigned mhi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(sm >> 32), l);
          const int e = mlo ? __builtin_ctz(mlo) : 32 + __builtin_ctz(mhi);
          const int64_t rj = (int64_t)pt * RP + wave * 32 + (l & 31);
          const int64_t ri = t * RR + 4 * (l >> 5) + range_elem_off(e);
          const double s = score64<0, METRIC>(a.qpad + rj * a.kp, a.G + ri * a.kp, lane, a.kp);
          if (lane == l) {
            const int N = e >> 2;
            const long long pos = run + __builtin_popcountll(lm & range_below(e)) +
                                  __builtin_popcountll(pm & (h ? range_below(4 * N + 4) : range_below(4 * N)));
            if (pos < a.cap) {
              a.rows[pos] = a.g_offset + ri;
              a.scores[pos] = METRIC == EF_METRIC_L2 ? (float)s : (float)-s;
            }
            sm &= ~(1ull << e);
          }
          pend = __ballot(sm != 0ull);
        }
        run += __builtin_popcountll(lm) + __builtin_popcountll(pm);
      }
    }
    dma_wait_all();
    __syncthreads();  // the next slice landed; everyone is done reading buffer buf
    if (!more) break;
    t = t_n;
    sl = sl_n;
    buf ^= 1;
  }

  if constexpr (RANK) {
    if (lane == 0 && nres) atomicAdd(a.counters + kRcResolved, (unsigned long long)nres);
  } else if constexpr (!FILL) {
    // a probe's two lane halves; half 0 publishes the chunk's count (0 for a probe past b)
    const unsigned both = nhits + __shfl_xor(nhits, 32);
    if (h == 0) *cnt = (int)both;
    if (lane == 0 && nres) atomicAdd(a.counters + kRcResolved, (unsigned long long)nres);
  }
}

}  // namespace ef
