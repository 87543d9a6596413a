// Range search (ef_search_range): for each probe, every resident gallery row
// within a threshold, as a CSR list (lims, rows, scores) in ascending row order.
//   * range_kernel is census_kernel's distance GEMM (ef_census.hip: 128 rows x 128 probes per
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
constexpr int kRangeAux0 = 4 * RSL;
constexpr int kRangeLdsFloats = kRangeAux0 + 2 * RR;
constexpr int64_t kRangeTargetItems = 2048;  // work items aimed for: 256 CUs x 2 workgroups x 4

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

template <int METRIC, bool FILL>
__global__ __launch_bounds__(256, 2) void range_kernel(const RangeArgs a) {
  __shared__ __attribute__((aligned(16))) float smem[kRangeLdsFloats];

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
  const bool valid = slot < a.b;
  const float qa = a.qaux[slot];
  const int pexcl = a.pexcl[slot];
  const float delta = range_delta<METRIC>(qa, a.gmax2, a.kp, a.terr);
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
            const bool lk = METRIC == EF_METRIC_L2 ? sc <= a.t : sc >= a.t;
            lm |= (ok && lk) ? bit : 0ull;
            nm |= (ok && fabsf(sc - a.t) <= delta) ? bit : 0ull;
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
        const bool d = METRIC == EF_METRIC_L2 ? s <= a.t64 : -s >= a.t64;
        if (lane == l) {
          const unsigned long long bit = 1ull << e;
          nm &= ~bit;
          lm = d ? (lm | bit) : (lm & ~bit);
          if constexpr (FILL) sm |= d ? bit : 0ull;
        }
        ++nres;
        pend = __ballot(nm != 0ull);
      }
      if constexpr (!FILL) {
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

  if constexpr (!FILL) {
    // a probe's two lane halves; half 0 publishes the chunk's count (0 for a probe past b)
    const unsigned both = nhits + __shfl_xor(nhits, 32);
    if (h == 0) *cnt = (int)both;
    if (lane == 0 && nres) atomicAdd(a.counters + kRcResolved, (unsigned long long)nres);
  }
}

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
