// Gallery clustering (ef_gallery_cluster): a self-join of the resident gallery
// that links every pair of rows within a threshold and returns the connected components.
//   * cluster_kernel is census_kernel's distance GEMM (ef_census.hip: 128 x 128 tiles, 16-k slices
//     of both operands double-buffered in LDS by global_load_lds, XOR-swizzled slice rows, four
//     independent fp32 accumulator chains per wave) with both operands taken from G: the "probes"
//     of a workgroup are the 128 rows of tile pt.  The accumulation chain is the census's, so
//     its error bound is (K8c): the probe side's |g|^2 or 1/|g| is rounded once from fp64
//     (census_probe_aux_kernel on G), the row side's is the gallery's own.
//   * epilogue: a pair is linked when its fp32 score s^ is on the linked side of t, decided by
//     s^ alone when |s^ - t| > delta.  The lanes inside the band are balloted and the whole wave
//     re-scores them one after another with score64 (no side list, nothing to overflow).  The
//     decisions of a tile's 64 accumulator registers are two 64-bit masks per lane.
//   * COUNT mode sweeps the full square and adds each probe lane's linked rows in a register:
//     one integer atomic per lane and work item gives degree[].  LINK mode sweeps the row tiles
//     up to the probe tile (within the diagonal tile only row < probe), so each unordered pair is
//     seen once, and joins the pair in the union-find of ef_union_find.hpp keyed by row index.
//   * rows past n re-read the last row through the clamped DMA and are masked by index, as are
//     the probes past n; a pair whose s^ is not finite is never linked and never re-scored.
// Density floor: with min_samples > 1 a row is core when degree + 1 >= min_samples; LINK joins
// core-core pairs only and takes atomicMin(attach[r], c) for a linked (core c, non-core r) pair.
// Labels: flatten, flag the core roots, two-level exclusive scan of the flags, rank of the root.
// Everything is integer or decided as in fp64, so the outputs do not depend on arrival order.
#include "ef_search_common.hpp"
#include "ef_union_find.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

namespace ef {

constexpr int KR = 128;        // rows per tile, on either side
constexpr int KBK = 16;        // k per slice
constexpr int KSL = KR * KBK;  // floats per slice of one operand
// LDS map in floats: [stage 0: rows | probes][stage 1: rows | probes][aux of even | odd tiles]
constexpr int kClusterAux0 = 4 * KSL;
constexpr int kClusterLdsFloats = kClusterAux0 + 2 * KR;
constexpr int64_t kClusterTargetItems = 2048;  // work items aimed for: 256 CUs x 2 workgroups x 4

// counters of one call (device)
enum { kCcLinks = 0, kCcResolved = 1, kCcFlag = 2, kCcNoise = 3, kCcClusters = 4, kCcCount = 8 };

// Row tiles per work item: about kClusterTargetItems items over the tile pairs of the sweep.
__host__ __device__ inline int64_t cluster_tiles_per_item(int64_t tiles, bool full) {
  const int64_t pairs = full ? tiles * tiles : tiles * (tiles + 1) / 2;
  const int64_t tpc = pairs / kClusterTargetItems;
  return tpc < 1 ? 1 : tpc > tiles ? tiles : tpc;
}
// Work item (chunk c, probe tile pt): row tiles [t0, t1); empty when t0 >= t1.  The triangle
// stops at the probe tile.
__host__ __device__ inline void cluster_item(int64_t tiles, int64_t tpc, bool full, int64_t c, int64_t pt, int64_t& t0,
                                             int64_t& t1) {
  const int64_t end = full ? tiles : pt + 1;
  t0 = c * tpc;
  t1 = t0 + tpc < end ? t0 + tpc : end;
}

struct ClusterArgs {
  const float* G;     // [n][kp]
  const float* aux;   // [n] row side: ||g||^2 (L2) or 1/||g|| (cosine)
  const float* qaux;  // [n] probe side: the same, rounded once from fp64
  int64_t n;
  int kp, n_tiles, tpc;
  float t, delta;  // fp32 threshold; half-width of the band decided in fp64
  double t64;
  int min_samples;
  const int* core_deg;  // LINK: degree[] for the core test, null when every row is core
  int* degree;          // COUNT
  int* parent;          // LINK
  int* attach;          // LINK with core_deg
  unsigned long long* counters;
};

// row offset inside a tile (less 4 h) of accumulator element e = 16 rb + 4 q + j
__device__ __forceinline__ int cluster_elem_off(int e) { return (e >> 4) * 32 + ((e >> 2) & 3) * 8 + (e & 3); }

template <int METRIC, bool LINK>
__global__ __launch_bounds__(256, 2) void cluster_kernel(const ClusterArgs a) {
  __shared__ __attribute__((aligned(16))) float smem[kClusterLdsFloats];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5;
  const int c32 = lane & 31;

  // the heaviest probe tiles (most row tiles below them) are dealt first
  const int64_t pt = (int64_t)a.n_tiles - 1 - blockIdx.x;
  int64_t t0, t1;
  cluster_item(a.n_tiles, a.tpc, !LINK, blockIdx.y, pt, t0, t1);
  if (t0 >= t1) return;

  const int ns = a.kp / KBK;  // slices per tile
  const int row_bytes = a.kp * 4;
  const int64_t jraw = pt * KR + wave * 32 + c32;  // this lane's probe row
  const bool valid = jraw < a.n;
  const int64_t j = valid ? jraw : a.n - 1;
  const float qa = a.qaux[j];
  int jcore = 1;
  if constexpr (LINK) {
    if (a.core_deg) jcore = a.core_deg[j] + 1 >= a.min_samples ? 1 : 0;
  }

  // DMA geometry (census_kernel's): a slice row is 64 B = four 16-B chunks, a piece is 1 KiB =
  // 16 rows, wave w issues pieces 2w, 2w + 1 of each operand; lane l of piece p carries row
  // 16 p + (l >> 2), physical chunk l & 3 = logical chunk (l & 3) ^ ((l >> 4) & 3).  The probe
  // tile's rows past n re-read the last row, as the row tile's do.
  const int prem = tile_rows<KR>(a.n, pt);
  unsigned goff[2], qoff[2];
#pragma unroll
  for (int jj = 0; jj < 2; ++jj) {
    const int row = (wave * 2 + jj) * 16 + (lane >> 2);
    const unsigned lch16 = (unsigned)(((lane & 3) ^ ((lane >> 4) & 3)) * 16);
    goff[jj] = (unsigned)row * row_bytes + lch16;
    qoff[jj] = wide_tail_clamp<KR>(goff[jj], prem, row_bytes);
  }
  // settle these loads before the loop (a loop-merged wait would drain the LDS-DMA)
  asm volatile("" ::"v"(qa), "v"(jcore));

  const unsigned lds_base = lds_addr(smem);
  const unsigned aoff = (unsigned)lane * 4;
  const float* const Qt = a.G + pt * KR * a.kp;
  auto issue = [&](int64_t t, int sl, int buf) {
    const int nrem = tile_rows<KR>(a.n, t);
    const unsigned long long gb = (unsigned long long)(size_t)(a.G + t * KR * a.kp + sl * KBK);
    const unsigned long long qb = (unsigned long long)(size_t)(Qt + sl * KBK);
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const int p = wave * 2 + jj;
      glds16s(wide_tail_clamp<KR>(goff[jj], nrem, row_bytes), gb, lds_base + (unsigned)((buf * 2 * KSL + p * 256) * 4));
      glds16s(qoff[jj], qb, lds_base + (unsigned)((buf * 2 * KSL + KSL + p * 256) * 4));
    }
    if (sl == 0 && wave == 0) {  // the tile's aux values; rows past the end re-read the last row's
      const int par = (int)((t - t0) & 1);
      const unsigned long long ab = (unsigned long long)(size_t)(a.aux + t * KR);
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int rr = 64 * q + lane;
        const unsigned ao = rr < nrem ? aoff + 256u * q : (unsigned)(nrem - 1) * 4;
        glds4s(ao, ab, lds_base + (unsigned)((kClusterAux0 + par * KR + 64 * q) * 4));
      }
    }
  };

  const float INF = __builtin_inff();
  unsigned nlinked = 0u;  // this lane's linked pairs (COUNT: its probe's degree)
  unsigned nres = 0u;     // pairs this wave settled in fp64 (wave-uniform)
  bool failed = false;

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
    const float* const sAux = smem + kClusterAux0 + par * KR;
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
    const float* sg = smem + buf * 2 * KSL;
    const float* sq = sg + KSL;
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const int pch = ((h * 2 + jj) ^ swk) * 4;  // lane half h owns k in [8h, 8h + 8) of the slice
      const float4 bq = *reinterpret_cast<const float4*>(sq + (wave * 32 + c32) * KBK + pch);
      float4 av[4];
#pragma unroll
      for (int rb = 0; rb < 4; ++rb) av[rb] = *reinterpret_cast<const float4*>(sg + (rb * 32 + c32) * KBK + pch);
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
      const int64_t tb = t * KR + 4 * h;
      const int64_t rem = a.n - tb;  // rows at off >= rem do not exist; a probe past n has none
      int nrel = !valid ? 0 : rem > KR ? KR : (int)rem;
      const int64_t dj = jraw - tb;  // the probe's own row as an off
      int erel = -1;
      if constexpr (LINK) {  // only rows before the probe
        if (dj < nrel) nrel = dj < 0 ? 0 : (int)dj;
      } else {
        erel = (dj >= 0 && dj < KR) ? (int)dj : -1;
      }
      unsigned long long lm = 0ull, nm = 0ull;  // linked by s^; inside the band
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
            nm |= (ok && fabsf(sc - a.t) <= a.delta) ? bit : 0ull;
          }
        }
      }
      // the band: the whole wave settles one pair at a time on its fp64 score
      unsigned long long pend = __ballot(nm != 0ull);
      while (pend) {
        const int l = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(pend));
        const unsigned mlo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)nm, l);
        const unsigned mhi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(nm >> 32), l);
        const int e = mlo ? __builtin_ctz(mlo) : 32 + __builtin_ctz(mhi);
        const int64_t rj = pt * KR + wave * 32 + (l & 31);
        const int64_t ri = t * KR + 4 * (l >> 5) + cluster_elem_off(e);
        const double s = score64<0, METRIC>(a.G + rj * a.kp, a.G + ri * a.kp, lane, a.kp);
        // score64's cosine is the negated similarity; a NaN score links nothing
        const bool d = METRIC == EF_METRIC_L2 ? s <= a.t64 : -s >= a.t64;
        if (lane == l) {
          const unsigned long long bit = 1ull << e;
          nm &= ~bit;
          lm = d ? (lm | bit) : (lm & ~bit);
        }
        ++nres;
        pend = __ballot(nm != 0ull);
      }
      nlinked += (unsigned)__builtin_popcountll(lm);
      if constexpr (LINK) {
        int pj = lm ? parent_load(a.parent + j) : 0;
        while (lm) {
          const int e = __builtin_ctzll(lm);
          lm &= lm - 1;
          const int i = (int)tb + cluster_elem_off(e);
          const bool icore = a.core_deg ? a.core_deg[i] + 1 >= a.min_samples : true;
          if (icore && jcore != 0) {
            if (parent_load(a.parent + i) == pj) continue;  // the cheap exit: same parent already
            if (!group_union(a.parent, i, (int)j, (int)a.n, [](int x, int y) { return x < y; })) failed = true;
            pj = parent_load(a.parent + j);
          } else if (icore != (jcore != 0)) {
            atomicMin(a.attach + (icore ? (int)j : i), icore ? i : (int)j);
          }
        }
      }
    }
    dma_wait_all();
    __syncthreads();  // the next slice landed; everyone is done reading buffer buf
    if (!more) break;
    t = t_n;
    sl = sl_n;
    buf ^= 1;
  }

  if constexpr (LINK) {
    unsigned long long s = nlinked;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) {
      if (s) atomicAdd(a.counters + kCcLinks, s);
      if (nres) atomicAdd(a.counters + kCcResolved, (unsigned long long)nres);
    }
    if (failed) atomicOr(a.counters + kCcFlag, 1ull);
  } else {
    if (valid && nlinked) atomicAdd(a.degree + j, (int)nlinked);
  }
}

// ---- labels -----------------------------------------------------------------------------
struct ClusterLabelArgs {
  int n, min_samples;
  int* parent;        // [n] the forest, flattened in place
  int* attach;        // [n] lowest linked core row of a non-core row (INT_MAX: none)
  const int* degree;  // [n] or null: every row is core
  int* rank;          // [n] exclusive scan of the root flags
  int* bsum;          // [ceil(n / 256)] flags per block, then their exclusive scan
  unsigned long long* counters;
};

__device__ __forceinline__ bool cluster_is_core(const ClusterLabelArgs& a, int i) {
  return a.degree ? a.degree[i] + 1 >= a.min_samples : true;
}

__global__ __launch_bounds__(256) void cluster_init_kernel(int n, int* __restrict__ parent, int* __restrict__ attach,
                                                           int* __restrict__ degree,
                                                           unsigned long long* __restrict__ counters) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < kCcCount) counters[i] = 0ull;
  if (i >= n) return;
  parent[i] = i;
  attach[i] = INT_MAX;
  if (degree) degree[i] = 0;
}

// parent[i] <- the root of i's chain; then the block's count of core roots and of noise rows
__global__ __launch_bounds__(256) void cluster_flatten_kernel(const ClusterLabelArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool root = false, noise = false;
  if (i < a.n) {
    int r = group_find<false>(a.parent, i, a.n);
    if (r < 0) {
      atomicOr(a.counters + kCcFlag, 1ull);
      r = i;
    }
    // a root keeps itself; any other row's chain only gets shorter, so walkers still reach the root
    if (r != i) __hip_atomic_store(a.parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool core = cluster_is_core(a, i);
    root = core && r == i;
    noise = !core && a.attach[i] == INT_MAX;
  }
  const int nroot = __syncthreads_count(root);
  const int nnoise = __syncthreads_count(noise);
  if (threadIdx.x == 0) {
    a.bsum[blockIdx.x] = nroot;
    if (nnoise) atomicAdd(a.counters + kCcNoise, (unsigned long long)nnoise);
  }
}

// second level: one workgroup turns the block counts into their exclusive scan, 256 at a time
__global__ __launch_bounds__(256) void cluster_scan_kernel(const ClusterLabelArgs a, int nblocks) {
  __shared__ int s[256];
  __shared__ int carry;
  const int tx = threadIdx.x;
  if (tx == 0) carry = 0;
  __syncthreads();
  for (int b0 = 0; b0 < nblocks; b0 += 256) {
    const int v = b0 + tx < nblocks ? a.bsum[b0 + tx] : 0;
    s[tx] = v;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
      const int add = tx >= d ? s[tx - d] : 0;
      __syncthreads();
      s[tx] += add;
      __syncthreads();
    }
    const int base = carry;
    if (b0 + tx < nblocks) a.bsum[b0 + tx] = base + s[tx] - v;
    __syncthreads();
    if (tx == 255) carry = base + s[255];
    __syncthreads();
  }
  if (tx == 0) a.counters[kCcClusters] = (unsigned long long)carry;
}

// rank[i] = core roots before row i
__global__ __launch_bounds__(256) void cluster_rank_kernel(const ClusterLabelArgs a) {
  __shared__ int wsum[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool root = i < a.n && cluster_is_core(a, i) && a.parent[i] == i;
  const unsigned long long m = __ballot(root);
  if (lane == 0) wsum[wave] = __builtin_popcountll(m);
  __syncthreads();
  int before = a.bsum[blockIdx.x];
  for (int w = 0; w < wave; ++w) before += wsum[w];
  before += __builtin_popcountll(m & ((1ull << lane) - 1ull));
  if (i < a.n) a.rank[i] = before;
}

// labels[i] = rank of the root of i's cluster (a non-core row: of its lowest linked core row's), -1 for noise
__global__ __launch_bounds__(256) void cluster_label_kernel(const ClusterLabelArgs a, int* __restrict__ labels,
                                                            long long* __restrict__ info) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) {
    info[0] = (long long)a.counters[kCcClusters];
    info[1] = (long long)a.counters[kCcNoise];
    info[2] = (long long)a.counters[kCcLinks];
    info[3] = (long long)a.counters[kCcResolved] | (a.counters[kCcFlag] ? EF_CLUSTER_UNCONVERGED : 0ll);
  }
  if (i >= a.n) return;
  int r;
  if (cluster_is_core(a, i)) {
    r = a.parent[i];
  } else {
    const int c = a.attach[i];
    r = c == INT_MAX ? -1 : a.parent[c];
  }
  labels[i] = r < 0 ? -1 : a.rank[r];
}

// delta of the call (include/eigenface.h, ef_gallery_cluster): the census's bound without its
// bin-index term, with |q|, |g| <= max|g| and |s| <= 4 max|g|^2, plus the rounding of the
// threshold to fp32.  +inf outside the scan's domain: every finite pair is then settled in fp64.
static float cluster_delta(const ef_ctx* c, int metric, double threshold) {
  const double u = 5.9604644775390625e-08;  // 2^-24
  const double gm2 = c->gmax2_host;
  const int kp = c->gal.kp;
  const float INF = __builtin_inff();
  double d;
  if (metric == EF_METRIC_L2) {
    // rows with a non-finite norm have no finite score; gmax2 is the maximum over the others
    if (!(gm2 >= (double)kScanNormFloor) || !(3.02 * gm2 <= (double)kScanMagMax)) return INF;
    d = 2.0 * ((kp + 4) * u * 1.01 * 3.0 * gm2 + 16.0 * u * gm2);
  } else {
    if ((c->gal_rows_host & (kRowNotFinite | kRowTiny)) || !(gm2 >= (double)kScanNormFloor) ||
        !(3.02 * gm2 <= (double)kScanMagMax))
      return INF;
    d = 2.0 * (kp + 12) * u * 1.01;
  }
  d += std::fabs((double)(float)threshold - threshold);
  if (!(d < 1e38)) return INF;
  return (float)(d * 1.000001);
}

template <int METRIC, bool LINK>
static hipError_t launch_cluster_pass(hipStream_t s, const ClusterArgs& a) {
  const int64_t nch = (a.n_tiles + a.tpc - 1) / a.tpc;
  const dim3 grid((unsigned)a.n_tiles, (unsigned)nch), block(256);
  hipLaunchKernelGGL((cluster_kernel<METRIC, LINK>), grid, block, 0, s, a);
  return hipGetLastError();
}
template <bool LINK>
static hipError_t launch_cluster(hipStream_t s, int metric, const ClusterArgs& a) {
  if (metric == EF_METRIC_L2) return launch_cluster_pass<EF_METRIC_L2, LINK>(s, a);
  return launch_cluster_pass<EF_METRIC_COSINE, LINK>(s, a);
}

}  // namespace ef

using namespace ef;

extern "C" int ef_cluster_schedule(int64_t n, int32_t kp, int64_t* items_out, int32_t max_items, int32_t* n_items) {
  if (n < 0 || n > INT_MAX || kp < KBK || kp % KBK != 0 || max_items < 0 || !n_items || (max_items > 0 && !items_out))
    return EF_E_INVALID;
  const int64_t tiles = (n + KR - 1) / KR;
  const int64_t tpc = tiles ? cluster_tiles_per_item(tiles, false) : 1;
  const int64_t nch = tiles ? (tiles + tpc - 1) / tpc : 0;
  int64_t cnt = 0;
  for (int64_t pt = tiles - 1; pt >= 0; --pt)
    for (int64_t c = 0; c < nch; ++c) {
      int64_t t0, t1;
      cluster_item(tiles, tpc, false, c, pt, t0, t1);
      if (t0 >= t1) continue;
      if (cnt < max_items) {
        items_out[3 * cnt] = t0;
        items_out[3 * cnt + 1] = t1;
        items_out[3 * cnt + 2] = pt;
      }
      ++cnt;
    }
  if (cnt > INT_MAX) return EF_E_INVALID;
  *n_items = (int32_t)cnt;
  return EF_OK;
}

extern "C" int ef_gallery_cluster(ef_ctx* c, int32_t metric, double threshold, int32_t min_samples, int32_t* labels,
                                  int32_t* degree, int64_t* info, uint32_t flags) {
  if (!c) return EF_E_INVALID;
  if (c->gal.k == 0) return set_err(c, EF_E_STATE, "ef_gallery_cluster: no gallery (call ef_gallery_set)");
  if (!labels || !info || (metric != EF_METRIC_L2 && metric != EF_METRIC_COSINE) || threshold != threshold)
    return set_err(c, EF_E_INVALID, "ef_gallery_cluster: bad arguments (labels and info required, metric L2 or "
                                    "cosine, threshold not NaN)");
  if (c->comm && c->comm_size > 1)
    return set_err(c, EF_E_STATE, "ef_gallery_cluster: no clustering over a communicator; cluster each shard on a "
                                  "context without one");
  const Gallery& g = c->gal;
  if (g.n > INT_MAX - KR) return set_err(c, EF_E_INVALID, "ef_gallery_cluster: more than 2^31 - 129 rows");
  EF_HIP(c, hipSetDevice(c->device), "hipSetDevice");
  hipStream_t s = c->stream;
  const bool dev = (flags & EF_MEM_DEVICE) != 0;
  if (g.n == 0) {
    if (dev) EF_HIP(c, hipMemsetAsync(info, 0, 4 * sizeof(int64_t), s), "zero info");
    else std::memset(info, 0, 4 * sizeof(int64_t));
    return EF_OK;
  }
  const int n = (int)g.n;
  const bool dens = min_samples > 1;
  const bool count = dens || degree;
  const int nblocks = (n + 255) / 256;
  const auto carve = [&](Carve& cv, float*& qaux, int*& parent, int*& attach, int*& rank, int*& bsum, int*& deg,
                         unsigned long long*& counters, int*& lab_st, long long*& info_st) {
    qaux = cv.take<float>((size_t)n);
    parent = cv.take<int>((size_t)n);
    attach = cv.take<int>((size_t)n);
    rank = cv.take<int>((size_t)n);
    bsum = cv.take<int>((size_t)nblocks);
    counters = cv.take<unsigned long long>(kCcCount);
    deg = (count && (dev ? !degree : true)) ? cv.take<int>((size_t)n) : nullptr;
    lab_st = dev ? nullptr : cv.take<int>((size_t)n);
    info_st = dev ? nullptr : cv.take<long long>(4);
  };
  float* qaux;
  int *parent, *attach, *rank, *bsum, *deg, *lab_st;
  unsigned long long* counters;
  long long* info_st;
  Carve size, cv;
  carve(size, qaux, parent, attach, rank, bsum, deg, counters, lab_st, info_st);
  EF_TRY(ensure(c, c->cluster_ws, size.total));
  cv.base = c->cluster_ws.p;
  carve(cv, qaux, parent, attach, rank, bsum, deg, counters, lab_st, info_st);
  if (count && !deg) deg = degree;  // a device call's own array

  TimerEvt tm;
  timer_begin(c, EF_KERNEL_CLUSTER, &tm);
  const float* G = static_cast<const float*>(g.G.p);
  EF_HIP(c, launch_census_probe_aux(s, G, n, g.kp, metric, qaux), "cluster probe norms");
  hipLaunchKernelGGL(cluster_init_kernel, dim3((unsigned)std::max(nblocks, 1)), dim3(256), 0, s, n, parent, attach,
                     count ? deg : nullptr, counters);
  EF_HIP(c, hipGetLastError(), "cluster init");

  const int tiles = (n + KR - 1) / KR;
  ClusterArgs a{};
  a.G = G;
  a.aux = static_cast<const float*>(metric == EF_METRIC_L2 ? g.gnorm2.p : g.ginv.p);
  a.qaux = qaux;
  a.n = n;
  a.kp = g.kp;
  a.n_tiles = tiles;
  a.t = (float)threshold;
  a.t64 = threshold;
  a.delta = cluster_delta(c, metric, threshold);
  a.min_samples = min_samples;
  a.degree = deg;
  a.parent = parent;
  a.attach = attach;
  a.counters = counters;
  if (count) {
    a.tpc = (int)cluster_tiles_per_item(tiles, true);
    a.core_deg = nullptr;
    EF_HIP(c, launch_cluster<false>(s, metric, a), "cluster count pass");
  }
  a.tpc = (int)cluster_tiles_per_item(tiles, false);
  a.core_deg = dens ? deg : nullptr;
  EF_HIP(c, launch_cluster<true>(s, metric, a), "cluster link pass");

  const ClusterLabelArgs la{n, min_samples, parent, attach, dens ? deg : nullptr, rank, bsum, counters};
  const dim3 rows((unsigned)nblocks), block(256);
  hipLaunchKernelGGL(cluster_flatten_kernel, rows, block, 0, s, la);
  hipLaunchKernelGGL(cluster_scan_kernel, dim3(1), block, 0, s, la, nblocks);
  hipLaunchKernelGGL(cluster_rank_kernel, rows, block, 0, s, la);
  hipLaunchKernelGGL(cluster_label_kernel, rows, block, 0, s, la, dev ? labels : lab_st,
                     dev ? reinterpret_cast<long long*>(info) : info_st);
  EF_HIP(c, hipGetLastError(), "cluster label kernels");
  timer_end(c, &tm);
  if (dev) return EF_OK;

  EF_HIP(c, hipMemcpyAsync(labels, lab_st, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s), "D2H labels");
  if (degree) EF_HIP(c, hipMemcpyAsync(degree, deg, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s), "D2H degree");
  EF_HIP(c, hipMemcpyAsync(info, info_st, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, s), "D2H info");
  EF_HIP(c, hipStreamSynchronize(s), "sync");
  if (info[3] & EF_CLUSTER_UNCONVERGED) {
    info[3] &= ~EF_CLUSTER_UNCONVERGED;
    return set_err(c, EF_E_NUMERIC, "ef_gallery_cluster: a union-find walk reached its iteration bound");
  }
  return EF_OK;
}
