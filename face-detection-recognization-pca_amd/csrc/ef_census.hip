// Score census (ef_score_census): a distance GEMM whose epilogue bins every
// (probe, gallery row) score into a genuine or an impostor histogram instead of taking an
// arg-best.  One kernel family for every padded k: both operands stream through LDS in
// 16-k slices, so kp = 16 .. 128 and the wide kp (256, 512, multiples of 128 up to 65536) run
// the same code.
//   * workgroup = 4 waves, tile = 128 gallery rows x 128 probes; one LDS stage = 8 KiB of
//     gallery + 8 KiB of probes, double-buffered (32 KiB), filled by global_load_lds; the
//     tile's aux values (||g||^2 or 1/||g||) and row labels ride with its first slice;
//   * wave w owns probes [32w, 32w + 32) of the tile (MFMA B operand) and all 128 rows as four
//     32-row A blocks: four independent fp32 accumulator chains (search_wide_kernel's shape);
//   * 64-B slice rows are XOR-swizzled by (row >> 2) & 3 on the source address: every
//     ds_read_b128 lane group (MI355X_MICROARCH.md, LDS) then covers all 64 banks once;
//   * the epilogue turns each accumulator into the user-facing score, the score into a slot of
//     counts[2][nbins + 3] (side, bin), and adds it to a histogram in LDS (ds_add_u32); rows
//     past n, the probe's excluded row and the probes past b go to a dump slot that is never
//     flushed, so the epilogue has no branch on them;
//   * the non-zero LDS bins are flushed to the 64-bit global counters once per work item
//     (vector integer atomics), before any 32-bit LDS counter could wrap (census_plan).
// Contention: a lane's consecutive scores that fall into one slot are merged
// in registers (a run-length of (slot, count) carried through the whole work item) and the
// histogram is kept twice, selected by lane parity, which halves what is left of the
// same-address serialisation inside one ds_add_u32.  Everything is integer addition: the
// counts do not depend on the order of arrival.
#include "ef_search_common.hpp"

#include <algorithm>

namespace ef {

constexpr int CR = 128;         // gallery rows per tile
constexpr int CP = 128;         // probes per workgroup
constexpr int CBK = 16;         // k per slice
constexpr int CSL = CR * CBK;   // floats per gallery slice (= per probe slice)
// LDS map in floats: [stage 0: gallery | probes][stage 1: gallery | probes][aux of even | odd
// tiles][row labels of even | odd tiles][histogram, two copies]
constexpr int kCensusAux0 = 4 * CSL;
constexpr int kCensusLab0 = kCensusAux0 + 2 * CR;
constexpr int kCensusHist0 = kCensusLab0 + 2 * CR;
// slots of one histogram copy: counts[2][nbins + 3], then the dump slot
__host__ __device__ constexpr int census_copy_slots(int nbins) { return 2 * (nbins + 3) + 1; }
constexpr int census_lds_bytes(int nbins) { return (kCensusHist0 + 2 * census_copy_slots(nbins)) * 4; }
// a work item holds at most 2^31 pairs: 128 probes x 128 rows x 2^17 tiles
constexpr int kCensusMaxTilesPerChunk = 1 << 17;
constexpr int kCensusTargetItems = 2048;  // work items aimed for: 256 CUs x 2 workgroups x 4

struct CensusArgs {
  const float* qpad;  // [bpad][kp]
  const float* G;     // [n][kp]
  const float* aux;   // [n] ||g||^2 (L2) or 1/||g|| (cosine)
  const int* glab;    // [n]
  const float* qaux;  // [bpad] ||q||^2 (L2) or 1/||q|| (cosine)
  const int* plab;    // [bpad]
  const int* pexcl;   // [bpad] excluded local row, -1 for none
  int64_t n, b;
  int kp, n_ptiles, tiles_per_chunk;
  float lo, inv_w;    // inv_w = nbins / (hi - lo)
  int nbins;
  unsigned long long* counts;  // [2][nbins + 3]
};

// What the epilogue needs of each probe: the fp64 sum of squares, rounded once.
template <int METRIC>
__global__ void census_probe_aux_kernel(const float* __restrict__ qpad, int64_t rows, int kp,
                                        float* __restrict__ qaux) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  double s = 0.0;
  for (int c = lane; c < kp; c += 64) {
    const double v = qpad[row * kp + c];
    s = fma(v, v, s);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if (lane == 0) {
    if constexpr (METRIC == EF_METRIC_L2) {
      qaux[row] = (float)s;  // +inf or NaN for a probe that has such a component
    } else {
      const bool finite = s < (double)__builtin_inff();  // false for NaN
      qaux[row] = !finite ? __builtin_nanf("") : s > 0.0 ? (float)(1.0 / sqrt(s)) : 0.f;
    }
  }
}

template <int METRIC>
__global__ __launch_bounds__(256, 2) void census_kernel(const CensusArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  unsigned* const hist = reinterpret_cast<unsigned*>(smem + kCensusHist0);
  const int NS = a.nbins + 3;               // slots per side
  const int HS = census_copy_slots(a.nbins);  // slots per copy; the last one is the dump

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
  chunk_range<CR>(a.n, gc, a.tiles_per_chunk, t0, t1);
  if (t0 >= t1) return;

  for (int i = tid; i < 2 * HS; i += 256) hist[i] = 0u;  // published by the prologue's barrier

  const int ns = a.kp / CBK;  // slices per tile
  const int row_bytes = a.kp * 4;
  const int64_t slot = (int64_t)pt * CP + wave * 32 + c32;  // this lane's probe (< bpad)
  const bool valid = slot < a.b;
  const float qa = a.qaux[slot];
  const int plab = a.plab[slot];
  const int pexcl = a.pexcl[slot];

  // DMA geometry: a slice row is 64 B = four 16-B chunks, a piece is 1 KiB = 16 rows, a slice
  // is 8 pieces per operand and wave w issues pieces 2w, 2w + 1 of each.  Lane l of piece j
  // carries row 16 j + (l >> 2), physical chunk l & 3, which holds logical chunk
  // (l & 3) ^ ((row >> 2) & 3) = (l & 3) ^ ((l >> 4) & 3).
  unsigned goff[2], qoff[2];
#pragma unroll
  for (int jj = 0; jj < 2; ++jj) {
    const int row = (wave * 2 + jj) * 16 + (lane >> 2);
    const unsigned lch16 = (unsigned)(((lane & 3) ^ ((lane >> 4) & 3)) * 16);
    goff[jj] = (unsigned)row * row_bytes + lch16;
    qoff[jj] = (unsigned)(pt * CP + row) * row_bytes + lch16;
  }
  // settle these loads before the loop (a loop-merged wait would drain the LDS-DMA)
  asm volatile("" ::"v"(qa), "v"(plab), "v"(pexcl));

  const unsigned lds_base = lds_addr(smem);
  const unsigned aoff = (unsigned)lane * 4;
  // DMA of slice sl of tile t into buffer buf (+ the tile's aux values and labels with slice 0)
  auto issue = [&](int64_t t, int sl, int buf) {
    const int nrem = tile_rows<CR>(a.n, t);
    const unsigned long long gb = (unsigned long long)(size_t)(a.G + t * CR * a.kp + sl * CBK);
    const unsigned long long qb = (unsigned long long)(size_t)(a.qpad + sl * CBK);
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const int j = wave * 2 + jj;
      glds16s(wide_tail_clamp<CR>(goff[jj], nrem, row_bytes), gb, lds_base + (unsigned)((buf * 2 * CSL + j * 256) * 4));
      glds16s(qoff[jj], qb, lds_base + (unsigned)((buf * 2 * CSL + CSL + j * 256) * 4));
    }
    if (sl == 0 && wave < 2) {  // rows past the end re-read the last row (sent to the dump slot later)
      const int par = (int)((t - t0) & 1);
      const unsigned long long ab = (unsigned long long)(size_t)(wave == 0 ? (const void*)(a.aux + t * CR)
                                                                             : (const void*)(a.glab + t * CR));
      const int dst = (wave == 0 ? kCensusAux0 : kCensusLab0) + par * CR;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int rr = 64 * q + lane;
        const unsigned ao = rr < nrem ? aoff + 256u * q : (unsigned)(nrem - 1) * 4;
        glds4s(ao, ab, lds_base + (unsigned)((dst + 64 * q) * 4));
      }
    }
  };

  // run-length of this lane's scores: `cnt` scores in a row fell into slot `cur`
  const int cbase = (c32 & 1) * HS;  // this lane's histogram copy
  const int dump = cbase + 2 * NS;
  int cur = dump;
  unsigned cnt = 0u;
  const float INF = __builtin_inff();
  const float top = (float)(a.nbins + 1);

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
    const float* const sAux = smem + kCensusAux0 + par * CR;
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
    const float* sg = smem + buf * 2 * CSL;
    const float* sq = sg + CSL;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int pch = ((h * 2 + j) ^ swk) * 4;  // lane half h owns k in [8h, 8h + 8) of the slice
      const float4 bq = *reinterpret_cast<const float4*>(sq + (wave * 32 + c32) * CBK + pch);
      float4 av[4];
#pragma unroll
      for (int rb = 0; rb < 4; ++rb) av[rb] = *reinterpret_cast<const float4*>(sg + (rb * 32 + c32) * CBK + pch);
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
      // register r of block rb is row tb + 4 h + off, off = 32 rb + (r & 3) + 8 (r >> 2)
      const int64_t tb = t * CR + 4 * h;
      const int64_t rem = a.n - tb;  // rows at off >= rem do not exist; a probe past b has none
      const int nrel = !valid ? 0 : rem > CR ? CR : (int)rem;
      const int64_t er = (int64_t)pexcl - tb;  // the excluded row as an off (negative: none)
      const int erel = (er >= 0 && er < CR) ? (int)er : -1;
      const int* const sLab = reinterpret_cast<const int*>(smem + kCensusLab0 + par * CR);
#pragma unroll
      for (int rb = 0; rb < 4; ++rb) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int4 lb = *reinterpret_cast<const int4*>(sLab + rb * 32 + 8 * q + 4 * h);
          const int l[4] = {lb.x, lb.y, lb.z, lb.w};
          float x[4] = {0.f, 0.f, 0.f, 0.f};
          if constexpr (METRIC != EF_METRIC_L2) {
            const float4 xa = *reinterpret_cast<const float4*>(sAux + rb * 32 + 8 * q + 4 * h);
            x[0] = xa.x, x[1] = xa.y, x[2] = xa.z, x[3] = xa.w;
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int off = rb * 32 + 8 * q + j;
            const float v = acc[rb][4 * q + j];
            float sc;
            if constexpr (METRIC == EF_METRIC_L2) sc = __builtin_fmaf(-2.f, v, qa);
            else sc = (v * x[j]) * qa;
            // slot of the score: 0 below lo, 1 + floor((sc - lo) / w), nbins + 1 from hi on
            const float tt = (sc - a.lo) * a.inv_w;
            int s = (int)fminf(fmaxf(floorf(tt) + 1.f, 0.f), top);
            s = fabsf(sc) < INF ? s : a.nbins + 2;  // NaN and +-inf
            s += l[j] != plab ? NS : 0;
            s += cbase;
            s = (off >= nrel || off == erel) ? dump : s;
            if (s != cur) {
              atomicAdd(&hist[cur], cnt);
              cur = s;
              cnt = 0u;
            }
            ++cnt;
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

  atomicAdd(&hist[cur], cnt);
  __syncthreads();
  for (int i = tid; i < 2 * NS; i += 256) {
    const unsigned v = hist[i] + hist[HS + i];
    if (v) atomicAdd(&a.counts[i], (unsigned long long)v);
  }
}

hipError_t launch_census_probe_aux(hipStream_t s, const float* qpad, int64_t rows, int kp, int metric, float* qaux) {
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  if (metric == EF_METRIC_L2)
    hipLaunchKernelGGL(census_probe_aux_kernel<EF_METRIC_L2>, grid, block, 0, s, qpad, rows, kp, qaux);
  else
    hipLaunchKernelGGL(census_probe_aux_kernel<EF_METRIC_COSINE>, grid, block, 0, s, qpad, rows, kp, qaux);
  return hipGetLastError();
}

hipError_t launch_census(hipStream_t s, int kp, int metric, const float* qpad, int64_t bpad, int64_t b, const float* G,
                         const float* aux, const int* glab, int64_t n, const float* qaux, const int* plab,
                         const int* pexcl, float lo, float hi, int nbins, unsigned long long* counts) {
  if (n <= 0 || b <= 0) return hipSuccess;
  // 32-bit geometry of the kernel: probe rows addressed by unsigned byte offsets
  if (kp % CBK != 0 || bpad % CP != 0 || b > bpad || bpad * (int64_t)kp * 4 >= ((int64_t)1 << 31) || nbins < 1 ||
      nbins > kCensusMaxBins)
    return hipErrorInvalidValue;
  // the plan: about kCensusTargetItems work items, each at most kCensusMaxTilesPerChunk tiles so
  // that no 32-bit LDS counter can wrap before the flush
  const int64_t n_ptiles = bpad / CP;
  const int64_t tiles_total = (n + CR - 1) / CR;
  const int64_t want = std::max<int64_t>(1, (kCensusTargetItems + n_ptiles - 1) / n_ptiles);
  int64_t tpc = (tiles_total + std::min(want, tiles_total) - 1) / std::min(want, tiles_total);
  tpc = std::min<int64_t>(tpc, kCensusMaxTilesPerChunk);
  const int64_t nchunks = (tiles_total + tpc - 1) / tpc;
  if (nchunks * n_ptiles >= ((int64_t)1 << 31)) return hipErrorInvalidValue;

  CensusArgs a{qpad, G, aux, glab, qaux, plab, pexcl, n, b, kp, (int)n_ptiles, (int)tpc, lo,
               (float)((double)nbins / ((double)hi - (double)lo)), nbins, counts};
  const int lds = census_lds_bytes(nbins);
  const dim3 grid((unsigned)(nchunks * n_ptiles)), block(256);
  const void* fn = metric == EF_METRIC_L2 ? reinterpret_cast<const void*>(census_kernel<EF_METRIC_L2>)
                                          : reinterpret_cast<const void*>(census_kernel<EF_METRIC_COSINE>);
  const hipError_t e = allow_dynamic_lds(fn, census_lds_bytes(kCensusMaxBins));
  if (e != hipSuccess) return e;
  if (metric == EF_METRIC_L2)
    hipLaunchKernelGGL(census_kernel<EF_METRIC_L2>, grid, block, lds, s, a);
  else
    hipLaunchKernelGGL(census_kernel<EF_METRIC_COSINE>, grid, block, lds, s, a);
  return hipGetLastError();
}

}  // namespace ef
