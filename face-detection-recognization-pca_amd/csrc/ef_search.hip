// Distance GEMM with fused arg-best epilogue.
//
// Replaces `cosine_similarity([f], face_features)` + `np.argmax`
// (scan-template-v4.py:274-275) and the per-row Python loop of useless/scan.py:122-127,
// batched over B probes, plus the north-star L2 argmin.
//
// Layout in HBM:  gallery G[n][KP] fp32 (k zero-padded to KP), gnorm2[n], ginv[n];
// probe features Qp[bpad][KP] (bpad a multiple of 256).
//
// Pass 1 — search_kernel (the hot kernel, v_mfma_f32_32x32x2_f32, exact fp32):
//   * workgroup = 8 waves = 256 probes; each wave keeps 32 probes (one 32-probe
//     B-operand block, KP/2 fp32 VGPRs, pre-scaled) in registers for the whole sweep;
//   * the workgroup sweeps one chunk of the gallery in 64-row tiles (two 32-row MFMA
//     blocks = two independent accumulator chains per wave) staged through
//     double-buffered LDS by LDS-DMA (global_load_lds, ef_dma.hpp), tile t+1's DMA in
//     flight under tile t's MFMAs;
//   * the gallery tile is the MFMA A operand so each lane's 16 accumulators hold 16
//     gallery rows of ONE probe: the arg-best is an in-lane running (best, index,
//     runner-up) with no cross-lane traffic until one __shfl_xor(32) at the end;
//   * K is permuted (lane half h owns k in [h*KP/2, (h+1)*KP/2)) so every A fragment is a
//     conflict-free ds_read_b128 feeding 4 MFMAs;
//   * blockIdx is remapped so the workgroups sharing a gallery chunk run on one XCD
//     (same blockIdx % 8) and hit its L2;
//   * each workgroup writes its per-probe (best key, runner-up score) for its chunk.
// Pass 2 — reduce_kernel: per probe, min over chunks -> winner + global runner-up; the
//   winner is re-scored in fp64 (difference form for L2).  A rigorous fp32 error bound
//   decides whether the runner-up could beat the winner; if so the probe is queued.  Outside
//   the bound's domain (scan_regular, ef_search_common.hpp: fp32 squares near overflow or
//   underflow, non-finite rows) the probe is queued for a sweep of every row instead, and a
//   probe with a NaN or an infinite component gets no key.
// Pass 3 (only for queued probes; a no-op launch otherwise) — the search kernel in
//   COLLECT mode gathers every row whose fp32 score is within the bound, and
//   resolve_kernel re-scores them in fp64 and keeps the lowest index among exact ties.
// Result: the argmin/argmax identity equals an fp64 evaluation with lowest-index
// tie-break (np.argmin / np.argmax semantics), independent of fp32 rounding.
//
// Split-bf16 scores (S3, EF_OPT_SEARCH_SPLIT_BF16): every fp32 operand x is carried as
// x = hi + lo + e with hi = bf16(x), lo = bf16(x - hi), |e| <= 2^-16 |x|, and the dot
// product is hi.hi' + hi.lo' + lo.hi' on v_mfma_f32_32x32x16_bf16 (products exact in fp32,
// fp32 accumulation): 3 bf16 MFMAs per 16 k instead of 8 fp32 ones, i.e. 16/3 x the
// arithmetic rate.  The gallery's split copy has the fp32 row's byte layout (per 8
// elements: 16 B of hi, 16 B of lo), so the tile DMA and the LDS reads are those of the
// fp32 kernel.  The pass-2 bound covers the dropped terms (lo.lo', e) and the longer
// chain; the winner is still re-scored from the fp32 gallery in fp64, so keys and match
// records equal the fp32 path's bit for bit whenever both resolve
// (tests/test_gpu_search_split.py; at the full C3 size, tests/test_gpu_c3_full.py).
//
// Prefix scan (EF_OPT_SEARCH_PREFIX; L2, EF_OPT_SEARCH_SPLIT_BF16 = 0): a scan over a compact
// copy of the rows' first K1 components, in split-bf16 arithmetic by default
// (EF_OPT_SEARCH_PREFIX_SPLIT; prefix64_kernel at K1 <= 32, search_kernel<K1, .., S3> at 64) or
// in fp32 (search_kernel<K1>), gives a lower bound of every distance;
// reduce_prefix_kernel proves the winner from it where it can, and only the unproven probes
// go through passes 1-3 at full k (launch_search_prefix).  At K1 <= 32 the split
// scan is the middle of a cascade (EF_OPT_SEARCH_PREFIX_SCREEN): a single-bf16 screen with a
// bound per row and per probe goes first (prefix64x_kernel, reduce_prefix_x_kernel) and the
// split scan runs for the probes it cannot prove alone.
//
// Top-m search (ef_search_topk.hip) launches pass 1 and the COLLECT pass of
// these kernels through launch_search_scan, with its own threshold and resolution kernels.
#include "ef_search_common.hpp"

#include <cstdlib>
#include <cmath>

namespace ef {

constexpr int TG = 64;  // gallery rows per LDS tile (two 32-row MFMA blocks)
// rows per tile of the prefix scans at K1 <= 32: fp32, and split bf16 (profiles/r11: 256 rows
// measured 0.847 ms per C3 step against 0.872 at 128 and 0.909 at 64)
constexpr int kPrefixTile = 128, kPrefixSplitTile = 256;
// probes per workgroup of the split-bf16 prefix scan at K1 <= 32 (prefix64_kernel: 8 waves x 64
// probes); search_plan takes it for the plans of kPrefixSplitTile rows
constexpr int kPrefixSplitProbes = 512;

// round-to-nearest-even fp32 -> bf16 bits (finite inputs) and back
__device__ __forceinline__ unsigned bf16_bits(float x) {
  const unsigned u = __float_as_uint(x);
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ float bf16_value(unsigned b) { return __uint_as_float(b << 16); }
// 8 consecutive fp32 values -> (hi, lo) bf16x8 fragments
__device__ __forceinline__ void split8(const float* x, bf16x8& hi, bf16x8& lo) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const unsigned h = bf16_bits(x[j]);
    hi[j] = (short)h;
    lo[j] = (short)bf16_bits(x[j] - bf16_value(h));
  }
}

// Workgroup = 8 waves x 32 probes = 256 probes (the gallery is swept Bpad/256 times).
// Each wave keeps its 32 probes as one B block (KP/2 VGPRs, pre-scaled) and runs the
// tile's two 32-row blocks as two independent accumulator chains; the arg-best epilogue
// is a branch-free top-2 in row order on registers.  <= 128 VGPRs -> 4 waves per SIMD.
// CNT (main pass of the prefix path's second run, launch_search_prefix): the probe count is
// on the device (ws.amb_count[1]); workgroups whose probe tile starts at or past it return.
// TGT: gallery rows per LDS tile, TGT / 32 independent accumulator chains per wave.  64
// everywhere but the fp32 prefix scan at K1 <= 32, whose tiles hold so few MFMAs that the
// per-tile costs (barrier, DMA issue and wait, first LDS reads) show; 128 rows halve them.
// The split-bf16 prefix scan at K1 <= 32 is a kernel of its own (prefix64_kernel below).
// LBL (ef_search_labelled): the tile's row labels are staged beside its aux
// values (wave 1 issues that DMA), and every finished block's scores pass label_mask before
// consume — the fp32 scan at TGT = 64 only.
template <int KP, int METRIC, bool COLLECT, bool S3 = false, bool CNT = false, int TGT = TG, bool LBL = false>
__global__ __launch_bounds__(512, 4) void search_kernel(
    const float* __restrict__ qpad, const float* __restrict__ G, const float* __restrict__ aux, int64_t n,
    int n_ptiles, int tiles_per_chunk, int64_t bpad, SearchWs ws) {
  constexpr int NW = 8;
  constexpr int KH = KP / 2;
  constexpr int CPR = KP / 4;                                          // 16-B chunks per row
  constexpr int SW = (CPR & 15) == 0 ? 16 : ((CPR & 7) == 0 ? 8 : 4);  // XOR swizzle width
  constexpr int NB = TGT / 32;                                         // 32-row MFMA blocks per tile
  constexpr int NI = TGT * CPR / 64;                                   // 1-KiB LDS-DMA pieces per tile
  constexpr int PPW = (NI + NW - 1) / NW;                              // pieces per wave
  constexpr int RP = 64 / CPR;                                         // rows per piece
  static_assert((NI % NW == 0 || NI < NW) && RP * CPR == 64 && TG == 64, "tile must be whole 1-KiB pieces");
  static_assert(TGT == 64 || (KP <= 32 && !COLLECT && !S3 && TGT == kPrefixTile),
                "larger tiles: the fp32 prefix scan at KP <= 32");
  static_assert(!LBL || (!S3 && !CNT && TGT == TG), "labelled: the fp32 scan in 64-row tiles");
  // KP = 128 (the k = 128 headline shape): no swizzle.  LDS piece p (1 KiB + 16 B pad)
  // holds row p of the tile's first 32-row block and row 32 + p of the second, so the
  // lane reading row c32 of either block uses one base (c32 * 1040 B) plus immediate
  // offsets — no per-read VALU address math, which costs MFMA issue cycles
  // (tools/micro/mfma_valu_probe.cpp) — and the 1040-B stride (260 = 4 mod 64 banks)
  // keeps every ds_read_b128 lane group conflict-free.  One full-wave DMA per piece.
  constexpr bool PAD = KP == 128;
  constexpr int PS = 2 * KP + 4;          // PAD: floats per piece (two rows + 16 B)
  constexpr int TGS = PAD ? 32 * PS : TGT * KP;  // floats per tile buffer

  // Unpadded [TG][KP] tiles filled by global_load_lds (lane-linear 1-KiB pieces); the
  // chunk order inside each row is XOR-swizzled by (row & (SW-1)) on the SOURCE address so
  // the A-fragment ds_read_b128s (16 lanes = 16 rows, same logical chunk) hit distinct
  // banks.  All LDS lives in one array (a second __shared__ object can de-pipeline).
  __shared__ __attribute__((aligned(16))) float smem[2 * TGS + 2 * TGT + (LBL ? 2 * TGT + 2 * 512 : 0)];
  float* const sG0 = smem;
  float* const sAux0 = smem + 2 * TGS;
  constexpr int LAB0 = 2 * TGS + 2 * TGT;  // LBL: the two tiles' row labels (int bits)
  // LBL: each lane's (probe label, excluded row - 4 h), parked in LDS and re-read per tile: held
  // in registers for the sweep, the pair costs search_kernel<128> (126 VGPRs without it) spills
  constexpr int STASH0 = LAB0 + 2 * TGT;

  // one (gallery chunk gc, probe tile pt) work item
  auto body = [&](const int gc, const int pt, const int n_amb) {

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5;
  const int c32 = lane & 31;
  const int lrow = lane / CPR, lc = lane % CPR;  // this lane's (row, chunk) inside a piece

  int64_t t0, t1;
  chunk_range<TGT>(n, gc, tiles_per_chunk, t0, t1);
  const int64_t s0 = (int64_t)pt * 256 + wave * 32 + c32;  // this lane's probe slot

  if (t0 >= t1) {  // empty chunk: publish "no candidate" so the reducer can skip it
    if constexpr (!COLLECT) {
      if (h == 0) top2_store_empty(ws, (int64_t)gc * bpad, s0);
    }
    return;
  }

  // Issue the LDS-DMA of tile t into buffer buf.  Wave w fills pieces [w*PPW, (w+1)*PPW);
  // a piece is RP whole rows.  The swizzle splits into a lane constant and a wave-uniform
  // part: row & (SW-1) == ((j*RP) & (SW-1)) ^ (lrow & (SW-1)) for power-of-two RP, SW.
  // Rows past n (tail tile only) are clamped to a valid row and masked in the epilogue.
  const int lcx = lc ^ (lrow & (SW - 1));
  const unsigned lds_base = lds_addr(smem);
  // Full tiles use the SGPR-base DMA form: per piece one v_xor + one v_lshl_add (every VALU
  // instruction in this loop costs MFMA issue time); the tail tile clamps rows instead.
  auto issue_tile = [&](int64_t t, int buf) {
    const int nrem = (int)((n - t * TGT) < TGT ? (n - t * TGT) : TGT);
    if constexpr (PAD) {  // piece p = rows p (lanes 0-31) and 32 + p (lanes 32-63)
      const unsigned m0 = lds_base + (unsigned)(buf * TGS * 4);
      unsigned lid;  // re-derived in place (a loop-long VGPR would be spilled by hipcc)
      asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lid));
      if (nrem == TGT) {
        const unsigned long long gb = uniform_ptr(G + t * TGT * KP);
        if (wave == 0) glds4s(lid * 4u, uniform_ptr(aux + t * TG), lds_base + (unsigned)((2 * TGS + buf * TG) * 4));
        if constexpr (LBL) {
          if (wave == 1 && ws.glab) glds4s(lid * 4u, uniform_ptr(ws.glab + t * TG), lds_base + (unsigned)((LAB0 + buf * TG) * 4));
        }
        const unsigned voff = ((lid >> 5) * 32 * KP + (lid & 31) * 4) * 4;
#pragma unroll
        for (int jj = 0; jj < PPW; ++jj) {
          const int p = wave * PPW + jj;
          glds16s(voff, gb + (unsigned long long)(p * KP * 4), m0 + (unsigned)(p * PS * 4));
        }
      } else {
        const float* gbase = G + t * TGT * KP;
#pragma unroll
        for (int jj = 0; jj < PPW; ++jj) {
          const int p = wave * PPW + jj;
          int row = p + (int)(lid >> 5) * 32;
          row = row < nrem ? row : nrem - 1;
          glds16(gbase + row * KP + (lid & 31) * 4, m0 + (unsigned)(p * PS * 4));
        }
        if (wave == 0) {
          const int row = (int)lid < nrem ? (int)lid : nrem - 1;
          glds4(aux + t * TG + row, lds_base + (unsigned)((2 * TGS + buf * TG) * 4));
        }
        if constexpr (LBL) {
          if (wave == 1 && ws.glab) {
            const int row = (int)lid < nrem ? (int)lid : nrem - 1;
            glds4(ws.glab + t * TG + row, lds_base + (unsigned)((LAB0 + buf * TG) * 4));
          }
        }
      }
      return;
    }
    int lx = lcx, lr = lrow;
    asm volatile("" : "+v"(lx), "+v"(lr));  // recompute per tile (no hoisted per-piece VGPRs)
    if (nrem == TGT) {
      const unsigned long long gb = uniform_ptr(G + t * TGT * KP);
      const unsigned lro = (unsigned)(lr * KP * 4);
#pragma unroll
      for (int jj = 0; jj < PPW; ++jj) {
        const int j = wave * PPW + jj;
        if (NI >= NW || wave < NI) {  // uniform
          const int sj = (j * RP) & (SW - 1);
          glds16s(lro + ((unsigned)(lx ^ sj) << 4), gb + (unsigned long long)(j * RP * KP * 4),
                  lds_base + (unsigned)((buf * TGS + j * 256) * 4));
        }
      }
      if constexpr (TGT == 64) {
        if (wave == 0) glds4s((unsigned)lane * 4u, uniform_ptr(aux + t * TG), lds_base + (unsigned)((2 * TGS + buf * TG) * 4));
        if constexpr (LBL) {
          if (wave == 1 && ws.glab) glds4s((unsigned)lane * 4u, uniform_ptr(ws.glab + t * TG), lds_base + (unsigned)((LAB0 + buf * TG) * 4));
        }
      } else {  // one 64-row half of the norms per wave
        if (wave < TGT / 64)
          glds4s((unsigned)lane * 4u, uniform_ptr(aux + t * TGT + wave * 64),
                 lds_base + (unsigned)((2 * TGS + buf * TGT + wave * 64) * 4));
      }
    } else {
      const float* gbase = G + t * TGT * KP;  // wave-uniform
#pragma unroll
      for (int jj = 0; jj < PPW; ++jj) {
        const int j = wave * PPW + jj;
        if (NI >= NW || wave < NI) {  // uniform
          const int sj = (j * RP) & (SW - 1);
          int row = j * RP + lr;
          row = row < nrem ? row : nrem - 1;
          glds16(gbase + row * KP + ((lx ^ sj) << 2), lds_base + (unsigned)((buf * TGS + j * 256) * 4));
        }
      }
      if constexpr (TGT == 64) {
        if (wave == 0) {
          const int row = lane < nrem ? lane : nrem - 1;
          glds4(aux + t * TG + row, lds_base + (unsigned)((2 * TGS + buf * TG) * 4));  // one 4-B piece per lane
        }
        if constexpr (LBL) {
          if (wave == 1 && ws.glab) {
            const int row = lane < nrem ? lane : nrem - 1;
            glds4(ws.glab + t * TG + row, lds_base + (unsigned)((LAB0 + buf * TG) * 4));
          }
        }
      } else {
        if (wave < TGT / 64) {
          const int row = wave * 64 + lane < nrem ? wave * 64 + lane : nrem - 1;
          glds4(aux + t * TGT + row, lds_base + (unsigned)((2 * TGS + buf * TGT + wave * 64) * 4));
        }
      }
    }
  };

  issue_tile(t0, 0);

  // Probe fragments (B operand): lane holds probe c32, k in [h*KH, h*KH+KH), pre-scaled
  // (exactly) so the chain yields the score: L2 acc = ||g||^2 + sum(-2q)g (the chain
  // starts from ||g||^2), cosine acc = -q.g (times 1/||g|| after the chain).
  constexpr float QS = METRIC == EF_METRIC_L2 ? -2.f : -1.f;
  // S3: the same k range as split (hi, lo) bf16x8 fragments, fragment i = k h*KH + 8i + [0, 8)
  constexpr int NF = KH / 8;
  float qb[S3 ? 1 : KH];
  bf16x8 qh[S3 ? NF : 1], ql[S3 ? NF : 1];
  {
    int64_t r0 = s0;
    bool v0 = true;
    if constexpr (COLLECT) {
      v0 = s0 < n_amb;
      r0 = v0 ? ws.amb_list[s0] : 0;
    }
    if constexpr (LBL) {  // read back by this lane alone: no barrier
      const LabelLane l = label_lane(ws, r0, h);
      *reinterpret_cast<int2*>(smem + STASH0 + 2 * tid) = make_int2(l.plab, l.excl_h);
    }
    const float4* q0 = reinterpret_cast<const float4*>(qpad + r0 * KP + h * KH);
    if constexpr (S3) {
#pragma unroll
      for (int i = 0; i < NF; ++i) {
        const float4 a = v0 ? q0[2 * i] : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 b = v0 ? q0[2 * i + 1] : make_float4(0.f, 0.f, 0.f, 0.f);
        const float t[8] = {QS * a.x, QS * a.y, QS * a.z, QS * a.w, QS * b.x, QS * b.y, QS * b.z, QS * b.w};
        split8(t, qh[i], ql[i]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < KH / 4; ++j) {
        const float4 a = v0 ? q0[j] : make_float4(0.f, 0.f, 0.f, 0.f);
        qb[4 * j] = QS * a.x; qb[4 * j + 1] = QS * a.y; qb[4 * j + 2] = QS * a.z; qb[4 * j + 3] = QS * a.w;
      }
    }
  }
  const float thr = collect_threshold<COLLECT>(ws, s0, n_amb);
  // Consume every probe register here, so hipcc places its waits for these loads before
  // the loop; otherwise its (loop-merged) wait state puts vmcnt(0) inside the tile loop,
  // which would also drain the asm LDS-DMA of the next tile.
  if constexpr (S3) {
#pragma unroll
    for (int i = 0; i < NF; ++i) asm volatile("" ::"v"(qh[i]), "v"(ql[i]));
  } else {
#pragma unroll
    for (int j = 0; j < KH; ++j) asm volatile("" ::"v"(qb[j]));
  }
  asm volatile("" ::"v"(thr));

  const float INF = __builtin_inff();
  float b1 = INF, b2 = INF;
  int i1 = INT_MAX;

  // Arg-best epilogue of one finished block of scores v (register r <-> row
  // rowbase + (r&3) + 8(r>>2) + 4h, increasing with r): branch-free top-2 in row order
  // (strict '<' keeps the lowest row on ties; v_med3 keeps the runner-up), then merged
  // into the running (best, index, runner-up).  COLLECT appends rows within thr instead.
  auto consume = [&](const f32x16& v, int rowbase) {
    if constexpr (COLLECT) {
#pragma unroll
      for (int r = 0; r < 16; ++r) collect_hit(ws, s0, thr, v[r], rowbase, (r & 3) + 8 * (r >> 2) + 4 * h);
    } else {
      // Screen: a block whose minimum is not below the lane's runner-up changes neither
      // b1, b2 nor i1 (the update below would keep all three), so when no lane of the wave
      // has such a row the block is skipped on a uniform branch — ~8 v_min3 per 16 scores
      // instead of ~64 VALU ops, once the running top-2 has settled.
      float mn = v[0];
#pragma unroll
      for (int r = 1; r < 16; ++r) mn = fminf(mn, v[r]);
      if (!__any(mn < b2)) return;
      float m1 = v[0], m2 = INF;
      int ir = 0;
#pragma unroll
      for (int r = 1; r < 16; ++r) {
        const bool lt = v[r] < m1;
        m2 = __builtin_amdgcn_fmed3f(m1, v[r], m2);
        ir = lt ? r : ir;
        m1 = lt ? v[r] : m1;
      }
      const bool lt = m1 < b1;
      b2 = lt ? fminf(b1, m2) : fminf(b2, m1);
      i1 = lt ? rowbase + (ir & 3) + 8 * (ir >> 2) + 4 * h : i1;
      b1 = lt ? m1 : b1;
    }
  };

  // Accumulator start value: ||g||^2 of the block's rows for L2 (four float4 reads of the
  // staged norms match the register <-> row map), 0 for cosine.
  auto acc_init = [&](const float* tileA_blk) {
    f32x16 a = {};
    if constexpr (METRIC == EF_METRIC_L2) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 x = *reinterpret_cast<const float4*>(tileA_blk + 8 * q + 4 * h);
        a[4 * q] = x.x;
        a[4 * q + 1] = x.y;
        a[4 * q + 2] = x.z;
        a[4 * q + 3] = x.w;
      }
    }
    return a;
  };

  dma_wait_all();
  __syncthreads();  // tile t0 landed

  for (int64_t t = t0; t < t1; ++t) {
    const int buf = (int)((t - t0) & 1);
    if (t + 1 < t1) issue_tile(t + 1, buf ^ 1);  // lands under this tile's MFMAs
    const float* tileG = sG0 + buf * TGS;
    const float* tileA = sAux0 + buf * TGT;
    const bool tail = (t + 1) * TGT > n;
    const int tbase = (int)(t * TGT);
    int swz = PAD ? 0 : c32 & (SW - 1);  // rows c32 and 32 + c32 share (row & (SW-1)), SW <= 16
    // opaque per tile: stops hipcc hoisting all KH/4 swizzled addresses out of the loop
    if constexpr (!PAD) asm volatile("" : "+v"(swz));
    if constexpr (TGT != 64 && !S3) {
      // NB blocks at once: NB independent accumulator chains sharing the B operand, block
      // bi = rows 32 bi + c32 (the same swizzle: 32 is a multiple of SW)
      const float* arow = tileG + c32 * KP;
      f32x16 acc[NB];
#pragma unroll
      for (int bi = 0; bi < NB; ++bi) acc[bi] = acc_init(tileA + 32 * bi);
#pragma unroll
      for (int s = 0; s < KH; s += 4) {
        const int chunk = (h * (CPR / 2) + s / 4) ^ swz;
        float4 a[NB];
#pragma unroll
        for (int bi = 0; bi < NB; ++bi) a[bi] = *reinterpret_cast<const float4*>(arow + bi * 32 * KP + chunk * 4);
#pragma unroll
        for (int bi = 0; bi < NB; ++bi) acc[bi] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[bi].x, qb[s], acc[bi], 0, 0, 0);
#pragma unroll
        for (int bi = 0; bi < NB; ++bi) acc[bi] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[bi].y, qb[s + 1], acc[bi], 0, 0, 0);
#pragma unroll
        for (int bi = 0; bi < NB; ++bi) acc[bi] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[bi].z, qb[s + 2], acc[bi], 0, 0, 0);
#pragma unroll
        for (int bi = 0; bi < NB; ++bi) acc[bi] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[bi].w, qb[s + 3], acc[bi], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);  // bound the A prefetch depth
      }
#pragma unroll
      for (int bi = 0; bi < NB; ++bi) {
        if constexpr (METRIC != EF_METRIC_L2) {  // cosine: -(q.g) * (1/||g||)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float4 x = *reinterpret_cast<const float4*>(tileA + 32 * bi + 8 * q + 4 * h);
            acc[bi][4 * q] *= x.x; acc[bi][4 * q + 1] *= x.y; acc[bi][4 * q + 2] *= x.z; acc[bi][4 * q + 3] *= x.w;
          }
        }
        if (tail) {  // uniform: only the last tile has rows past n
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (tbase + 32 * bi + (r & 3) + 8 * (r >> 2) + 4 * h >= n) acc[bi][r] = INF;
        }
      }
#pragma unroll
      for (int bi = 0; bi < NB; ++bi) consume(acc[bi], tbase + 32 * bi);  // in row order (tie rule)
      dma_wait_all();
      __syncthreads();  // tile t+1 landed; everyone is done reading buffer buf
      continue;
    }
    const float* arow0 = tileG + (PAD ? c32 * PS : c32 * KP);
    const float* arow1 = PAD ? arow0 + KP : tileG + (32 + c32) * KP;

    // both 32-row blocks at once: two independent accumulator chains sharing the B operand
    f32x16 acc0 = acc_init(tileA), acc1 = acc_init(tileA + 32);
    if constexpr (S3) {
      // fragment i: chunks 2i (hi) and 2i + 1 (lo) of this lane half's k range
#pragma unroll
      for (int i = 0; i < NF; ++i) {
        const int c0 = h * (CPR / 2) + 2 * i;
        const int ch = PAD ? c0 : c0 ^ swz, cl = PAD ? c0 + 1 : (c0 + 1) ^ swz;
        const bf16x8 ah = as_bf16x8(*reinterpret_cast<const float4*>(arow0 + ch * 4));
        const bf16x8 bh = as_bf16x8(*reinterpret_cast<const float4*>(arow1 + ch * 4));
        const bf16x8 al = as_bf16x8(*reinterpret_cast<const float4*>(arow0 + cl * 4));
        const bf16x8 bl = as_bf16x8(*reinterpret_cast<const float4*>(arow1 + cl * 4));
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, qh[i], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bh, qh[i], acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, ql[i], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bh, ql[i], acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, qh[i], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bl, qh[i], acc1, 0, 0, 0);
        if (i % 2 == 1) __builtin_amdgcn_sched_barrier(0);  // bound the A prefetch depth
      }
    } else
#pragma unroll
    for (int s = 0; s < KH; s += 4) {
      const int chunk = PAD ? h * (CPR / 2) + s / 4 : (h * (CPR / 2) + s / 4) ^ swz;
      const float4 a = *reinterpret_cast<const float4*>(arow0 + chunk * 4);
      const float4 b = *reinterpret_cast<const float4*>(arow1 + chunk * 4);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, qb[s], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(b.x, qb[s], acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, qb[s + 1], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(b.y, qb[s + 1], acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, qb[s + 2], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(b.z, qb[s + 2], acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, qb[s + 3], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(b.w, qb[s + 3], acc1, 0, 0, 0);
      if ((s / 4) % 2 == 1) __builtin_amdgcn_sched_barrier(0);  // bound the A prefetch depth
    }
    if constexpr (METRIC != EF_METRIC_L2) {  // cosine: -(q.g) * (1/||g||)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 x = *reinterpret_cast<const float4*>(tileA + 8 * q + 4 * h);
        const float4 y = *reinterpret_cast<const float4*>(tileA + 32 + 8 * q + 4 * h);
        acc0[4 * q] *= x.x; acc0[4 * q + 1] *= x.y; acc0[4 * q + 2] *= x.z; acc0[4 * q + 3] *= x.w;
        acc1[4 * q] *= y.x; acc1[4 * q + 1] *= y.y; acc1[4 * q + 2] *= y.z; acc1[4 * q + 3] *= y.w;
      }
    }
    if (tail) {  // uniform: only the last tile has rows past n
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = tbase + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (row >= n) acc0[r] = INF;
        if (row + 32 >= n) acc1[r] = INF;
      }
    }
    if constexpr (LBL) {  // rows that do not qualify for this lane's probe: +inf as well
      const float* tileL = smem + LAB0 + buf * TGT;
      unsigned lid;  // re-derived in place, as in issue_tile
      asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lid));
      const int2 pe = *reinterpret_cast<const int2*>(smem + STASH0 + 2 * (wave * 64 + (int)lid));
      const LabelLane lab{pe.x, pe.y, ws.lbl == EF_LABEL_OTHER + 1, ws.lbl == EF_LABEL_ANY + 1};
      // block 1 is masked after block 0 is consumed: its label registers take block 0's place
      label_mask(acc0, tileL, tbase, h, lab);
      consume(acc0, tbase);
      label_mask(acc1, tileL + 32, tbase + 32, h, lab);
      consume(acc1, tbase + 32);
    } else {
      consume(acc0, tbase);  // rows of block 0 precede block 1 (row-order tie rule)
      consume(acc1, tbase + 32);
    }
    dma_wait_all();
    __syncthreads();  // tile t+1 landed; everyone is done reading buffer buf
  }

  if constexpr (!COLLECT) {
    // Merge the two lane halves (same probe, disjoint rows).
    const float ob1 = __shfl_xor(b1, 32);
    const int oi1 = __shfl_xor(i1, 32);
    const float ob2 = __shfl_xor(b2, 32);
    top2_merge(b1, b2, i1, ob1, ob2, oi1);
    if (h == 0) top2_store(ws, (int64_t)gc * bpad, s0, b1, b2, i1);
  }
  };  // body
  if constexpr (COLLECT) {
    collect_items<kSearchProbeTile>(ws, n_ptiles, body);  // n_ptiles carries the collect plan's chunk count
  } else {
    // each XCD gets a contiguous run of (chunk, probe-tile) pairs, so the probe tiles of
    // one chunk are co-resident on it
    const int lin = xcd_lin();
    const int gc = lin / n_ptiles;
    if constexpr (CNT) {
      if ((lin - gc * n_ptiles) * kSearchProbeTile >= ws.amb_count[1]) return;  // workgroup-uniform
    }
    body(gc, lin - gc * n_ptiles, 0);
  }
}

// Split-bf16 scan on v_mfma_f32_16x16x32_bf16, KP = 128 (the C3 shape).  Same workgroup,
// tile, LDS layout (the padded two-row pieces) and SearchWs contract as search_kernel; the
// 16 x 16 shape is chosen because under the clock the chip holds on bf16 MFMA loads it
// delivers more FLOP/s than 32 x 32 at equal cycles per FLOP (MI355X_MICROARCH.md, DVFS
// give-back item 7).  Lane l = (quarter qd = l >> 4, r16 = l & 15): it supplies row r16
// of each 16-row A block and probe r16 of each 16-probe B block for k-quarter qd, where
// quarter qd of step i is elements 32 qd + 8 i + [0, 8) (chunks 8 qd + 2i = hi, + 1 = lo
// of the row: one ds_read_b128 each, conflict-free on the 1040-B piece stride).  A wave
// keeps 32 probes as two B blocks (pb) and runs the tile's four 16-row blocks (rb) against
// both: 8 accumulators of 4 rows (row 16 rb + 4 qd + reg, probe 16 pb + r16), 96 MFMAs per
// 64-row tile.  Each lane carries the running top-2 of its two probes; the four quarters
// are merged by two shuffles at the end.
template <int METRIC, bool COLLECT>
__global__ __launch_bounds__(512, 4) void search16_kernel(
    const float* __restrict__ qpad, const float* __restrict__ G3, const float* __restrict__ aux, int64_t n,
    int n_ptiles, int tiles_per_chunk, int64_t bpad, SearchWs ws) {
  constexpr int KP = 128, PS = 2 * KP + 4, TGS = 32 * PS, PPW = 4;  // 8 waves x 4 pieces
  __shared__ __attribute__((aligned(16))) float smem[2 * TGS + 2 * TG];
  float* const sAux0 = smem + 2 * TGS;

  // one (gallery chunk gc, probe tile pt) work item
  auto body = [&](const int gc, const int pt, const int n_amb) {
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qd = lane >> 4, r16 = lane & 15;
  int64_t t0, t1;
  chunk_range<TG>(n, gc, tiles_per_chunk, t0, t1);
  int64_t sl0[2];
  sl0[0] = (int64_t)pt * 256 + wave * 32 + r16;
  sl0[1] = sl0[0] + 16;

  if (t0 >= t1) {
    if constexpr (!COLLECT) {
      if (qd == 0) {
#pragma unroll
        for (int pb = 0; pb < 2; ++pb) top2_store_empty(ws, (int64_t)gc * bpad, sl0[pb]);
      }
    }
    return;
  }

  // tile DMA: search_kernel's padded layout (piece p = rows p and 32 + p + 16 B)
  const unsigned lds_base = lds_addr(smem);
  auto issue_tile = [&](int64_t t, int buf) {
    const int nrem = (int)((n - t * TG) < TG ? (n - t * TG) : TG);
    const unsigned m0 = lds_base + (unsigned)(buf * TGS * 4);
    unsigned lid;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lid));
    if (nrem == TG) {
      const unsigned long long gb = uniform_ptr(G3 + t * TG * KP);
      if (wave == 0) glds4s(lid * 4u, uniform_ptr(aux + t * TG), lds_base + (unsigned)((2 * TGS + buf * TG) * 4));
      const unsigned voff = ((lid >> 5) * 32 * KP + (lid & 31) * 4) * 4;
#pragma unroll
      for (int jj = 0; jj < PPW; ++jj) {
        const int p = wave * PPW + jj;
        // rows 4..11 of every 16 land with their 128-B quarter pairs swapped (see abase)
        glds16s(((p >> 2) & 3) - 1u < 2u ? voff ^ 128u : voff, gb + (unsigned long long)(p * KP * 4),
                m0 + (unsigned)(p * PS * 4));
      }
    } else {
      const float* gbase = G3 + t * TG * KP;
#pragma unroll
      for (int jj = 0; jj < PPW; ++jj) {
        const int p = wave * PPW + jj;
        int row = p + (int)(lid >> 5) * 32;
        row = row < nrem ? row : nrem - 1;
        glds16(gbase + row * KP + ((lid & 31) ^ (((p >> 2) & 3) - 1u < 2u ? 8u : 0u)) * 4, m0 + (unsigned)(p * PS * 4));
      }
      if (wave == 0) {
        const int row = (int)lid < nrem ? (int)lid : nrem - 1;
        glds4(aux + t * TG + row, lds_base + (unsigned)((2 * TGS + buf * TG) * 4));
      }
    }
  };
  issue_tile(t0, 0);

  // probes: lane's k-quarter of probes 16 pb + r16, pre-scaled like search_kernel
  constexpr float QS = METRIC == EF_METRIC_L2 ? -2.f : -1.f;
  bf16x8 qh[2][4], ql[2][4];
  float thr[2] = {-__builtin_inff(), -__builtin_inff()};
#pragma unroll
  for (int pb = 0; pb < 2; ++pb) {
    int64_t r0 = sl0[pb];
    bool v0 = true;
    if constexpr (COLLECT) {
      v0 = sl0[pb] < n_amb;
      r0 = v0 ? ws.amb_list[sl0[pb]] : 0;
      if (v0) thr[pb] = ws.thr[sl0[pb]];
    }
    const float4* q0 = reinterpret_cast<const float4*>(qpad + r0 * KP + qd * 32);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float4 a = v0 ? q0[2 * i] : make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 b = v0 ? q0[2 * i + 1] : make_float4(0.f, 0.f, 0.f, 0.f);
      const float t[8] = {QS * a.x, QS * a.y, QS * a.z, QS * a.w, QS * b.x, QS * b.y, QS * b.z, QS * b.w};
      split8(t, qh[pb][i], ql[pb][i]);
    }
  }
#pragma unroll
  for (int pb = 0; pb < 2; ++pb)
#pragma unroll
    for (int i = 0; i < 4; ++i) asm volatile("" ::"v"(qh[pb][i]), "v"(ql[pb][i]));
  asm volatile("" ::"v"(thr[0]), "v"(thr[1]));

  const float INF = __builtin_inff();
  float b1[2] = {INF, INF}, b2[2] = {INF, INF};
  int i1[2] = {INT_MAX, INT_MAX};
  // v[rb] = rows 16 rb + 4 qd + reg of probe block pb (increasing with (rb, reg))
  auto consume = [&](const f32x4 (&v)[4], int tbase, int pb) {
    if constexpr (COLLECT) {
#pragma unroll
      for (int rb = 0; rb < 4; ++rb)
#pragma unroll
        for (int r = 0; r < 4; ++r) collect_hit(ws, sl0[pb], thr[pb], v[rb][r], tbase, 16 * rb + 4 * qd + r);
    } else {
      float mn = v[0][0];
#pragma unroll
      for (int rb = 0; rb < 4; ++rb)
#pragma unroll
        for (int r = 0; r < 4; ++r) mn = fminf(mn, v[rb][r]);
      if (!__any(mn < b2[pb])) return;  // exact skip (search_kernel consume)
      float m1 = INF, m2 = INF;
      int ir = 0;
#pragma unroll
      for (int rb = 0; rb < 4; ++rb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float x = v[rb][r];
          const bool lt = x < m1;
          m2 = __builtin_amdgcn_fmed3f(m1, x, m2);
          ir = lt ? 16 * rb + r : ir;
          m1 = lt ? x : m1;
        }
      const bool lt = m1 < b1[pb];
      b2[pb] = lt ? fminf(b1[pb], m2) : fminf(b2[pb], m1);
      i1[pb] = lt ? tbase + ir + 4 * qd : i1[pb];
      b1[pb] = lt ? m1 : b1[pb];
    }
  };

  dma_wait_all();
  __syncthreads();
  // lane's A base: row r16 of block rb lives in piece 16 (rb & 1) + r16, half rb >> 1.
  // ds_read_b128 serves lanes {0-3,12-15,20-27}, {4-11,16-19,28-31}, ... together
  // (MI355X_MICROARCH.md §LDS): quarters qd and qd + 1 of rows 4..11 vs 0-3 / 12-15 would
  // share banks on the 1040-B piece stride, so those rows hold their 128-B quarter pairs
  // swapped (chunk ^ 8, applied by the DMA) — every lane group then covers all 64 banks.
  const int qsw = ((r16 >> 2) - 1u) < 2u ? 8 : 0;
  const int abase = r16 * PS + ((8 * qd) ^ qsw) * 4;  // floats, + 16 PS (rb & 1) + KP (rb >> 1) + 8 i
  for (int64_t t = t0; t < t1; ++t) {
    const int buf = (int)((t - t0) & 1);
    if (t + 1 < t1) issue_tile(t + 1, buf ^ 1);
    const float* tileG = smem + buf * TGS + abase;
    const float* tileA = sAux0 + buf * TG;
    f32x4 acc[4][2];
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
      if constexpr (METRIC == EF_METRIC_L2) {
        const float4 x = *reinterpret_cast<const float4*>(tileA + 16 * rb + 4 * qd);
        a = f32x4{x.x, x.y, x.z, x.w};
      }
      acc[rb][0] = a;
      acc[rb][1] = a;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int rb = 0; rb < 4; ++rb) {
        const float* ar = tileG + 16 * PS * (rb & 1) + KP * (rb >> 1) + 8 * i;
        const bf16x8 ah = as_bf16x8(*reinterpret_cast<const float4*>(ar));
        const bf16x8 al = as_bf16x8(*reinterpret_cast<const float4*>(ar + 4));
#pragma unroll
        for (int pb = 0; pb < 2; ++pb) {
          acc[rb][pb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, qh[pb][i], acc[rb][pb], 0, 0, 0);
          acc[rb][pb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, ql[pb][i], acc[rb][pb], 0, 0, 0);
          acc[rb][pb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, qh[pb][i], acc[rb][pb], 0, 0, 0);
        }
      }
      if (i % 2 == 1) __builtin_amdgcn_sched_barrier(0);
    }
    const int tbase = (int)(t * TG);
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
      if constexpr (METRIC != EF_METRIC_L2) {  // cosine: -(q.g) * (1/||g||)
        const float4 x = *reinterpret_cast<const float4*>(tileA + 16 * rb + 4 * qd);
#pragma unroll
        for (int pb = 0; pb < 2; ++pb) {
          acc[rb][pb][0] *= x.x; acc[rb][pb][1] *= x.y; acc[rb][pb][2] *= x.z; acc[rb][pb][3] *= x.w;
        }
      }
      if ((t + 1) * TG > n) {  // uniform: only the last tile has rows past n
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (tbase + 16 * rb + 4 * qd + r >= n) {
            acc[rb][0][r] = INF;
            acc[rb][1][r] = INF;
          }
      }
    }
#pragma unroll
    for (int pb = 0; pb < 2; ++pb) {
      const f32x4 v[4] = {acc[0][pb], acc[1][pb], acc[2][pb], acc[3][pb]};
      consume(v, tbase, pb);
    }
    dma_wait_all();
    __syncthreads();
  }

  if constexpr (!COLLECT) {
#pragma unroll
    for (int pb = 0; pb < 2; ++pb) {
#pragma unroll
      for (int off = 16; off <= 32; off <<= 1) {  // merge the four row quarters
        const float ob1 = __shfl_xor(b1[pb], off);
        const int oi1 = __shfl_xor(i1[pb], off);
        const float ob2 = __shfl_xor(b2[pb], off);
        top2_merge(b1[pb], b2[pb], i1[pb], ob1, ob2, oi1);
      }
      if (qd == 0) top2_store(ws, (int64_t)gc * bpad, sl0[pb], b1[pb], b2[pb], i1[pb]);
    }
  }
  };  // body
  if constexpr (COLLECT) {
    collect_items<kSearchProbeTile>(ws, n_ptiles, body);  // n_ptiles carries the collect plan's chunk count
  } else {
    const int lin = xcd_lin();
    const int gc = lin / n_ptiles;
    body(gc, lin - gc * n_ptiles, 0);
  }
}

// Split-bf16 prefix scan at K1 <= 32 (L2, main pass only; launch_search_prefix).
// At these shapes the matrix work per row is so short that the LDS reads and the arg-best
// epilogue weigh as much as the MFMAs (profiles/r11, r14), so this kernel spends less on both:
//   * workgroup = 8 waves x 32 PB probes, PB = 2 (kPrefixSplitProbes = 512): each wave keeps PB
//     32-probe B blocks (pb; K1 VGPRs of hi / lo fragments for the two) and runs every A
//     fragment it reads against each, so the tile's 32-row blocks go RB = 4 / PB at a time (rb)
//     as RB x PB = 4 accumulator chains — half the LDS reads, tile DMAs, barriers and gallery
//     sweeps per MFMA.  PB = 1 (search_kernel's shape) compiles too and measured slower;
//   * the epilogue merges only the accumulator registers that can change a record (consume);
//   * the staged norms of a row block are read once and start both probe blocks' chains;
//   * rows of K1 floats lie in LDS with chunk c of row r at chunk c ^ ((r >> SS) & (CPR - 1)),
//     SS = 1 at K1 = 32 (128-byte rows: two rows span the 64 banks), 2 at K1 = 16 (four rows).
//     ds_read_b128 is served in the lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} (and
//     + 32; MI355X LDS): in either group the rows that share a bank range (equal row & 1, or
//     row & 3) have distinct (r >> SS) & (CPR - 1), so a group covers 64 distinct banks.  Rows
//     c32 and 32 bi + c32 share a swizzle;
//   * the probes are read from qpad itself (row stride KP), once per workgroup: no prefix copy.
// The arithmetic of every (probe, row) score is search_kernel<K1, L2, false, true>'s: the same
// MFMA, the chain started from the row's fp32 norm, fragments in ascending k, per fragment
// hi.hi', hi.lo', lo.hi', the same k split over the lane halves — part_key / part_b2 hold the
// same values, and each probe block consumes its row blocks in row order (the tie rule).
// 123 VGPRs, no scratch, 66 KiB of LDS at K1 = 32: two workgroups per CU, as search_kernel.
// bpad is a multiple of 256 only: the upper four waves of the last workgroup may own no probe
// (live = false).  They read no probe, run the sweep on zeros (they issue tile DMAs and take
// part in the barriers like the others) and store nothing.
template <int KP, int K1, int PB>
__global__ __launch_bounds__(512, 4) void prefix64_kernel(
    const float* __restrict__ qpad, const float* __restrict__ G1, const float* __restrict__ gnorm1, int64_t n,
    int n_ptiles, int tiles_per_chunk, int64_t bpad, SearchWs ws) {
  static_assert((K1 == 16 || K1 == 32) && K1 < KP, "the prefix lengths that take 256-row tiles");
  constexpr int NW = 8, TGT = kPrefixSplitTile;
  constexpr int RB = 4 / PB;  // row blocks run at once: RB x PB = 4 accumulator chains
  constexpr int KH = K1 / 2, NF = KH / 8;  // k per lane half, 8-element fragments of it
  constexpr int CPR = K1 / 4;              // 16-B chunks per row
  constexpr int SS = K1 == 32 ? 1 : 2;     // swizzle: chunk ^ ((row >> SS) & (CPR - 1))
  constexpr int RP = 64 / CPR;             // rows per 1-KiB DMA piece
  constexpr int NI = TGT / RP, PPW = NI / NW;
  constexpr int TGS = TGT * K1;            // floats per tile buffer
  static_assert(PPW * NW == NI && RP % (1 << SS) == 0, "whole pieces per wave, swizzle splits per piece");
  __shared__ __attribute__((aligned(16))) float smem[2 * TGS + 2 * TGT];
  float* const sAux0 = smem + 2 * TGS;

  const int lin = xcd_lin();  // the probe tiles of one chunk co-resident on an XCD
  const int gc = lin / n_ptiles, pt = lin - gc * n_ptiles;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // The lane id is re-derived where it is needed (two VALU instructions) instead of living in
  // VGPRs through the sweep with what is computed from it: 64 accumulators, 32 probe registers
  // and 16 of A fragments leave 16 for everything else
  auto lane_id = [] {
    unsigned l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return (int)l;
  };

  int64_t t0, t1;
  chunk_range<TGT>(n, gc, tiles_per_chunk, t0, t1);
  // this lane's probe slots: block 0 at s0, block 1 at s0 + 32; a wave's 64 slots lie on one
  // side of bpad (a multiple of 256)
  const int64_t w0 = (int64_t)pt * (NW * 32 * PB) + wave * (32 * PB);
  const bool live = w0 < bpad;  // wave-uniform

  if (t0 >= t1) {  // empty chunk: publish "no candidate" so the reducer can skip it
    const int lane = lane_id();
    const int64_t s0 = w0 + lane;
    if (live && lane < 32) {
#pragma unroll
      for (int pb = 0; pb < PB; ++pb) top2_store_empty(ws, (int64_t)gc * bpad, s0 + 32 * pb);
    }
    return;
  }

  // LDS-DMA of tile t into buffer buf: wave w fills pieces [w PPW, (w + 1) PPW), a piece is RP
  // whole rows, lane-linear.  The swizzle is applied on the source address and splits into a
  // lane constant and a wave-uniform part: ((j RP + lrow) >> SS) = (j RP >> SS) + (lrow >> SS),
  // a sum without carries.  Rows past n (tail tile) re-read the last row, masked below.
  const unsigned lds_base = lds_addr(smem);
  auto issue_tile = [&](int64_t t, int buf) {
    const int nrem = (int)((n - t * TGT) < TGT ? (n - t * TGT) : TGT);
    const int lane = lane_id();
    const int lr = lane / CPR;                                // this lane's (row, chunk) inside a piece
    const int lx = (lane % CPR) ^ ((lr >> SS) & (CPR - 1));  // chunk, with the lane's swizzle part
    if (nrem == TGT) {
      const unsigned long long gb = uniform_ptr(G1 + t * TGT * K1);
      const unsigned lro = (unsigned)(lr * K1 * 4);
#pragma unroll
      for (int jj = 0; jj < PPW; ++jj) {
        const int j = wave * PPW + jj;
        const int sj = ((j * RP) >> SS) & (CPR - 1);
        glds16s(lro + ((unsigned)(lx ^ sj) << 4), gb + (unsigned long long)(j * RP * K1 * 4),
                lds_base + (unsigned)((buf * TGS + j * 256) * 4));
      }
      if (wave < TGT / 64)  // one 64-row piece of the norms per wave
        glds4s((unsigned)lane * 4u, uniform_ptr(gnorm1 + t * TGT + wave * 64),
               lds_base + (unsigned)((2 * TGS + buf * TGT + wave * 64) * 4));
    } else {
      const float* gbase = G1 + t * TGT * K1;  // wave-uniform
#pragma unroll
      for (int jj = 0; jj < PPW; ++jj) {
        const int j = wave * PPW + jj;
        const int sj = ((j * RP) >> SS) & (CPR - 1);
        int row = j * RP + lr;
        row = row < nrem ? row : nrem - 1;
        glds16(gbase + row * K1 + ((lx ^ sj) << 2), lds_base + (unsigned)((buf * TGS + j * 256) * 4));
      }
      if (wave < TGT / 64) {
        const int row = wave * 64 + lane < nrem ? wave * 64 + lane : nrem - 1;
        glds4(gnorm1 + t * TGT + row, lds_base + (unsigned)((2 * TGS + buf * TGT + wave * 64) * 4));
      }
    }
  };

  issue_tile(t0, 0);

  // Probe fragments (B operands): lane holds probes c32 and 32 + c32 of the wave, k in
  // [h KH, h KH + KH) of the row's first K1 columns, scaled by -2 (exact) and split, so that a
  // chain started from ||g||^2 ends at the L2 prefix score
  bf16x8 qh[PB][NF], ql[PB][NF];
#pragma unroll
  for (int pb = 0; pb < PB; ++pb) {
    const int lane = lane_id();
    const float4* q0 =
        reinterpret_cast<const float4*>(qpad + (live ? w0 + (lane & 31) + 32 * pb : 0) * KP + (lane >> 5) * KH);
#pragma unroll
    for (int i = 0; i < NF; ++i) {
      const float4 a = live ? q0[2 * i] : make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 b = live ? q0[2 * i + 1] : make_float4(0.f, 0.f, 0.f, 0.f);
      const float t[8] = {-2.f * a.x, -2.f * a.y, -2.f * a.z, -2.f * a.w, -2.f * b.x, -2.f * b.y, -2.f * b.z, -2.f * b.w};
      split8(t, qh[pb][i], ql[pb][i]);
    }
  }
  // consumed here so that the waits for these loads stand before the loop (search_kernel)
#pragma unroll
  for (int pb = 0; pb < PB; ++pb)
#pragma unroll
    for (int i = 0; i < NF; ++i) asm volatile("" ::"v"(qh[pb][i]), "v"(ql[pb][i]));

  const float INF = __builtin_inff();
  float b1[PB], b2[PB];
  int i1[PB];
#pragma unroll
  for (int pb = 0; pb < PB; ++pb) b1[pb] = b2[pb] = INF, i1[pb] = INT_MAX;

  // Arg-best epilogue of one finished block of scores v (register r <-> row rowbase + (r & 3) +
  // 8 (r >> 2) + 4 h, increasing with r), merged into probe block pb's running record.  The
  // screen is search_kernel's: a block whose minimum is not below the lane's runner-up changes
  // nothing, and when that holds for every lane the block is skipped on a uniform branch.  A
  // block that passes is walked in row order, and only the registers in which some lane has a
  // score below its runner-up are merged (a uniform branch each; a score that is not below b2
  // leaves b1, b2 and i1 as they are): with b1 <= b2 the new runner-up is the median of (b1,
  // score, b2), and strict '<' keeps the lowest row on ties.  The chunk sweeps are short enough
  // that about half the blocks pass the screen for one or two lanes, and search_kernel's
  // branch-free top-2 of all 16 registers (64 VALU instructions) was most of this scan's
  // non-MFMA work.  The record is the same: minimum, its first row, second smallest of the
  // multiset.
  auto consume = [&](const f32x16& v, int rowbase, int pb, int h) {
    float mn = v[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mn = fminf(mn, v[r]);
    if (!__any(mn < b2[pb])) return;  // exact skip: the block changes nothing
    const int row0 = rowbase + 4 * h;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      // expected not taken: the merges then lie out of line and a walk falls through 16 compares
      if (__builtin_expect(!__any(v[r] < b2[pb]), 1)) continue;
      const bool lt = v[r] < b1[pb];
      b2[pb] = __builtin_amdgcn_fmed3f(b1[pb], v[r], b2[pb]);
      i1[pb] = lt ? row0 + (r & 3) + 8 * (r >> 2) : i1[pb];
      b1[pb] = lt ? v[r] : b1[pb];
    }
  };

  dma_wait_all();
  __syncthreads();  // tile t0 landed

  for (int64_t t = t0; t < t1; ++t) {
    const int buf = (int)((t - t0) & 1);
    if (t + 1 < t1) issue_tile(t + 1, buf ^ 1);  // lands under this tile's MFMAs
    const float* tileA = sAux0 + buf * TGT;
    const bool tail = (t + 1) * TGT > n;
    const int tbase = (int)(t * TGT);
    const int lane = lane_id();
    const int h = lane >> 5, c32 = lane & 31;
    const int swz = (c32 >> SS) & (CPR - 1);  // rows c32 and 32 bi + c32 share it
    const float* arow = smem + buf * TGS + c32 * K1;
#pragma unroll
    for (int g0 = 0; g0 < TGT / 32; g0 += RB) {  // row blocks g0 .. g0 + RB - 1 against every probe block
      f32x16 acc[RB][PB];
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) {
        f32x16 a;  // ||g||^2 of the block's rows, in the register <-> row map
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 x = *reinterpret_cast<const float4*>(tileA + 32 * (g0 + rb) + 8 * q + 4 * h);
          a[4 * q] = x.x;
          a[4 * q + 1] = x.y;
          a[4 * q + 2] = x.z;
          a[4 * q + 3] = x.w;
        }
#pragma unroll
        for (int pb = 0; pb < PB; ++pb) acc[rb][pb] = a;
      }
      // fragment i: chunks 2i (hi) and 2i + 1 (lo) of this lane half's k range
#pragma unroll
      for (int i = 0; i < NF; ++i) {
        const int c0 = h * (CPR / 2) + 2 * i;
        const int ch = c0 ^ swz, cl = (c0 + 1) ^ swz;
        bf16x8 ah[RB], al[RB];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
          ah[rb] = as_bf16x8(*reinterpret_cast<const float4*>(arow + (g0 + rb) * 32 * K1 + ch * 4));
          al[rb] = as_bf16x8(*reinterpret_cast<const float4*>(arow + (g0 + rb) * 32 * K1 + cl * 4));
        }
#pragma unroll
        for (int c = 0; c < 4; ++c)
          acc[c / PB][c % PB] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[c / PB], qh[c % PB][i], acc[c / PB][c % PB], 0, 0, 0);
#pragma unroll
        for (int c = 0; c < 4; ++c)
          acc[c / PB][c % PB] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[c / PB], ql[c % PB][i], acc[c / PB][c % PB], 0, 0, 0);
#pragma unroll
        for (int c = 0; c < 4; ++c)
          acc[c / PB][c % PB] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[c / PB], qh[c % PB][i], acc[c / PB][c % PB], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);  // bound the A prefetch depth
      }
      if (tail) {  // uniform: only the last tile has rows past n
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (tbase + 32 * (g0 + rb) + (r & 3) + 8 * (r >> 2) + 4 * h >= n) {
#pragma unroll
              for (int pb = 0; pb < PB; ++pb) acc[rb][pb][r] = INF;
            }
      }
#pragma unroll
      for (int pb = 0; pb < PB; ++pb)
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) consume(acc[rb][pb], tbase + 32 * (g0 + rb), pb, h);  // in row order (tie rule)
    }
    dma_wait_all();
    __syncthreads();  // tile t+1 landed; everyone is done reading buffer buf
  }

#pragma unroll
  for (int pb = 0; pb < PB; ++pb) {  // merge the two lane halves (same probe, disjoint rows)
    const float ob1 = __shfl_xor(b1[pb], 32);
    const int oi1 = __shfl_xor(i1[pb], 32);
    const float ob2 = __shfl_xor(b2[pb], 32);
    top2_merge(b1[pb], b2[pb], i1[pb], ob1, ob2, oi1);
    const int lane = lane_id();
    if (live && lane < 32) top2_store(ws, (int64_t)gc * bpad, w0 + lane + 32 * pb, b1[pb], b2[pb], i1[pb]);
  }
}

// The cascade's other two forms of the scan (EF_OPT_SEARCH_PREFIX_SCREEN; search_prefix_t), one
// kernel template of their own: prefix64_kernel above stays as it is, text and name, for the
// launch sequence of option 0.  What differs from it is marked HI1 / CNT; the rest is its code
// with the row length in LDS (RF floats) in place of K1.
//
// Screen (HI1, not CNT): one product per fragment, hi(g).hi(-2 q), over the single-bf16 copy of
// the prefix (G1 = G1h: n rows of K1 bf16 values, round to nearest even as bf16_bits; 64- or
// 32-byte rows, so four or eight rows span the 64 banks: SS = 2 or 3, and the lane groups of
// ds_read_b128 again meet each bank range in distinct (r >> SS) & (CPR - 1)).  A chain starts from
// the row's value of gnorm1 = gstart, a rounded-down ||g[:K1]||^2 (1 - es - cg) (prefix_hi_kernel),
// and so ends at a lower bound L(g) of the row's prefix score plus the probe's share of the bound
// (reduce_prefix_x_kernel, S3 = 2).  Rows are ranked by L: the record is (min L, its first row, second
// smallest L).  Half the tile bytes, DMAs and A reads of the split form, a third of its MFMAs;
// 108 VGPRs at K1 = 32, 96 at 16, no scratch.
//
// Split scan of the listed probes (CNT, not HI1): prefix64_kernel's arithmetic for the probes
// list[0 .. cnt), cnt = ws.amb_count[kScreenCount] on the device, read from qpad through the
// list; slot s of the records belongs to probe list[s].  The grid is sized for bpad; a workgroup
// whose probe tile starts at or past cnt returns at once.
template <int KP, int K1, int PB, bool HI1, bool CNT>
__global__ __launch_bounds__(512, 4) void prefix64x_kernel(
    const float* __restrict__ qpad, const float* __restrict__ G1, const float* __restrict__ gnorm1, int64_t n,
    int n_ptiles, int tiles_per_chunk, int64_t bpad, SearchWs ws, const int* __restrict__ list) {
  static_assert((K1 == 16 || K1 == 32) && K1 < KP, "the prefix lengths that take 256-row tiles");
  constexpr int NW = 8, TGT = kPrefixSplitTile;
  constexpr int RB = 4 / PB;  // row blocks run at once: RB x PB = 4 accumulator chains
  constexpr int KH = K1 / 2, NF = KH / 8;  // k per lane half, 8-element fragments of it
  constexpr int CPR = HI1 ? K1 / 8 : K1 / 4;  // 16-B chunks per row (HI1: K1 bf16 values)
  constexpr int RF = CPR * 4;                 // a row's length in floats
  constexpr int SS = CPR == 8 ? 1 : CPR == 4 ? 2 : 3;  // swizzle: chunk ^ ((row >> SS) & (CPR - 1))
  constexpr int RP = 64 / CPR;             // rows per 1-KiB DMA piece
  constexpr int NI = TGT / RP, PPW = NI / NW;
  constexpr int TGS = TGT * RF;            // floats per tile buffer
  static_assert(PPW * NW == NI && RP % (1 << SS) == 0, "whole pieces per wave, swizzle splits per piece");
  __shared__ __attribute__((aligned(16))) float smem[2 * TGS + 2 * TGT];
  float* const sAux0 = smem + 2 * TGS;

  const int lin = xcd_lin();  // the probe tiles of one chunk co-resident on an XCD
  const int gc = lin / n_ptiles, pt = lin - gc * n_ptiles;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // The lane id is re-derived where it is needed (two VALU instructions) instead of living in
  // VGPRs through the sweep with what is computed from it: 64 accumulators, 32 probe registers
  // and 16 of A fragments leave 16 for everything else
  auto lane_id = [] {
    unsigned l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return (int)l;
  };

  int64_t t0, t1;
  chunk_range<TGT>(n, gc, tiles_per_chunk, t0, t1);
  // this lane's probe slots: block 0 at s0, block 1 at s0 + 32; a wave's 64 slots lie on one
  // side of bpad (a multiple of 256)
  const int64_t w0 = (int64_t)pt * (NW * 32 * PB) + wave * (32 * PB);
  // CNT: slot s holds probe list[s] for s < cnt, the device count; workgroups and waves wholly
  // past it have nothing to do, and the slots past it inside a live wave are swept as zeros
  int cnt = 0;
  if constexpr (CNT) {
    cnt = ws.amb_count[kScreenCount];
    if ((int64_t)pt * (NW * 32 * PB) >= cnt) return;
  }
  const bool live = CNT ? w0 < cnt : w0 < bpad;  // wave-uniform

  if (t0 >= t1) {  // empty chunk: publish "no candidate" so the reducer can skip it
    const int lane = lane_id();
    const int64_t s0 = w0 + lane;
    if (live && lane < 32) {
#pragma unroll
      for (int pb = 0; pb < PB; ++pb) top2_store_empty(ws, (int64_t)gc * bpad, s0 + 32 * pb);
    }
    return;
  }

  // LDS-DMA of tile t into buffer buf: wave w fills pieces [w PPW, (w + 1) PPW), a piece is RP
  // whole rows, lane-linear.  The swizzle is applied on the source address and splits into a
  // lane constant and a wave-uniform part: ((j RP + lrow) >> SS) = (j RP >> SS) + (lrow >> SS),
  // a sum without carries.  Rows past n (tail tile) re-read the last row, masked below.
  const unsigned lds_base = lds_addr(smem);
  auto issue_tile = [&](int64_t t, int buf) {
    const int nrem = (int)((n - t * TGT) < TGT ? (n - t * TGT) : TGT);
    const int lane = lane_id();
    const int lr = lane / CPR;                                // this lane's (row, chunk) inside a piece
    const int lx = (lane % CPR) ^ ((lr >> SS) & (CPR - 1));  // chunk, with the lane's swizzle part
    if (nrem == TGT) {
      const unsigned long long gb = uniform_ptr(G1 + t * TGT * RF);
      const unsigned lro = (unsigned)(lr * RF * 4);
#pragma unroll
      for (int jj = 0; jj < PPW; ++jj) {
        const int j = wave * PPW + jj;
        const int sj = ((j * RP) >> SS) & (CPR - 1);
        glds16s(lro + ((unsigned)(lx ^ sj) << 4), gb + (unsigned long long)(j * RP * RF * 4),
                lds_base + (unsigned)((buf * TGS + j * 256) * 4));
      }
      if (wave < TGT / 64)  // one 64-row piece of the norms per wave
        glds4s((unsigned)lane * 4u, uniform_ptr(gnorm1 + t * TGT + wave * 64),
               lds_base + (unsigned)((2 * TGS + buf * TGT + wave * 64) * 4));
    } else {
      const float* gbase = G1 + t * TGT * RF;  // wave-uniform
#pragma unroll
      for (int jj = 0; jj < PPW; ++jj) {
        const int j = wave * PPW + jj;
        const int sj = ((j * RP) >> SS) & (CPR - 1);
        int row = j * RP + lr;
        row = row < nrem ? row : nrem - 1;
        glds16(gbase + row * RF + ((lx ^ sj) << 2), lds_base + (unsigned)((buf * TGS + j * 256) * 4));
      }
      if (wave < TGT / 64) {
        const int row = wave * 64 + lane < nrem ? wave * 64 + lane : nrem - 1;
        glds4(gnorm1 + t * TGT + row, lds_base + (unsigned)((2 * TGS + buf * TGT + wave * 64) * 4));
      }
    }
  };

  issue_tile(t0, 0);

  // Probe fragments (B operands): lane holds probes c32 and 32 + c32 of the wave, k in
  // [h KH, h KH + KH) of the row's first K1 columns, scaled by -2 (exact) and split, so that a
  // chain started from ||g||^2 ends at the L2 prefix score
  bf16x8 qh[PB][NF], ql[PB][HI1 ? 1 : NF];  // HI1: the hi fragments alone
#pragma unroll
  for (int pb = 0; pb < PB; ++pb) {
    const int lane = lane_id();
    bool have = live;
    const float4* q0;
    if constexpr (CNT) {
      const int64_t slot = w0 + (lane & 31) + 32 * pb;
      have = live && slot < cnt;
      q0 = reinterpret_cast<const float4*>(qpad + (int64_t)(have ? list[slot] : 0) * KP + (lane >> 5) * KH);
    } else {
      q0 = reinterpret_cast<const float4*>(qpad + (live ? w0 + (lane & 31) + 32 * pb : 0) * KP + (lane >> 5) * KH);
    }
#pragma unroll
    for (int i = 0; i < NF; ++i) {
      const float4 a = have ? q0[2 * i] : make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 b = have ? q0[2 * i + 1] : make_float4(0.f, 0.f, 0.f, 0.f);
      const float t[8] = {-2.f * a.x, -2.f * a.y, -2.f * a.z, -2.f * a.w, -2.f * b.x, -2.f * b.y, -2.f * b.z, -2.f * b.w};
      if constexpr (HI1) {
#pragma unroll
        for (int j = 0; j < 8; ++j) qh[pb][i][j] = (short)bf16_bits(t[j]);
      } else {
        split8(t, qh[pb][i], ql[pb][i]);
      }
    }
  }
  // consumed here so that the waits for these loads stand before the loop (search_kernel)
#pragma unroll
  for (int pb = 0; pb < PB; ++pb)
#pragma unroll
    for (int i = 0; i < NF; ++i) {
      if constexpr (HI1) asm volatile("" ::"v"(qh[pb][i]));
      else asm volatile("" ::"v"(qh[pb][i]), "v"(ql[pb][i]));
    }

  const float INF = __builtin_inff();
  float b1[PB], b2[PB];
  int i1[PB];
#pragma unroll
  for (int pb = 0; pb < PB; ++pb) b1[pb] = b2[pb] = INF, i1[pb] = INT_MAX;

  // Arg-best epilogue of one finished block of scores v (register r <-> row rowbase + (r & 3) +
  // 8 (r >> 2) + 4 h, increasing with r), merged into probe block pb's running record.  The
  // screen is search_kernel's: a block whose minimum is not below the lane's runner-up changes
  // nothing, and when that holds for every lane the block is skipped on a uniform branch.  A
  // block that passes is walked in row order, and only the registers in which some lane has a
  // score below its runner-up are merged (a uniform branch each; a score that is not below b2
  // leaves b1, b2 and i1 as they are): with b1 <= b2 the new runner-up is the median of (b1,
  // score, b2), and strict '<' keeps the lowest row on ties.  The chunk sweeps are short enough
  // that about half the blocks pass the screen for one or two lanes, and search_kernel's
  // branch-free top-2 of all 16 registers (64 VALU instructions) was most of this scan's
  // non-MFMA work.  The record is the same: minimum, its first row, second smallest of the
  // multiset.
  auto consume = [&](const f32x16& v, int rowbase, int pb, int h) {
    float mn = v[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mn = fminf(mn, v[r]);
    if (!__any(mn < b2[pb])) return;  // exact skip: the block changes nothing
    const int row0 = rowbase + 4 * h;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      // expected not taken: the merges then lie out of line and a walk falls through 16 compares
      if (__builtin_expect(!__any(v[r] < b2[pb]), 1)) continue;
      const bool lt = v[r] < b1[pb];
      b2[pb] = __builtin_amdgcn_fmed3f(b1[pb], v[r], b2[pb]);
      i1[pb] = lt ? row0 + (r & 3) + 8 * (r >> 2) : i1[pb];
      b1[pb] = lt ? v[r] : b1[pb];
    }
  };

  dma_wait_all();
  __syncthreads();  // tile t0 landed

  for (int64_t t = t0; t < t1; ++t) {
    const int buf = (int)((t - t0) & 1);
    if (t + 1 < t1) issue_tile(t + 1, buf ^ 1);  // lands under this tile's MFMAs
    const float* tileA = sAux0 + buf * TGT;
    const bool tail = (t + 1) * TGT > n;
    const int tbase = (int)(t * TGT);
    const int lane = lane_id();
    const int h = lane >> 5, c32 = lane & 31;
    const int swz = (c32 >> SS) & (CPR - 1);  // rows c32 and 32 bi + c32 share it
    const float* arow = smem + buf * TGS + c32 * RF;
#pragma unroll
    for (int g0 = 0; g0 < TGT / 32; g0 += RB) {  // row blocks g0 .. g0 + RB - 1 against every probe block
      f32x16 acc[RB][PB];
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) {
        f32x16 a;  // ||g||^2 of the block's rows, in the register <-> row map
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 x = *reinterpret_cast<const float4*>(tileA + 32 * (g0 + rb) + 8 * q + 4 * h);
          a[4 * q] = x.x;
          a[4 * q + 1] = x.y;
          a[4 * q + 2] = x.z;
          a[4 * q + 3] = x.w;
        }
#pragma unroll
        for (int pb = 0; pb < PB; ++pb) acc[rb][pb] = a;
      }
      if constexpr (HI1) {
        // one product per fragment: chunk i of this lane half's k range, every fragment of the
        // group read ahead of its MFMAs (8 NF registers where the split form holds 16)
        bf16x8 a1[RB][NF];
#pragma unroll
        for (int i = 0; i < NF; ++i)
#pragma unroll
          for (int rb = 0; rb < RB; ++rb)
            a1[rb][i] = as_bf16x8(*reinterpret_cast<const float4*>(arow + (g0 + rb) * 32 * RF + ((h * (CPR / 2) + i) ^ swz) * 4));
#pragma unroll
        for (int i = 0; i < NF; ++i)
#pragma unroll
          for (int c = 0; c < 4; ++c)
            acc[c / PB][c % PB] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1[c / PB][i], qh[c % PB][i], acc[c / PB][c % PB], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      // fragment i: chunks 2i (hi) and 2i + 1 (lo) of this lane half's k range
#pragma unroll
      for (int i = 0; i < (HI1 ? 0 : NF); ++i) {
        const int c0 = h * (CPR / 2) + 2 * i;
        const int ch = c0 ^ swz, cl = (c0 + 1) ^ swz;
        bf16x8 ah[RB], al[RB];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
          ah[rb] = as_bf16x8(*reinterpret_cast<const float4*>(arow + (g0 + rb) * 32 * RF + ch * 4));
          al[rb] = as_bf16x8(*reinterpret_cast<const float4*>(arow + (g0 + rb) * 32 * RF + cl * 4));
        }
#pragma unroll
        for (int c = 0; c < 4; ++c)
          acc[c / PB][c % PB] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[c / PB], qh[c % PB][i], acc[c / PB][c % PB], 0, 0, 0);
#pragma unroll
        for (int c = 0; c < 4; ++c)
          acc[c / PB][c % PB] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[c / PB], ql[c % PB][i], acc[c / PB][c % PB], 0, 0, 0);
#pragma unroll
        for (int c = 0; c < 4; ++c)
          acc[c / PB][c % PB] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[c / PB], qh[c % PB][i], acc[c / PB][c % PB], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);  // bound the A prefetch depth
      }
      if (tail) {  // uniform: only the last tile has rows past n
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (tbase + 32 * (g0 + rb) + (r & 3) + 8 * (r >> 2) + 4 * h >= n) {
#pragma unroll
              for (int pb = 0; pb < PB; ++pb) acc[rb][pb][r] = INF;
            }
      }
#pragma unroll
      for (int pb = 0; pb < PB; ++pb)
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) consume(acc[rb][pb], tbase + 32 * (g0 + rb), pb, h);  // in row order (tie rule)
    }
    dma_wait_all();
    __syncthreads();  // tile t+1 landed; everyone is done reading buffer buf
  }

#pragma unroll
  for (int pb = 0; pb < PB; ++pb) {  // merge the two lane halves (same probe, disjoint rows)
    const float ob1 = __shfl_xor(b1[pb], 32);
    const int oi1 = __shfl_xor(i1[pb], 32);
    const float ob2 = __shfl_xor(b2[pb], 32);
    top2_merge(b1[pb], b2[pb], i1[pb], ob1, ob2, oi1);
    const int lane = lane_id();
    if (live && lane < 32) top2_store(ws, (int64_t)gc * bpad, w0 + lane + 32 * pb, b1[pb], b2[pb], i1[pb]);
  }
}

// One wave per probe: winner over chunks, global runner-up, fp64 re-score, ambiguity test.
// KP = 0: row length kp_rt at run time (k > 512).
// S3: the scan's arithmetic — 0 fp32, 1 split bf16 (hi + lo), 2 single bf16 (the screen of
// EF_OPT_SEARCH_SPLIT_BF16 = 3) — which sets the bound below.
// CNT: the probe count is on the device (ws.amb_count[1], the prefix path's second run).
template <int KP, int METRIC, int S3 = 0, bool CNT = false>
__global__ __launch_bounds__(256) void reduce_kernel(const float* __restrict__ qpad, int64_t b, int64_t bpad,
                                                     int nchunks, const float* __restrict__ G, int64_t n,
                                                     int64_t g_offset, float gmax2, SearchWs ws,
                                                     long long* __restrict__ keys, int kp_rt) {
  const int kpv = KP > 0 ? KP : kp_rt;
  const int lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= b) return;
  if constexpr (CNT) {
    if (p >= ws.amb_count[1]) return;
  }
  long long kmin = LLONG_MAX;
  for (int c = lane; c < nchunks; c += 64) {
    const long long k = ws.part_key[(int64_t)c * bpad + p];
    kmin = k < kmin ? k : kmin;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const long long o = __shfl_xor(kmin, off);
    kmin = o < kmin ? o : kmin;
  }
  const float* q = qpad + p * kpv;
  // fp32 ||q||^2 for the bound, fp64 for the tie window's scale (resolve_kernel sums it alike)
  float qq = 0.f;
  for (int c = lane; c < kpv; c += 64) qq = __builtin_fmaf(q[c], q[c], qq);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) qq += __shfl_xor(qq, off);
  double qq64 = 0.0;
  for (int c = lane; c < kpv; c += 64) qq64 = fma((double)q[c], (double)q[c], qq64);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) qq64 += __shfl_xor(qq64, off);
  const bool regular = scan_regular<METRIC>(qq, gmax2);  // ef_search_common.hpp
  auto no_key = [&] {  // lane 0
    keys[p] = LLONG_MAX;
    if (ws.match) ws.match[p] = ef_match{__builtin_inf(), 0.0, LLONG_MAX};
  };
  // lane 0: queue the probe for resolve_kernel's fp64 sweep of every row (a count past kCandMax);
  // the NaN threshold keeps the COLLECT pass from counting anything for it
  auto queue_sweep = [&] {
    const int slot = atomicAdd(ws.amb_count, 1);
    ws.amb_list[slot] = (int)p;
    ws.thr[slot] = __builtin_nanf("");
    ws.cand_cnt[slot] = kCandMax + 1;
  };
  // a probe with a NaN or an infinite component (the fp64 sum of finite fp32 squares is finite)
  if (!(qq64 < __builtin_inf())) {
    if (lane == 0) no_key();
    return;
  }
  // outside the bound's domain the scan's scores may be NaN or +-inf: neither its winner nor "no
  // row scored" is believed, and the sweep decides, starting from "no key"
  if (!regular) {
    if (lane == 0) {
      no_key();
      queue_sweep();
    }
    return;
  }
  if (kmin == LLONG_MAX) {  // no row scored: an empty gallery, no qualifying row
    if (lane == 0) no_key();
    return;
  }
  float r2 = __builtin_inff();
  for (int c = lane; c < nchunks; c += 64) {
    const long long k = ws.part_key[(int64_t)c * bpad + p];
    r2 = fminf(r2, ws.part_b2[(int64_t)c * bpad + p]);
    if (k != kmin && k != LLONG_MAX) r2 = fminf(r2, key_value(k));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) r2 = fminf(r2, __shfl_xor(r2, off));

  const float b1 = key_value(kmin);
  const unsigned row = (unsigned)(kmin & 0xffffffffll);
  const double v = score64<KP, METRIC>(q, G + (int64_t)row * kpv, lane, kpv);
  // rigorous bound on |fp32 score - exact score|, doubled for the two compared scores
  const float delta = scan_delta<METRIC, S3>(kpv, sqrtf(qq), gmax2, b1);  // ef_search_common.hpp
  if (lane == 0) {
    keys[p] = pack_key((float)v, (unsigned)(row + g_offset));
    if (ws.match)
      ws.match[p] = ef_match{v, METRIC == EF_METRIC_L2 ? qq64 + (double)gmax2 : 1.0,
                             pack_key((float)v, (unsigned)(row + g_offset))};
    // queued unless proven: a NaN on either side of the comparison leaves the probe unproven
    if (!(r2 - b1 > delta)) {
      if (fabsf(b1) + delta < __builtin_inff()) {
        const int slot = atomicAdd(ws.amb_count, 1);
        ws.amb_list[slot] = (int)p;
        ws.thr[slot] = b1 + delta;
        ws.cand_cnt[slot] = 0;
      } else {  // a threshold that is not finite cannot select candidates
        queue_sweep();
      }
    }
  }
}

// fp64 resolution of queued probes: lowest index among candidates whose fp64 score is
// within 1e-12 (relative) of the best — exact ties resolve like np.argmin/argmax.
// LBL (ef_search_labelled): rows that do not qualify for the probe are passed over.  The
// COLLECT pass queued qualifying rows only; the overflow sweep over all rows needs the rule.
template <int KP, int METRIC, bool LBL = false>
__global__ __launch_bounds__(256) void resolve_kernel(const float* __restrict__ qpad, const float* __restrict__ G,
                                                      int64_t n, int64_t g_offset, float gmax2, SearchWs ws,
                                                      long long* __restrict__ keys, int kp_rt) {
  const int kpv = KP > 0 ? KP : kp_rt;
  const int lane = threadIdx.x & 63;
  const int slot = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (slot >= *ws.amb_count) return;
  const int64_t p = ws.amb_list[slot];
  const float* q = qpad + p * kpv;
  const int cnt = ws.cand_cnt[slot];
  const bool overflow = cnt > kCandMax;
  const int64_t m = overflow ? n : cnt;
  auto row_of = [&](int64_t j) -> int64_t { return overflow ? j : (int64_t)ws.cand[slot * kCandMax + j]; };
  double vmin = INFINITY;
  for (int64_t j = 0; j < m; ++j) {
    if constexpr (LBL) {
      if (!label_row_ok(ws, p, row_of(j))) continue;  // wave-uniform
    }
    const double v = score64<KP, METRIC>(q, G + row_of(j) * kpv, lane, kpv);
    vmin = v < vmin ? v : vmin;
  }
  double qq = 0.0;
  for (int c = lane; c < kpv; c += 64) qq = fma((double)q[c], (double)q[c], qq);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) qq += __shfl_xor(qq, off);
  const double scale = METRIC == EF_METRIC_L2 ? qq + (double)fabsf(gmax2) : 1.0;  // negated: scan_regular
  const double tol = 1e-12 * (fabs(vmin) + scale);
  int64_t best_row = LLONG_MAX;
  double best_v = vmin;
  // a row with a NaN or an infinite component scores NaN or +inf against a finite probe; it is
  // never below vmin, and vmin < inf keeps it out when every row is such a row
  for (int64_t j = 0; j < m && vmin < INFINITY; ++j) {
    const int64_t r = row_of(j);
    if constexpr (LBL) {
      if (!label_row_ok(ws, p, r)) continue;
    }
    const double v = score64<KP, METRIC>(q, G + r * kpv, lane, kpv);
    if (v <= vmin + tol && r < best_row) { best_row = r; best_v = v; }
  }
  if (lane == 0 && best_row != LLONG_MAX) {
    const long long key = pack_key((float)best_v, (unsigned)(best_row + g_offset));
    keys[p] = key;
    if (ws.match) ws.match[p] = ef_match{best_v, scale, key};  // the scale as reduce_kernel forms it
  }
}

// ---- prefix path (EF_OPT_SEARCH_PREFIX, launch_search_prefix) ---------------------------
// Reduce of the prefix scan, one wave per probe.  The scan ran search_kernel<K1, L2> over
// the first K1 components of every row, so the per-chunk records hold fp32 prefix scores
// s1(g) = fl(||g[:K1]||^2 - 2 q[:K1].g[:K1]).  w = the scan's winner, r2 = its runner-up
// score = min of s1 over every row other than w (ties included).
//
// Proof that w is the answer.  In exact arithmetic, for every row g,
//   D(g) = ||q - g||^2 >= ||q[:K1] - g[:K1]||^2 = q1 + S1(g),  q1 = ||q[:K1]||^2,
// S1 the exact prefix score (the other KP - K1 squared differences are >= 0), and the scan's
// rounding obeys |s1(g) - S1(g)| <= e1: the fp32 L2 bound of reduce_kernel with the chain
// length K1 (||q|| and gmax2 of the full rows are upper bounds of the prefix's).  Hence
//   D(g) >= q1 + r2 - e1   for every g != w.
// The test is  q1 + r2 - delta1 > Dw + tol  with Dw = D(w) in fp64 (score64, the value the
// key is built from), tol the tie window of resolve_kernel and delta1 = 4 e1 (reduce_kernel's
// doubling for two compared scores and its x2 safety factor are kept).  When it holds,
// every other row's distance exceeds Dw + tol: w is the unique arg-min outside the tie
// window, which is what the full-k pipeline returns (its fp64 resolution keeps the lowest
// index among rows within tol of the minimum — only w).  One-sided safety of the test's own
// rounding: q1 and Dw are fp64 sums of <= 128 terms (relative error < 2^-45), r2 converts
// exactly, and the three fp64 adds round to 2^-53 relative — together below 1e-13 of
// (q1 + |r2| + Dw), while the 3 e1 of slack in delta1 is >= 3 (K1 + 4) 2^-24 gmax2 and tol
// adds 1e-12 (Dw + ||q||^2 + gmax2) on the same side; |r2| <= ||q||^2 + gmax2 + 2 ||q|| gm.
// A NaN anywhere makes the comparison false.  Unproven probes are appended to `list`
// (count at ws.amb_count[1]) for the full-k pipeline.
//
// S3 = 1 (EF_OPT_SEARCH_PREFIX_SPLIT, the default): the scan ran the split-bf16 chain
// hi.hi' + hi.lo' + lo.hi' over the split copy of the prefix, started from the same fp32
// ||g[:K1]||^2.  The argument is unchanged with e1 the split chain's bound at chain length
// K1: the dropped terms (3.05 2^-16 per element product, summed by Cauchy-Schwarz to
// 2 ||q|| gm), 3 K1 + 4 fp32 adds at 2u each and the K1 u gmax2 of the fp32 norm
// (scan_delta<L2, 1>, ef_search_common.hpp, which returns 4 e1); ||q|| and gmax2 of the full
// rows again bound the prefix's.  delta1 = 2 scan_delta<L2, 1>(K1, ..) = 8 e1, so 7 e1 of
// slack cover the test's own rounding as above.  The fp32 form keeps delta1 =
// scan_delta<L2, 0>(K1, ..) = 4 e1, the value it always had.  Nothing else depends on the
// arithmetic: Dw, q1, tol, the key and the record come from the fp32 rows in fp64.
template <int KP, int K1, int S3>
__global__ __launch_bounds__(256) void reduce_prefix_kernel(const float* __restrict__ qpad, int64_t b, int64_t bpad,
                                                            int nchunks, const float* __restrict__ G,
                                                            int64_t g_offset, float gmax2, SearchWs ws,
                                                            long long* __restrict__ keys, int* __restrict__ list) {
  const int lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= b) return;
  long long kmin = LLONG_MAX;
  for (int c = lane; c < nchunks; c += 64) {
    const long long k = ws.part_key[(int64_t)c * bpad + p];
    kmin = k < kmin ? k : kmin;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const long long o = __shfl_xor(kmin, off);
    kmin = o < kmin ? o : kmin;
  }
  if (kmin == LLONG_MAX) {  // no row scored (cannot happen with n > 0): the full-k run decides
    if (lane == 0) list[atomicAdd(ws.amb_count + 1, 1)] = (int)p;
    return;
  }
  float r2 = __builtin_inff();
  for (int c = lane; c < nchunks; c += 64) {
    const long long k = ws.part_key[(int64_t)c * bpad + p];
    r2 = fminf(r2, ws.part_b2[(int64_t)c * bpad + p]);
    if (k != kmin && k != LLONG_MAX) r2 = fminf(r2, key_value(k));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) r2 = fminf(r2, __shfl_xor(r2, off));

  const float b1 = key_value(kmin);
  const unsigned row = (unsigned)(kmin & 0xffffffffll);
  const float* q = qpad + p * KP;
  const double dw = score64<KP, EF_METRIC_L2>(q, G + (int64_t)row * KP, lane);
  double qq64 = 0.0, q1 = 0.0;
  for (int c = lane; c < KP; c += 64) {
    const double t = (double)q[c] * (double)q[c];
    qq64 += t;
    if (c < K1) q1 += t;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    qq64 += __shfl_xor(qq64, off);
    q1 += __shfl_xor(q1, off);
  }
  const float delta1 = (S3 ? 2.f : 1.f) * scan_delta<EF_METRIC_L2, S3>(K1, sqrtf((float)qq64), gmax2, b1);
  const double scale = qq64 + (double)gmax2;
  const double tol = 1e-12 * (fabs(dw) + scale);
  // outside the bound's domain (scan_regular: a negated gmax2 among them) nothing is proven here
  const bool regular = scan_regular<EF_METRIC_L2>((float)qq64, gmax2);
  if (lane == 0) {
    if (regular && q1 + (double)r2 - (double)delta1 > dw + tol) {
      const long long key = pack_key((float)dw, (unsigned)(row + g_offset));
      keys[p] = key;
      if (ws.match) ws.match[p] = ef_match{dw, scale, key};
    } else {
      list[atomicAdd(ws.amb_count + 1, 1)] = (int)p;
    }
  }
}

// The cascade's reduces (EF_OPT_SEARCH_PREFIX_SCREEN), a kernel template of their own:
// reduce_prefix_kernel above stays as it is, text and name, for option 0.  The code is its code
// with the slot p of the records apart from the probe pr.
//
// S3 = 2 (the first stage of the cascade): the scan was
// prefix64x_kernel<.., HI1>, one bf16 product per element.  With q^ = bf16(q), g^ = bf16(g) rounded
// to nearest, |x - x^| <= 2^-8 |x|, so per element
//   |2 q_i g_i - 2 q^_i g^_i| <= es 2 |q_i| |g_i| <= es (q_i^2 + g_i^2),  es = 2.01 2^-8
// (bf16(-2 q) = -2 q^ exactly), and over the K1 elements, with g1 = ||g[:K1]||^2,
//   |S~1(g) - S1(g)| <= es (q1 + g1),  S~1(g) = g1 - 2 q^.g^ in exact arithmetic.
// The row's share es g1 is a constant of the row and the probe's share es q1 one of the probe,
// so neither needs the largest norm of the gallery (scan_delta<L2, 2>'s 2 es ||q|| gm proves
// nothing as soon as one row is long).  The fp32 terms of scan_delta<L2, 2> at chain length K1
// split the same way: every partial sum of a row's chain is at most g1 + 2.02 ||q[:K1]||
// ||g[:K1]|| <= 1.01 q1 + 2.01 g1 in magnitude, so K1 + 4 adds and the final rounding (K1 + 6
// roundings at 2u each, 1 % for the products of rounded operands) cost at most
// cf (1.01 q1 + 2.01 g1), cf = (K1 + 6) 2u 1.01, and the fp32 norm itself K1 u g1.  With the
// project's safety factor 2 on these (none on es, a rounding theorem):
//   cg = 2 (2.01 cf + K1 u),  cq = 2 (1.01 cf)        (prefix_screen_cg / _cq),
// and a chain started from gstart(g) <= g1 (1 - es - cg) (rounded down, prefix_hi_kernel) ends at
//   L(g) <= S1(g) + (es + cq) q1   for every row g.
// Rows are ranked by L, not by the score: w = arg-min L (lowest row on ties), r2L = min of L over
// every other row.  Then for every g != w
//   D(g) >= q1 + S1(g) >= q1 (1 - es - cq) + L(g) >= q1 (1 - es - cq) + r2L,
// and the test  q1 (1 - es - cq) + r2L - uf > Dw + tol  proves D(g) > Dw + tol for all of them:
// w is the unique arg-min outside the tie window, as above.  If w is not the nearest row, or
// another row lies within tol of it, that row t has D(t) <= Dw + tol and L(t) >= r2L, and the
// test fails.  uf = (4 K1 + 8) 2^-126 (1 + 2.02 ||q|| + gm) covers operands, products and sums
// that underflow (2^-126 each, times the other operand), which the relative terms do not; the
// gate scan_regular and the negated gmax2 are the split form's.  The test's own fp64 rounding
// is below 1e-13 (q1 + |r2L| + Dw) as above, against cq q1 + cg g1 >= 1e-5 (q1 + g1) of slack
// whose safety factor's half is unused.  Unproven probes are appended to `list` with the count
// at ws.amb_count[kScreenCount].
//
// LST (the cascade's second stage; S3 = 1): slot p < ws.amb_count[kScreenCount] of the records
// belongs to probe src[p] (prefix64x_kernel<.., CNT>).  Its key and record go to the probe's own
// place and an unproven probe is listed by its own index, so nothing is scattered back; thread
// 0 adds the piece's screen count to the search's total (ws.amb_count[kScreenTotal]).
__host__ __device__ inline double prefix_screen_cf(int k1) { return (k1 + 6) * 2.0 * 5.9604644775390625e-08 * 1.01; }
__host__ __device__ inline double prefix_screen_cg(int k1) {
  return 2.0 * (2.01 * prefix_screen_cf(k1) + k1 * 5.9604644775390625e-08);
}
__host__ __device__ inline double prefix_screen_cq(int k1) { return 2.0 * 1.01 * prefix_screen_cf(k1); }
constexpr double kScreenEs = 2.01 * 0.00390625;  // 2.01 2^-8

template <int KP, int K1, int S3, bool LST>
__global__ __launch_bounds__(256) void reduce_prefix_x_kernel(const float* __restrict__ qpad, int64_t b, int64_t bpad,
                                                              int nchunks, const float* __restrict__ G,
                                                              int64_t g_offset, float gmax2, SearchWs ws,
                                                              long long* __restrict__ keys, int* __restrict__ list,
                                                              const int* __restrict__ src) {
  const int lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // the records' slot
  int* const unproven = ws.amb_count + (S3 == 2 ? kScreenCount : 1);
  int64_t pr = p;  // the probe
  if constexpr (LST) {
    if (blockIdx.x == 0 && threadIdx.x == 0) ws.amb_count[kScreenTotal] += ws.amb_count[kScreenCount];
    if (p >= ws.amb_count[kScreenCount]) return;
    pr = src[p];
  } else {
    if (p >= b) return;
  }
  long long kmin = LLONG_MAX;
  for (int c = lane; c < nchunks; c += 64) {
    const long long k = ws.part_key[(int64_t)c * bpad + p];
    kmin = k < kmin ? k : kmin;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const long long o = __shfl_xor(kmin, off);
    kmin = o < kmin ? o : kmin;
  }
  if (kmin == LLONG_MAX) {  // no row scored (cannot happen with n > 0): the full-k run decides
    if (lane == 0) list[atomicAdd(unproven, 1)] = (int)pr;
    return;
  }
  float r2 = __builtin_inff();
  for (int c = lane; c < nchunks; c += 64) {
    const long long k = ws.part_key[(int64_t)c * bpad + p];
    r2 = fminf(r2, ws.part_b2[(int64_t)c * bpad + p]);
    if (k != kmin && k != LLONG_MAX) r2 = fminf(r2, key_value(k));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) r2 = fminf(r2, __shfl_xor(r2, off));

  const float b1 = key_value(kmin);
  const unsigned row = (unsigned)(kmin & 0xffffffffll);
  const float* q = qpad + pr * KP;
  const double dw = score64<KP, EF_METRIC_L2>(q, G + (int64_t)row * KP, lane);
  double qq64 = 0.0, q1 = 0.0;
  for (int c = lane; c < KP; c += 64) {
    const double t = (double)q[c] * (double)q[c];
    qq64 += t;
    if (c < K1) q1 += t;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    qq64 += __shfl_xor(qq64, off);
    q1 += __shfl_xor(q1, off);
  }
  // the probe's side of the bound: what is taken off q1 + r2
  double off1;
  if constexpr (S3 == 2) {
    const double uf = (4 * K1 + 8) * 1.1754943508222875e-38 * (1.0 + 2.02 * sqrt(qq64) + sqrt(fabs((double)gmax2)));
    off1 = (kScreenEs + prefix_screen_cq(K1)) * q1 + uf;
  } else {
    off1 = (double)((S3 ? 2.f : 1.f) * scan_delta<EF_METRIC_L2, S3>(K1, sqrtf((float)qq64), gmax2, b1));
  }
  const double scale = qq64 + (double)gmax2;
  const double tol = 1e-12 * (fabs(dw) + scale);
  // outside the bound's domain (scan_regular: a negated gmax2 among them) nothing is proven here
  const bool regular = scan_regular<EF_METRIC_L2>((float)qq64, gmax2);
  if (lane == 0) {
    if (regular && q1 + (double)r2 - off1 > dw + tol) {
      const long long key = pack_key((float)dw, (unsigned)(row + g_offset));
      keys[pr] = key;
      if (ws.match) ws.match[pr] = ef_match{dw, scale, key};
    } else {
      list[atomicAdd(unproven, 1)] = (int)pr;
    }
  }
}

// dst[rows][c4_dst] <- the first c4_dst 16-B chunks of src[rows][c4_src] (the prefix copies of
// the gallery and of the probes).
__global__ void prefix_cols_kernel(const float4* __restrict__ src, int64_t rows, int c4_src, int c4_dst,
                                   float4* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * c4_dst) return;
  const int64_t r = i / c4_dst;
  dst[i] = src[r * c4_src + (i - r * c4_dst)];
}

// Second run's probes: out[slot] <- qpad[list[slot]] for the *count unproven probes; the
// rest of their last 256-probe tile is zeroed (scanned, never reduced).
__global__ void prefix_gather_kernel(const float4* __restrict__ qpad, const int* __restrict__ list,
                                     const int* __restrict__ count, int64_t bpad, int c4, float4* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= bpad * c4) return;
  const int64_t r = i / c4;
  const int cnt = *count;
  if (r >= ((int64_t)cnt + kSearchProbeTile - 1) / kSearchProbeTile * kSearchProbeTile) return;
  out[i] = r < cnt ? qpad[(int64_t)list[r] * c4 + (i - r * c4)] : make_float4(0.f, 0.f, 0.f, 0.f);
}

// Second run's results back to their probes; counters = ws.amb_count ([1] this piece's
// count, [2] the search's running total for ef_search_stats and the guard).
__global__ void prefix_scatter_kernel(const int* __restrict__ list, int* __restrict__ counters,
                                      const long long* __restrict__ keys2, const ef_match* __restrict__ match2,
                                      long long* __restrict__ keys, ef_match* __restrict__ match) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int cnt = counters[1];
  if (i == 0) counters[2] += cnt;  // one thread of the launch; kernels of a stream run in order
  if (i >= cnt) return;
  const int p = list[i];
  keys[p] = keys2[i];
  if (match) match[p] = match2[i];
}

// dst[rows_pad][kp] <- src[rows][k] with zero padding.
__global__ void pad_rows_kernel(const float* __restrict__ src, int64_t rows, int k, int64_t rows_pad,
                                float* __restrict__ dst, int kp) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows_pad * kp) return;
  const int64_t r = i / kp;
  const int c = (int)(i - r * kp);
  dst[i] = (r < rows && c < k) ? src[r * k + c] : 0.f;
}

// ||g||^2 and 1/||g|| per gallery row (K7: computed once at enrolment, not per probe as
// sklearn's cosine_similarity does, pairwise.py:1734), and max ||g||^2 for the bound.
// irregular (null: not wanted): bits set when a row is outside the scans' error model
// (scan_regular, ef_search_common.hpp): kRowNotFinite for a row whose fp32 ||g||^2 is +inf or
// NaN (a non-finite component, or finite components whose squares overflow), kRowTiny for a row
// that is not all zeros with ||g||^2 below kScanNormFloor, whose 1/||g|| is inexact or 0.
__global__ void gallery_aux_kernel(const float* __restrict__ G, int64_t n, int kp, float* __restrict__ gnorm2,
                                   float* __restrict__ ginv, unsigned* __restrict__ irregular) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  float s = 0.f;
  bool nz = false;
  for (int c = lane; c < kp; c += 64) {
    const float v = G[row * kp + c];
    s = __builtin_fmaf(v, v, s);
    nz = nz || v != 0.f;  // true for a NaN too
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  nz = __any(nz);
  if (lane == 0) {
    gnorm2[row] = s;
    ginv[row] = s > 0.f ? 1.0f / sqrtf(s) : 0.f;
    if (irregular) {
      if (!(s < __builtin_inff())) atomicOr(irregular, kRowNotFinite);
      else if (nz && s < kScanNormFloor) atomicOr(irregular, kRowTiny);
    }
  }
}

// Split-bf16 copy of the gallery (S3 search): per 8 fp32 elements, 16 B of hi = bf16(x)
// then 16 B of lo = bf16(x - hi); same row bytes as the fp32 gallery.  out may be G itself
// (the prefix copy is split in place): a thread reads its 32 B before it writes them.
__global__ void split_rows_kernel(const float* G, int64_t groups, uint4* out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= groups) return;
  const float4 a = reinterpret_cast<const float4*>(G)[2 * i];
  const float4 b = reinterpret_cast<const float4*>(G)[2 * i + 1];
  const float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  unsigned hi[8], lo[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    hi[j] = bf16_bits(x[j]);
    lo[j] = bf16_bits(x[j] - bf16_value(hi[j]));
  }
  out[2 * i] = make_uint4(hi[0] | hi[1] << 16, hi[2] | hi[3] << 16, hi[4] | hi[5] << 16, hi[6] | hi[7] << 16);
  out[2 * i + 1] = make_uint4(lo[0] | lo[1] << 16, lo[2] | lo[3] << 16, lo[4] | lo[5] << 16, lo[6] | lo[7] << 16);
}

// Single-bf16 copy (the bf16 screen, EF_OPT_SEARCH_SPLIT_BF16 = 3; wide kernels): per 64
// fp32 elements, 128 B = eight 16-B chunks, chunk 2q = bf16(x[8q .. 8q + 7]) and chunk
// 2q + 1 = bf16(x[32 + 8q .. 32 + 8q + 7]) — the split copy's slice row bytes and fragment
// order, so search_wide16_kernel<.., HI1> reads it with the split code (half the bytes).
__global__ void hi_rows_kernel(const float* __restrict__ G, int64_t blocks, uint4* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= blocks) return;
  const float4* x = reinterpret_cast<const float4*>(G) + 16 * i;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int e0 = (c & 1) * 32 + (c >> 1) * 8;  // first element of chunk c
    const float4 a = x[e0 / 4], b = x[e0 / 4 + 1];
    out[8 * i + c] = make_uint4(bf16_bits(a.x) | bf16_bits(a.y) << 16, bf16_bits(a.z) | bf16_bits(a.w) << 16,
                                bf16_bits(b.x) | bf16_bits(b.y) << 16, bf16_bits(b.z) | bf16_bits(b.w) << 16);
  }
}

// The screen's copy of the prefix (EF_OPT_SEARCH_PREFIX_SCREEN): out[n][c8] 16-B chunks, chunk c
// of row r = bf16(G[r][8 c .. 8 c + 7]), and the chains' start values gstart[r] = gnorm1[r] fac
// rounded down, fac = 1 - es - cg (reduce_prefix_x_kernel): fac's own rounding and the two
// products' are 3 2^-24 at the most, the factor 1 - 2^-22 takes them off again.
__global__ void prefix_hi_kernel(const float* __restrict__ G, int64_t n, int kp, int c8,
                                 const float* __restrict__ gnorm1, float fac, uint4* __restrict__ out,
                                 float* __restrict__ gstart) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * c8) return;
  const int64_t r = i / c8;
  const int c = (int)(i - r * c8);
  const float4* x = reinterpret_cast<const float4*>(G + r * kp + 8 * c);
  const float4 a = x[0], b = x[1];
  out[i] = make_uint4(bf16_bits(a.x) | bf16_bits(a.y) << 16, bf16_bits(a.z) | bf16_bits(a.w) << 16,
                      bf16_bits(b.x) | bf16_bits(b.y) << 16, bf16_bits(b.z) | bf16_bits(b.w) << 16);
  if (c == 0) gstart[r] = gnorm1[r] * fac * 0.99999976158142089844f;
}

// max ||g||^2 (one atomic per block; non-negative floats order as their bit patterns)
__global__ __launch_bounds__(256) void max_kernel(const float* __restrict__ x, int64_t n, unsigned* __restrict__ out) {
  __shared__ float red[4];
  float m = 0.f;
  // the finite values only: a row whose fp32 ||g||^2 is +inf or NaN is flagged by
  // gallery_aux_kernel, and the tie window's scale is taken over the other rows
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float v = x[i];
    m = fmaxf(m, v < __builtin_inff() ? v : 0.f);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    atomicMax(out, __float_as_uint(m));
  }
}

// ------------------------------------------------------------------------ launchers
int prefix_tile_rows(int k1, bool split) { return k1 <= 32 ? (split ? kPrefixSplitTile : kPrefixTile) : TG; }

SearchPlan search_plan(int64_t bpad, int64_t n, int kp, bool s3, int tile_rows, int min_chunks) {
  SearchPlan pl;
  const bool wide = kp > 128;
  const bool w3 = wide && s3;  // split-bf16 wide kernel: 256 x 256 tiles, one workgroup per CU
  // probes per workgroup.  The plans of kPrefixSplitTile rows are prefix64_kernel's (512 probes);
  // bpad is a multiple of 256 only, so its probe tiles are counted rounding up and the last one
  // may be half empty (the other tile sizes divide bpad)
  const int64_t ptile = w3 ? kWide3ProbeTile : wide ? kWideProbeTile
                        : tile_rows == kPrefixSplitTile ? kPrefixSplitProbes : kSearchProbeTile;
  pl.n_ptiles = (int)((bpad + ptile - 1) / ptile);
  const int64_t rows_per_tile = tile_rows ? tile_rows : w3 ? kWide3RowTile : wide ? kWideRowTile : TG;
  const int64_t tiles = (n + rows_per_tile - 1) / rows_per_tile;
  // ~512 workgroups = one resident wave of them (2 per CU): every chunk is swept by a
  // workgroup that starts at launch, so there is no tail round (measured: 90.1 % vs 89.6 %
  // at 1M rows, 82 % vs 80.5 % at 125k rows for 2048); the chunk count is a multiple of 8
  // so the XCD remap is a bijection.  EF_SEARCH_WGS overrides (experiments).
#ifdef EF_DIAGNOSTICS
  static const int64_t target0 = [] { const char* e = getenv("EF_SEARCH_WGS"); return e ? atoll(e) : 512; }();
  int64_t target = target0;
#else
  int64_t target = 512;
#endif
  if (w3) target = 256;
  int64_t want = (target + pl.n_ptiles - 1) / pl.n_ptiles;
  if (want > tiles) want = tiles;
  if (want < 1) want = 1;
  pl.nchunks = (int)(((want + 7) / 8) * 8);
  // top-m search: 2 nchunks per-chunk scores bound the m-th best, so at least m chunks
  if (min_chunks > 0) pl.nchunks = std::max(pl.nchunks, (min_chunks + 7) / 8 * 8);
  pl.tiles_per_chunk = (int)((tiles + pl.nchunks - 1) / pl.nchunks);
  if (pl.tiles_per_chunk < 1) pl.tiles_per_chunk = 1;
  // Wide kernel: the probes stream through LDS with every gallery tile, so an XCD whose
  // workgroups span all probe tiles re-fetches them from beyond its L2 (32 tiles x 256 KiB
  // at C5 = 8 MiB > 4 MiB L2: 27x the gallery bytes measured).  Deal blocks of 8 probe
  // tiles x cblk chunks to each XCD instead: 2 MiB of probes stay L2-resident and each
  // chunk is read by n_ptiles / 8 XCDs.
  // collect plan: ~512 chunks (a few queued probes then spread over the whole chip; with
  // every probe tile queued the grid strides over all items, a main pass's work)
  pl.c_tpc = (int)std::max<int64_t>(1, (tiles + 511) / 512);
  pl.c_chunks = (int)((tiles + pl.c_tpc - 1) / pl.c_tpc);
  pl.c_grid = w3 ? 256 : 512;
  // probe tiles per XCD block.  The split-bf16 wide kernels' probe tiles are 256 x KP x 4 B
  // (512 KiB at KP = 512), so 8 of them fill an XCD's L2; with the serpentine k order of
  // search_wide16_kernel that still fetches least from HBM (profiles/r04/c5_hbm_ab.txt), and
  // 16, 4 and 2 measured slower (profiles/r04/c5_screen_pb16_ab.txt)
  constexpr int pb = 8;
  pl.pblk = pl.n_ptiles;
  pl.cblk = 1;
  if (wide && pl.n_ptiles % pb == 0 && pl.n_ptiles > pb) {
    const int64_t per_xcd = (int64_t)pl.nchunks * pl.n_ptiles / 8;
    if (per_xcd % pb == 0 && pl.nchunks % (per_xcd / pb) == 0) {
      pl.pblk = pb;
      pl.cblk = (int)(per_xcd / pb);
    }
  }
  // a raised chunk count can leave the block deal no bijection: one block per chunk then
  if (min_chunks > 0 && wide && !block_deal_ok(pl, w3 ? kWide3ProbeTile : kWideProbeTile, bpad)) {
    pl.pblk = pl.n_ptiles;
    pl.cblk = 1;
  }
  return pl;
}

// One scan launch (ef_internal.hpp): the only place a scan kernel of KP <= 128 is named.  The
// CNT form exists for the fp32 L2 kernels of KP >= 32 alone (the prefix path's second run).
template <int KP, int M>
static hipError_t scan_t(hipStream_t s, bool collect, int variant, bool cnt, const SearchPlan& pl, const float* q,
                         const float* G, const float* aux, int64_t n, int64_t bpad, const SearchWs& ws) {
  const dim3 grid(collect ? (unsigned)pl.c_grid : (unsigned)(pl.nchunks * pl.n_ptiles)), block(512);
  const int a = collect ? pl.c_chunks : pl.n_ptiles, t = collect ? pl.c_tpc : pl.tiles_per_chunk;
  if (ws.lbl) {  // labelled search: the fp32 scan's labelled instantiations
    if (cnt || variant) return hipErrorInvalidValue;
    if (collect)
      hipLaunchKernelGGL((search_kernel<KP, M, true, false, false, TG, true>), grid, block, 0, s, q, G, aux, n, a, t, bpad, ws);
    else
      hipLaunchKernelGGL((search_kernel<KP, M, false, false, false, TG, true>), grid, block, 0, s, q, G, aux, n, a, t, bpad, ws);
  } else if (cnt) {
    if constexpr (M == EF_METRIC_L2 && KP >= 32) {
      if (collect || variant) return hipErrorInvalidValue;
      hipLaunchKernelGGL((search_kernel<KP, M, false, false, true>), grid, block, 0, s, q, G, aux, n, a, t, bpad, ws);
    } else {
      return hipErrorInvalidValue;
    }
  } else if (variant && KP == 128 && variant != 2) {
    if (collect)
      hipLaunchKernelGGL((search16_kernel<M, true>), grid, block, 0, s, q, G, aux, n, a, t, bpad, ws);
    else
      hipLaunchKernelGGL((search16_kernel<M, false>), grid, block, 0, s, q, G, aux, n, a, t, bpad, ws);
  } else if (variant) {
    if (collect)
      hipLaunchKernelGGL((search_kernel<KP, M, true, true>), grid, block, 0, s, q, G, aux, n, a, t, bpad, ws);
    else
      hipLaunchKernelGGL((search_kernel<KP, M, false, true>), grid, block, 0, s, q, G, aux, n, a, t, bpad, ws);
  } else if (collect) {
    hipLaunchKernelGGL((search_kernel<KP, M, true>), grid, block, 0, s, q, G, aux, n, a, t, bpad, ws);
  } else {
    hipLaunchKernelGGL((search_kernel<KP, M, false>), grid, block, 0, s, q, G, aux, n, a, t, bpad, ws);
  }
  return hipGetLastError();
}

hipError_t launch_search_scan(hipStream_t s, int kp, int metric, bool collect, int variant, bool cnt,
                              const SearchPlan& pl, const float* q, const float* G, const float* aux, int64_t n,
                              int64_t bpad, const SearchWs& ws) {
  if (kp > 128)
    return cnt ? hipErrorInvalidValue : launch_search_wide(s, kp, metric, collect, variant, pl, q, G, aux, n, bpad, ws);
#define EF_SCAN_CASE(KPV)                                                                                          \
  case KPV:                                                                                                        \
    return metric == EF_METRIC_L2 ? scan_t<KPV, EF_METRIC_L2>(s, collect, variant, cnt, pl, q, G, aux, n, bpad, ws) \
                                  : scan_t<KPV, EF_METRIC_COSINE>(s, collect, variant, cnt, pl, q, G, aux, n, bpad, ws);
  switch (kp) {
    EF_SCAN_CASE(16)
    EF_SCAN_CASE(32)
    EF_SCAN_CASE(64)
    EF_SCAN_CASE(128)
    default:
      return hipErrorInvalidValue;
  }
#undef EF_SCAN_CASE
}

hipError_t launch_scan_probes(hipStream_t s, const SplitScan& sp, const float* qpad, int64_t bpad, int kp,
                              const float** qs) {
  *qs = qpad;
  if (!sp.variant || kp <= 128) return hipSuccess;
  // the wide kernels stream the probes too, in the layout of the gallery copy
  if (!sp.Q3) return hipErrorInvalidValue;
  *qs = sp.Q3;
  return sp.variant == 3 ? launch_hi_rows(s, qpad, bpad, kp, sp.Q3) : launch_split_rows(s, qpad, bpad, kp, sp.Q3);
}

// The top-1 sequence, the only copy: the main scan of (variant, cnt) over (qs, Gs), timed when
// timer is given; the queue counter's memset (cnt: the caller zeroed it with its own counters);
// reduce_kernel in the variant's flavour (1 split scores, 2 the screen's single-bf16 ones), which
// queues the probes the scan's arithmetic cannot decide; the COLLECT scan over the queue;
// resolve_kernel in fp64.  reduce / resolve re-score from the fp32 probes q and gallery G; the
// last two exit at once when nothing is queued.  KP = 0: k > 512, row length kp at run time.
template <int KP, int M>
static hipError_t top1_t(hipStream_t s, int variant, bool cnt, const SearchPlan& pl, const float* q, const float* qs,
                         const float* Gs, int64_t bpad, int64_t b, const float* G, const float* aux, int64_t n,
                         int64_t g_offset, float gmax2, const SearchWs& ws, long long* keys, ef_ctx* timer, int kp) {
  constexpr bool wide = KP > 128 || KP == 0;
  if (!wide && variant == 3) variant = 1;
  TimerEvt tev;
  if (timer) timer_begin(timer, EF_KERNEL_SEARCH, &tev);
  hipError_t e = launch_search_scan(s, kp, M, false, variant, cnt, pl, qs, Gs, aux, n, bpad, ws);
  if (timer) timer_end(timer, &tev);
  if (e != hipSuccess) return e;
  if (!cnt && (e = hipMemsetAsync(ws.amb_count, 0, sizeof(int), s)) != hipSuccess) return e;
  const dim3 pgrid((unsigned)((b + 3) / 4)), pblock(256);
#define EF_REDUCE(...)                                                                                          \
  hipLaunchKernelGGL((reduce_kernel<KP, M, __VA_ARGS__>), pgrid, pblock, 0, s, q, b, bpad, pl.nchunks, G, n, \
                     g_offset, gmax2, ws, keys, kp)
  if (cnt) {
    if constexpr (!wide && M == EF_METRIC_L2 && KP >= 32) EF_REDUCE(0, true);
  } else if (variant == 3) {
    if constexpr (wide) EF_REDUCE(2);
  } else if (variant) {
    EF_REDUCE(1);
  } else {
    EF_REDUCE(0);
  }
#undef EF_REDUCE
  if ((e = launch_search_scan(s, kp, M, true, variant, false, pl, qs, Gs, aux, n, bpad, ws)) != hipSuccess) return e;
  if (ws.lbl)
    hipLaunchKernelGGL((resolve_kernel<KP, M, true>), pgrid, pblock, 0, s, q, G, n, g_offset, gmax2, ws, keys, kp);
  else
    hipLaunchKernelGGL((resolve_kernel<KP, M>), pgrid, pblock, 0, s, q, G, n, g_offset, gmax2, ws, keys, kp);
  return hipGetLastError();
}

hipError_t launch_search(hipStream_t s, int kp, int metric, const SplitScan& sp, const SearchPlan& pl,
                         const float* qpad, int64_t bpad, int64_t b, const float* G, const float* aux, int64_t n,
                         int64_t g_offset, float gmax2, const SearchWs& ws, long long* keys, ef_ctx* timer) {
  if (sp.variant && !sp.G3) return hipErrorInvalidValue;
  const float* qs = nullptr;
  const hipError_t e = launch_scan_probes(s, sp, qpad, bpad, kp, &qs);
  if (e != hipSuccess) return e;
  const float* Gs = sp.variant ? sp.G3 : G;
#define EF_SEARCH_CASE(KPV)                                                                                        \
  case KPV:                                                                                                        \
    return metric == EF_METRIC_L2                                                                                  \
               ? top1_t<KPV, EF_METRIC_L2>(s, sp.variant, false, pl, qpad, qs, Gs, bpad, b, G, aux, n, g_offset, gmax2, \
                                           ws, keys, timer, kp)                                                    \
               : top1_t<KPV, EF_METRIC_COSINE>(s, sp.variant, false, pl, qpad, qs, Gs, bpad, b, G, aux, n, g_offset,  \
                                               gmax2, ws, keys, timer, kp);
  // k > 512 (a multiple of 128): the wide kernels with the row length at run time, KP = 0
  switch (kp > 512 ? (kp % 128 == 0 ? 0 : -1) : kp > 0 ? kp : -1) {
    EF_SEARCH_CASE(16)
    EF_SEARCH_CASE(32)
    EF_SEARCH_CASE(64)
    EF_SEARCH_CASE(128)
    EF_SEARCH_CASE(256)
    EF_SEARCH_CASE(512)
    EF_SEARCH_CASE(0)
    default:
      return hipErrorInvalidValue;
  }
#undef EF_SEARCH_CASE
}

// Step 3 of the prefix search below: the probes of pw.list (count at ws.amb_count[1]) through
// top1_t's cnt form, their keys and records scattered back.
template <int KP>
static hipError_t prefix_second_run(hipStream_t s, const SearchPlan& pl, const float* qpad, int64_t bpad, int64_t b,
                                    const float* G, const float* gnorm2, int64_t n, int64_t g_offset, float gmax2,
                                    const SearchWs& ws, const PrefixWs& pw, long long* keys) {
  hipLaunchKernelGGL(prefix_gather_kernel, dim3((unsigned)((bpad * (KP / 4) + 255) / 256)), dim3(256), 0, s,
                     reinterpret_cast<const float4*>(qpad), pw.list, ws.amb_count + 1, bpad, KP / 4,
                     reinterpret_cast<float4*>(pw.qpad2));
  SearchWs w2 = ws;
  w2.match = ws.match ? pw.match2 : nullptr;
  const hipError_t e = top1_t<KP, EF_METRIC_L2>(s, 0, true, pl, pw.qpad2, pw.qpad2, G, bpad, b, G, gnorm2, n, g_offset,
                                                gmax2, w2, pw.keys2, nullptr, KP);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(prefix_scatter_kernel, dim3((unsigned)((b + 255) / 256)), dim3(256), 0, s, pw.list, ws.amb_count,
                     pw.keys2, w2.match, keys, ws.match);
  return hipGetLastError();
}

// Prefix search.  pl1 = search_plan(bpad, n, K1, false, prefix_tile_rows(K1, S3)) plans the
// prefix scan, pl the second run (the plain plan of KP).
//   1. Q1 <- the probes' first K1 columns; search_kernel<K1> over (Q1, G1, gnorm1): the
//      timed main launch, a K1 / KP share of the full scan's MFMAs, in 128-row tiles at
//      K1 <= 32 (prefix_tile_rows; profiles/r08).  S3 (EF_OPT_SEARCH_PREFIX_SPLIT): G1 holds
//      split-bf16 rows, the kernel splits the probes in registers and runs the split chain, 3
//      bf16 MFMAs of 32 cycles per 16 k against 8 fp32 ones of 64.  At K1 <= 32 that is
//      prefix64_kernel: 512 probes per workgroup (pl1 counts those tiles), 256-row tiles, the
//      probes read from qpad in place — no Q1 copy and no launch for it (profiles/r14).
//   2. reduce_prefix_kernel: proven probes get their key / match record, the others are listed.
//   3. The listed probes' rows are gathered into qpad2 and go through top1_t's sequence
//      in its cnt form (untimed, the device count in place of b, no memset of its own); the grids
//      are sized for bpad and the work past the count returns at once, so the host never
//      learns the count.  Their keys / records are scattered back by the list.
// G1h (EF_OPT_SEARCH_PREFIX_SCREEN; S3 and K1 <= 32 only): the cascade.  Step 1 becomes three:
//   1a. prefix64x_kernel<.., HI1> over (G1h, gstart): the timed main launch, one bf16 product per
//       element; reduce_prefix_x_kernel<.., 2> proves what its per-row bound can and lists the
//       rest in a list of its own (in pw.q1, which this form does not use; count at
//       ws.amb_count[kScreenCount]).
//   1b. prefix64x_kernel<.., CNT>: step 1's split scan for the listed probes alone, read through the
//       list, the count on the device and the grid sized for bpad.
//   1c. reduce_prefix_x_kernel<.., 1, LST>: step 2 for them; keys and records go to the probes' own
//       places, and pw.list receives the probes neither stage proved, by their own index.
// Step 3 is unchanged.  The caller zeroes ws.amb_count[kScreenCount] ahead of every piece.
template <int KP, int K1, bool S3>
static hipError_t search_prefix_t(hipStream_t s, const SearchPlan& pl, const SearchPlan& pl1, const float* qpad, int64_t bpad, int64_t b,
                                  const float* G, const float* gnorm2, const float* G1, const float* gnorm1,
                                  const float* G1h, int64_t n, int64_t g_offset, float gmax2, const SearchWs& ws,
                                  const PrefixWs& pw, long long* keys, ef_ctx* c) {
  constexpr int M = EF_METRIC_L2;
  const dim3 block(512), pgrid((unsigned)((b + 3) / 4)), sgrid((unsigned)(pl1.nchunks * pl1.n_ptiles));
  constexpr bool W64 = S3 && K1 <= 32;  // prefix64_kernel reads the probes' rows in place
  if (G1h && !W64) return hipErrorInvalidValue;
  if constexpr (!W64)
    hipLaunchKernelGGL(prefix_cols_kernel, dim3((unsigned)((bpad * (K1 / 4) + 255) / 256)), dim3(256), 0, s,
                       reinterpret_cast<const float4*>(qpad), bpad, KP / 4, K1 / 4, reinterpret_cast<float4*>(pw.q1));
  TimerEvt tev;
  timer_begin(c, EF_KERNEL_SEARCH, &tev);
  if constexpr (W64) {
    if (G1h)
      hipLaunchKernelGGL((prefix64x_kernel<KP, K1, kPrefixSplitProbes / 256, true, false>), sgrid, block, 0, s, qpad, G1h, gnorm1 + n,
                         n, pl1.n_ptiles, pl1.tiles_per_chunk, bpad, ws, nullptr);
    else
      hipLaunchKernelGGL((prefix64_kernel<KP, K1, kPrefixSplitProbes / 256>), sgrid, block, 0, s, qpad, G1, gnorm1, n, pl1.n_ptiles,
                         pl1.tiles_per_chunk, bpad, ws);
  } else {
    hipLaunchKernelGGL((search_kernel<K1, M, false, S3, false, (K1 <= 32 ? kPrefixTile : TG)>), sgrid, block, 0, s,
                       pw.q1, G1, gnorm1, n, pl1.n_ptiles, pl1.tiles_per_chunk, bpad, ws);
  }
  timer_end(c, &tev);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(ws.amb_count, 0, 2 * sizeof(int), s);  // [0] queued for fp64, [1] unproven
  if (e != hipSuccess) return e;
  if constexpr (W64) {
    if (G1h) {
      int* const list1 = reinterpret_cast<int*>(pw.q1);  // no Q1 copy in this form: the screen's list
      hipLaunchKernelGGL((reduce_prefix_x_kernel<KP, K1, 2, false>), pgrid, dim3(256), 0, s, qpad, b, bpad, pl1.nchunks, G,
                         g_offset, gmax2, ws, keys, list1, nullptr);
      hipLaunchKernelGGL((prefix64x_kernel<KP, K1, kPrefixSplitProbes / 256, false, true>), sgrid, block, 0, s, qpad, G1, gnorm1, n,
                         pl1.n_ptiles, pl1.tiles_per_chunk, bpad, ws, list1);
      hipLaunchKernelGGL((reduce_prefix_x_kernel<KP, K1, 1, true>), pgrid, dim3(256), 0, s, qpad, b, bpad, pl1.nchunks, G,
                         g_offset, gmax2, ws, keys, pw.list, list1);
      return prefix_second_run<KP>(s, pl, qpad, bpad, b, G, gnorm2, n, g_offset, gmax2, ws, pw, keys);
    }
  }
  hipLaunchKernelGGL((reduce_prefix_kernel<KP, K1, S3 ? 1 : 0>), pgrid, dim3(256), 0, s, qpad, b, bpad, pl1.nchunks, G, g_offset,
                     gmax2, ws, keys, pw.list);
  return prefix_second_run<KP>(s, pl, qpad, bpad, b, G, gnorm2, n, g_offset, gmax2, ws, pw, keys);
}

hipError_t launch_search_prefix(hipStream_t s, int kp, int k1, const SearchPlan& pl, const SearchPlan& pl1,
                                const float* qpad, int64_t bpad,
                                int64_t b, const float* G, const float* gnorm2, const float* G1, const float* gnorm1,
                                bool split, const float* G1h, int64_t n, int64_t g_offset, float gmax2,
                                const SearchWs& ws, const PrefixWs& pw, long long* keys, ef_ctx* c) {
#define EF_PREFIX_CASE(KPV, K1V)                                                                                  \
  if (kp == KPV && k1 == K1V)                                                                                     \
    return split ? search_prefix_t<KPV, K1V, true>(s, pl, pl1, qpad, bpad, b, G, gnorm2, G1, gnorm1, G1h, n, g_offset, gmax2, ws, pw, keys, c) \
                 : search_prefix_t<KPV, K1V, false>(s, pl, pl1, qpad, bpad, b, G, gnorm2, G1, gnorm1, G1h, n, g_offset, gmax2, ws, pw, keys, c);
  EF_PREFIX_CASE(128, 64)
  EF_PREFIX_CASE(128, 32)
  EF_PREFIX_CASE(128, 16)
  EF_PREFIX_CASE(64, 32)
  EF_PREFIX_CASE(64, 16)
  EF_PREFIX_CASE(32, 16)
#undef EF_PREFIX_CASE
  return hipErrorInvalidValue;
}

hipError_t launch_prefix_screen_gallery(hipStream_t s, const float* G, int64_t n, int kp, int k1, void* G1h, float* gnorm1) {
  const float fac = (float)(1.0 - kScreenEs - prefix_screen_cg(k1));
  hipLaunchKernelGGL(prefix_hi_kernel, dim3((unsigned)((n * (k1 / 8) + 255) / 256)), dim3(256), 0, s, G, n, kp, k1 / 8,
                     gnorm1, fac, static_cast<uint4*>(G1h), gnorm1 + n);
  return hipGetLastError();
}

hipError_t launch_prefix_gallery(hipStream_t s, const float* G, int64_t n, int kp, int k1, bool split, float* G1,
                                 float* gnorm1) {
  hipLaunchKernelGGL(prefix_cols_kernel, dim3((unsigned)((n * (k1 / 4) + 255) / 256)), dim3(256), 0, s,
                     reinterpret_cast<const float4*>(G), n, kp / 4, k1 / 4, reinterpret_cast<float4*>(G1));
  // the norms as gallery_aux_kernel computes gnorm2 (its 1/||g|| output goes to the spare half)
  hipLaunchKernelGGL(gallery_aux_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, G1, n, k1, gnorm1, gnorm1 + n, nullptr);
  // the split scan reads (hi, lo) rows: split the copy in place, after its fp32 norms are taken
  if (split) return launch_split_rows(s, G1, n, k1, G1);
  return hipGetLastError();
}

__global__ void keys_fill_kernel(long long* keys, int64_t b, ef_match* match) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < b) {
    keys[i] = LLONG_MAX;
    if (match) match[i] = ef_match{__builtin_inf(), 0.0, LLONG_MAX};
  }
}

hipError_t launch_keys_none(hipStream_t s, long long* keys, int64_t b, ef_match* match) {
  hipLaunchKernelGGL(keys_fill_kernel, dim3((unsigned)((b + 255) / 256)), dim3(256), 0, s, keys, b, match);
  return hipGetLastError();
}

// Labelled search: the probes' labels and excluded rows as the scan kernels read them
__global__ void label_prep_kernel(const int32_t* __restrict__ plabels, const int64_t* __restrict__ excl, int64_t b,
                                  int64_t rows, int64_t g_offset, int64_t n, int* __restrict__ plab,
                                  int* __restrict__ pexcl) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows) return;
  plab[i] = (i < b && plabels) ? plabels[i] : 0;
  int64_t e = -1;
  if (i < b && excl && excl[i] >= g_offset) e = excl[i] - g_offset;
  pexcl[i] = (e >= 0 && e < n) ? (int)e : -1;
}

hipError_t launch_label_prep(hipStream_t s, const int32_t* plabels, const int64_t* excl, int64_t b, int64_t rows,
                             int64_t g_offset, int64_t n, int* plab, int* pexcl) {
  hipLaunchKernelGGL(label_prep_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, plabels, excl, b, rows,
                     g_offset, n, plab, pexcl);
  return hipGetLastError();
}

hipError_t launch_pad_rows(hipStream_t s, const float* src, int64_t rows, int k, int64_t rows_pad, float* dst,
                           int kp) {
  const int64_t tot = rows_pad * kp;
  hipLaunchKernelGGL(pad_rows_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, src, rows, k,
                     rows_pad, dst, kp);
  return hipGetLastError();
}

hipError_t launch_split_rows(hipStream_t s, const float* G, int64_t n, int kp, void* out) {
  const int64_t groups = n * kp / 8;
  hipLaunchKernelGGL(split_rows_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, s, G, groups,
                     static_cast<uint4*>(out));
  return hipGetLastError();
}

hipError_t launch_hi_rows(hipStream_t s, const float* G, int64_t n, int kp, void* out) {
  if (kp % 64 != 0) return hipErrorInvalidValue;
  const int64_t blocks = n * kp / 64;
  hipLaunchKernelGGL(hi_rows_kernel, dim3((unsigned)((blocks + 255) / 256)), dim3(256), 0, s, G, blocks,
                     static_cast<uint4*>(out));
  return hipGetLastError();
}

hipError_t launch_gallery_aux(hipStream_t s, const float* G, int64_t n, int kp, float* gnorm2, float* ginv,
                              unsigned* gmax2_bits) {
  // gmax2_bits[0] max ||g||^2 over the rows whose norm is finite, [1] the kRow* bits
  hipError_t e = hipMemsetAsync(gmax2_bits, 0, 2 * sizeof(unsigned), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(gallery_aux_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, G, n, kp, gnorm2, ginv,
                     gmax2_bits + 1);
  hipLaunchKernelGGL(max_kernel, dim3(256), dim3(256), 0, s, gnorm2, n, gmax2_bits);
  return hipGetLastError();
}

}  // namespace ef
