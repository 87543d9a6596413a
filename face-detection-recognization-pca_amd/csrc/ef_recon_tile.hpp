// The back-projection GEMM's workgroup walk, shared by recon_kernel (ef_recon.hip) and the model
// bank's grouped residual (ef_bank_recon.hip): 128 probes against the 128-pixel tiles
// [t_beg, t_end) of x^ = mean + f . R, KP swept in RK-component stages (double-buffered LDS,
// register-staged prefetch that runs on across tile boundaries), then one of three epilogues on
// the accumulators: store fp32, store uint8 (clamp, round half to even), or the residual, whose
// row sums stay in registers along the walk and leave the workgroup as one partial per probe.
#pragma once

#include "ef_internal.hpp"

namespace ef {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int RM = 128;       // probes per workgroup
constexpr int RN = 128;       // pixels per tile
// RK, the components per stage, is a template parameter: 32, or 16 for the one padded k (16) that
// 32 does not divide; the feature tile's LDS rows are RK + 4 floats (16-B aligned b128 reads)

enum { EPI_F32 = 0, EPI_U8 = 1, EPI_RESID = 2 };

struct ReconArgs {
  const float* qpad;  // [>= m0 + 128][kp], zero past b and past k
  const float* R;     // [kp][dp]
  const float* mean;  // [d]
  const float* wgt;   // [d]
  const void* P;      // [b][d] pixels (residual)
  void* out;          // [b][d] fp32 | uint8 (store forms)
  float* part;        // [2][part_rows][bp] partial eps^2, then partial E (residual)
  int64_t b, d, dp, bp;
  int kp, ntiles, tiles_per_split;
};

// m0: first probe of the workgroup (a multiple of 128).  The residual's partials of probes
// m0 .. m0 + 127 go to row part_row of the part_rows rows of a.part (eps^2), and to the same row
// of the second block of part_rows rows (E); where(&part_row, &part_rows) is asked for the two
// only where they are used, after the walk, so they occupy no registers along it.
// VEC (residual): rows of P, mean and the weight can be read four pixels at a time
template <int EPI, int PDT, bool VEC, int RK, class Where>
__device__ __forceinline__ void recon_tile(const ReconArgs a, const int64_t m0, const int t_beg, const int t_end,
                                           const Where where) {
  constexpr int RSA = RK + 4;
  constexpr int NL = RK / 8;  // float4 of each operand per thread and stage
  __shared__ __attribute__((aligned(16))) float sA[2][RM * RSA];
  __shared__ __attribute__((aligned(16))) float sB[2][RK * RN];
  __shared__ float sRed[2][2][RM];  // [eps^2 | E][column half][probe]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, c32 = lane & 31;
  const int wm = wave >> 1, wn = wave & 1;  // 2 x 2 waves of 64 probes x 64 pixels
  const int nst = a.kp / RK;
  const int nsteps = (t_end - t_beg) * nst;

  // staging: NL float4 of each operand per thread and stage, in registers between the loads
  // (issued before a stage's MFMAs) and the LDS stores (after them); plain registers, not arrays,
  // which stayed in scratch in some of the kernel's forms
#define EF_RECON_LOAD1(j, A_, B_, tile_, st_)                                                                \
  {                                                                                                           \
    const int idx = tid + 256 * (j);                                                                          \
    A_ = *reinterpret_cast<const float4*>(a.qpad + (m0 + idx / (RK / 4)) * a.kp + (st_) * RK +                \
                                          4 * (idx % (RK / 4)));                                              \
    B_ = *reinterpret_cast<const float4*>(a.R + (int64_t)((st_) * RK + (idx >> 5)) * a.dp +                   \
                                          (int64_t)(tile_) * RN + 4 * (idx & 31));                            \
  }
#define EF_RECON_LOAD(tile_, st_)                 \
  EF_RECON_LOAD1(0, ga0, gb0, tile_, st_)         \
  EF_RECON_LOAD1(1, ga1, gb1, tile_, st_)         \
  if constexpr (NL > 2) {                         \
    EF_RECON_LOAD1(2, ga2, gb2, tile_, st_)       \
    EF_RECON_LOAD1(3, ga3, gb3, tile_, st_)       \
  }
#define EF_RECON_STORE1(j, A_, B_, buf_)                                                                      \
  {                                                                                                           \
    const int idx = tid + 256 * (j);                                                                          \
    *reinterpret_cast<float4*>(&sA[buf_][(idx / (RK / 4)) * RSA + 4 * (idx % (RK / 4))]) = A_;                \
    *reinterpret_cast<float4*>(&sB[buf_][(idx >> 5) * RN + 4 * (idx & 31)]) = B_;                             \
  }
#define EF_RECON_STORE(buf_)                \
  EF_RECON_STORE1(0, ga0, gb0, buf_)        \
  EF_RECON_STORE1(1, ga1, gb1, buf_)        \
  if constexpr (NL > 2) {                   \
    EF_RECON_STORE1(2, ga2, gb2, buf_)      \
    EF_RECON_STORE1(3, ga3, gb3, buf_)      \
  }
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x16{};
  // residual sums of this lane's probe (one per probe block) over the pixels it has seen
  float rs[2] = {0.f, 0.f}, es[2] = {0.f, 0.f};

  if (nsteps > 0) {
    float4 ga0, gb0, ga1, gb1, ga2 = z4, gb2 = z4, ga3 = z4, gb3 = z4;
    EF_RECON_LOAD(t_beg, 0)
    EF_RECON_STORE(0)
  }
  __syncthreads();
  int tile = t_beg, st = 0;
  for (int step = 0; step < nsteps; ++step) {
    const int buf = step & 1;
    const bool more = step + 1 < nsteps;
    const bool last = st + 1 == nst;  // this tile's accumulators are complete after this stage
    // (the prefetch after the last step re-reads it: no branch around the loads)
    const int tile_n = more && last ? tile + 1 : tile, st_n = !more ? st : last ? 0 : st + 1;
    float4 ga0, gb0, ga1, gb1, ga2 = z4, gb2 = z4, ga3 = z4, gb3 = z4;
    EF_RECON_LOAD(tile_n, st_n)
    // k order inside the stage: lane half h owns components [h RK/2, (h + 1) RK/2) for both operands
#pragma unroll
    for (int s4 = 0; s4 < RK / 2; s4 += 4) {
      float4 fa[2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
        fa[i] = *reinterpret_cast<const float4*>(&sA[buf][(wm * 64 + i * 32 + c32) * RSA + (RK / 2) * h + s4]);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float fb[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) fb[j] = sB[buf][((RK / 2) * h + s4 + e) * RN + wn * 64 + j * 32 + c32];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const float x = e == 0 ? fa[i].x : e == 1 ? fa[i].y : e == 2 ? fa[i].z : fa[i].w;
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            // both operands map lane & 31 to their own index, so swapping them transposes the tile:
            // the store forms keep the pixel on the lane (coalesced rows of x^), the residual
            // keeps the probe there and sums its pixels inside the lane
            if constexpr (EPI == EPI_RESID)
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fb[j], x, acc[i][j], 0, 0, 0);
            else
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(x, fb[j], acc[i][j], 0, 0, 0);
          }
        }
      }
    }
    if (last) {
      if constexpr (EPI == EPI_RESID) {
        // element r of block (i, j): probe = lane & 31, pixel = (r & 3) + 8 (r >> 2) + 4 h, so a lane
        // holds runs of four consecutive pixels of its probe: one 4-byte (16-byte) load each
        const uint8_t* P8 = static_cast<const uint8_t*>(a.P);
        const float* P32 = static_cast<const float*>(a.P);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int64_t col = (int64_t)tile * RN + wn * 64 + j * 32 + 8 * q + 4 * h;
            float mu[4], w[4];
            if (VEC && col < a.d) {
              const float4 m4 = *reinterpret_cast<const float4*>(a.mean + col);
              const float4 w4 = *reinterpret_cast<const float4*>(a.wgt + col);
              mu[0] = m4.x; mu[1] = m4.y; mu[2] = m4.z; mu[3] = m4.w;
              w[0] = w4.x; w[1] = w4.y; w[2] = w4.z; w[3] = w4.w;
            } else {
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const bool ok = !VEC && col + e < a.d;
                mu[e] = ok ? a.mean[col + e] : 0.f;
                w[e] = ok ? a.wgt[col + e] : 0.f;  // weight 0 past d: no contribution
              }
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
              const int64_t row = m0 + wm * 64 + i * 32 + c32;
              float pv[4] = {0.f, 0.f, 0.f, 0.f};
              if (row < a.b && col < a.d) {
                const int64_t at = row * a.d + col;
                if constexpr (VEC && PDT == EF_U8) {
                  const unsigned u4 = *reinterpret_cast<const unsigned*>(P8 + at);
                  pv[0] = (float)(u4 & 0xffu); pv[1] = (float)((u4 >> 8) & 0xffu);
                  pv[2] = (float)((u4 >> 16) & 0xffu); pv[3] = (float)(u4 >> 24);
                } else if constexpr (VEC) {
                  const float4 v = *reinterpret_cast<const float4*>(P32 + at);
                  pv[0] = v.x; pv[1] = v.y; pv[2] = v.z; pv[3] = v.w;
                } else {
#pragma unroll
                  for (int e = 0; e < 4; ++e)
                    if (col + e < a.d) pv[e] = PDT == EF_U8 ? (float)P8[at + e] : P32[at + e];
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                  const float c = pv[e] - mu[e];
                  const float t = w[e] * (c - acc[i][j][4 * q + e]);
                  const float u = w[e] * c;
                  rs[i] += t * t;
                  es[i] += u * u;
                }
              }
            }
          }
        }
      } else {
        // element r of block (i, j): pixel = lane & 31, probe = (r & 3) + 8 (r >> 2) + 4 h
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int64_t col = (int64_t)tile * RN + wn * 64 + j * 32 + c32;
          const bool col_ok = col < a.d;
          const float mu = col_ok ? a.mean[col] : 0.f;
#pragma unroll
          for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int64_t row = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
              if (col_ok && row < a.b) {
                const int64_t at = row * a.d + col;
                if constexpr (EPI == EPI_F32) {
                  static_cast<float*>(a.out)[at] = mu + acc[i][j][r];
                } else {
                  const float v = fminf(fmaxf(mu + acc[i][j][r], 0.f), 255.f);
                  static_cast<uint8_t*>(a.out)[at] = (uint8_t)__builtin_rintf(v);
                }
              }
            }
          }
        }
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x16{};
    }
    EF_RECON_STORE(buf ^ 1)  // (after the last step: the re-read stage, into the buffer nobody reads)
    __syncthreads();
    if (last) {
      ++tile;
      st = 0;
    } else {
      ++st;
    }
  }

  if constexpr (EPI == EPI_RESID) {
    // the two lane halves (pixels 4h ..), then the two 64-pixel column halves in LDS
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const float v = rs[i] + __shfl_xor(rs[i], 32);
      const float u = es[i] + __shfl_xor(es[i], 32);
      if (h == 0) {
        sRed[0][wn][wm * 64 + i * 32 + c32] = v;
        sRed[1][wn][wm * 64 + i * 32 + c32] = u;
      }
    }
    __syncthreads();
    if (tid < RM) {
      int64_t part_row, part_rows;
      where(&part_row, &part_rows);
      const int64_t at = part_row * a.bp + m0 + tid;
      a.part[at] = sRed[0][0][tid] + sRed[0][1][tid];
      a.part[part_rows * a.bp + at] = sRed[1][0][tid] + sRed[1][1][tid];
    }
  }
#undef EF_RECON_LOAD
#undef EF_RECON_LOAD1
#undef EF_RECON_STORE
#undef EF_RECON_STORE1
}

}  // namespace ef
