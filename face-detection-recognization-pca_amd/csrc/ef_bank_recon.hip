// Model bank: the distance from face space against every slot at once ("Model
// bank").  The grouped form of recon_kernel's residual epilogue: one launch over
// (slot, 128-probe tile, pixel split) work items, each of which runs the tile walk of
// ef_recon_tile.hpp on its slot's operands.
//
//   A   the bank's own feature block of the slot, q + bpad * kp_off, [bpad][kp_m]: bank_reduce_kernel
//       zeroes it past b and past k_m, and bpad is a multiple of 128, so nothing is copied
//   B   the slot's R, [kp_m][DP] with DP = round_up(d, 128), zero past k_m and past d
//   the slot's folded mean and weight; every slot shares d, so the tiles and the split are the
//   launch's, and the stage depth RK is too: 16 when any slot has kp = 16 (a 32-wide stage
//   would read the next probe's row of a 16-float feature row), else 32
//
// Partials [2][nsplit][M][bpad]; bank_recon_reduce_kernel adds them in split order into the
// probe-major dffs2[b][M] and energy[b][M].  No atomics: the same bits on every call.
#include <algorithm>
#include <climits>

#include "ef_recon_tile.hpp"

namespace ef {

namespace {

constexpr int64_t kBankReconWgs = 512;  // ~2 residual workgroups per CU

struct BankReconArgs {
  const BankReconDev* tab;
  const float* q;
  const void* P;
  float* part;
  int64_t b, d, dp, bpad;
  int n_slots, n_ptiles, nsplit, ntiles, tiles_per_split;
};

template <int PDT, bool VEC, int RK>
__global__ __launch_bounds__(256, 2) void bank_recon_kernel(const BankReconArgs g) {
  // probe tiles of one (slot, split) are neighbours: they read the same piece of R
  const int pt = blockIdx.x % g.n_ptiles;
  const int rest = blockIdx.x / g.n_ptiles;
  const int split = rest % g.nsplit;
  const int slot = rest / g.nsplit;
  const BankReconDev T = g.tab[slot];
  ReconArgs a;
  a.qpad = g.q + g.bpad * T.kp_off;
  a.R = T.R;
  a.mean = T.mean;
  a.wgt = T.wgt;
  a.P = g.P;
  a.out = nullptr;
  a.part = g.part;
  a.b = g.b;
  a.d = g.d;
  a.dp = g.dp;
  a.bp = g.bpad;
  a.kp = T.kp;
  a.ntiles = g.ntiles;
  a.tiles_per_split = g.tiles_per_split;
  const int t_beg = split * g.tiles_per_split;
  const int t_end = min(t_beg + g.tiles_per_split, g.ntiles);
  const int n_slots = g.n_slots, nsplit = g.nsplit;
  recon_tile<EPI_RESID, PDT, VEC, RK>(a, (int64_t)pt * RM, t_beg, t_end, [=](int64_t* row, int64_t* rows) {
    *row = (int64_t)split * n_slots + slot;
    *rows = (int64_t)nsplit * n_slots;
  });
}

// dffs2[p][m] = sum_z part[0][z][m][p], energy[p][m] = sum_z part[1][z][m][p] (fixed z order).
// One thread per (slot, probe), probe fastest: coalesced reads of the partials.
__global__ void bank_recon_reduce_kernel(const float* __restrict__ part, int nsplit, int n_slots, int64_t b,
                                         int64_t bpad, float* __restrict__ dffs2, float* __restrict__ energy) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b * n_slots) return;
  const int64_t m = i / b, p = i - m * b;
  const int64_t blk = (int64_t)nsplit * n_slots * bpad;
  float s = 0.f, e = 0.f;
  for (int z = 0; z < nsplit; ++z) {
    const int64_t at = ((int64_t)z * n_slots + m) * bpad + p;
    s += part[at];
    e += part[blk + at];
  }
  dffs2[p * n_slots + m] = s;
  if (energy) energy[p * n_slots + m] = e;
}

}  // namespace

BankReconPlan bank_recon_plan(int64_t b, int64_t d, int64_t n_slots) {
  const int64_t ptiles = (b + RM - 1) / RM;
  const int64_t ntiles = (d + RN - 1) / RN;
  const int64_t items = std::max<int64_t>(1, ptiles * n_slots);
  int64_t ns = (kBankReconWgs + items - 1) / items;
  ns = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(ns, ntiles), 64));
  const int64_t tps = (ntiles + ns - 1) / ns;
  BankReconPlan pl;
  pl.tiles_per_split = (int)tps;
  pl.nsplit = (int)((ntiles + tps - 1) / tps);  // no empty split
  pl.n_workgroups = ptiles * n_slots * pl.nsplit;
  pl.scratch_bytes = (int64_t)2 * pl.nsplit * n_slots * round_up(b, RM) * (int64_t)sizeof(float);
  return pl;
}

hipError_t launch_bank_recon(hipStream_t s, const BankReconDev* tab, int n_slots, int rk, int p_dtype, const float* q,
                             const void* P, int64_t b, int64_t bpad, int64_t d, float* part, const BankReconPlan& pl) {
  if (b < 1 || n_slots < 1 || bpad % RM != 0 || bpad < b || (rk != 16 && rk != 32) || pl.n_workgroups > INT_MAX)
    return hipErrorInvalidValue;
  BankReconArgs g;
  g.tab = tab;
  g.q = q;
  g.P = P;
  g.part = part;
  g.b = b;
  g.d = d;
  g.dp = recon_dpad(d);
  g.bpad = bpad;
  g.n_slots = n_slots;
  g.n_ptiles = (int)((b + RM - 1) / RM);
  g.nsplit = pl.nsplit;
  g.ntiles = (int)(g.dp / RN);
  g.tiles_per_split = pl.tiles_per_split;
  // (the slots' means and weights are allocations of their own: 256-byte aligned)
  const bool vec = d % 4 == 0 && (reinterpret_cast<uintptr_t>(P) & 15) == 0;
  const void* fn = nullptr;
#define EF_BANK_RECON_FN(T, V) \
  (rk == 32 ? reinterpret_cast<const void*>(&bank_recon_kernel<T, V, 32>) : reinterpret_cast<const void*>(&bank_recon_kernel<T, V, 16>))
  if (p_dtype == EF_U8) fn = vec ? EF_BANK_RECON_FN(EF_U8, true) : EF_BANK_RECON_FN(EF_U8, false);
  else fn = vec ? EF_BANK_RECON_FN(EF_F32, true) : EF_BANK_RECON_FN(EF_F32, false);
#undef EF_BANK_RECON_FN
  void* args[] = {&g};
  return hipLaunchKernel(fn, dim3((unsigned)pl.n_workgroups), dim3(256), args, 0, s);
}

hipError_t launch_bank_recon_reduce(hipStream_t s, const float* part, int nsplit, int n_slots, int64_t b, int64_t bpad,
                                    float* dffs2, float* energy) {
  hipLaunchKernelGGL(bank_recon_reduce_kernel, dim3((unsigned)((b * n_slots + 255) / 256)), dim3(256), 0, s, part, nsplit,
                     n_slots, b, bpad, dffs2, energy);
  return hipGetLastError();
}

}  // namespace ef

using namespace ef;

extern "C" int ef_bank_recon_schedule(int64_t b, int64_t d, int32_t n_models, int32_t* nsplit, int32_t* tiles_per_split,
                                      int64_t* n_workgroups, int64_t* scratch_bytes) {
  if (b < 1 || b > EF_BANK_MAX_PROBES || d < 1 || n_models < 1 || n_models > EF_BANK_MAX_MODELS) return EF_E_INVALID;
  const BankReconPlan pl = bank_recon_plan(b, d, n_models);
  if (nsplit) *nsplit = pl.nsplit;
  if (tiles_per_split) *tiles_per_split = pl.tiles_per_split;
  if (n_workgroups) *n_workgroups = pl.n_workgroups;
  if (scratch_bytes) *scratch_bytes = pl.scratch_bytes;
  return EF_OK;
}
