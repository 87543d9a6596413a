// Back-projection out of face space: x^ = mean + f . R, and the distance from
// face space eps^2 = sum_j (s_j (p_j - x^_j))^2 with the total energy E = sum_j (s_j (p_j - mean_j))^2.
//
// The other half of the eigenfaces method (Turk-Pentland's face / non-face test): sklearn's
// scaler.inverse_transform(pca.inverse_transform(f)) and the residual of a face against it.
//
// GEMM M = b probes, N = d pixels, K = KP padded components on v_mfma_f32_32x32x2_f32.  A is the
// padded probe-feature buffer project_reduce_kernel fills ([Bpad][KP], zero past b and past k),
// B the resident R padded to [KP][DP] (DP = round_up(d, 128), zero past k and past d), so the
// main loop has no bounds checks.  A workgroup owns 128 probes and walks a run of 128-pixel
// tiles; per tile it sweeps KP in RK-component stages (double-buffered LDS, register-staged
// prefetch that runs on across tile boundaries) and then applies one of three epilogues to the
// accumulators: store fp32, store uint8 (clamp, round half to even), or the residual, whose row
// sums stay in registers along the walk and leave the workgroup as one partial per probe.  The
// pixel axis is split over gridDim.y; recon_reduce_kernel adds the partials in split order, so
// the result is the same bits on every call.  x^ is never written by the residual form.
#include <algorithm>

#include "ef_recon_tile.hpp"

namespace ef {

namespace {

template <int EPI, int PDT, bool VEC, int RK>
__global__ __launch_bounds__(256, 2) void recon_kernel(const ReconArgs a) {
  const int64_t m0 = (int64_t)blockIdx.x * RM;
  const int t_beg = blockIdx.y * a.tiles_per_split;
  const int t_end = min(t_beg + a.tiles_per_split, a.ntiles);
  recon_tile<EPI, PDT, VEC, RK>(a, m0, t_beg, t_end, [](int64_t* row, int64_t* rows) {
    *row = blockIdx.y;
    *rows = gridDim.y;
  });
}

// dffs2[row] = sum_z part[0][z][row], energy[row] = sum_z part[1][z][row] (fixed z order)
__global__ void recon_reduce_kernel(const float* __restrict__ part, int nsplit, int64_t b, int64_t bp,
                                    float* __restrict__ dffs2, float* __restrict__ energy) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= b) return;
  float s = 0.f, e = 0.f;
  for (int z = 0; z < nsplit; ++z) {
    s += part[(int64_t)z * bp + row];
    e += part[((int64_t)nsplit + z) * bp + row];
  }
  dffs2[row] = s;
  if (energy) energy[row] = e;
}

}  // namespace

int64_t recon_dpad(int64_t d) { return round_up(d, RN); }

int recon_nsplit(int64_t b, int64_t d, int* tiles_per_split) {
  const int64_t mtiles = (b + RM - 1) / RM;
  const int64_t ntiles = recon_dpad(d) / RN;
  int64_t ns = (512 + mtiles - 1) / mtiles;  // ~2 workgroups per CU
  ns = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(ns, ntiles), 64));
  const int64_t tps = (ntiles + ns - 1) / ns;
  *tiles_per_split = (int)tps;
  return (int)((ntiles + tps - 1) / tps);
}

hipError_t launch_recon(hipStream_t s, int epi, int p_dtype, const float* qpad, int kp, const float* R, const float* mean,
                        const float* wgt, const void* P, int64_t b, int64_t d, void* out, float* part, int nsplit,
                        int tiles_per_split) {
  if (b < 1 || kp % 16 != 0) return hipErrorInvalidValue;
  ReconArgs a;
  a.qpad = qpad;
  a.R = R;
  a.mean = mean;
  a.wgt = wgt;
  a.P = P;
  a.out = out;
  a.part = part;
  a.b = b;
  a.d = d;
  a.dp = recon_dpad(d);
  a.bp = round_up(b, RM);
  a.kp = kp;
  a.ntiles = (int)(a.dp / RN);
  a.tiles_per_split = tiles_per_split;
  const dim3 grid((unsigned)(a.bp / RM), (unsigned)nsplit);
  const auto aligned = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  const bool vec = d % 4 == 0 && aligned(P) && aligned(mean) && aligned(wgt);
  const bool k32 = kp % 32 == 0;
  const void* fn = nullptr;
#define EF_RECON_FN(E, T, V) \
  (k32 ? reinterpret_cast<const void*>(&recon_kernel<E, T, V, 32>) : reinterpret_cast<const void*>(&recon_kernel<E, T, V, 16>))
  if (epi == 0) fn = EF_RECON_FN(EPI_F32, EF_F32, false);
  else if (epi == 1) fn = EF_RECON_FN(EPI_U8, EF_F32, false);
  else if (p_dtype == EF_U8) fn = vec ? EF_RECON_FN(EPI_RESID, EF_U8, true) : EF_RECON_FN(EPI_RESID, EF_U8, false);
  else fn = vec ? EF_RECON_FN(EPI_RESID, EF_F32, true) : EF_RECON_FN(EPI_RESID, EF_F32, false);
#undef EF_RECON_FN
  void* args[] = {&a};
  return hipLaunchKernel(fn, grid, dim3(256), args, 0, s);
}

hipError_t launch_recon_reduce(hipStream_t s, const float* part, int nsplit, int64_t b, float* dffs2, float* energy) {
  hipLaunchKernelGGL(recon_reduce_kernel, dim3((unsigned)((b + 255) / 256)), dim3(256), 0, s, part, nsplit, b,
                     round_up(b, RM), dffs2, energy);
  return hipGetLastError();
}

}  // namespace ef
