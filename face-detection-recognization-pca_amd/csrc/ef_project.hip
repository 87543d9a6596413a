// Probe projection f = (p - mean) . W  (SURVEY.md K6).
//
// Replaces project_face_to_eigenspace (useless/scan.py:93-96) and the folded
// scaler.transform + pca.transform of extract_face_features (scan-template-v4.py:265-266),
// batched over B probes.  uint8 pixels are converted and mean-subtracted while they are
// staged into LDS (the centred matrix is never materialised in HBM).
//
// GEMM M=B probes, N=KPW (64|128) components, K=d pixels on v_mfma_f32_32x32x2_f32.
// Workgroup tile 128 probes x KPW, BK=32 pixels per stage, double-buffered LDS with
// register-staged prefetch.  K is split over gridDim.y into fp32 partial slabs that a
// second kernel sums in a fixed order (deterministic) straight into the padded probe
// buffer the search kernel reads.
#include "ef_project_tile.hpp"

namespace ef {

// KPW = columns of this workgroup's tile (64 | 128); ldw = total padded columns of W and of
// the partial slabs (KPW, or a multiple of 128 with gridDim.z = ldw / 128 column tiles).
// The tile body, and what FAST means, are in ef_project_tile.hpp.
template <int KPW, int PDT, bool VEC, bool FAST = false>
__global__ __launch_bounds__(256, 2) void project_kernel(const void* __restrict__ Pv, int64_t b,
                                                         int64_t d, const float* __restrict__ mu,
                                                         const float* __restrict__ W, int ldw,
                                                         float* __restrict__ part, int64_t bpad,
                                                         int64_t pix_per_split) {
  const int col0 = blockIdx.z * KPW;
  const int64_t k_beg = (int64_t)blockIdx.y * pix_per_split;
  int64_t k_end = k_beg + pix_per_split;
  if (k_end > d) k_end = d;
  // partial slab [split][bpad][ldw]
  project_tile<KPW, PDT, VEC, FAST>(Pv, b, d, mu, W, ldw, col0, (int64_t)blockIdx.x * BM, k_beg, k_end,
                                    part + (int64_t)blockIdx.y * bpad * ldw + col0, ldw);
}

// qpad[row][c] = sum_z part[z][row][c] (c < kp, rows < bpad; fixed z order);
// f_out[row][c] for row < b, c < k when requested.
// corr (bf16 model only): per-column correction subtracted after the sum.
__global__ void project_reduce_kernel(const float* __restrict__ part, int nsplit, int64_t b,
                                      int64_t bpad, int kpw, int k, int kp, const float* __restrict__ corr,
                                      float* __restrict__ qpad, float* __restrict__ f_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= bpad * kp) return;
  const int64_t row = i / kp;
  const int c = (int)(i - row * kp);
  float s = 0.f;
  if (row < b && c < k)
  {
    for (int z = 0; z < nsplit; ++z) s += part[((int64_t)z * bpad + row) * kpw + c];
    if (corr) s -= corr[c];
  }
  qpad[i] = s;
  if (f_out && row < b && c < k) f_out[row * k + c] = s;
}

int project_nsplit(int64_t bpad, int64_t d, int kpw, int64_t* pix_per_split) {
  const int64_t mtiles = bpad / BM * (kpw > 128 ? kpw / 128 : 1);
  int64_t ns = (512 + mtiles - 1) / mtiles;  // ~2 workgroups per CU
  const int64_t steps = (d + BK - 1) / BK;
  if (ns > steps) ns = steps;
  if (ns < 1) ns = 1;
  if (ns > 64) ns = 64;
  const int64_t steps_per = (steps + ns - 1) / ns;
  *pix_per_split = steps_per * BK;
  return (int)((d + *pix_per_split - 1) / *pix_per_split);
}

template <int KPW, int PDT>
static hipError_t proj_t(hipStream_t s, const void* P, int64_t b, int64_t bpad, int64_t d,
                         const float* mean, const float* W, int ldw, float* part, int nsplit, int64_t pps) {
  const dim3 grid((unsigned)(bpad / BM), (unsigned)nsplit, (unsigned)(ldw / KPW));
  const bool vec = (d % 16 == 0) && ((reinterpret_cast<uintptr_t>(P) & 15) == 0) && (pps % 16 == 0);
  bool fast = PDT == EF_U8 && vec && d % BK == 0 && pps % BK == 0 && b >= 1;
#ifdef EF_DIAGNOSTICS  // EF_PROJ_FAST=0: the generic kernel (A/B)
  if (const char* e = getenv("EF_PROJ_FAST")) fast = fast && atoi(e) != 0;
#endif
  if (fast)
    hipLaunchKernelGGL((project_kernel<KPW, PDT, true, true>), grid, dim3(256), 0, s, P, b, d, mean, W, ldw, part,
                       bpad, pps);
  else if (vec)
    hipLaunchKernelGGL((project_kernel<KPW, PDT, true>), grid, dim3(256), 0, s, P, b, d, mean, W, ldw, part,
                       bpad, pps);
  else
    hipLaunchKernelGGL((project_kernel<KPW, PDT, false>), grid, dim3(256), 0, s, P, b, d, mean, W, ldw,
                       part, bpad, pps);
  return hipGetLastError();
}

hipError_t launch_project(hipStream_t s, int kpw, int p_dtype, const void* P, int64_t b,
                          int64_t bpad, int64_t d, const float* mean, const float* W, float* part,
                          int nsplit, int64_t pps) {
  if (kpw == 64)
    return p_dtype == EF_U8 ? proj_t<64, EF_U8>(s, P, b, bpad, d, mean, W, kpw, part, nsplit, pps)
                            : proj_t<64, EF_F32>(s, P, b, bpad, d, mean, W, kpw, part, nsplit, pps);
  if (kpw % 128 == 0)
    return p_dtype == EF_U8 ? proj_t<128, EF_U8>(s, P, b, bpad, d, mean, W, kpw, part, nsplit, pps)
                            : proj_t<128, EF_F32>(s, P, b, bpad, d, mean, W, kpw, part, nsplit, pps);
  return hipErrorInvalidValue;
}

hipError_t launch_project_reduce(hipStream_t s, const float* part, int nsplit, int64_t b,
                                 int64_t bpad, int kpw, int k, int kp, const float* corr, float* qpad,
                                 float* f_out) {
  const int64_t tot = bpad * kp;
  hipLaunchKernelGGL(project_reduce_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, part,
                     nsplit, b, bpad, kpw, k, kp, corr, qpad, f_out);
  return hipGetLastError();
}

}  // namespace ef
