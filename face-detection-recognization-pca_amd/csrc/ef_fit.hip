// ef_fit: the eigenfaces fit on the GPU (mean -> centre -> covariance -> eigensolve ->
// back-project -> unit eigenfaces -> training projection), float64 throughout.
//
// Restates manual_pca (useless/train.py:56-128) and, with EF_FIT_STANDARDIZE, the
// StandardScaler + PCA(svd_solver='full') fit of train-v4.py:126-146:
//   * covariance: Gram A.A^T/(n-1) when n < d (useless/train.py:82-85), else the d x d
//     A^T.A/(n-1) (np.cov branch, :97-99).  Exact integer products on the int8 matrix
//     cores (ef_cov_i8.hip) whenever the StandardScaler weights commute with them
//     (covariance path, and the Gram path without scaling); the standardised Gram runs
//     the f64 MFMA GEMM with centring and 1/scale applied in the operand loads;
//   * eigensolve: orders <= kJacobiMax go straight to the LDS Jacobi kernel, k > 80 on
//     orders <= 1024 to the grid-parallel Jacobi (ef_jacobi_big.hip); larger problems
//     run block subspace iteration (Y = C.Q; G = Y^T.Y; G = W.L.W^T by Jacobi;
//     Q = Y.W.L^-1/2) to convergence, then a Rayleigh-Ritz step (T = Q^T.C.Q, Jacobi)
//     — the top-k pairs are all manual_pca keeps (:114-116) and all sklearn reports
//     (explained_variance_ratio_ uses trace(C) as the total, _pca.py:644-646);
//   * eigenfaces: E = A^T.U (:91), unit columns (:94-95), sklearn svd_flip sign rule.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <vector>

#include "ef_fit_policy.hpp"
#include "ef_linalg.hpp"

namespace {

using namespace ef;

// Workspaces of one fit: slots of the context's pool (ef_ctx::fit_pool), grown on demand
// and kept for the next fit — a C3 fit otherwise spends tens of ms in hipMalloc/hipFree of
// its ~30 GB of operand copies and blocks.  ef_trim releases the pool.  Slots are indexed
// by position, so the order of the get calls is part of a fit's layout.
struct Bufs {
  size_t next = 0;
  template <class T>
  int get(ef_ctx* c, size_t count, T** out) {
    if (c->fit_pool.size() <= next) c->fit_pool.resize(next + 1);
    DevBuf& b = c->fit_pool[next++];
    const int rc = ensure(c, b, count * sizeof(T) + 16);
    *out = static_cast<T*>(b.p);
    return rc;
  }
};

// An input of `count` elements on the device: a device pointer passes through, a host
// array is copied into the pool's next slot.
template <class T>
int stage_in(ef_ctx* c, Bufs& B, bool dev, const T* src, size_t count, const char* what, const T** out) {
  *out = src;
  if (dev) return EF_OK;
  T* p;
  EF_TRY(B.get(c, count, &p));
  EF_HIP(c, hipMemcpyAsync(p, src, count * sizeof(T), hipMemcpyHostToDevice, c->stream), what);
  *out = p;
  return EF_OK;
}

// The outputs of one call: each (dst, src, bytes) with a destination is copied to the
// caller's memory (device or host), then one synchronise.  A null dst is an output the
// caller did not ask for (the entry points reject a missing required one before any work).
struct Out {
  void* dst;
  const void* src;
  size_t bytes;
  const char* what;
};
int copy_out(ef_ctx* c, bool dev, std::initializer_list<Out> outs) {
  const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  for (const Out& o : outs)
    if (o.dst) EF_HIP(c, hipMemcpyAsync(o.dst, o.src, o.bytes, kind, c->stream), o.what);
  EF_HIP(c, hipStreamSynchronize(c->stream), "sync");
  return EF_OK;
}

// The solver's tuning values: the defaults, or in the diagnostic build what the environment
// names.  Read once per eigensolve; the product library contains no getenv.
FitKnobs read_fit_knobs() {
  FitKnobs k;
#ifdef EF_DIAGNOSTICS
  auto num = [](const char* name, double* v) {
    if (const char* e = getenv(name)) *v = atof(e);
  };
  auto count = [](const char* name, int* v) {
    if (const char* e = getenv(name)) *v = atoi(e);
  };
  auto flag = [](const char* name, bool* v) {
    if (const char* e = getenv(name)) *v = atoi(e) != 0;
  };
  num("EF_FIT_RR_LOOSE", &k.rr_loose);
  num("EF_FIT_RR_FIRST", &k.rr_first);
  num("EF_FIT_RESID_TOL", &k.resid_tol);
  num("EF_FIT_GAP_TOL", &k.gap_tol);
  num("EF_FIT_COARSE_TOL", &k.coarse_tol);
  num("EF_FIT_COARSE_PRED", &k.coarse_pred);
  num("EF_FIT_GAP_MARGIN", &k.gap_margin);
  count("EF_FIT_EARLY", &k.early_rule);
  count("EF_FIT_M", &k.m);  // experiments only
  flag("EF_FIT_TN_TALL", &k.tn_tall);
  flag("EF_FIT_SHIFT", &k.shift);
  flag("EF_FIT_CQ_I8", &k.cq_i8);
  flag("EF_FIT_CQ_MED", &k.cq_med);
  flag("EF_FIT_SIDE", &k.side);
  flag("EF_FIT_DEFER", &k.defer);
  k.proj_f64 = getenv("EF_FIT_PROJ_F64") != nullptr;
  k.debug = getenv("EF_FIT_DEBUG") != nullptr;
#endif
  return k;
}

// Plain dense fp64 products of the subspace iteration with a large output (C.Q, Y.V, Q.V)
// run on the tall matrix-core GEMM (ef_dgemm.hip), which takes B transposed: B^T is
// written into bt_scratch (>= K x N doubles) first — at most dim x m, 32 MiB at C3, a few
// microseconds.  Products with a small output over a long K (Y^T.Y, Q^T.Y) and the
// pixel-operand products keep gemm64's split-K.
hipError_t dense_gemm(hipStream_t s, const Operand& A, const Operand& B, int64_t M, int64_t N, int64_t K, double alpha,
                      double* C, int64_t ldc, double* work, size_t work_elems, double* bt_scratch, bool tn_tall) {
  const bool small_out = M * N <= (int64_t)512 * 512 && K >= 4096;
  // Y^T.Y, Q^T.Y (small output, long K, A given transposed): B transposed once into
  // bt_scratch, then the register-direct tall kernel walking down A's rows with split-K —
  // the LDS-staged split-K gemm64 is latency-bound here (C3: 79 + 18 us per product).
  // A as stored: the tall kernel for every large output.
  const bool tall = A.trans ? tn_tall && small_out : !small_out;
  if (tall && bt_scratch && !B.trans && !A.u8 && !B.u8 && tall_gemm_supported(A.ld, A.p, 8) &&
      tall_gemm_supported(K, bt_scratch, 8)) {
    hipError_t e = launch_transpose_f64(s, B.p, B.ld, K, N, bt_scratch, K);
    if (e != hipSuccess) return e;
    return tall_gemm_f64(s, A.p, A.ld, A.trans != 0, bt_scratch, K, C, ldc, M, N, K, alpha, work, work_elems);
  }
  return gemm64(s, A, B, M, N, K, alpha, C, ldc, work, work_elems);
}

constexpr int kMaxSweeps = 60;
constexpr int kDirectMax = 1024;                 // direct grid-Jacobi up to this order
constexpr size_t kWorkElems = size_t(1) << 24;  // split-K slab budget (128 MiB)

// Small symmetric eigenproblem G (m x m) -> descending eigenvalues + eigenvectors:
// the LDS Jacobi up to kJacobiMax, the grid-parallel Jacobi beyond.
struct SmallEig {
  int m = 0;
  int* info = nullptr;
  double* jwork = nullptr;
  JacobiBig big;
  long sweeps = 0, calls = 0;  // grid-Jacobi statistics (EF_FIT_DEBUG)
  int init(ef_ctx* c, Bufs& B, int m_) {
    m = m_;
    EF_TRY(B.get(c, 4, &info));
    if (m > kJacobiMax) {
      EF_TRY(B.get(c, jacobi_big_work_elems(m), &jwork));
      EF_HIP(c, big.init(m, jwork, info, c->own_stream), "jacobi graph");
    }
    return EF_OK;
  }
  // tol: the block-Jacobi stopping tolerance (relative off-diagonal size); 1e-12 except
  // for Rayleigh-Ritz solves whose Ritz values cannot decide convergence (see below)
  int solve(ef_ctx* c, const double* G, int64_t ldg, double* lam, double* V, int64_t ldv, const char* what,
            double tol = 1e-12) {
    hipStream_t s = c->stream;
    if (m <= kJacobiMax) {
      EF_HIP(c, launch_jacobi(s, G, m, ldg, lam, V, ldv, kMaxSweeps, info), what);
      int hinfo = 0;
      EF_HIP(c, hipMemcpyAsync(&hinfo, info, sizeof(int), hipMemcpyDeviceToHost, s), "D2H info");
      EF_HIP(c, hipStreamSynchronize(s), "sync");
      if (hinfo < 0) return set_err(c, EF_E_NUMERIC, std::string(what) + ": Jacobi did not converge");
      return EF_OK;
    }
    hipError_t e = hipSuccess;
    int sw = 0;
    const int rc = big.solve(s, G, ldg, lam, V, ldv, kMaxSweeps, &sw, &e, tol);
    sweeps += sw;
    ++calls;
    if (rc < 0) return hip_err(c, e, what);
    if (rc > 0) return set_err(c, EF_E_NUMERIC, std::string(what) + ": Jacobi did not converge");
    return EF_OK;
  }
};

// Wide-block subspace iteration (m > kJacobiMax): orthonormalise by CholQR every
// iteration (G = Y^T.Y = L.L^T, Q = Y.L^-T — one small Cholesky instead of an m x m
// eigensolve), Rayleigh-Ritz (H = Q^T.C.Q, block Jacobi) at iterations (1, 2, 4,) 8 and every
// rr_period(dim) after: its Ritz values give the convergence test, its vectors re-order the
// block (Y <- Y.V), and the converged RR is the final one.  A numerically rank-deficient
// block (Cholesky pivot <= 1e-13 of the largest) falls back to the eigen-orthonormalisation
// Q = Y.W.L^-1/2 for that iteration.  The pieces: RitzPolicy (ef_fit_policy.hpp) holds the
// convergence and scheduling rules, BlockProduct the forms of Y = (C - sigma I).Q, WideBlock
// the block's workspaces with the orthonormalisation and the Rayleigh-Ritz step, and
// subspace_wide the loop over them.
constexpr int kCholeskyMax = 512;  // launch_cholesky's LDS panel limit (wider: eigen-orthonormalise)

__global__ void f64_to_f32_kernel(const double* __restrict__ a, int64_t n, float* __restrict__ b) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    b[i] = (float)a[i];
}
// Y (-)= sigma Q: the shifted product (C - sigma I) Q of the subspace iteration; the fp32
// coarse phase converts its product and shifts in one pass
__global__ void shift_kernel(double* __restrict__ y, const double* __restrict__ q, int64_t n, double sigma) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    y[i] = fma(-sigma, q[i], y[i]);
}
__global__ void f32_to_f64_shift_kernel(const float* __restrict__ a, const double* __restrict__ q, int64_t n,
                                        double sigma, double* __restrict__ b) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    b[i] = fma(-sigma, q[i], (double)a[i]);
}
// Deferred CholQR check: the fit's sticky failure flag |= this factor's info
__global__ void sticky_info_kernel(const int* __restrict__ info, int* __restrict__ sticky) {
  if (*info != 0) *sticky = 1;
}
// subspace_wide's "a deferred Cholesky failed: run again with a host check per iteration"
constexpr int kRetryChecked = 1000;

// Chebyshev step of the subspace iteration: y = s * y - w (w null: y = s * y)
__global__ void cheb_combine_kernel(double* __restrict__ y, const double* __restrict__ w, int64_t n, double sc) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    y[i] = w ? fma(sc, y[i], -w[i]) : sc * y[i];
}
// Ritz residuals of a Rayleigh-Ritz step: partial sums of |YV_i - lam_i U_i|^2 over row
// chunk blockIdx.y for columns 64 blockIdx.x + (tid & 63) (rows strided by the four
// 64-thread groups), YV = (C - sigma I) Q V and U = Q V; summed in chunk order on the host
// (deterministic).  part: [gridDim.y][kk].
constexpr int kResidChunks = 16;
__global__ __launch_bounds__(256) void ritz_resid_kernel(const double* __restrict__ YV, int64_t ldy,
                                                         const double* __restrict__ U, int64_t ldu,
                                                         const double* __restrict__ lam, int64_t dim, int kk,
                                                         double* __restrict__ part) {
  __shared__ double red[4][64];
  const int col = blockIdx.x * 64 + (threadIdx.x & 63), g = threadIdx.x >> 6;
  const int64_t r0 = dim * blockIdx.y / gridDim.y, r1 = dim * (blockIdx.y + 1) / gridDim.y;
  double acc = 0.0;
  if (col < kk) {
    const double l = lam[col];
    for (int64_t r = r0 + g; r < r1; r += 4) {
      const double d = fma(-l, U[r * ldu + col], YV[r * ldy + col]);
      acc = fma(d, d, acc);
    }
  }
  red[g][threadIdx.x & 63] = acc;
  __syncthreads();
  if (g == 0 && col < kk)
    part[(int64_t)blockIdx.y * kk + col] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) +
                                           red[3][threadIdx.x];
}

static void cvt64to32(hipStream_t s, const double* a, int64_t n, float* b) {
  hipLaunchKernelGGL(f64_to_f32_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 8192)), dim3(256), 0, s, a, n,
                     b);
}

// grid of the element-wise kernels over the dim x m block
inline unsigned ew_blocks(int64_t n) { return (unsigned)std::min<int64_t>((n + 255) / 256, 8192); }

// Y = (C - sigma I).Q in the form the problem and the phase allow, with what only the
// products need: the reduced-precision copy of C and the int8 digit planes.
//
// Coarse phase in fp32: while the Ritz values still move by > 1e-4 between Rayleigh-Ritz
// steps, Y = C.Q runs as an fp32 sgemm on an fp32 copy of C (twice the fp64 matrix
// rate); the iteration is self-correcting, and convergence is only declared between two
// Rayleigh-Ritz steps that both follow fp64 products, so the result is the fp64 one.
// Its products run on the split-bf16 matrix cores (ef_gemm_s3.hip: hi.hi' + hi.lo' +
// lo.hi', ~2^-17 relative per product, 16/3 x the fp32 rate) when the block is 256 wide
// (option value 1, the default), else — or with option value 2 — as fp32 MFMA GEMMs.
//
// Fine phase: fp64-accuracy products on the int8 matrix cores (launch_cq_i8, ef_cq_i8.hip:
// C and Q in base-256 digits, 21 exact digit-pair products) where the shape allows, else
// the fp64 dense product plus the shift kernel.
// C's digit planes are built on the fit's side stream while the coarse phase runs (its
// Jacobi rounds and small GEMMs leave most CUs idle); the first fine product waits for
// them.  The guard orders the main stream after the side work on every exit, so no
// later work (or a pool reallocation on the next fit) can overtake it.
struct BlockProduct {
  ef_ctx* c;
  hipStream_t s;
  const double* C;
  int64_t dim;
  int m;
  double *work, *Bt;  // the fit's split-K slabs and the block's B^T scratch (dense form)
  const FitKnobs& kn;
  bool coarse = false, coarse_s3 = false, cq_i8 = false, cq_ready = false;
  float *C32 = nullptr, *Q32 = nullptr, *Y32 = nullptr;
  uint8_t *cq_planes = nullptr, *cq_work = nullptr;
  SideJoin side_join;

  BlockProduct(ef_ctx* c_, const double* C_, int64_t dim_, int m_, double* work_, double* Bt_, const FitKnobs& kn_)
      : c(c_), s(c_->stream), C(C_), dim(dim_), m(m_), work(work_), Bt(Bt_), kn(kn_), side_join(c_->fit_side, c_->stream) {}

  // the pool slots after the block's, the copy of C, and the planes' side work started
  int init(Bufs& B) {
    coarse = dim >= 4096 && c->opt_fit_fp32_coarse != 0 && tall_gemm_supported(dim, C, 8);
    coarse_s3 = coarse && c->opt_fit_fp32_coarse == 1 && gemm_s3_supported(dim, dim, m);
    if (coarse) {
      EF_TRY(B.get(c, (size_t)dim * dim, &C32));  // fp32 C, or its split-bf16 copy (same bytes)
      EF_TRY(B.get(c, (size_t)dim * m, &Q32));    // Q^T in fp32 / split-bf16 (the GEMM's transposed B)
      EF_TRY(B.get(c, coarse_s3 ? gemm_s3_part_elems(dim) : (size_t)dim * m, &Y32));
      if (coarse_s3)
        EF_HIP(c, launch_split_f64(s, C, dim * dim, C32), "C (split-bf16)");
      else
        cvt64to32(s, C, dim * dim, C32);
    }
    cq_i8 = cq_i8_supported(dim, m) && tall_gemm_supported(dim, C, 8) && kn.cq_i8;
    if (cq_i8) {
      EF_TRY(B.get(c, cq_i8_plane_bytes(dim), &cq_planes));
      EF_TRY(B.get(c, cq_i8_work_bytes(dim, m), &cq_work));
    }
    if (cq_i8 && kn.side) {
      EF_HIP(c, side_join.fork(), "fit side stream (C ready)");
      EF_HIP(c, launch_cq_i8_planes(c->fit_side.s, C, dim, cq_planes), "C (int8 digit planes)");
      EF_HIP(c, side_join.done(), "planes ready");
    }
    return EF_OK;
  }

  // fine: the fp64-accuracy forms; medium: the int8 form with 15 digit pairs (RitzPolicy::medium)
  int apply(const double* Q, double sigma, bool fine, bool medium, double* Y) {
    if (!fine && coarse_s3) {
      EF_HIP(c, launch_transpose_split(s, Q, dim, Q32), "Q^T (split-bf16)");
      EF_HIP(c, gemm_s3(s, C32, dim, Q32, dim, dim, dim, Y32, Q, sigma, Y), "Y = C.Q (split-bf16)");
    } else if (!fine) {
      EF_HIP(c, launch_transpose_f64_to_f32(s, Q, m, dim, m, Q32, dim), "Q^T (fp32)");
      EF_HIP(c, tall_gemm_f32(s, C32, dim, false, Q32, dim, Y32, m, dim, m, dim, 1.f, reinterpret_cast<float*>(work),
                              kWorkElems * 2),
             "Y = C.Q (fp32)");
      hipLaunchKernelGGL(f32_to_f64_shift_kernel, dim3(ew_blocks(dim * m)), dim3(256), 0, s, Y32, Q, dim * m, sigma, Y);
    } else if (cq_i8) {
      if (!cq_ready) {
        if (kn.side) EF_HIP(c, side_join.join(), "planes ready");
        else EF_HIP(c, launch_cq_i8_planes(s, C, dim, cq_planes), "C (int8 digit planes)");
      }
      cq_ready = true;
      EF_HIP(c, launch_cq_i8(s, cq_planes, dim, Q, m, sigma, cq_work, Y, medium), "Y = C.Q (int8 digits)");
    } else {
      EF_HIP(c, dense_gemm(s, Operand::symmetric(C, dim), Operand::dense(Q, m, false), dim, m, dim, 1.0, Y, m, work,
                           kWorkElems, Bt, kn.tn_tall),
             "Y = C.Q");
      if (sigma != 0.0)
        hipLaunchKernelGGL(shift_kernel, dim3(ew_blocks(dim * m)), dim3(256), 0, s, Y, Q, dim * m, sigma);
    }
    return EF_OK;
  }
};

// The block of one wide solve: its pool slots, the orthonormalisation and the Rayleigh-Ritz step.
struct WideBlock {
  ef_ctx* c;
  hipStream_t s;
  int64_t dim;
  int kk, m;
  double* work;
  const FitKnobs& kn;
  bool defer = false;  // CholQR factors checked at the next Rayleigh-Ritz step (sticky)
  SmallEig se;
  // Pool slots, in the order they are taken.  Qold, Wc: the Chebyshev recurrence state
  // (EF_OPT_FIT_CHEBYSHEV): Qold = the block before the last orthonormalisation, Wc = the
  // previous filter iterate in the current block's frame.
  double *Li, *Bt, *Q, *Y, *Y2, *G, *V, *W2, *lam;
  int* cinfo;
  double* CW;  // blocked Cholesky + inverse scratch
  double* RP;  // Ritz residual partial sums [kResidChunks][kk]
  double *Qold, *Wc;
  int* sticky;  // deferred Cholesky failures since the fit began
  std::vector<double> th, rp, rnorm;  // host: raw Ritz values, residual partials, residual norms

  WideBlock(ef_ctx* c_, int64_t dim_, int kk_, int m_, double* work_, const FitKnobs& kn_)
      : c(c_), s(c_->stream), dim(dim_), kk(kk_), m(m_), work(work_), kn(kn_), th(m_),
        rp((size_t)kResidChunks * kk_), rnorm(kk_) {}

  int init(Bufs& B, bool deferred) {
    EF_TRY(se.init(c, B, m));
    EF_TRY(B.get(c, (size_t)m * m, &Li));
    EF_TRY(B.get(c, (size_t)dim * m, &Bt));
    EF_TRY(B.get(c, (size_t)dim * m, &Q));
    EF_TRY(B.get(c, (size_t)dim * m, &Y));
    EF_TRY(B.get(c, (size_t)dim * m, &Y2));
    EF_TRY(B.get(c, (size_t)m * m, &G));
    EF_TRY(B.get(c, (size_t)m * m, &V));
    EF_TRY(B.get(c, (size_t)m * m, &W2));
    EF_TRY(B.get(c, (size_t)m, &lam));
    EF_TRY(B.get(c, 4, &cinfo));
    EF_TRY(B.get(c, chol_inv_work_elems(m), &CW));
    EF_TRY(B.get(c, (size_t)kResidChunks * kk, &RP));
    EF_TRY(B.get(c, (size_t)dim * m, &Qold));
    EF_TRY(B.get(c, (size_t)dim * m, &Wc));
    EF_TRY(B.get(c, 4, &sticky));
    defer = deferred && chol_inv_supported(m);
    if (defer) EF_HIP(c, hipMemsetAsync(sticky, 0, sizeof(int), s), "sticky");
    return EF_OK;
  }

  hipError_t gemm(const Operand& A, const Operand& B, int64_t M, int64_t N, int64_t K, double* C, int64_t ldc) {
    return dense_gemm(s, A, B, M, N, K, 1.0, C, ldc, work, kWorkElems, Bt, kn.tn_tall);
  }

  // Q <- orthonormal basis of span(Y) (Y is overwritten).  carry: also map the block
  // being replaced into the new frame, Wc = Qold . L^-T (the same right factor), which is
  // what the three-term recurrence needs (*carried; the rank-deficient fallback
  // does not carry, and the recurrence restarts).
  int orthonormalise(bool carry, bool* carried) {
    *carried = false;
    if (carry) std::swap(Q, Qold);
    EF_HIP(c, gemm(Operand::dense(Y, m, true), Operand::dense(Y, m, false), m, m, dim, G, m), "G = Y^T.Y");
    int hinfo = -1;
    const bool fused = chol_inv_supported(m);  // blocked Cholesky + L^-1 (ef_chol_blk.hip)
    if (fused) {
      EF_HIP(c, launch_chol_inv(s, G, m, m, 1e-13, Li, cinfo, CW), "cholesky + L^-1");
    } else if (m <= kCholeskyMax) {
      EF_HIP(c, launch_cholesky(s, G, m, m, 1e-13, cinfo), "cholesky");
    }
    if (defer) {  // checked at the next Rayleigh-Ritz step (a failed factor leaves Li as it was)
      hipLaunchKernelGGL(sticky_info_kernel, dim3(1), dim3(1), 0, s, cinfo, sticky);
      hinfo = 0;
    } else if (fused || m <= kCholeskyMax) {
      EF_HIP(c, hipMemcpyAsync(&hinfo, cinfo, sizeof(int), hipMemcpyDeviceToHost, s), "D2H info");
      EF_HIP(c, hipStreamSynchronize(s), "sync");
    }
    if (hinfo == 0) {  // Q = Y . L^-T: explicit inverse of the m x m factor (it IS (L^-T)^T), one GEMM
      if (!fused) EF_HIP(c, launch_tri_inv(s, G, m, Li), "L^-1");
      // the tall kernel's 16-byte row rule always holds here: m is even (eig_topk) and the
      // blocks are pool slots
      EF_HIP(c, tall_gemm_f64(s, Y, m, false, Li, m, Q, m, dim, m, m, 1.0, work, kWorkElems), "Q = Y.L^-T");
      if (carry)
        EF_HIP(c, tall_gemm_f64(s, Qold, m, false, Li, m, Wc, m, dim, m, m, 1.0, work, kWorkElems), "W = Q'.L^-T");
      *carried = carry;
      return EF_OK;
    }
    // rank-deficient block: eigen-orthonormalisation with a floored spectrum
    EF_HIP(c, gemm(Operand::dense(Y, m, true), Operand::dense(Y, m, false), m, m, dim, G, m), "G = Y^T.Y");
    EF_TRY(se.solve(c, G, m, lam, V, m, "jacobi(G)"));
    EF_HIP(c, launch_scale_cols_rsqrt(s, V, m, m, lam, W2), "W.L^-1/2");
    EF_HIP(c, gemm(Operand::dense(Y, m, false), Operand::dense(W2, m, false), dim, m, m, Q, m), "Q = Y.W");
    return EF_OK;
  }

  // U (dim x kk) = Q.V, the Ritz vectors of the kept pairs
  int ritz_vectors(double* U) {
    EF_HIP(c, gemm(Operand::dense(Q, m, false), Operand::dense(V, m, false), dim, kk, m, U, kk), "U = Q.V");
    return EF_OK;
  }
  // Y2 = Y.V = C.(Q.V): the product the iteration continues from
  int continuation() {
    EF_HIP(c, gemm(Operand::dense(Y, m, false), Operand::dense(V, m, false), dim, m, m, Y2, m), "Y.V");
    return EF_OK;
  }

  // One Rayleigh-Ritz step on Y = (C - sigma I).Q: H = Q^T.Y, its eigenpairs (lam, V), and
  // what the policy makes of them.  *formed: the step needed the residuals, so Y2 = Y.V and
  // U = Q.V exist already.
  int rr_step(RitzPolicy& pol, int it, double* U, RitzStep* st, bool* formed) {
    EF_HIP(c, gemm(Operand::dense(Q, m, true), Operand::dense(Y, m, false), m, m, dim, G, m), "H = Q^T.C.Q");
    EF_TRY(se.solve(c, G, m, lam, V, m, "jacobi(H)", pol.jacobi_tol()));
    // Ritz residuals |C u_i - theta_i u_i| of the kept pairs after an fp64 product: YV = Y.V
    // is the continuation product anyway, U = Q.V the result's
    const bool resid = pol.wants_resid();
    if (resid) {
      EF_TRY(continuation());
      EF_TRY(ritz_vectors(U));
      hipLaunchKernelGGL(ritz_resid_kernel, dim3((unsigned)((kk + 63) / 64), kResidChunks), dim3(256), 0, s, Y2,
                         (int64_t)m, U, (int64_t)kk, lam, dim, kk, RP);
      EF_HIP(c, hipMemcpyAsync(rp.data(), RP, rp.size() * sizeof(double), hipMemcpyDeviceToHost, s), "D2H resid");
    }
    EF_HIP(c, hipMemcpyAsync(th.data(), lam, m * sizeof(double), hipMemcpyDeviceToHost, s), "D2H lam");
    EF_HIP(c, hipStreamSynchronize(s), "sync");
    if (resid)
      for (int i = 0; i < kk; ++i) {
        double a = 0.0;
        for (int q = 0; q < kResidChunks; ++q) a += rp[(size_t)q * kk + i];
        rnorm[i] = std::sqrt(a);
      }
#ifdef EF_DIAGNOSTICS
    const bool fine = pol.fine();
#endif
    *st = pol.step(it, th.data(), resid ? rnorm.data() : nullptr);
    *formed = resid;
    if (st->diverged) return set_err(c, EF_E_NUMERIC, "subspace iteration diverged");
#ifdef EF_DIAGNOSTICS
    if (kn.debug)
      fprintf(stderr,
              "[ef_fit] rr it=%d %s sweeps_total=%ld worst_rel=%.3e at %d theta_k=%.6g theta_m=%.6g resid=%.3e "
              "r/gap=%.3e at %d ok=%d\n",
              it, fine ? "fp64" : "fp32", se.sweeps, st->worst, st->worst_i, pol.theta()[kk - 1], pol.theta()[m - 1],
              st->resid_max, st->gap_worst, st->gap_i, (int)st->accepted);
#endif
    return EF_OK;
  }
};

// deferred: the per-iteration Cholesky success check is made at the next Rayleigh-Ritz
// step instead of by a host round trip every iteration; a failure found there returns
// kRetryChecked (the caller runs the checked form, which takes the rank-deficient fallback
// in the iteration that needs it).
int subspace_wide(ef_ctx* c, Bufs& B, const FitKnobs& kn, const double* C, int64_t dim, int kk, int m, double* work,
                  double* U_out, double* lam_out, int* iters, bool deferred) {
  hipStream_t s = c->stream;
  WideBlock w(c, dim, kk, m, work, kn);
  EF_TRY(w.init(B, deferred));
  EF_HIP(c, launch_rand_init(s, w.Y, dim * m, 0x5eedULL), "rand init");
  bool carried = false;
  EF_TRY(w.orthonormalise(false, &carried));
  BlockProduct prod(c, C, dim, m, work, w.Bt, kn);
  EF_TRY(prod.init(B));

  const bool cheb_on = c->opt_fit_chebyshev != 0;
  const int max_iters = (int)std::max<int64_t>(1, std::min<int64_t>(c->opt_fit_max_iters, 1 << 20));
  RitzPolicy pol(dim, kk, m, max_iters, cheb_on, kn.shift, prod.coarse, kn);
  int cheb_j = 0;  // recurrence steps since the last restart (Wc valid when > 0)
  bool converged = false;
  int it = 0;
  for (it = 1; it <= max_iters; ++it) {
    const double sig_it = pol.sigma;  // the shift this iteration's product carries
    EF_TRY(prod.apply(w.Q, sig_it, pol.fine(), pol.medium(it), w.Y));
    bool restarted = false;
    if (pol.rr_due(it)) {
      if (w.defer) {  // the deferred Cholesky checks, before anything reads this block
        int hs = 0;
        EF_HIP(c, hipMemcpyAsync(&hs, w.sticky, sizeof(int), hipMemcpyDeviceToHost, s), "D2H sticky");
        EF_HIP(c, hipStreamSynchronize(s), "sync");
        if (hs != 0) return kRetryChecked;
      }
      RitzStep st;
      bool formed = false;  // Y2 = Y.V and U_out = Q.V (the residual check forms both)
      EF_TRY(w.rr_step(pol, it, U_out, &st, &formed));
      converged = st.accepted;
      // the iteration cap ends the loop with EF_E_NUMERIC (useless/train.py has no cap:
      // LAPACK either converges or raises LinAlgError; train-v4.py:114-120 returns False)
      if (converged || it == max_iters) {
        if (!formed) EF_TRY(w.ritz_vectors(U_out));
        EF_HIP(c, hipMemcpyAsync(lam_out, pol.theta().data(), kk * sizeof(double), hipMemcpyHostToDevice, s), "lam");
        EF_HIP(c, hipStreamSynchronize(s), "sync");
        break;
      }
      // continue from the Ritz basis: C.(Q.V) = Y.V (and restart the recurrence there)
      if (!formed) EF_TRY(w.continuation());
      std::swap(w.Y, w.Y2);
      restarted = true;
    }
    if (cheb_on && sig_it > 0.0 && !restarted) {
      // X_1 = A~ X_0, X_{j+1} = 2 A~ X_j - X_{j-1}; Y holds (C - sigma I) Q, Wc the carried X_{j-1}
      hipLaunchKernelGGL(cheb_combine_kernel, dim3(ew_blocks(dim * m)), dim3(256), 0, s, w.Y,
                         cheb_j > 0 ? w.Wc : nullptr, dim * m, (cheb_j > 0 ? 2.0 : 1.0) / sig_it);
      EF_TRY(w.orthonormalise(true, &carried));
      cheb_j = carried ? cheb_j + 1 : 0;
    } else {
      EF_TRY(w.orthonormalise(false, &carried));
      cheb_j = 0;
    }
  }
  if (it > max_iters) it = max_iters;
#ifdef EF_DIAGNOSTICS
  if (kn.debug)
    fprintf(stderr, "[ef_fit] wide dim=%lld k=%d m=%d iters=%d jacobi calls=%ld sweeps=%ld\n", (long long)dim, kk, m,
            it, w.se.calls, w.se.sweeps);
#endif
  *iters = it;
  if (!converged) {
    char msg[160];
    snprintf(msg, sizeof msg,
             "eigensolver did not converge: %d subspace iterations, Ritz values still moving by %.3e (relative)",
             it, pol.last_worst);
    return set_err(c, EF_E_NUMERIC, msg);
  }
  return EF_OK;
}

// Top-kk eigenpairs of the symmetric dim x dim matrix C (device, ld = dim).
// U_out: dim x kk (row-major, ld kk), lam_out: kk (device).  iters: host.
int eig_topk(ef_ctx* c, Bufs& B, const FitKnobs& kn, const double* C, int64_t dim, int kk, double* work, double* U_out,
             double* lam_out, int* iters) {
  hipStream_t s = c->stream;
  if (dim <= kJacobiMax || (kk > kJacobiMax - 8 && dim <= kDirectMax)) {  // direct
    SmallEig se;
    EF_TRY(se.init(c, B, (int)dim));
    double *ev, *V;
    EF_TRY(B.get(c, (size_t)dim, &ev));
    EF_TRY(B.get(c, (size_t)dim * dim, &V));
    EF_TRY(se.solve(c, C, dim, ev, V, dim, "eigensolve"));
    EF_HIP(c, hipMemcpy2DAsync(U_out, kk * sizeof(double), V, dim * sizeof(double), kk * sizeof(double), dim,
                               hipMemcpyDeviceToDevice, s),
           "copy U");
    EF_HIP(c, hipMemcpyAsync(lam_out, ev, kk * sizeof(double), hipMemcpyDeviceToDevice, s), "copy lam");
    EF_HIP(c, hipStreamSynchronize(s), "sync");
    *iters = 0;
    return EF_OK;
  }

  // Block width m = max(2k, 88) (Ritz values converge as (lambda_{m+1} / lambda_k)^2 per
  // iteration), even, <= dim: CholQR subspace iteration with periodic Rayleigh-Ritz.
  int64_t mm = std::max<int64_t>(2 * (int64_t)kk, kJacobiMax);
  mm = (mm + 7) / 8 * 8;
  if (mm > dim) mm = dim & ~int64_t(1);
  int m = (int)mm;
  if (kn.m >= kk + 2 && kn.m <= dim) m = kn.m & ~1;
  const size_t mark = B.next;  // a checked rerun reuses the same pool slots
  int rc = subspace_wide(c, B, kn, C, dim, kk, m, work, U_out, lam_out, iters, kn.defer);
  if (rc == kRetryChecked) {
    B.next = mark;
    rc = subspace_wide(c, B, kn, C, dim, kk, m, work, U_out, lam_out, iters, false);
  }
  return rc;
}

// Numerically null components.  With k = n (train-v5.py:540-545 sets n_components to the
// face count) the centred data has rank n - 1 and the last eigenvalue is rounding noise:
// the Gram path's back-projection A^T.u of its eigenvector is itself rounding noise, and
// normalising it would give an arbitrary direction with large projections.  In exact
// arithmetic any unit vector orthogonal to the data span is a valid component (sklearn's
// full SVD returns LAPACK's choice); this takes a fixed one: a seeded vector, made
// orthogonal (two Gram-Schmidt passes) to every other component, unit length, svd_flip
// sign rule.  Rare and small (k x d), so on the host.
int complete_null_components(ef_ctx* c, int64_t n, int64_t d, int kk, const double* lam_dev, double* comps_dev,
                             double* En_dev) {
  hipStream_t s = c->stream;
  std::vector<double> lam(kk);
  EF_HIP(c, hipMemcpyAsync(lam.data(), lam_dev, kk * sizeof(double), hipMemcpyDeviceToHost, s), "D2H lam");
  EF_HIP(c, hipStreamSynchronize(s), "sync");
  const double tol = 1e-14 * (double)std::max(n, d) * std::fabs(lam[0]);
  std::vector<int> null_cols;
  for (int j = 0; j < kk; ++j)
    if (!(lam[j] > tol)) null_cols.push_back(j);
  if (null_cols.empty() || (int)null_cols.size() == kk) return EF_OK;
  std::vector<double> C((size_t)kk * d);
  EF_HIP(c, hipMemcpyAsync(C.data(), comps_dev, C.size() * sizeof(double), hipMemcpyDeviceToHost, s), "D2H comps");
  EF_HIP(c, hipStreamSynchronize(s), "sync");
  std::vector<char> done(kk, 0);
  for (int j = 0; j < kk; ++j) done[j] = lam[j] > tol;
  unsigned long long st = 0x9e3779b97f4a7c15ULL;
  for (int j : null_cols) {
    double* v = &C[(size_t)j * d];
    for (int64_t i = 0; i < d; ++i) {  // splitmix64 -> uniform(-1, 1)
      st += 0x9e3779b97f4a7c15ULL;
      unsigned long long z = st;
      z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
      z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
      z ^= z >> 31;
      v[i] = (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0;
    }
    for (int pass = 0; pass < 2; ++pass)
      for (int q = 0; q < kk; ++q) {
        if (!done[q]) continue;
        const double* u = &C[(size_t)q * d];
        double dot = 0.0;
        for (int64_t i = 0; i < d; ++i) dot += u[i] * v[i];
        for (int64_t i = 0; i < d; ++i) v[i] -= dot * u[i];
      }
    double nrm = 0.0, mx = -1.0;
    int64_t mi = 0;
    for (int64_t i = 0; i < d; ++i) {
      nrm += v[i] * v[i];
      if (std::fabs(v[i]) > mx) mx = std::fabs(v[i]), mi = i;
    }
    const double f = (v[mi] < 0 ? -1.0 : 1.0) / std::sqrt(nrm);
    for (int64_t i = 0; i < d; ++i) v[i] *= f;
    done[j] = 1;
  }
  std::vector<double> T((size_t)d * kk);
  for (int j = 0; j < kk; ++j)
    for (int64_t i = 0; i < d; ++i) T[(size_t)i * kk + j] = C[(size_t)j * d + i];
  EF_HIP(c, hipMemcpyAsync(comps_dev, C.data(), C.size() * sizeof(double), hipMemcpyHostToDevice, s), "H2D comps");
  EF_HIP(c, hipMemcpyAsync(En_dev, T.data(), T.size() * sizeof(double), hipMemcpyHostToDevice, s), "H2D En");
  EF_HIP(c, hipStreamSynchronize(s), "sync");
  return EF_OK;
}

// What ef_fit_ex and ef_fit_from_stats share once the covariance C (dim x dim) stands: the
// model's pool slots and everything from the trace to the outputs.  One copy, so the
// sharded fit equals the single fit on the same C by construction.
struct FitModel {
  double *mean, *var, *scale, *w, *C, *work, *U, *lam, *comps, *En, *tv;
  int iters = 0;

  int take(ef_ctx* c, Bufs& B, int64_t d, int64_t dim, int kk) {
    EF_TRY(B.get(c, (size_t)d, &mean));
    EF_TRY(B.get(c, (size_t)d, &var));
    EF_TRY(B.get(c, (size_t)d, &scale));
    EF_TRY(B.get(c, (size_t)d, &w));
    EF_TRY(B.get(c, (size_t)dim * dim, &C));
    EF_TRY(B.get(c, kWorkElems, &work));
    EF_TRY(B.get(c, (size_t)dim * kk, &U));
    EF_TRY(B.get(c, (size_t)kk, &lam));
    EF_TRY(B.get(c, (size_t)kk * d, &comps));
    EF_TRY(B.get(c, (size_t)d * kk, &En));
    EF_TRY(B.get(c, 1, &tv));
    return EF_OK;
  }

  // trace -> top-kk eigenpairs -> unit components with the sign rule -> null components.
  // At: the Gram path's pixel operand A^T (d x n), whose product with U back-projects the
  // eigenvectors (E = A^T.U); null on the covariance path, where U holds them already.
  int components(ef_ctx* c, Bufs& B, const FitKnobs& kn, int64_t n, int64_t d, int64_t dim, int kk, const Operand* At) {
    hipStream_t s = c->stream;
    EF_HIP(c, launch_trace(s, C, dim, dim, tv), "trace");
    EF_TRY(eig_topk(c, B, kn, C, dim, kk, work, U, lam, &iters));
    const double* E = U;
    if (At) {
      double* Eb;
      EF_TRY(B.get(c, (size_t)d * kk, &Eb));
      EF_HIP(c, gemm64(s, *At, Operand::dense(U, kk, false), d, kk, n, 1.0, Eb, kk, work, kWorkElems), "E = A^T.U");
      E = Eb;
    }
    EF_HIP(c, launch_normalize_sign(s, E, d, kk, kk, comps, En), "normalize");
    return complete_null_components(c, n, d, kk, lam, comps, En);
  }

  // proj: the n x kk training projection, or null
  int outputs(ef_ctx* c, bool dev, int64_t n, int64_t d, int kk, const double* proj, double* mean_out, double* var_out,
              double* scale_out, double* comps_out, double* eig_out, double* proj_out, double* tv_out, int32_t* k_out,
              int32_t* iters_out) {
    EF_TRY(copy_out(c, dev, {{mean_out, mean, d * sizeof(double), "out mean"},
                             {var_out, var, d * sizeof(double), "out var"},
                             {scale_out, scale, d * sizeof(double), "out scale"},
                             {comps_out, comps, (size_t)kk * d * sizeof(double), "out comps"},
                             {eig_out, lam, kk * sizeof(double), "out eig"},
                             {proj ? proj_out : nullptr, proj, (size_t)n * kk * sizeof(double), "out proj"},
                             {tv_out, tv, sizeof(double), "out tv"}}));
    if (k_out) *k_out = kk;
    if (iters_out) *iters_out = iters;
    return EF_OK;
  }
};

}  // namespace

extern "C" int ef_fit_ex(ef_ctx* c, const void* Xv, int32_t x_dtype, int64_t n, int64_t d, int32_t k,
                         uint32_t flags, double* mean_out, double* var_out, double* scale_out, double* comps_out,
                         double* eig_out, double* proj_out, double* tv_out, int32_t* k_out, int32_t* iters_out) {
  if (!c) return EF_E_INVALID;
  if (!Xv || n < 2 || d < 1 || k < 1 || !mean_out || !comps_out || !eig_out)
    return set_err(c, EF_E_INVALID, "ef_fit: bad arguments (need X, n >= 2, d >= 1, k >= 1, outputs)");
  if (x_dtype != EF_U8 && x_dtype != EF_F32 && x_dtype != EF_F64)
    return set_err(c, EF_E_INVALID, "ef_fit: x_dtype must be EF_U8, EF_F32 or EF_F64");
  const bool u8 = x_dtype == EF_U8;
  const size_t esize = u8 ? 1 : (x_dtype == EF_F32 ? 4 : 8);
  (void)hipSetDevice(c->device);
  hipStream_t s = c->stream;
  const bool dev = flags & EF_MEM_DEVICE;
  const bool stdz = flags & EF_FIT_STANDARDIZE;
  const bool gram = n < d;
  const int64_t dim = gram ? n : d;
  const int kk = (int)(k < dim ? k : dim);
  const FitKnobs kn = read_fit_knobs();

  Bufs B;
  // uint8 pixels take the exact integer kernels; float input the fp64 loaders
  const uint8_t* Xb;
  EF_TRY(stage_in(c, B, dev, static_cast<const uint8_t*>(Xv), (size_t)n * d * esize, "H2D X", &Xb));
  const void* Xdv = Xb;
  const uint8_t* Xd = u8 ? Xb : nullptr;
  auto pix = [&](bool trans, const double* mu, const double* wv) {
    return Operand::pixels(Xdv, x_dtype, d, trans, mu, wv);
  };
  unsigned long long *S1, *S2;
  FitModel f;
  EF_TRY(B.get(c, (size_t)d, &S1));
  EF_TRY(B.get(c, (size_t)d, &S2));
  EF_TRY(f.take(c, B, d, dim, kk));

  // K1: exact column statistics -> mean / var / scale / centring weights.  On the int8
  // covariance path the operand transpose produces the sums in the same pass over X.
  const double inv = 1.0 / (double)(n - 1);
  const bool int8_path = u8 && (!gram || !stdz);
  uint8_t* At = nullptr;
  if (u8) {
    EF_HIP(c, hipMemsetAsync(S1, 0, d * sizeof(unsigned long long), s), "memset");
    EF_HIP(c, hipMemsetAsync(S2, 0, d * sizeof(unsigned long long), s), "memset");
    const bool fused = int8_path && !gram && cov_i8_fused_stats(Xd, d);
    if (int8_path) {
      EF_TRY(B.get(c, (size_t)dim * cov_i8_kpad(gram ? d : n) + kSyrkPadBytes, &At));
      EF_HIP(c, launch_cov_i8_prep(s, Xd, n, d, gram, At, fused ? S1 : nullptr, fused ? S2 : nullptr), "cov prep");
    }
    if (!fused) EF_HIP(c, launch_colstats(s, Xd, n, d, S1, S2), "colstats");
    EF_HIP(c, launch_stats_finalize(s, S1, S2, n, d, stdz ? 1 : 0, f.mean, f.var, f.scale, f.w), "stats");
  } else {
    double* part;
    EF_TRY(B.get(c, colstats_float_work_elems(n, d), &part));
    EF_HIP(c, launch_colstats_float(s, Xdv, x_dtype, n, d, stdz ? 1 : 0, part, f.mean, f.var, f.scale, f.w),
           "colstats (float)");
  }
  const double* wp = stdz ? f.w : nullptr;

  // K2+K3: covariance.  Exact integer product on the int8 matrix cores whenever the
  // pixel scaling commutes with it (covariance path; Gram path without StandardScaler),
  // else the fp64 GEMM with the centring/scaling fused into the operand loads.
  if (int8_path) {
    const CovPlan plan = cov_i8_plan(dim, gram ? d : n, c->opt_cov_slab_bytes);
    int* slabs;
    long long *S64 = nullptr, *cvec, *R;
    unsigned long long* Q2;
    EF_TRY(B.get(c, (size_t)plan.slab_elems, &slabs));
    if (plan.passes > 1) EF_TRY(B.get(c, (size_t)dim * dim, &S64));
    EF_TRY(B.get(c, (size_t)d, &cvec));
    EF_TRY(B.get(c, (size_t)(gram ? n : 1), &R));
    EF_TRY(B.get(c, 2, &Q2));
    uint8_t* order;
    EF_TRY(B.get(c, (size_t)cov_i8_order_bytes(dim), &order));
    TimerEvt tev;
    timer_arm(c, EF_KERNEL_SYRK, &tev);
    const hipError_t ecov = launch_cov_i8(s, plan, n, d, gram, S1, wp, At, slabs, S64, cvec, R, Q2, order, f.C,
                                          tev.kernel >= 0 ? tev.a : nullptr, tev.kernel >= 0 ? tev.b : nullptr);
    timer_commit(c, &tev);  // (the drain skips a pair whose end was never recorded)
    EF_HIP(c, ecov, "covariance (int8)");
  } else if (gram)
    EF_HIP(c, gemm64(s, pix(false, f.mean, wp), pix(true, f.mean, wp), n, n, d, inv, f.C, n, f.work, kWorkElems),
           "Gram");
  else
    EF_HIP(c, gemm64(s, pix(true, f.mean, wp), pix(false, f.mean, wp), d, d, n, inv, f.C, d, f.work, kWorkElems),
           "covariance");

  // K4 + K5: top-kk eigenpairs, back-projection (Gram path), unit columns + sign rule
  Operand back;
  if (gram) back = pix(true, f.mean, wp);
  EF_TRY(f.components(c, B, kn, n, d, dim, kk, gram ? &back : nullptr));
  // training projection A.E (projected_data / fit_transform output)
  double* proj = nullptr;
  if (proj_out) {
    EF_TRY(B.get(c, (size_t)n * kk, &proj));
    if (u8 && proj_i8_supported(Xd, n, d, kk) && !kn.proj_f64) {  // exact int8 digits (ef_proj_i8.hip)
      uint8_t* pw;
      EF_TRY(B.get(c, proj_i8_work_bytes(n, d, kk), &pw));
      EF_HIP(c, launch_proj_i8(s, Xd, n, d, f.mean, wp, f.En, kk, pw, proj), "F = A.E (int8 digits)");
    } else {
      EF_HIP(c, gemm64(s, pix(false, f.mean, wp), Operand::dense(f.En, kk, false), n, kk, d, 1.0, proj, kk, f.work,
                       kWorkElems),
             "F = A.E");
    }
  }
  return f.outputs(c, dev, n, d, kk, proj, mean_out, var_out, scale_out, comps_out, eig_out, proj_out, tv_out, k_out,
                   iters_out);
}

extern "C" int ef_fit(ef_ctx* c, const uint8_t* X, int64_t n, int64_t d, int32_t k, uint32_t flags,
                      double* mean_out, double* var_out, double* scale_out, double* comps_out,
                      double* eig_out, double* proj_out, double* tv_out, int32_t* k_out, int32_t* iters_out) {
  return ef_fit_ex(c, X, EF_U8, n, d, k, flags, mean_out, var_out, scale_out, comps_out, eig_out, proj_out, tv_out,
                   k_out, iters_out);
}

// ---------------------------------------------------------------- sample-sharded fit
// SURVEY.md §8(e), the fit collective: rank r holds rows X_r; the exact integer pieces
// (column sums of x and x^2, X'_r^T X'_r) of every rank add up to the pieces of the whole
// set, so after a sum over ranks the covariance, and everything computed from it, equals
// ef_fit's on the concatenated rows bit for bit (covariance path: n_total >= d).
extern "C" int ef_fit_shard_stats(ef_ctx* c, const uint8_t* X, int64_t n, int64_t d, uint64_t* sum_out,
                                  uint64_t* sumsq_out, int64_t* cross_out, uint32_t flags) {
  if (!c) return EF_E_INVALID;
  if ((!X && n > 0) || n < 0 || d < 1 || !sum_out || !sumsq_out || !cross_out)
    return set_err(c, EF_E_INVALID, "ef_fit_shard_stats: bad arguments (need X, n >= 0, d >= 1, outputs)");
  (void)hipSetDevice(c->device);
  hipStream_t s = c->stream;
  const bool dev = flags & EF_MEM_DEVICE;
  Bufs B;
  unsigned long long *S1, *S2;
  long long* S64;
  EF_TRY(B.get(c, (size_t)d, &S1));
  EF_TRY(B.get(c, (size_t)d, &S2));
  if (dev) {
    S64 = reinterpret_cast<long long*>(cross_out);
  } else {
    EF_TRY(B.get(c, (size_t)d * d, &S64));
  }
  EF_HIP(c, hipMemsetAsync(S1, 0, d * sizeof(unsigned long long), s), "memset");
  EF_HIP(c, hipMemsetAsync(S2, 0, d * sizeof(unsigned long long), s), "memset");
  if (n == 0) {  // an empty shard contributes nothing
    EF_HIP(c, hipMemsetAsync(S64, 0, (size_t)d * d * sizeof(long long), s), "memset");
  } else {
    const uint8_t* Xd;
    EF_TRY(stage_in(c, B, dev, X, (size_t)n * d, "H2D X", &Xd));
    uint8_t* At;
    EF_TRY(B.get(c, (size_t)d * cov_i8_kpad(n) + kSyrkPadBytes, &At));
    const bool fused = cov_i8_fused_stats(Xd, d);
    EF_HIP(c, launch_cov_i8_prep(s, Xd, n, d, false, At, fused ? S1 : nullptr, fused ? S2 : nullptr), "cov prep");
    if (!fused) EF_HIP(c, launch_colstats(s, Xd, n, d, S1, S2), "colstats");
    const CovPlan plan = cov_i8_plan(d, n, c->opt_cov_slab_bytes);
    int* slabs;
    uint8_t* order;
    EF_TRY(B.get(c, (size_t)plan.slab_elems, &slabs));
    EF_TRY(B.get(c, (size_t)cov_i8_order_bytes(d), &order));
    EF_HIP(c, launch_cov_i8_cross(s, plan, d, At, slabs, S64, order), "X'^T X' (int8)");
  }
  // (device memory: the cross products were formed in place)
  return copy_out(c, dev, {{sum_out, S1, d * sizeof(uint64_t), "out sum"},
                           {sumsq_out, S2, d * sizeof(uint64_t), "out sumsq"},
                           {dev ? nullptr : cross_out, S64, (size_t)d * d * sizeof(int64_t), "out cross"}});
}

extern "C" int ef_fit_from_stats(ef_ctx* c, const uint64_t* sum, const uint64_t* sumsq, const int64_t* cross,
                                 int64_t n_total, int64_t d, int32_t k, uint32_t flags, double* mean_out,
                                 double* var_out, double* scale_out, double* comps_out, double* eig_out, double* tv_out,
                                 int32_t* k_out, int32_t* iters_out) {
  if (!c) return EF_E_INVALID;
  if (!sum || !sumsq || !cross || d < 1 || k < 1 || !mean_out || !comps_out || !eig_out)
    return set_err(c, EF_E_INVALID, "ef_fit_from_stats: bad arguments (need the pieces, d >= 1, k >= 1, outputs)");
  if (n_total < 2 || n_total < d)
    return set_err(c, EF_E_INVALID, "ef_fit_from_stats: the sample-sharded fit is the covariance path (n_total >= d, "
                                    "n_total >= 2)");
  (void)hipSetDevice(c->device);
  hipStream_t s = c->stream;
  const bool dev = flags & EF_MEM_DEVICE;
  const bool stdz = flags & EF_FIT_STANDARDIZE;
  const int kk = (int)(k < d ? k : d);
  const FitKnobs kn = read_fit_knobs();
  Bufs B;
  const unsigned long long *S1, *S2;
  const long long* S64;
  EF_TRY(stage_in(c, B, dev, reinterpret_cast<const unsigned long long*>(sum), (size_t)d, "H2D sum", &S1));
  EF_TRY(stage_in(c, B, dev, reinterpret_cast<const unsigned long long*>(sumsq), (size_t)d, "H2D sumsq", &S2));
  EF_TRY(stage_in(c, B, dev, reinterpret_cast<const long long*>(cross), (size_t)d * d, "H2D cross", &S64));
  FitModel f;
  long long* cvec;
  EF_TRY(f.take(c, B, d, d, kk));
  EF_TRY(B.get(c, (size_t)d, &cvec));
  EF_HIP(c, launch_stats_finalize(s, S1, S2, n_total, d, stdz ? 1 : 0, f.mean, f.var, f.scale, f.w), "stats");
  EF_HIP(c, launch_cov_from_cross(s, S64, S1, n_total, d, stdz ? f.w : nullptr, cvec, f.C), "covariance (from pieces)");
  EF_TRY(f.components(c, B, kn, n_total, d, d, kk, nullptr));
  return f.outputs(c, dev, n_total, d, kk, nullptr, mean_out, var_out, scale_out, comps_out, eig_out, nullptr, tv_out,
                   k_out, iters_out);
}

namespace {
__global__ void recip_kernel(const double* __restrict__ a, int64_t n, double* __restrict__ b) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) b[i] = 1.0 / a[i];  // the division stats_finalize_kernel makes for w
}
}  // namespace

extern "C" int ef_fit_transform(ef_ctx* c, const uint8_t* X, int64_t n, int64_t d, const double* mean,
                                const double* scale, const double* comps, int32_t k, uint32_t flags, double* proj_out) {
  if (!c) return EF_E_INVALID;
  if (!X || n < 1 || d < 1 || k < 1 || !mean || !comps || !proj_out)
    return set_err(c, EF_E_INVALID, "ef_fit_transform: bad arguments (need X, n >= 1, d >= 1, k >= 1, model, out)");
  (void)hipSetDevice(c->device);
  hipStream_t s = c->stream;
  const bool dev = flags & EF_MEM_DEVICE;
  Bufs B;
  const uint8_t* Xd;
  const double *mu, *sc = nullptr, *cp;
  EF_TRY(stage_in(c, B, dev, X, (size_t)n * d, "H2D X", &Xd));
  EF_TRY(stage_in(c, B, dev, mean, (size_t)d, "H2D mean", &mu));
  EF_TRY(stage_in(c, B, dev, comps, (size_t)k * d, "H2D comps", &cp));
  if (scale) EF_TRY(stage_in(c, B, dev, scale, (size_t)d, "H2D scale", &sc));
  double *w = nullptr, *En, *proj, *work;
  if (sc) {
    EF_TRY(B.get(c, (size_t)d, &w));
    hipLaunchKernelGGL(recip_kernel, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, s, sc, d, w);
  }
  EF_TRY(B.get(c, (size_t)d * k, &En));
  EF_TRY(B.get(c, (size_t)n * k, &proj));
  EF_TRY(B.get(c, kWorkElems, &work));
  EF_HIP(c, launch_transpose_f64(s, cp, d, k, d, En, k), "E = comps^T");
  if (proj_i8_supported(Xd, n, d, k)) {
    uint8_t* pw;
    EF_TRY(B.get(c, proj_i8_work_bytes(n, d, k), &pw));
    EF_HIP(c, launch_proj_i8(s, Xd, n, d, mu, w, En, k, pw, proj), "F = A.E (int8 digits)");
  } else {
    EF_HIP(c, gemm64(s, Operand::pixels(Xd, EF_U8, d, false, mu, w), Operand::dense(En, k, false), n, k, d, 1.0, proj,
                     k, work, kWorkElems),
           "F = A.E");
  }
  return copy_out(c, dev, {{proj_out, proj, (size_t)n * k * sizeof(double), "out proj"}});
}

// Column statistics alone (ManualStandardScaler.fit, scripts/manual/train-v2.py:58-64, and
// StandardScaler.fit): exact integer sums for uint8, two-pass fp64 for float input.
extern "C" int ef_colstats(ef_ctx* c, const void* Xv, int32_t x_dtype, int64_t n, int64_t d, uint32_t flags,
                           double* mean_out, double* var_out) {
  if (!c) return EF_E_INVALID;
  if (!Xv || n < 1 || d < 1 || !mean_out)
    return set_err(c, EF_E_INVALID, "ef_colstats: bad arguments (need X, n >= 1, d >= 1, mean_out)");
  if (x_dtype != EF_U8 && x_dtype != EF_F32 && x_dtype != EF_F64)
    return set_err(c, EF_E_INVALID, "ef_colstats: x_dtype must be EF_U8, EF_F32 or EF_F64");
  (void)hipSetDevice(c->device);
  hipStream_t s = c->stream;
  const bool dev = flags & EF_MEM_DEVICE;
  const size_t esize = x_dtype == EF_U8 ? 1 : (x_dtype == EF_F32 ? 4 : 8);
  Bufs B;
  const uint8_t* Xb;
  EF_TRY(stage_in(c, B, dev, static_cast<const uint8_t*>(Xv), (size_t)n * d * esize, "H2D X", &Xb));
  double *mean, *var, *scale, *w;
  EF_TRY(B.get(c, (size_t)d, &mean));
  EF_TRY(B.get(c, (size_t)d, &var));
  EF_TRY(B.get(c, (size_t)d, &scale));
  EF_TRY(B.get(c, (size_t)d, &w));
  if (x_dtype == EF_U8) {
    unsigned long long *S1, *S2;
    EF_TRY(B.get(c, (size_t)d, &S1));
    EF_TRY(B.get(c, (size_t)d, &S2));
    EF_HIP(c, hipMemsetAsync(S1, 0, d * sizeof(unsigned long long), s), "memset");
    EF_HIP(c, hipMemsetAsync(S2, 0, d * sizeof(unsigned long long), s), "memset");
    EF_HIP(c, launch_colstats(s, Xb, n, d, S1, S2), "colstats");
    EF_HIP(c, launch_stats_finalize(s, S1, S2, n, d, 0, mean, var, scale, w), "stats");
  } else {
    double* part;
    EF_TRY(B.get(c, colstats_float_work_elems(n, d), &part));
    EF_HIP(c, launch_colstats_float(s, Xb, x_dtype, n, d, 0, part, mean, var, scale, w), "colstats (float)");
  }
  return copy_out(c, dev, {{mean_out, mean, d * sizeof(double), "out mean"},
                           {var_out, var, d * sizeof(double), "out var"}});
}

// The fit's CholQR factor on its own (API v7; ADVICE r5: a direct check of the blocked
// factor for padded and odd orders and of the failed-pivot contract): Li = L^-1 for
// G = L L^T (m <= 256, row-major, ldg >= m), host pointers.  A pivot <= tol_rel x max diag(G)
// sets *info = -(column + 1) and leaves Li as given (the subspace iteration then
// eigen-orthonormalises); *info = 0 on success.
extern "C" int ef_chol_inv(ef_ctx* c, const double* G, int32_t m, int64_t ldg, double tol_rel, double* Li,
                           int32_t* info) {
  using namespace ef;
  if (!c) return EF_E_INVALID;
  if (!G || !Li || !info || m < 1 || ldg < m || !chol_inv_supported(m))
    return set_err(c, EF_E_INVALID, "ef_chol_inv: bad arguments (1 <= m <= 256, ldg >= m)");
  EF_HIP(c, hipSetDevice(c->device), "hipSetDevice");
  hipStream_t s = c->stream;
  // locals: every return below follows the synchronise, or a failed call after which the
  // frees themselves wait for the device
  DevBuf dG, dL, dW, dI;
  EF_TRY(ensure(c, dG, (size_t)m * ldg * sizeof(double)));
  EF_TRY(ensure(c, dL, (size_t)m * m * sizeof(double)));
  EF_TRY(ensure(c, dW, chol_inv_work_elems(m) * sizeof(double)));
  EF_TRY(ensure(c, dI, sizeof(int)));
  hipError_t e = hipMemcpyAsync(dG.p, G, (size_t)m * ldg * sizeof(double), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(dL.p, Li, (size_t)m * m * sizeof(double), hipMemcpyHostToDevice, s);
  if (e == hipSuccess)
    e = launch_chol_inv(s, static_cast<const double*>(dG.p), m, ldg, tol_rel, static_cast<double*>(dL.p),
                        static_cast<int*>(dI.p), static_cast<double*>(dW.p));
  int hinfo = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(Li, dL.p, (size_t)m * m * sizeof(double), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(&hinfo, dI.p, sizeof(int), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return hip_err(c, e, "ef_chol_inv");
  *info = hinfo;
  return EF_OK;
}
