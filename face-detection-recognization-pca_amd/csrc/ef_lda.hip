// Fisherfaces: the class-aware discriminant fit on top of the eigenface features
// (Belhumeur, Hespanha, Kriegman 1997): the class statistics of labelled features
// (ef_lda_scatter) and the generalised symmetric eigenproblem Sb a = lambda Sw a
// (ef_lda_fit), float64 throughout.  DESIGN.md "Fisher discriminant" has the layout, the
// pass count and the determinism argument.
//
// Scatter, for features F[n][k] (fp32 / fp64) and labels in [0, C):
//   0. lda_label_check_kernel: a label outside [0, C) raises a flag the host reads before
//      anything indexes with a label (EF_E_INVALID; nothing else has run).
//   1. host: ef_lda_order, the stable grouping of the rows by label (order[n], offsets[C+1]).
//   2. lda_pivot_kernel: p = the mean of up to 1024 evenly spaced rows.  Every later sum is
//      taken of f - p, so its size is that of the spread of the data, not of its offset.
//   3. lda_class_sum_kernel: one workgroup per 64 consecutive ORDERED rows, one thread per
//      16-byte column group, the rows added one after the other.  A class that lies inside
//      one chunk is written straight to S[c]; a class that crosses a chunk border leaves one
//      partial per chunk it touches (slot 0: it began in an earlier chunk, slot 1: it begins
//      here and goes on), which lda_span_kernel adds in chunk order.  No accumulator is per
//      class in LDS, so any C up to n works; no atomics, so the bytes repeat.
//   4. lda_colsum_kernel (two levels, fixed order): sum_c S[c] -> the global mean;
//      lda_means_kernel: M_c - p = S_c / n_c.
//   5. lda_syrk_dd_kernel over the rows f_i - M_c(i): Sw, formed directly; the same kernel
//      over the C rows M_c - m with weights n_c: Sb.  64 x 64 output tiles of the upper
//      triangle x row slices, each slice's partial tile added in slice order by
//      lda_syrk_reduce_kernel, which also mirrors the triangle (exactly symmetric output).
//
// Arithmetic.  The discriminant's error is the scatters' error times cond(Sw), so steps 3 to 5
// carry every value as an unevaluated sum hi + lo of two doubles: differences by TwoSum,
// products by an fma-based TwoProduct, sums by compensated accumulation (Ogita, Rump, Oishi,
// "Accurate sum and dot product", 2005).  What comes out is the rounding of a result good to
// about 2^-100 relative to sum |terms|, i.e. the scatters of the long-double definition to the
// last bit or two, at ~12 fp64 instructions per multiply-add instead of one.
//
// Fit, all on the device from the fit's fp64 pieces:
//   G = (1 - g) Sw + g tr(Sw)/k I = L L^T (launch_chol_inv), T = L^-1 Sb L^-T (gemm64),
//   T + (tr T / k) I = V diag(lam + tr T / k) V^T (LDS Jacobi up to kJacobiMax, the grid
//   Jacobi beyond; the shift gives the k - C + 1 null directions of Sb a scale the relative
//   stopping rule can work with, and costs 2^-52 tr T / k in the eigenvalues),
//   A = sqrt(n - C+) L^-T V, sign rule, leading m columns.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "ef_linalg.hpp"

// the error-free transformations below are exact only as written: no a * b + c -> fma(a, b, c)
#pragma clang fp contract(off)

namespace {

using namespace ef;

constexpr int kLdaChunk = 64;         // ordered rows per workgroup of the class-sum pass
constexpr int kLdaPivotRows = 1024;   // rows sampled for the pivot
constexpr int kLdaColsumBlocks = 256; // first level of the column sum over classes
constexpr int kLdaMaxK = 1024;        // scatter: widest feature row
constexpr double kLdaPivotTol = 1e-12;  // Cholesky pivot floor, relative to max diag
constexpr int kLdaMaxSweeps = 60;
constexpr int kSyT = 64;              // scatter product: output tile
constexpr int kSyR = 16;              // rows staged per step
constexpr int kSySliceRows = 512;     // fewest rows per slice
constexpr size_t kSyPartBytes = size_t(128) << 20;  // budget of the slices' partial tiles

// slots of the context's fit pool, as the fit takes them (ef_fit.hip Bufs)
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

// s + e = a + b exactly (Knuth)
__device__ __forceinline__ void two_sum(double a, double b, double& s, double& e) {
  s = a + b;
  const double z = s - a;
  e = (a - (s - z)) + (b - z);
}
// (s, c) += v + e: s by TwoSum, its error and the small term e into c
__device__ __forceinline__ void dd_acc(double& s, double& c, double v, double e) {
  double t, err;
  two_sum(s, v, t, err);
  s = t;
  c += err + e;
}
// (qh, ql) = (hi + lo) / n for a whole number n
__device__ __forceinline__ void dd_div(double hi, double lo, double n, double& qh, double& ql) {
  qh = hi / n;
  ql = (fma(-qh, n, hi) + lo) / n;
}

__global__ void lda_label_check_kernel(const int* __restrict__ labels, int64_t n, int C, int* __restrict__ bad) {
  bool b = false;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int l = labels[i];
    b |= l < 0 || l >= C;
  }
  if (__any(b) && (threadIdx.x & 63) == 0) *bad = 1;
}

// pivot[j] = mean of rows 0, stride, 2 stride, ... (S of them), added in that order
template <class T>
__global__ void lda_pivot_kernel(const T* __restrict__ F, int k, int S, int64_t stride, double* __restrict__ pivot) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= k) return;
  double s = 0.0;
  for (int r = 0; r < S; ++r) s += (double)F[(int64_t)r * stride * k + j];
  pivot[j] = s / (double)S;
}

template <class T, int VEC>
__device__ __forceinline__ void lda_load(const T* p, double (&v)[VEC]) {
  if constexpr (VEC == 1) {
    v[0] = (double)p[0];
  } else if constexpr (VEC == 2) {
    const double2 t = *reinterpret_cast<const double2*>(p);
    v[0] = t.x, v[1] = t.y;
  } else {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = (double)t.x, v[1] = (double)t.y, v[2] = (double)t.z, v[3] = (double)t.w;
  }
}

// Class sums of f - pivot over the ordered rows [q * kLdaChunk, ...) of chunk q = blockIdx.x.
// G = k / VEC column groups, one per thread (strided when G > blockDim.x).  (Sh, Sl)[C][k]:
// classes inside one chunk; (Ph, Pl)[chunks][2][k]: the partials of classes that cross a
// chunk border.
template <class T, int VEC>
__global__ __launch_bounds__(256) void lda_class_sum_kernel(const T* __restrict__ F, int64_t n, int k,
                                                            const int64_t* __restrict__ order,
                                                            const int64_t* __restrict__ offsets,
                                                            const int* __restrict__ labels,
                                                            const double* __restrict__ pivot, double* __restrict__ Sh,
                                                            double* __restrict__ Sl, double* __restrict__ Ph,
                                                            double* __restrict__ Pl) {
  const int64_t q = blockIdx.x;
  const int64_t p0 = q * kLdaChunk;
  const int64_t p1 = p0 + kLdaChunk < n ? p0 + kLdaChunk : n;
  const int G = k / VEC;
  for (int g = threadIdx.x; g < G; g += blockDim.x) {
    const int j0 = g * VEC;
    double piv[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) piv[v] = pivot[j0 + v];
    int64_t p = p0;
    while (p < p1) {
      const int c = labels[order[p]];
      const int64_t cs = offsets[c], cend = offsets[c + 1];
      int64_t ce = cend < p1 ? cend : p1;
      if (ce <= p) ce = p + 1;  // cannot happen for a consistent order / offsets pair; never spin
      const int64_t a = p;
      double s[VEC], cc[VEC];
#pragma unroll
      for (int v = 0; v < VEC; ++v) s[v] = cc[v] = 0.0;
#pragma unroll 4
      for (; p < ce; ++p) {
        double x[VEC];
        lda_load<T, VEC>(F + order[p] * (int64_t)k + j0, x);
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          double d, e;
          two_sum(x[v], -piv[v], d, e);
          dd_acc(s[v], cc[v], d, e);
        }
      }
      const bool complete = a == cs && cend <= p1;
      const int64_t at = complete ? (int64_t)c * k : (q * 2 + (a > cs ? 0 : 1)) * k;
      double* dh = complete ? Sh : Ph;
      double* dl = complete ? Sl : Pl;
#pragma unroll
      for (int v = 0; v < VEC; ++v) two_sum(s[v], cc[v], dh[at + j0 + v], dl[at + j0 + v]);
    }
  }
}

// S[c] of the classes the chunk pass did not finish: zero for an empty class, the partials in
// chunk order for one that crosses a chunk border.
__global__ void lda_span_kernel(const int64_t* __restrict__ offsets, int C, int k, const double* __restrict__ Ph,
                                const double* __restrict__ Pl, double* __restrict__ Sh, double* __restrict__ Sl) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)C * k) return;
  const int64_t c = e / k;
  const int j = (int)(e - c * k);
  const int64_t cs = offsets[c], cend = offsets[c + 1];
  if (cend == cs) {
    Sh[e] = Sl[e] = 0.0;
    return;
  }
  const int64_t qa = cs / kLdaChunk, qb = (cend - 1) / kLdaChunk;
  if (qa == qb) return;
  double s = Ph[(qa * 2 + 1) * k + j], cc = Pl[(qa * 2 + 1) * k + j];
  for (int64_t q = qa + 1; q <= qb; ++q) dd_acc(s, cc, Ph[(q * 2) * k + j], Pl[(q * 2) * k + j]);
  two_sum(s, cc, Sh[e], Sl[e]);
}

// part[y][j] = sum of S[c][j] over the classes of slice y, in class order
__global__ void lda_colsum_kernel(const double* __restrict__ Sh, const double* __restrict__ Sl, int64_t C, int k,
                                  int64_t per, double* __restrict__ part_h, double* __restrict__ part_l) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= k) return;
  const int64_t c0 = (int64_t)blockIdx.y * per;
  const int64_t c1 = c0 + per < C ? c0 + per : C;
  double s = 0.0, cc = 0.0;
  for (int64_t c = c0; c < c1; ++c) dd_acc(s, cc, Sh[c * k + j], Sl[c * k + j]);
  two_sum(s, cc, part_h[(int64_t)blockIdx.y * k + j], part_l[(int64_t)blockIdx.y * k + j]);
}

// out = the rounding of pivot + (h + l)
__device__ __forceinline__ double lda_unshift(double pivot, double h, double l) {
  double s, e;
  two_sum(pivot, h, s, e);
  return s + (e + l);
}

// (mch, mcl)[j] = (sum_y part[y][j]) / n: the global mean less the pivot; mean[j] = pivot[j] + it
__global__ void lda_mean_kernel(const double* __restrict__ part_h, const double* __restrict__ part_l, int ny, int k,
                                int64_t n, const double* __restrict__ pivot, double* __restrict__ mch,
                                double* __restrict__ mcl, double* __restrict__ mean) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= k) return;
  double s = 0.0, cc = 0.0;
  for (int y = 0; y < ny; ++y) dd_acc(s, cc, part_h[(int64_t)y * k + j], part_l[(int64_t)y * k + j]);
  double h, l, qh, ql;
  two_sum(s, cc, h, l);
  dd_div(h, l, (double)n, qh, ql);
  mch[j] = qh;
  mcl[j] = ql;
  mean[j] = lda_unshift(pivot[j], qh, ql);
}

// (Mh, Ml)[c] = S[c] / n_c (the class mean less the pivot), M[c] = pivot + it; zero for an empty class
__global__ void lda_means_kernel(const double* __restrict__ Sh, const double* __restrict__ Sl,
                                 const int64_t* __restrict__ offsets, int64_t C, int k,
                                 const double* __restrict__ pivot, double* __restrict__ Mh, double* __restrict__ Ml,
                                 double* __restrict__ M) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= C * k) return;
  const int64_t c = e / k;
  const int j = (int)(e - c * k);
  const int64_t cnt = offsets[c + 1] - offsets[c];
  double qh = 0.0, ql = 0.0, m = 0.0;
  if (cnt > 0) {
    dd_div(Sh[e], Sl[e], (double)cnt, qh, ql);
    m = lda_unshift(pivot[j], qh, ql);
  }
  Mh[e] = qh;
  Ml[e] = ql;
  M[e] = m;
}

// Row sources of the scatter product: value(row, col) as hi + lo, and the row's weight.
template <class T>
struct FeatRows {  // f_i - M_c(i), weight 1: Sw
  const T* F;
  int k;
  const int* labels;
  const double *piv, *Mh, *Ml;
  __device__ __forceinline__ void value(int64_t r, int col, double& hi, double& lo) const {
    const int64_t at = (int64_t)labels[r] * k + col;
    double d, e, d2, e2;
    two_sum((double)F[r * k + col], -piv[col], d, e);
    two_sum(d, -Mh[at], d2, e2);
    two_sum(d2, (e + e2) - Ml[at], hi, lo);
  }
  __device__ __forceinline__ double weight(int64_t) const { return 1.0; }
};
struct MeanRows {  // M_c - m, weight n_c: Sb (an empty class has weight 0)
  const double *Mh, *Ml;
  int k;
  const double *mch, *mcl;
  const int64_t* offsets;
  __device__ __forceinline__ void value(int64_t r, int col, double& hi, double& lo) const {
    double d, e;
    two_sum(Mh[r * k + col], -mch[col], d, e);
    two_sum(d, (e + Ml[r * k + col]) - mcl[col], hi, lo);
  }
  __device__ __forceinline__ double weight(int64_t r) const { return (double)(offsets[r + 1] - offsets[r]); }
};

__device__ __forceinline__ void lda_tile(int t, int nt, int& ta, int& tb) {
  ta = 0;
  while (t >= nt - ta) t -= nt - ta, ++ta;
  tb = ta + t;
}

// One 64 x 64 tile (ta <= tb: blockIdx.x) of sum_r w_r v_r v_r^T over the rows of slice
// blockIdx.y, in compensated arithmetic; 16 x 16 threads, 4 x 4 outputs each.  The tile goes
// out whole (zeros past k) as an unevaluated pair to part[slice][tile][64][64].
template <class Rows>
__global__ __launch_bounds__(256) void lda_syrk_dd_kernel(Rows rows, int64_t n, int k, int64_t rows_per_slice, int nt,
                                                          double* __restrict__ part_h, double* __restrict__ part_l) {
  __shared__ double Ah[kSyR][kSyT], Al[kSyR][kSyT], Bh[kSyR][kSyT], Bl[kSyR][kSyT];
  int ta, tb;
  lda_tile((int)blockIdx.x, nt, ta, tb);
  const int a0 = ta * kSyT, b0 = tb * kSyT;
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_slice;
  const int64_t r1 = r0 + rows_per_slice < n ? r0 + rows_per_slice : n;
  double s[4][4], c[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) s[i][j] = c[i][j] = 0.0;

  for (int64_t rb = r0; rb < r1; rb += kSyR) {
    for (int e = tid; e < kSyR * kSyT; e += 256) {
      const int rr = e / kSyT, col = e - rr * kSyT;
      const int64_t row = rb + rr;
      double ah = 0.0, al = 0.0, bh = 0.0, bl = 0.0;
      if (row < r1) {
        if (a0 + col < k) rows.value(row, a0 + col, ah, al);
        if (b0 + col < k) {
          double h, l;
          rows.value(row, b0 + col, h, l);
          const double w = rows.weight(row);
          const double p = h * w;
          two_sum(p, fma(h, w, -p) + l * w, bh, bl);
        }
      }
      Ah[rr][col] = ah, Al[rr][col] = al, Bh[rr][col] = bh, Bl[rr][col] = bl;
    }
    __syncthreads();
#pragma unroll 2
    for (int rr = 0; rr < kSyR; ++rr) {
      double ah[4], al[4], bh[4], bl[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        ah[i] = Ah[rr][ty * 4 + i], al[i] = Al[rr][ty * 4 + i];
        bh[i] = Bh[rr][tx * 4 + i], bl[i] = Bl[rr][tx * 4 + i];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const double p = ah[i] * bh[j];
          const double e = fma(al[i], bh[j], fma(ah[i], bl[j], fma(ah[i], bh[j], -p)));
          dd_acc(s[i][j], c[i][j], p, e);
        }
    }
    __syncthreads();
  }
  const int64_t base = ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (kSyT * kSyT);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t at = base + (ty * 4 + i) * kSyT + tx * 4 + j;
      two_sum(s[i][j], c[i][j], part_h[at], part_l[at]);
    }
}

// out[a][b] = out[b][a] = the slices' partials of entry (a <= b), added in slice order
__global__ void lda_syrk_reduce_kernel(const double* __restrict__ part_h, const double* __restrict__ part_l, int slices,
                                       int ntiles, int nt, int k, double* __restrict__ out) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (int64_t)ntiles * kSyT * kSyT) return;
  const int t = (int)(g / (kSyT * kSyT)), e = (int)(g - (int64_t)t * kSyT * kSyT);
  int ta, tb;
  lda_tile(t, nt, ta, tb);
  const int la = e / kSyT, lb = e - la * kSyT;
  const int a = ta * kSyT + la, b = tb * kSyT + lb;
  if (a >= k || b >= k || a > b) return;
  double s = 0.0, c = 0.0;
  for (int z = 0; z < slices; ++z) {
    const int64_t at = ((int64_t)z * ntiles + t) * (kSyT * kSyT) + e;
    dd_acc(s, c, part_h[at], part_l[at]);
  }
  const double v = s + c;
  out[(int64_t)a * k + b] = v;
  out[(int64_t)b * k + a] = v;
}

// G = (1 - gamma) Sw + gamma tr(Sw) / k I; one workgroup, the trace added in index order
__global__ __launch_bounds__(256) void lda_shrink_kernel(const double* __restrict__ Sw, int k, double gamma,
                                                         double* __restrict__ G) {
  __shared__ double tr_s;
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < k; ++i) t += Sw[i * k + i];
    tr_s = t / (double)k;
  }
  __syncthreads();
  const double mu = gamma * tr_s;
  for (int e = threadIdx.x; e < k * k; e += blockDim.x) {
    const int a = e / k, b = e - a * k;
    G[e] = (1.0 - gamma) * Sw[e] + (a == b ? mu : 0.0);
  }
}

// T += (tr T / k) I; *sigma = the shift
__global__ __launch_bounds__(256) void lda_shift_kernel(double* __restrict__ T, int k, double* __restrict__ sigma) {
  __shared__ double sh;
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < k; ++i) t += T[i * k + i];
    sh = t > 0.0 ? t / (double)k : 0.0;
    *sigma = sh;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < k; i += blockDim.x) T[i * k + i] += sh;
}

// A[i][j] = sgn_j scale A0[i][j] for the m leading columns, sgn_j making the entry of largest
// magnitude positive (first index on ties); evals[j] = lam[j] - sigma
__global__ void lda_finalize_kernel(const double* __restrict__ A0, const double* __restrict__ lam, int k, int m,
                                    const double* __restrict__ sigma, double scale, double* __restrict__ A,
                                    double* __restrict__ evals) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  double best = -1.0, sgn = 1.0;
  for (int i = 0; i < k; ++i) {
    const double v = A0[i * k + j];
    if (fabs(v) > best) best = fabs(v), sgn = v < 0.0 ? -1.0 : 1.0;
  }
  for (int i = 0; i < k; ++i) A[i * m + j] = sgn * scale * A0[i * k + j];
  evals[j] = lam[j] - *sigma;
}

// The slices of a scatter product over `rows` rows for a k x k output.
struct SyrkPlan {
  int nt, ntiles, slices;
  int64_t rows_per_slice;
  size_t part_elems() const { return (size_t)slices * ntiles * kSyT * kSyT; }
};
SyrkPlan syrk_plan(int64_t rows, int k) {
  SyrkPlan p;
  p.nt = (k + kSyT - 1) / kSyT;
  p.ntiles = p.nt * (p.nt + 1) / 2;
  const int64_t cap = std::max<int64_t>(1, (int64_t)(kSyPartBytes / ((size_t)p.ntiles * kSyT * kSyT * 16)));
  int64_t slices = std::min<int64_t>(std::max<int64_t>(1, (rows + kSySliceRows - 1) / kSySliceRows), cap);
  p.rows_per_slice = round_up((rows + slices - 1) / slices, kSyR);
  p.slices = (int)((rows + p.rows_per_slice - 1) / p.rows_per_slice);
  return p;
}
template <class Rows>
hipError_t launch_syrk_dd(hipStream_t s, const Rows& rows, int64_t n, int k, const SyrkPlan& p, double* part_h,
                          double* part_l, double* out) {
  hipLaunchKernelGGL((lda_syrk_dd_kernel<Rows>), dim3((unsigned)p.ntiles, (unsigned)p.slices), dim3(256), 0, s, rows, n,
                     k, p.rows_per_slice, p.nt, part_h, part_l);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int64_t tot = (int64_t)p.ntiles * kSyT * kSyT;
  hipLaunchKernelGGL(lda_syrk_reduce_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, part_h, part_l,
                     p.slices, p.ntiles, p.nt, k, out);
  return hipGetLastError();
}

// What the scatter leaves on the device for its caller.
struct Scatter {
  std::vector<int64_t> offsets;  // host, [C + 1]
  int64_t n_nonempty = 0;
  double *mean = nullptr, *M = nullptr, *Sw = nullptr, *Sb = nullptr;
};

template <class T>
hipError_t launch_class_sums(hipStream_t s, const T* F, int64_t n, int k, const int64_t* order, const int64_t* offsets,
                             const int* labels, const double* pivot, double* Sh, double* Sl, double* Ph, double* Pl,
                             int64_t chunks) {
  constexpr int VEC = 16 / (int)sizeof(T);
  const bool vec = (k % VEC) == 0 && (reinterpret_cast<uintptr_t>(F) & 15) == 0;
  const int G = vec ? k / VEC : k;
  const int threads = G <= 64 ? 64 : G <= 128 ? 128 : 256;
  if (vec)
    hipLaunchKernelGGL((lda_class_sum_kernel<T, VEC>), dim3((unsigned)chunks), dim3(threads), 0, s, F, n, k, order,
                       offsets, labels, pivot, Sh, Sl, Ph, Pl);
  else
    hipLaunchKernelGGL((lda_class_sum_kernel<T, 1>), dim3((unsigned)chunks), dim3(threads), 0, s, F, n, k, order,
                       offsets, labels, pivot, Sh, Sl, Ph, Pl);
  return hipGetLastError();
}

int check_scatter_args(ef_ctx* c, const char* who, const void* F, int32_t f_dtype, int64_t n, int32_t k,
                       const int32_t* labels, int32_t C) {
  if (!F || !labels || (f_dtype != EF_F32 && f_dtype != EF_F64) || n < 1 || k < 1 || k > kLdaMaxK || C < 1 ||
      n > ((int64_t)1 << 31) * kLdaChunk - 1)
    return set_err(c, EF_E_INVALID, std::string(who) + ": bad arguments (F, labels non-null; fp32 / fp64 features; "
                                                       "n >= 1, 1 <= k <= 1024, n_classes >= 1)");
  return EF_OK;
}

// The statistics on the device (step list at the top of the file).  Synchronises c->stream
// for the label flag (and a device caller's labels) and once more at the end.
template <class T>
int scatter_run_t(ef_ctx* c, Bufs& B, const char* who, const T* Fd, int64_t n, int32_t k, int* lab_d,
                  const int32_t* lab_host, int32_t C, Scatter* out) {
  hipStream_t s = c->stream;
  const int64_t kk = (int64_t)k * k, Ck = (int64_t)C * k;

  // the stable grouping
  std::vector<int64_t> order((size_t)n);
  out->offsets.assign((size_t)C + 1, 0);
  if (ef_lda_order(lab_host, n, C, order.data(), out->offsets.data()) != EF_OK)
    return set_err(c, EF_E_INVALID, std::string(who) + ": a label lies outside [0, n_classes)");
  out->n_nonempty = 0;
  for (int32_t cc = 0; cc < C; ++cc) out->n_nonempty += out->offsets[cc + 1] > out->offsets[cc];

  const int64_t chunks = (n + kLdaChunk - 1) / kLdaChunk;
  const int64_t per = (C + kLdaColsumBlocks - 1) / kLdaColsumBlocks;
  const int ny = (int)((C + per - 1) / per);
  const SyrkPlan pw = syrk_plan(n, k), pb = syrk_plan(C, k);
  const size_t part_elems = std::max(pw.part_elems(), pb.part_elems());

  int64_t *order_d, *off_d;
  double *pivot, *Sh, *Sl, *Ph, *Pl, *part_h, *part_l, *mch, *mcl, *Mh, *Ml, *yh, *yl;
  EF_TRY(B.get(c, (size_t)n, &order_d));
  EF_TRY(B.get(c, (size_t)C + 1, &off_d));
  EF_TRY(B.get(c, (size_t)k, &pivot));
  EF_TRY(B.get(c, (size_t)Ck, &Sh));
  EF_TRY(B.get(c, (size_t)Ck, &Sl));
  EF_TRY(B.get(c, (size_t)chunks * 2 * k, &Ph));
  EF_TRY(B.get(c, (size_t)chunks * 2 * k, &Pl));
  EF_TRY(B.get(c, (size_t)ny * k, &yh));
  EF_TRY(B.get(c, (size_t)ny * k, &yl));
  EF_TRY(B.get(c, (size_t)k, &mch));
  EF_TRY(B.get(c, (size_t)k, &mcl));
  EF_TRY(B.get(c, (size_t)k, &out->mean));
  EF_TRY(B.get(c, (size_t)Ck, &Mh));
  EF_TRY(B.get(c, (size_t)Ck, &Ml));
  EF_TRY(B.get(c, (size_t)Ck, &out->M));
  EF_TRY(B.get(c, part_elems, &part_h));
  EF_TRY(B.get(c, part_elems, &part_l));
  EF_TRY(B.get(c, (size_t)kk, &out->Sw));
  EF_TRY(B.get(c, (size_t)kk, &out->Sb));
  EF_HIP(c, hipMemcpyAsync(order_d, order.data(), (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, s), "H2D order");
  EF_HIP(c, hipMemcpyAsync(off_d, out->offsets.data(), ((size_t)C + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s),
         "H2D offsets");

  const int S_rows = (int)std::min<int64_t>(n, kLdaPivotRows);
  const dim3 colgrid((unsigned)((k + 63) / 64));
  hipLaunchKernelGGL(lda_pivot_kernel<T>, colgrid, dim3(64), 0, s, Fd, k, S_rows, n / S_rows, pivot);
  EF_HIP(c, hipGetLastError(), "pivot");
  EF_HIP(c, launch_class_sums(s, Fd, n, k, order_d, off_d, lab_d, pivot, Sh, Sl, Ph, Pl, chunks), "class sums");
  const unsigned ck_blocks = (unsigned)((Ck + 255) / 256);
  hipLaunchKernelGGL(lda_span_kernel, dim3(ck_blocks), dim3(256), 0, s, off_d, C, k, Ph, Pl, Sh, Sl);
  hipLaunchKernelGGL(lda_colsum_kernel, dim3(colgrid.x, (unsigned)ny), dim3(64), 0, s, Sh, Sl, (int64_t)C, k, per, yh,
                     yl);
  hipLaunchKernelGGL(lda_mean_kernel, colgrid, dim3(64), 0, s, yh, yl, ny, k, n, pivot, mch, mcl, out->mean);
  hipLaunchKernelGGL(lda_means_kernel, dim3(ck_blocks), dim3(256), 0, s, Sh, Sl, off_d, (int64_t)C, k, pivot, Mh, Ml,
                     out->M);
  EF_HIP(c, hipGetLastError(), "class means");

  EF_HIP(c, launch_syrk_dd(s, FeatRows<T>{Fd, k, lab_d, pivot, Mh, Ml}, n, k, pw, part_h, part_l, out->Sw),
         "within-class scatter");
  EF_HIP(c, launch_syrk_dd(s, MeanRows{Mh, Ml, k, mch, mcl, off_d}, (int64_t)C, k, pb, part_h, part_l, out->Sb),
         "between-class scatter");
  // order and offsets were read from host vectors that die with this frame
  EF_HIP(c, hipStreamSynchronize(s), "sync");
  return EF_OK;
}

int scatter_run(ef_ctx* c, Bufs& B, const char* who, const void* F, int32_t f_dtype, int64_t n, int32_t k,
                const int32_t* labels, int32_t C, bool dev, Scatter* out) {
  hipStream_t s = c->stream;
  const size_t esz = f_dtype == EF_F32 ? 4 : 8;

  // features and labels on the device
  const void* Fd = F;
  if (!dev) {
    char* p;
    EF_TRY(B.get(c, (size_t)n * k * esz, &p));
    EF_HIP(c, hipMemcpyAsync(p, F, (size_t)n * k * esz, hipMemcpyHostToDevice, s), "H2D features");
    Fd = p;
  }
  int* lab_d;
  int* bad;
  EF_TRY(B.get(c, (size_t)n, &lab_d));
  EF_TRY(B.get(c, 4, &bad));
  EF_HIP(c, hipMemcpyAsync(lab_d, labels, (size_t)n * sizeof(int), dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s),
         "labels");
  EF_HIP(c, hipMemsetAsync(bad, 0, sizeof(int), s), "memset");
  {
    const int64_t blocks = std::min<int64_t>((n + 255) / 256, 1024);
    hipLaunchKernelGGL(lda_label_check_kernel, dim3((unsigned)blocks), dim3(256), 0, s, lab_d, n, C, bad);
    EF_HIP(c, hipGetLastError(), "label check");
  }
  std::vector<int32_t> lab_h;
  const int32_t* lab_host = labels;
  int hbad = 0;
  if (dev) {
    lab_h.resize((size_t)n);
    EF_HIP(c, hipMemcpyAsync(lab_h.data(), lab_d, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s), "D2H labels");
    lab_host = lab_h.data();
  }
  EF_HIP(c, hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, s), "D2H flag");
  EF_HIP(c, hipStreamSynchronize(s), "sync");
  if (hbad) return set_err(c, EF_E_INVALID, std::string(who) + ": a label lies outside [0, n_classes)");
  if (f_dtype == EF_F32) return scatter_run_t(c, B, who, static_cast<const float*>(Fd), n, k, lab_d, lab_host, C, out);
  return scatter_run_t(c, B, who, static_cast<const double*>(Fd), n, k, lab_d, lab_host, C, out);
}

struct Out {
  void* dst;
  const void* src;
  size_t bytes;
};
int copy_out(ef_ctx* c, bool dev, std::initializer_list<Out> outs) {
  for (const Out& o : outs)
    if (o.dst)
      EF_HIP(c, hipMemcpyAsync(o.dst, o.src, o.bytes, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream),
             "copy out");
  EF_HIP(c, hipStreamSynchronize(c->stream), "sync");
  return EF_OK;
}

}  // namespace

extern "C" int ef_lda_order(const int32_t* labels, int64_t n, int32_t n_classes, int64_t* order, int64_t* offsets) {
  if (n < 0 || n_classes < 1 || !offsets || (n > 0 && (!labels || !order))) return EF_E_INVALID;
  for (int64_t i = 0; i < n; ++i)
    if (labels[i] < 0 || labels[i] >= n_classes) return EF_E_INVALID;
  for (int32_t c = 0; c <= n_classes; ++c) offsets[c] = 0;
  for (int64_t i = 0; i < n; ++i) ++offsets[labels[i] + 1];
  for (int32_t c = 0; c < n_classes; ++c) offsets[c + 1] += offsets[c];
  std::vector<int64_t> next(offsets, offsets + n_classes);
  for (int64_t i = 0; i < n; ++i) order[next[labels[i]]++] = i;
  return EF_OK;
}

extern "C" int ef_lda_scatter(ef_ctx* c, const void* F, int32_t f_dtype, int64_t n, int32_t k, const int32_t* labels,
                              int32_t n_classes, int64_t* counts, double* mean, double* class_means, double* Sw,
                              double* Sb, uint32_t flags) {
  using namespace ef;
  if (!c) return EF_E_INVALID;
  EF_TRY(check_scatter_args(c, "ef_lda_scatter", F, f_dtype, n, k, labels, n_classes));
  EF_HIP(c, hipSetDevice(c->device), "hipSetDevice");
  const bool dev = (flags & EF_MEM_DEVICE) != 0;
  Bufs B;
  Scatter sc;
  EF_TRY(scatter_run(c, B, "ef_lda_scatter", F, f_dtype, n, k, labels, n_classes, dev, &sc));
  std::vector<int64_t> cnt((size_t)n_classes);
  for (int32_t cc = 0; cc < n_classes; ++cc) cnt[cc] = sc.offsets[cc + 1] - sc.offsets[cc];
  if (counts) {
    if (dev)
      EF_HIP(c, hipMemcpyAsync(counts, cnt.data(), cnt.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream),
             "H2D counts");
    else
      memcpy(counts, cnt.data(), cnt.size() * sizeof(int64_t));
  }
  const size_t kb = (size_t)k * sizeof(double);
  return copy_out(c, dev, {{mean, sc.mean, kb}, {class_means, sc.M, (size_t)n_classes * kb}, {Sw, sc.Sw, k * kb},
                           {Sb, sc.Sb, k * kb}});
}

extern "C" int ef_lda_fit(ef_ctx* c, const void* F, int32_t f_dtype, int64_t n, int32_t k, const int32_t* labels,
                          int32_t n_classes, int32_t m, double shrinkage, double* A, double* evals, double* mean,
                          double* class_means, uint32_t flags) {
  using namespace ef;
  if (!c) return EF_E_INVALID;
  EF_TRY(check_scatter_args(c, "ef_lda_fit", F, f_dtype, n, k, labels, n_classes));
  if (!A || !evals || !(shrinkage >= 0.0 && shrinkage <= 1.0) || m < 1)
    return set_err(c, EF_E_INVALID, "ef_lda_fit: bad arguments (A, evals non-null; 0 <= shrinkage <= 1; m >= 1)");
  if (!chol_inv_supported(k))
    return set_err(c, EF_E_INVALID, "ef_lda_fit: k > 256 is not supported (the Cholesky-inverse kernel's limit)");
  EF_HIP(c, hipSetDevice(c->device), "hipSetDevice");
  const bool dev = (flags & EF_MEM_DEVICE) != 0;
  hipStream_t s = c->stream;
  Bufs B;
  Scatter sc;
  EF_TRY(scatter_run(c, B, "ef_lda_fit", F, f_dtype, n, k, labels, n_classes, dev, &sc));
  const int64_t cplus = sc.n_nonempty, dof = n - cplus;
  if (m > std::min<int64_t>(k, cplus - 1))
    return set_err(c, EF_E_INVALID, "ef_lda_fit: m must satisfy 1 <= m <= min(k, non-empty classes - 1) = " +
                                        std::to_string(std::min<int64_t>(k, cplus - 1)));
  const std::string singular = "ef_lda_fit: Sw is singular: n - C+ = " + std::to_string(dof) + " rows of freedom for k = " +
                               std::to_string(k) + " (too few rows per identity); shrinkage = " +
                               std::to_string(shrinkage) + ", raise it or lower k";
  // rank(Sw) <= n - C+: without shrinkage the factorisation cannot succeed, whatever rounding
  // leaves on the last pivots
  if (dof < 1 || (shrinkage == 0.0 && dof < k)) return set_err(c, EF_E_NUMERIC, singular);

  const int64_t kk = (int64_t)k * k;
  const size_t work_elems = (size_t)4 * kk + 64;
  double *G, *Li, *X, *T, *V, *lam, *A0, *Am, *ev, *sigma, *cwork, *work, *jwork = nullptr;
  int* info;
  EF_TRY(B.get(c, (size_t)kk, &G));
  EF_TRY(B.get(c, (size_t)kk, &Li));
  EF_TRY(B.get(c, (size_t)kk, &X));
  EF_TRY(B.get(c, (size_t)kk, &T));
  EF_TRY(B.get(c, (size_t)kk, &V));
  EF_TRY(B.get(c, (size_t)k, &lam));
  EF_TRY(B.get(c, (size_t)kk, &A0));
  EF_TRY(B.get(c, (size_t)k * m, &Am));
  EF_TRY(B.get(c, (size_t)m, &ev));
  EF_TRY(B.get(c, 2, &sigma));
  EF_TRY(B.get(c, chol_inv_work_elems(k), &cwork));
  EF_TRY(B.get(c, work_elems, &work));
  EF_TRY(B.get(c, 4, &info));
  JacobiBig big;
  if (k > kJacobiMax) {
    EF_TRY(B.get(c, jacobi_big_work_elems(k), &jwork));
    EF_HIP(c, big.init(k, jwork, info, c->own_stream), "jacobi graph");
  }

  hipLaunchKernelGGL(lda_shrink_kernel, dim3(1), dim3(256), 0, s, sc.Sw, k, shrinkage, G);
  EF_HIP(c, hipGetLastError(), "shrinkage");
  EF_HIP(c, hipMemsetAsync(Li, 0, (size_t)kk * sizeof(double), s), "memset");
  EF_HIP(c, hipMemsetAsync(info, 0, sizeof(int), s), "memset");
  EF_HIP(c, launch_chol_inv(s, G, k, k, kLdaPivotTol, Li, info, cwork), "cholesky + L^-1");
  int hinfo = 0;
  EF_HIP(c, hipMemcpyAsync(&hinfo, info, sizeof(int), hipMemcpyDeviceToHost, s), "D2H info");
  EF_HIP(c, hipStreamSynchronize(s), "sync");
  if (hinfo < 0) return set_err(c, EF_E_NUMERIC, singular + " (pivot " + std::to_string(-hinfo - 1) + " not positive)");

  EF_HIP(c, gemm64(s, Operand::dense(Li, k, false), Operand::dense(sc.Sb, k, false), k, k, k, 1.0, X, k, work, work_elems),
         "L^-1 Sb");
  EF_HIP(c, gemm64(s, Operand::dense(X, k, false), Operand::dense(Li, k, true), k, k, k, 1.0, T, k, work, work_elems),
         "L^-1 Sb L^-T");
  hipLaunchKernelGGL(lda_shift_kernel, dim3(1), dim3(256), 0, s, T, k, sigma);
  EF_HIP(c, hipGetLastError(), "shift");
  if (k <= kJacobiMax) {
    EF_HIP(c, launch_jacobi(s, T, k, k, lam, V, k, kLdaMaxSweeps, info), "jacobi");
    EF_HIP(c, hipMemcpyAsync(&hinfo, info, sizeof(int), hipMemcpyDeviceToHost, s), "D2H info");
    EF_HIP(c, hipStreamSynchronize(s), "sync");
    if (hinfo < 0) return set_err(c, EF_E_NUMERIC, "ef_lda_fit: Jacobi did not converge");
  } else {
    hipError_t e = hipSuccess;
    const int rc = big.solve(s, T, k, lam, V, k, kLdaMaxSweeps, nullptr, &e);
    if (rc < 0) return hip_err(c, e, "jacobi");
    if (rc > 0) return set_err(c, EF_E_NUMERIC, "ef_lda_fit: Jacobi did not converge");
  }
  EF_HIP(c, gemm64(s, Operand::dense(Li, k, true), Operand::dense(V, k, false), k, k, k, 1.0, A0, k, work, work_elems),
         "L^-T V");
  hipLaunchKernelGGL(lda_finalize_kernel, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, s, A0, lam, k, m, sigma,
                     std::sqrt((double)dof), Am, ev);
  EF_HIP(c, hipGetLastError(), "finalize");
  const size_t kb = (size_t)k * sizeof(double);
  return copy_out(c, dev, {{A, Am, (size_t)m * kb}, {evals, ev, (size_t)m * sizeof(double)}, {mean, sc.mean, kb},
                           {class_means, sc.M, (size_t)n_classes * kb}});
}
