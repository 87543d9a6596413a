// Kernel-level checks of the fit's matrix-product and eigen-solver kernels (Makefile target
// `kernel_units`, run by tests/test_gpu_kernel_units.py).  The program links the product
// objects, creates one stream and calls the ef:: launchers of csrc/ef_linalg.hpp directly;
// every case has a host reference of its own in plain loops (long double for real-valued
// cases, int64 for integer ones).
//
//   kernel_units --list            groups and cases
//   kernel_units <group> [case]    tall | s3 | cq | chol | jacobi  (GPU)
//   kernel_units --host            the references against their own bounds; no HIP call
//
// One line per case:  case=<id> worst=<measured/bound> rms=<...> PASS|FAIL   (exit 1 on any
// FAIL).  The first failing HIP call prints its error and ends the process (exit 2) with
// nothing more launched.
//
// Two kinds of product case:
//   E  small-integer inputs: every product and partial sum is representable, so the result
//      must be bit-equal to the integer reference whatever the summation order (worst = the
//      number of entries that differ);
//   R  real inputs, magnitudes in [0.5, 1] with random sign: a componentwise bound, written
//      out with its derivation where it is used.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <atomic>
#include <map>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../face-detection-recognization-pca_amd/csrc/ef_linalg.hpp"

typedef long double ld;

// ------------------------------------------------------------------ plumbing
static void hip_ok(hipError_t e, const char* what, int line) {
  if (e == hipSuccess) return;
  std::printf("HIP error at line %d: %s: %s\n", line, what, hipGetErrorString(e));
  std::fflush(stdout);
  std::_Exit(2);
}
#define HIP(x) hip_ok((x), #x, __LINE__)

static hipStream_t g_stream = nullptr;
static int g_fail = 0;
static const char* g_only = nullptr;  // [case] filter (substring of the id)

struct Dev {  // device buffer with 256 bytes of slack
  void* p = nullptr;
  size_t bytes = 0;
  explicit Dev(size_t b, size_t slack = 256) : bytes(b) {
    HIP(hipMalloc(&p, b + slack));
    HIP(hipMemset(p, 0, b + slack));
  }
  Dev(const Dev&) = delete;
  ~Dev() { (void)hipFree(p); }
  template <class T>
  T* as() const { return static_cast<T*>(p); }
  template <class T>
  void up(const std::vector<T>& v) const {
    HIP(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  }
  template <class T>
  void down(std::vector<T>& v) const {
    HIP(hipStreamSynchronize(g_stream));
    HIP(hipMemcpy(v.data(), p, v.size() * sizeof(T), hipMemcpyDeviceToHost));
  }
};

struct Rng {
  uint64_t s;
  explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 0x1234567ull) {}
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }  // [0, 1)
  int range(int lo, int hi) { return lo + (int)(next() % (uint64_t)(hi - lo + 1)); }
  // magnitude in [0.5, 1], random sign, exactly representable in fp32
  double real() {
    const float v = (float)(0.5 + 0.5 * uni());
    return (next() & 1) ? -(double)v : (double)v;
  }
  // the same with all 53 bits of the significand in play
  double real64() {
    const double v = 0.5 + 0.5 * uni();
    return (next() & 1) ? -v : v;
  }
  double gauss() {
    double a = 0;
    for (int i = 0; i < 12; ++i) a += uni();
    return a - 6.0;
  }
};

struct Stat {
  double worst = 0.0, sumsq = 0.0;
  int64_t n = 0, mism = 0;
  void add(ld err, ld bound) {
    double r;
    if (!(err == err)) r = std::numeric_limits<double>::infinity();  // NaN
    else if (bound > 0) r = (double)(err / bound);
    else r = err == 0 ? 0.0 : std::numeric_limits<double>::infinity();
    worst = std::max(worst, r);
    if (std::isfinite(r)) sumsq += r * r;
    ++n;
  }
  void exact(bool same) {
    mism += same ? 0 : 1;
    ++n;
  }
  double rms() const { return n ? std::sqrt(sumsq / (double)n) : 0.0; }
};

static bool wanted(const std::string& id) { return !g_only || id.find(g_only) != std::string::npos; }
static bool g_list = false;

// R case / certificate: passes when every ratio is <= 1
static void report(const std::string& id, const Stat& st, const std::string& extra = "") {
  const bool ok = st.worst <= 1.0 && st.mism == 0;
  std::printf("case=%s worst=%.4g rms=%.4g %s%s%s\n", id.c_str(), st.worst, st.rms(), ok ? "PASS" : "FAIL",
              extra.empty() ? "" : " ", extra.c_str());
  std::fflush(stdout);
  if (!ok) ++g_fail;
}
// E case: worst = the count of entries that are not bit-equal
static void report_exact(const std::string& id, const Stat& st, const std::string& extra = "") {
  const bool ok = st.mism == 0;
  std::printf("case=%s worst=%lld rms=0 %s (bit-equal %lld of %lld)%s%s\n", id.c_str(), (long long)st.mism,
              ok ? "PASS" : "FAIL", (long long)(st.n - st.mism), (long long)st.n, extra.empty() ? "" : " ",
              extra.c_str());
  std::fflush(stdout);
  if (!ok) ++g_fail;
}

template <class T>
static bool same_bits(T a, T b) {
  return std::memcmp(&a, &b, sizeof(T)) == 0;
}

// rows a sampled reference covers: all of them up to 512 rows, else the first and last row
// of every 64-row tile (which holds those of every 256-row tile) and the last row
static std::vector<int64_t> sample_rows(int64_t M) {
  std::vector<int64_t> r;
  if (M <= 512) {
    for (int64_t i = 0; i < M; ++i) r.push_back(i);
    return r;
  }
  for (int64_t t = 0; t * 64 < M; ++t) {
    r.push_back(t * 64);
    if (t * 64 + 63 < M) r.push_back(t * 64 + 63);
  }
  if (r.back() != M - 1) r.push_back(M - 1);
  return r;
}

static const double kU64 = std::ldexp(1.0, -53), kU32 = std::ldexp(1.0, -24);
static ld gamma_n(int n) { return (ld)n * kU64 / (1 - (ld)n * kU64); }

// ------------------------------------------------------------------ tall
// The product's split plan (ef_dgemm.hip plan_split / launch_tall), for the bound's nsplit
static int64_t tall_nsplit(int64_t M, int64_t N, int64_t K, size_t work_elems) {
  const int cw = N > 128 ? 4 : (N > 64 ? 2 : 1), rw = 4 / cw;
  const int64_t tiles = ((M + 64 * rw - 1) / (64 * rw)) * ((N + 64 * cw - 1) / (64 * cw));
  const int64_t chunks = (K + 31) / 32;
  int64_t ns = 1;
  if (tiles < 256 && work_elems > 0) {
    ns = (256 + tiles - 1) / tiles;
    ns = std::min<int64_t>(ns, std::max<int64_t>(chunks / 4, 1));
    while (ns > 1 && (size_t)(ns * M * N) > work_elems) --ns;
  }
  const int64_t kps = ((chunks + ns - 1) / ns) * 32;
  return (K + kps - 1) / kps;
}

struct TallCase {
  int M, N, K;
  bool at, half, work;
};

static std::vector<TallCase> tall_cases() {
  // every M, N, K of the list, both a_trans settings, both alphas, with and without a work
  // buffer, crossed by co-prime strides (42 of the 672 combinations)
  const int Ms[4] = {1, 63, 65, 257}, Ns[6] = {1, 64, 65, 128, 129, 300}, Ks[7] = {1, 15, 17, 33, 100, 517, 2050};
  std::vector<TallCase> v;
  for (int i = 0; i < 42; ++i)
    v.push_back({Ms[(i + i / 4) % 4], Ns[i % 6], Ks[i % 7], ((i / 7 + i) & 1) != 0, ((i / 3) & 1) != 0,
                 ((i / 2 + i / 14) & 1) != 0});
  // the largest of everything, split and unsplit, both walks
  v.push_back({257, 300, 2050, false, false, true});
  v.push_back({257, 300, 2050, true, true, true});
  v.push_back({257, 129, 517, true, false, true});
  v.push_back({65, 65, 2050, false, true, true});
  v.push_back({65, 128, 517, false, true, true});  // the cross has K = 517 only without a work buffer
  return v;
}

static int64_t pad4(int64_t x) { return (x + 3) / 4 * 4 + 4; }

template <class T>
static void tall_run(const TallCase& c, bool exact, const std::string& id) {
  const int M = c.M, N = c.N, K = c.K;
  const int64_t lda = c.at ? pad4(M) : pad4(K), ldbt = pad4(K), ldc = N + 3;
  const int64_t arows = c.at ? K : M;
  const double alpha = c.half ? 0.5 : 1.0;
  Rng rng(1000003ull * M + 1009ull * N + K + (exact ? 7 : 0));
  std::vector<double> a((size_t)M * K), b((size_t)K * N);  // a[i][k], b[k][j]
  for (auto& x : a) x = exact ? rng.range(-2, 2) : rng.real();
  for (auto& x : b) x = exact ? rng.range(-2, 2) : rng.real();
  const T pad = (T)-777.25;
  std::vector<T> hA((size_t)arows * lda, pad), hB((size_t)N * ldbt, pad), hC((size_t)M * ldc, pad);
  for (int i = 0; i < M; ++i)
    for (int k = 0; k < K; ++k) hA[c.at ? (size_t)k * lda + i : (size_t)i * lda + k] = (T)a[(size_t)i * K + k];
  for (int j = 0; j < N; ++j)
    for (int k = 0; k < K; ++k) hB[(size_t)j * ldbt + k] = (T)b[(size_t)k * N + j];
  const size_t work_elems = c.work ? (size_t)16 * M * N : 0;
  Dev dA(hA.size() * sizeof(T)), dB(hB.size() * sizeof(T)), dC(hC.size() * sizeof(T)),
      dW(std::max<size_t>(work_elems, 1) * sizeof(T));
  dA.up(hA);
  dB.up(hB);
  dC.up(hC);
  if (!ef::tall_gemm_supported(lda, dA.p, sizeof(T)) || !ef::tall_gemm_supported(ldbt, dB.p, sizeof(T))) {
    std::printf("case=%s worst=inf rms=0 FAIL (operands not 16-byte aligned)\n", id.c_str());
    ++g_fail;
    return;
  }
  if constexpr (sizeof(T) == 8)
    HIP(ef::tall_gemm_f64(g_stream, dA.as<double>(), lda, c.at, dB.as<double>(), ldbt, dC.as<double>(), ldc, M, N, K,
                          alpha, c.work ? dW.as<double>() : nullptr, work_elems));
  else
    HIP(ef::tall_gemm_f32(g_stream, dA.as<float>(), lda, c.at, dB.as<float>(), ldbt, dC.as<float>(), ldc, M, N, K,
                          (float)alpha, c.work ? dW.as<float>() : nullptr, work_elems));
  dC.down(hC);
  const int64_t ns = tall_nsplit(M, N, K, work_elems);
  // R bound: K products and K + nsplit - 1 additions in some order, the scaling by alpha and
  // (fp32) nothing else: |C - C_ref| <= 2 (K + nsplit + 2) u 1.01 |alpha| sum_k |a_ik||b_kj|;
  // the factor 2 per operation allows matrix-core additions that do not round to nearest
  // (the allowance ef_search.hip makes), 1.01 the second-order terms.
  const double u = sizeof(T) == 8 ? kU64 : kU32;
  Stat st;
  for (int i = 0; i < M; ++i)
    for (int j = 0; j < N; ++j) {
      const T got = hC[(size_t)i * ldc + j];
      if (exact) {
        int64_t s = 0;
        for (int k = 0; k < K; ++k) s += (int64_t)a[(size_t)i * K + k] * (int64_t)b[(size_t)k * N + j];
        st.exact(same_bits<T>(got, (T)(alpha * (double)s)));
      } else {
        ld s = 0, sa = 0;
        for (int k = 0; k < K; ++k) {
          const ld p = (ld)a[(size_t)i * K + k] * (ld)b[(size_t)k * N + j];
          s += p;
          sa += fabsl(p);
        }
        st.add(fabsl((ld)got - (ld)alpha * s), 2 * (ld)(K + ns + 2) * u * 1.01L * std::fabs(alpha) * sa);
      }
    }
  // nothing written between the rows of C (ldc > N)
  for (int i = 0; i < M; ++i)
    for (int64_t j = N; j < ldc; ++j) st.exact(same_bits<T>(hC[(size_t)i * ldc + j], pad));
  char extra[64];
  std::snprintf(extra, sizeof extra, "nsplit=%lld", (long long)ns);
  if (exact) report_exact(id, st, extra);
  else report(id, st, extra);
}

static void transpose_case(int rows, int cols) {
  char idb[64];
  std::snprintf(idb, sizeof idb, "tall/transpose/%dx%d", rows, cols);
  if (g_list) { std::printf("%s\n", idb); return; }
  if (!wanted(idb)) return;
  const int64_t ldin = cols + 3, ldout = rows + 5;
  Rng rng(rows * 131 + cols);
  std::vector<double> in((size_t)rows * ldin), o64((size_t)cols * ldout, -777.25);
  std::vector<float> o32((size_t)cols * ldout, -777.25f);
  for (auto& x : in) x = rng.gauss() * std::ldexp(1.0, rng.range(-30, 30));
  Dev dI(in.size() * 8), d64(o64.size() * 8), d32(o32.size() * 4);
  dI.up(in);
  d64.up(o64);
  d32.up(o32);
  HIP(ef::launch_transpose_f64(g_stream, dI.as<double>(), ldin, rows, cols, d64.as<double>(), ldout));
  HIP(ef::launch_transpose_f64_to_f32(g_stream, dI.as<double>(), ldin, rows, cols, d32.as<float>(), ldout));
  d64.down(o64);
  d32.down(o32);
  Stat st;
  for (int c = 0; c < cols; ++c)
    for (int64_t r = 0; r < ldout; ++r) {
      const double e64 = r < rows ? in[(size_t)r * ldin + c] : -777.25;
      const float e32 = r < rows ? (float)in[(size_t)r * ldin + c] : -777.25f;
      st.exact(same_bits(o64[(size_t)c * ldout + r], e64));
      st.exact(same_bits(o32[(size_t)c * ldout + r], e32));
    }
  report_exact(idb, st);
}

static void group_tall() {
  for (const TallCase& c : tall_cases())
    for (int f32 = 0; f32 < 2; ++f32)
      for (int ex = 1; ex >= 0; --ex) {
        char idb[128];
        std::snprintf(idb, sizeof idb, "tall/%s/%s/M%d_N%d_K%d_%s_a%s_%s", f32 ? "f32" : "f64", ex ? "E" : "R", c.M, c.N,
                      c.K, c.at ? "at" : "an", c.half ? "0.5" : "1", c.work ? "work" : "nowork");
        if (g_list) { std::printf("%s\n", idb); continue; }
        if (!wanted(idb)) continue;
        if (f32) tall_run<float>(c, ex != 0, idb);
        else tall_run<double>(c, ex != 0, idb);
      }
  transpose_case(1, 1);
  transpose_case(31, 33);
  transpose_case(100, 257);
}

// ------------------------------------------------------------------ s3
// bf16 round-to-nearest-even of an fp32 value's bits, as split_f64_kernel computes it
static unsigned bf16_rne(float v) {
  unsigned u;
  std::memcpy(&u, &v, 4);
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
static float bf16_val(unsigned h) {
  const unsigned u = h << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
static void split_host(double x, float& hi, float& lo) {
  const float v = (float)x;
  const unsigned h = bf16_rne(v);
  hi = bf16_val(h);
  lo = bf16_val(bf16_rne(v - hi));
}

enum S3Kind { S3_E1, S3_E2, S3_R };

static double s3_entry(Rng& rng, S3Kind kind) {
  if (kind == S3_E1) return rng.range(-4, 4);
  if (kind == S3_R) return rng.real();
  // split-exact: h in +-{1, 2, 4}, l in +-{1, 2} 2^-10: bf16(x) = h and bf16(x - h) = l exactly
  const double h = (double)(1 << rng.range(0, 2)) * ((rng.next() & 1) ? -1 : 1);
  const double l = std::ldexp((double)rng.range(1, 2), -10) * ((rng.next() & 1) ? -1 : 1);
  return h + l;
}

// The R bound of the split product (the S3 == 1 branch of ef_fit.hip's reduce_kernel, applied
// componentwise).  Each operand x is carried as hi + lo with |x - hi - lo| <= 2^-17 |x|
// (two bf16 roundings of 2^-9 each, 2^-18, plus the fp32 rounding of x), and lo.lo' <=
// 2^-18 |x||x'| is dropped: per product at most (2 2^-17 + 2^-18 + ...) < 3.05 2^-16 |x||x'|.
// The 3K products of a sum, their K-range partial sums and the `splits` partial tiles are
// added in fp32: 2 (3K + splits + 2) 2^-24 1.01 (2 per operation for matrix-core adds that
// may not round to nearest).  The shift is one fp64 fma: 2^-52 |sigma q_ij| covers it and
// the rounding of the result.
static ld s3_bound(int64_t K, int splits, ld sabs, double sigma, double q) {
  return (3.05L * std::ldexp(1.0, -16) + 2 * (ld)(3 * K + splits + 2) * kU32 * 1.01L) * sabs +
         (ld)std::ldexp(1.0, -52) * fabsl((ld)sigma * q);
}

// host model of the split product: sum of hi.hi' + hi.lo' + lo.hi' in double
static double s3_model(const double* crow, const double* Q, int64_t K, int col) {
  double s = 0;
  for (int64_t k = 0; k < K; ++k) {
    float ch, cl, qh, ql;
    split_host(crow[k], ch, cl);
    split_host(Q[k * 256 + col], qh, ql);
    s += (double)ch * qh + (double)ch * ql + (double)cl * qh;
  }
  return s;
}

static void s3_case(int64_t M, int64_t K, S3Kind kind) {
  const char* kn = kind == S3_E1 ? "E1" : kind == S3_E2 ? "E2" : "R";
  char idb[96];
  std::snprintf(idb, sizeof idb, "s3/%s/M%lld_K%lld", kn, (long long)M, (long long)K);
  if (g_list) {
    std::printf("%s_s0\n%s_s0.37\n", idb, idb);
    return;
  }
  if (!wanted(idb)) return;
  Rng rng(77 + 3 * M + K + 1000 * (int)kind);
  std::vector<double> C((size_t)M * K), Q((size_t)K * 256), S((size_t)M * 256);
  for (auto& x : C) x = s3_entry(rng, kind);
  for (auto& x : Q) x = s3_entry(rng, kind);
  if (M == K) S = Q;  // the product's own use: Y = C.Q - sigma Q
  else
    for (auto& x : S) x = rng.real();
  Dev dC(C.size() * 8), dQ(Q.size() * 8), dS(S.size() * 8), dA3(C.size() * 4), dB3(Q.size() * 4),
      dP(ef::gemm_s3_part_elems(M) * 4), dY((size_t)M * 256 * 8);
  dC.up(C);
  dQ.up(Q);
  dS.up(S);
  if (!ef::gemm_s3_supported(M, K, 256)) {
    std::printf("case=%s worst=inf rms=0 FAIL (shape not supported)\n", idb);
    ++g_fail;
    return;
  }
  HIP(ef::launch_split_f64(g_stream, dC.as<double>(), M * K, dA3.p));
  HIP(ef::launch_transpose_split(g_stream, dQ.as<double>(), K, dB3.p));
  const int64_t mt = (M + 255) / 256;
  const int splits = (int)(ef::gemm_s3_part_elems(M) / (size_t)(mt * 256 * 256));

  // the split layouts themselves (per 8 elements 16 bytes of hi, then 16 of lo), on the
  // first tile's worth of rows
  if (M * K <= 512 * 512) {
    std::vector<uint16_t> a3(C.size() * 2), b3(Q.size() * 2);
    dA3.down(a3);
    dB3.down(b3);
    Stat st;
    for (int64_t e = 0; e < M * K; ++e) {
      float hi, lo;
      split_host(C[e], hi, lo);
      st.exact(a3[(e / 8) * 16 + e % 8] == bf16_rne(hi) && a3[(e / 8) * 16 + 8 + e % 8] == bf16_rne(lo));
    }
    for (int c = 0; c < 256; ++c)
      for (int64_t k = 0; k < K; ++k) {
        float hi, lo;
        split_host(Q[k * 256 + c], hi, lo);
        const int64_t e = (int64_t)c * K + k;
        st.exact(b3[(e / 8) * 16 + e % 8] == bf16_rne(hi) && b3[(e / 8) * 16 + 8 + e % 8] == bf16_rne(lo));
      }
    report_exact(std::string(idb) + "_layout", st);
  }

  // references on the sampled rows, once for both shifts
  const std::vector<int64_t> rows = sample_rows(M);
  std::vector<ld> ref(rows.size() * 256), sab(rows.size() * 256);
  std::vector<double> exact(rows.size() * 256);
  for (size_t ri = 0; ri < rows.size(); ++ri) {
    const double* cr = &C[(size_t)rows[ri] * K];
    if (kind == S3_R) {
      std::vector<ld> s(256, 0), sa(256, 0);
      for (int64_t k = 0; k < K; ++k) {
        const ld ck = cr[k];
        const double* qr = &Q[(size_t)k * 256];
        for (int c = 0; c < 256; ++c) {
          const ld p = ck * qr[c];
          s[c] += p;
          sa[c] += fabsl(p);
        }
      }
      for (int c = 0; c < 256; ++c) ref[ri * 256 + c] = s[c], sab[ri * 256 + c] = sa[c];
    } else {
      // integer reference in units of 2^-10: x = (1024 h + l') / 1024, the kept terms are
      // h h' + h l' + l h' (E1: l = 0), i.e. the full product minus l l'
      std::vector<int64_t> s(256, 0);
      for (int64_t k = 0; k < K; ++k) {
        const double x = cr[k], xh = std::nearbyint(x);
        const int64_t h = (int64_t)xh, l = (int64_t)std::nearbyint((x - xh) * 1024.0);
        const double* qr = &Q[(size_t)k * 256];
        for (int c = 0; c < 256; ++c) {
          const double y = qr[c], yh = std::nearbyint(y);
          const int64_t h2 = (int64_t)yh, l2 = (int64_t)std::nearbyint((y - yh) * 1024.0);
          s[c] += 1024 * h * h2 + h * l2 + l * h2;
        }
      }
      for (int c = 0; c < 256; ++c) exact[ri * 256 + c] = (double)s[c] / 1024.0;  // < 2^24 units: exact
    }
  }
  for (double sigma : {0.0, 0.37}) {
    HIP(ef::gemm_s3(g_stream, dA3.as<float>(), K, dB3.as<float>(), K, M, K, dP.as<float>(), dS.as<double>(), sigma,
                    dY.as<double>()));
    std::vector<double> Y((size_t)M * 256);
    dY.down(Y);
    Stat st;
    for (size_t ri = 0; ri < rows.size(); ++ri)
      for (int c = 0; c < 256; ++c) {
        const double got = Y[(size_t)rows[ri] * 256 + c], q = S[(size_t)rows[ri] * 256 + c];
        if (kind == S3_R)
          st.add(fabsl((ld)got - (ref[ri * 256 + c] - (ld)sigma * q)), s3_bound(K, splits, sab[ri * 256 + c], sigma, q));
        else
          st.exact(same_bits(got, std::fma(-sigma, q, exact[ri * 256 + c])));
      }
    char id2[128], extra[64];
    std::snprintf(id2, sizeof id2, "%s_s%g", idb, sigma);
    std::snprintf(extra, sizeof extra, "splits=%d rows=%zu", splits, rows.size());
    if (kind == S3_R) report(id2, st, extra);
    else report_exact(id2, st, extra);
  }
}

static void group_s3() {
  const int64_t shapes[4][2] = {{256, 32}, {288, 96}, {511, 512}, {4128, 4128}};
  for (auto& sh : shapes) {
    s3_case(sh[0], sh[1], S3_E1);
    if (sh[1] <= 512) s3_case(sh[0], sh[1], S3_E2);
    s3_case(sh[0], sh[1], S3_R);
  }
}

// ------------------------------------------------------------------ cq
// Host emulation of ef_cq_i8.hip, step by step as its header states the scheme.
static int oz_shift(double mx) {  // t with 2^t mx in [2^45, 2^46); 0 for an all-zero row / column
  int e = 0;
  if (mx > 0.0) (void)std::frexp(mx, &e);
  return mx > 0.0 ? 46 - e : 0;
}
static void oz_digits_host(double x, int t, int32_t* d, int stride) {
  long long v = (long long)std::rint(std::ldexp(x, t));
  for (int a = 0; a < 6; ++a) {
    const long long lo = ((v + 128) & 255) - 128;
    d[a * stride] = (int32_t)lo;
    v = (v - lo) / 256;
  }
}

struct CqData {
  int64_t dim;
  std::vector<double> C, Q;
};

static CqData cq_data(int64_t dim, bool exact) {
  CqData d;
  d.dim = dim;
  d.C.assign((size_t)dim * dim, 0.0);
  d.Q.assign((size_t)dim * 256, 0.0);
  Rng rng(4242 + dim + (exact ? 1 : 0));
  if (exact) {
    for (int64_t i = 0; i < dim; ++i)
      for (int64_t j = 0; j <= i; ++j) d.C[i * dim + j] = d.C[j * dim + i] = rng.range(-3, 3);
    for (auto& x : d.Q) x = rng.range(-3, 3);
    return d;
  }
  // (full 53-bit entries: every one of the six digits of both operands is in play)
  // C = D S D, S symmetric with |s| in [0.5, 1]: row maxima 2^(e_i + 20) span 2^-40..2^40;
  // row / column 5 all zero; row 100 at 1/16 the scale of rows 99 and 101
  std::vector<int> ex(dim);
  for (int64_t i = 0; i < dim; ++i) ex[i] = (i & 1) ? rng.range(16, 20) : rng.range(-60, 20);
  ex[0] = -60;
  ex[1] = 20;
  ex[99] = ex[101] = 10;
  ex[100] = 6;
  for (int64_t i = 0; i < dim; ++i)
    for (int64_t j = 0; j <= i; ++j) {
      double v = std::ldexp(rng.real64(), ex[i] + ex[j]);
      if (i == 5 || j == 5) v = 0.0;
      d.C[i * dim + j] = d.C[j * dim + i] = v;
    }
  // Q: column 7 zero, column 9 larger by 2^30
  for (int64_t k = 0; k < dim; ++k)
    for (int c = 0; c < 256; ++c) d.Q[k * 256 + c] = c == 7 ? 0.0 : (c == 9 ? std::ldexp(rng.real64(), 30) : rng.real64());
  return d;
}

// The digit pairs each form keeps, as ef_cq_i8.hip's header states them (not taken from the
// product's oz_pair, which --host compares against this): full, every pair within 2^-40 of
// the top, a + b >= 5 (21 pairs); medium, a, b >= 1 and a + b >= 6 (15 pairs).
static bool cq_kept(bool med, int a, int b) { return med ? (a >= 1 && b >= 1 && a + b >= 6) : (a + b >= 5); }

struct CqRef {
  std::vector<int64_t> rows;
  std::vector<double> emu[2];  // [medium]: the emulated C.Q before the shift (bit-equal target)
  std::vector<ld> bnd[2];      // [medium]: bound (b) without the final fma's rounding
  std::vector<ld> ref;         // long-double C.Q
};

// Bound (b), per entry, in the scaled integers X = 2^t_i c_ik, Z = 2^u_c q_kc and their
// roundings X', Z' (|X - X'|, |Z - Z'| <= 1/2):
//   roundings   |sum XZ - sum X'Z'| <= sum_k (|X'_ik| + |Z'_kc| + 1/2) / 2
//               (XZ - X'Z' = (X - X')Z + X'(Z - Z'), |Z| <= |Z'| + 1/2)
//   dropped     sum_k sum over the digit pairs (a, b) NOT kept of 256^(a+b) |x_a||z_b|
//               (full: a + b <= 4; medium: a = 0 or b = 0 or a + b <= 5)
//   Horner      nlev - 1 fp64 fma roundings, each of a partial value no larger than
//               T = sum_L 256^L |S_L|:  (nlev - 1) 2^-53 1.01 T 256^lev
// all times 2^-(t_i + u_c); plus 2^-53 1.01 |y| for the rounding of the final fma(-sigma, q, .).
// The sums S_L themselves are exact (int64) and ldexp is exact.
static CqRef cq_reference(const CqData& d) {
  const int64_t dim = d.dim;
  CqRef r;
  r.rows = sample_rows(dim);
  // and the rows cq_data makes special: the all-zero row, the row at 1/16 and its neighbours
  for (int64_t i : {5, 99, 100, 101})
    if (std::find(r.rows.begin(), r.rows.end(), i) == r.rows.end()) r.rows.push_back(i);
  const size_t nr = r.rows.size();
  for (int med = 0; med < 2; ++med) r.emu[med].assign(nr * 256, 0.0), r.bnd[med].assign(nr * 256, 0);
  r.ref.assign(nr * 256, 0);
  // Q's digits [k][b][c] and column shifts
  std::vector<int> tc(256);
  for (int c = 0; c < 256; ++c) {
    double mx = 0;
    for (int64_t k = 0; k < dim; ++k) mx = std::fmax(mx, std::fabs(d.Q[k * 256 + c]));
    tc[c] = oz_shift(mx);
  }
  std::vector<int32_t> qd((size_t)dim * 6 * 256);
  // W[med][k][a][c] = sum over b with (a, b) dropped of 256^b |z_b|; zabs[k][c] = |Z'|
  std::vector<double> W[2], zabs((size_t)dim * 256);
  bool kept[2][6][6] = {};
  for (int med = 0; med < 2; ++med) {
    for (int a = 0; a < 6; ++a)
      for (int b = 0; b < 6; ++b) kept[med][a][b] = cq_kept(med != 0, a, b);
    W[med].assign((size_t)dim * 6 * 256, 0.0);
  }
  for (int64_t k = 0; k < dim; ++k)
    for (int c = 0; c < 256; ++c) {
      oz_digits_host(d.Q[k * 256 + c], tc[c], &qd[(size_t)k * 6 * 256 + c], 256);
      zabs[k * 256 + c] = std::fabs(std::rint(std::ldexp(d.Q[k * 256 + c], tc[c])));
      for (int med = 0; med < 2; ++med)
        for (int a = 0; a < 6; ++a) {
          double w = 0;
          for (int b = 0; b < 6; ++b)
            if (!kept[med][a][b]) w += std::ldexp((double)std::abs(qd[((size_t)k * 6 + b) * 256 + c]), 8 * b);
          W[med][((size_t)k * 6 + a) * 256 + c] = w;
        }
    }
  if (6 * dim * 16384 >= (int64_t)1 << 31) {
    std::printf("cq reference: order too large for the int32 level sums\n");
    std::exit(1);
  }
  for (size_t ri = 0; ri < nr; ++ri) {
    const int64_t i = r.rows[ri];
    const double* row = &d.C[(size_t)i * dim];
    double mx = 0;
    for (int64_t k = 0; k < dim; ++k) mx = std::fmax(mx, std::fabs(row[k]));
    const int tr = oz_shift(mx);
    static int32_t S[2][6][256];
    static double drop[2][256], rnd[256];
    static ld ref[256];
    std::memset(S, 0, sizeof S);
    std::memset(drop, 0, sizeof drop);
    std::memset(rnd, 0, sizeof rnd);
    for (int c = 0; c < 256; ++c) ref[c] = 0;
    for (int64_t k = 0; k < dim; ++k) {
      int32_t ca[6];
      oz_digits_host(row[k], tr, ca, 1);
      const double xabs = std::fabs(std::rint(std::ldexp(row[k], tr)));
      const int32_t* q = &qd[(size_t)k * 6 * 256];
      for (int a = 0; a < 6; ++a) {
        if (ca[a] == 0) continue;
        const int32_t x = ca[a];
        for (int b = 0; b < 6; ++b) {
          if (!kept[0][a][b]) continue;
          int32_t* sf = S[0][a + b - 5];
          const int32_t* qb = q + b * 256;
          for (int c = 0; c < 256; ++c) sf[c] += x * qb[c];
          if (kept[1][a][b]) {
            int32_t* sm = S[1][a + b - 6];
            for (int c = 0; c < 256; ++c) sm[c] += x * qb[c];
          }
        }
        const double xa = std::ldexp((double)std::abs(x), 8 * a);
        for (int med = 0; med < 2; ++med) {
          const double* w = &W[med][((size_t)k * 6 + a) * 256];
          for (int c = 0; c < 256; ++c) drop[med][c] += xa * w[c];
        }
      }
      const double* za = &zabs[(size_t)k * 256];
      for (int c = 0; c < 256; ++c) rnd[c] += 0.5 * (xabs + za[c] + 0.5);
      const ld ck = row[k];
      const double* qr = &d.Q[(size_t)k * 256];
      for (int c = 0; c < 256; ++c) ref[c] += ck * qr[c];
    }
    for (int c = 0; c < 256; ++c) {
      r.ref[ri * 256 + c] = ref[c];
      for (int med = 0; med < 2; ++med) {
        const int lev = med ? 6 : 5, nlev = 11 - lev;
        double v = (double)S[med][nlev - 1][c];
        ld T = 0;
        for (int L = 0; L < nlev; ++L) T += ldexpl(fabsl((ld)S[med][L][c]), 8 * L);
        for (int L = nlev - 2; L >= 0; --L) v = std::fma(v, 256.0, (double)S[med][L][c]);
        r.emu[med][ri * 256 + c] = std::ldexp(v, 8 * lev - tr - tc[c]);
        const ld horner = (ld)(nlev - 1) * kU64 * 1.01L * ldexpl(T, 8 * lev);
        // 1.0001: the bound's own sums are accumulated in double
        r.bnd[med][ri * 256 + c] = ldexpl(1.0001L * ((ld)rnd[c] + (ld)drop[med][c]) + horner, -(tr + tc[c]));
      }
    }
  }
  return r;
}

static void cq_case(int64_t dim, bool exact, const std::vector<double>& sigmas) {
  char idb[64];
  std::snprintf(idb, sizeof idb, "cq/%s/dim%lld", exact ? "E" : "R", (long long)dim);
  if (g_list) {
    for (double s : sigmas)
      for (int med = 0; med < 2; ++med) std::printf("%s_%s_s%g\n", idb, med ? "medium" : "full", s);
    return;
  }
  if (!wanted(idb)) return;
  const CqData d = cq_data(dim, exact);
  const CqRef r = cq_reference(d);
  if (!ef::cq_i8_supported(dim, 256)) {
    std::printf("case=%s worst=inf rms=0 FAIL (order not supported)\n", idb);
    ++g_fail;
    return;
  }
  Dev dC(d.C.size() * 8), dQ(d.Q.size() * 8), dPl(ef::cq_i8_plane_bytes(dim), 65536),
      dW(ef::cq_i8_work_bytes(dim, 256), 65536), dY((size_t)dim * 256 * 8);
  dC.up(d.C);
  dQ.up(d.Q);
  HIP(ef::launch_cq_i8_planes(g_stream, dC.as<double>(), dim, dPl.p));
  std::vector<double> Y((size_t)dim * 256);
  for (double sigma : sigmas)
    for (int med = 0; med < 2; ++med) {
      HIP(ef::launch_cq_i8(g_stream, dPl.p, dim, dQ.as<double>(), 256, sigma, dW.p, dY.as<double>(), med != 0));
      dY.down(Y);
      Stat sa, sb;
      int64_t wrow = -1;  // where the worst ratio of the bound case sits
      int wcol = -1;
      for (size_t ri = 0; ri < r.rows.size(); ++ri)
        for (int c = 0; c < 256; ++c) {
          const size_t e = (size_t)r.rows[ri] * 256 + c;
          const double q = d.Q[e], got = Y[e];
          const double emu = std::fma(-sigma, q, r.emu[med][ri * 256 + c]);
          sa.exact(same_bits(got, emu));
          if (exact) {  // the integer product itself: every digit pair of it is kept
            int64_t s = 0;  // (computed from the long-double sum, exact for these inputs)
            s = (int64_t)llrintl(r.ref[ri * 256 + c]);
            sb.exact(same_bits(got, std::fma(-sigma, q, (double)s)));
          } else {
            const ld want = r.ref[ri * 256 + c] - (ld)sigma * q;
            const double before = sb.worst;
            sb.add(fabsl((ld)got - want), r.bnd[med][ri * 256 + c] + (ld)kU64 * 1.01L * fabsl((ld)emu));
            if (sb.worst > before) wrow = r.rows[ri], wcol = c;
          }
        }
      char id2[128];
      std::snprintf(id2, sizeof id2, "%s_%s_s%g", idb, med ? "medium" : "full", sigma);
      report_exact(std::string(id2) + "/emulation", sa);
      if (exact) report_exact(std::string(id2) + "/integer", sb);
      else report(std::string(id2) + "/bound", sb, "at row " + std::to_string(wrow) + " col " + std::to_string(wcol));
    }
}

static void group_cq() {
  cq_case(2048, true, {0.0, 0.37});
  cq_case(2048, false, {0.0, 0.37});
  cq_case(4096, false, {0.37});
}

// ------------------------------------------------------------------ symmetric test matrices
// D (a spectrum on the diagonal) under nrefl random Householder reflections, in long double:
// an orthogonal similarity, rounded to double once at the end and exactly symmetric.
static std::vector<double> sym_from_spectrum(const std::vector<double>& spec, int nrefl, Rng& rng) {
  const int m = (int)spec.size();
  std::vector<ld> A((size_t)m * m, 0), v(m), p(m);
  for (int i = 0; i < m; ++i) A[(size_t)i * m + i] = spec[i];
  for (int t = 0; t < nrefl && m > 1; ++t) {
    ld vv = 0;
    for (int i = 0; i < m; ++i) v[i] = rng.gauss(), vv += v[i] * v[i];
    const ld beta = 2 / vv;
    ld pv = 0;
    for (int i = 0; i < m; ++i) {
      ld s = 0;
      for (int j = 0; j < m; ++j) s += A[(size_t)i * m + j] * v[j];
      p[i] = beta * s;
      pv += p[i] * v[i];
    }
    const ld kk = beta * pv / 2;
    for (int i = 0; i < m; ++i) p[i] -= kk * v[i];
    for (int i = 0; i < m; ++i)
      for (int j = 0; j < m; ++j) A[(size_t)i * m + j] -= v[i] * p[j] + p[i] * v[j];
  }
  std::vector<double> out((size_t)m * m);
  for (int i = 0; i < m; ++i)
    for (int j = 0; j <= i; ++j)
      out[(size_t)i * m + j] = out[(size_t)j * m + i] = (double)((A[(size_t)i * m + j] + A[(size_t)j * m + i]) / 2);
  return out;
}

static std::vector<double> spd_matrix(int m, double cond, uint64_t seed) {
  Rng rng(seed);
  std::vector<double> spec(m);
  for (int i = 0; i < m; ++i) spec[i] = m == 1 ? 1.0 : std::pow(cond, -(double)i / (m - 1));
  return sym_from_spectrum(spec, std::min(m, 48), rng);
}

// ------------------------------------------------------------------ chol
// plain host Cholesky (double, long-double dot products); false on a non-positive pivot
static bool chol_host(const std::vector<double>& A, int m, std::vector<double>& L) {
  L.assign((size_t)m * m, 0.0);
  for (int j = 0; j < m; ++j)
    for (int i = j; i < m; ++i) {
      ld s = A[(size_t)i * m + j];
      for (int k = 0; k < j; ++k) s -= (ld)L[(size_t)i * m + k] * L[(size_t)j * m + k];
      if (i == j) {
        if (!(s > 0)) return false;
        L[(size_t)j * m + j] = (double)sqrtl(s);
      } else {
        L[(size_t)i * m + j] = (double)(s / L[(size_t)j * m + j]);
      }
    }
  return true;
}
static void tri_inv_host(const std::vector<double>& L, int m, std::vector<double>& Li) {
  Li.assign((size_t)m * m, 0.0);
  for (int j = 0; j < m; ++j)
    for (int i = j; i < m; ++i) {
      ld s = i == j ? 1 : 0;
      for (int k = j; k < i; ++k) s -= (ld)L[(size_t)i * m + k] * Li[(size_t)k * m + j];
      Li[(size_t)i * m + j] = (double)(s / L[(size_t)i * m + i]);
    }
}

// |A - L L^T| <= 4 gamma_{m+1} |L||L^T| componentwise (Higham, Accuracy and Stability, thm
// 10.3 has gamma_{m+1}; the 4 allows a reciprocal / reciprocal square root by Newton steps
// instead of correctly rounded division and square root), and zeros above the diagonal.
// L row-major with stride ldl.
static Stat chol_certificate(const std::vector<double>& A, int m, const double* L, int64_t ldl) {
  Stat st;
  const ld g = 4 * gamma_n(m + 1);
  for (int i = 0; i < m; ++i)
    for (int j = 0; j <= i; ++j) {
      ld s = 0, sa = 0;
      for (int k = 0; k <= j; ++k) {
        const ld p = (ld)L[(size_t)i * ldl + k] * L[(size_t)j * ldl + k];
        s += p;
        sa += fabsl(p);
      }
      st.add(fabsl((ld)A[(size_t)i * m + j] - s), g * sa);
    }
  for (int i = 0; i < m; ++i)
    for (int j = i + 1; j < m; ++j) st.exact(L[(size_t)i * ldl + j] == 0.0);
  return st;
}
// |L Li - I| <= 2 gamma_m |L||Li| componentwise (forward substitution per column: Higham thm
// 8.5 gives gamma_m; the 2 for the dot products' lane-split summation order and the
// division), zeros above the diagonal of Li
static Stat tri_certificate(const std::vector<double>& L, int m, const std::vector<double>& Li) {
  Stat st;
  const ld g = 2 * gamma_n(m);
  for (int i = 0; i < m; ++i)
    for (int j = 0; j <= i; ++j) {
      ld s = 0, sa = 0;
      for (int k = j; k <= i; ++k) {
        const ld p = (ld)L[(size_t)i * m + k] * Li[(size_t)k * m + j];
        s += p;
        sa += fabsl(p);
      }
      st.add(fabsl(s - (i == j ? 1 : 0)), g * sa);
    }
  for (int i = 0; i < m; ++i)
    for (int j = i + 1; j < m; ++j) st.exact(Li[(size_t)i * m + j] == 0.0);
  return st;
}

// L0 D L0^T with L0 = 2 I + strictly lower entries in {-1, 0, 1} / 8 and D = I except
// D_jj = -1: the leading j x j block is positive definite and pivot j is -4 exactly in exact
// arithmetic (about -4 in floating point), whatever the rest
static std::vector<double> failing_matrix(int m, int jbad, uint64_t seed) {
  Rng rng(seed);
  std::vector<double> L0((size_t)m * m, 0.0), A((size_t)m * m);
  for (int i = 0; i < m; ++i) {
    L0[(size_t)i * m + i] = 2.0;
    for (int j = 0; j < i; ++j) L0[(size_t)i * m + j] = rng.range(-1, 1) / 8.0;
  }
  for (int i = 0; i < m; ++i)
    for (int j = 0; j <= i; ++j) {
      ld s = 0;
      for (int k = 0; k <= j; ++k) s += (ld)L0[(size_t)i * m + k] * L0[(size_t)j * m + k] * (k == jbad ? -1 : 1);
      A[(size_t)i * m + j] = A[(size_t)j * m + i] = (double)s;
    }
  return A;
}

static const double kCholTol = 1e-13;  // the relative pivot tolerance ef_fit.hip passes

static void group_chol() {
  for (int m : {1, 31, 32, 33, 257, 300, 512})
    for (double cond : {1e2, 1e10}) {
      char idb[64];
      std::snprintf(idb, sizeof idb, "chol/factor/m%d_cond%g", m, cond);
      if (g_list) { std::printf("%s\n", idb); continue; }
      if (!wanted(idb)) continue;
      const std::vector<double> A = spd_matrix(m, cond, 900 + m);
      const int64_t lda = m + 3;
      std::vector<double> hA((size_t)m * lda, -777.25);
      for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) hA[(size_t)i * lda + j] = A[(size_t)i * m + j];
      std::vector<int> info(1, 12345);
      Dev dA(hA.size() * 8), dI(16);
      dA.up(hA);
      dI.up(info);
      HIP(ef::launch_cholesky(g_stream, dA.as<double>(), m, lda, kCholTol, dI.as<int>()));
      dA.down(hA);
      dI.down(info);
      Stat st = chol_certificate(A, m, hA.data(), lda);
      st.exact(info[0] == 0);
      for (int i = 0; i < m; ++i)
        for (int64_t j = m; j < lda; ++j) st.exact(hA[(size_t)i * lda + j] == -777.25);
      char extra[32];
      std::snprintf(extra, sizeof extra, "info=%d", info[0]);
      report(idb, st, extra);
    }
  for (int m : {31, 257, 512})
    for (int jb : {0, 17, m - 1}) {
      char idb[64];
      std::snprintf(idb, sizeof idb, "chol/pivot/m%d_j%d", m, jb);
      if (g_list) { std::printf("%s\n", idb); continue; }
      if (!wanted(idb)) continue;
      std::vector<double> A = failing_matrix(m, jb, 31 * m + jb);
      std::vector<int> info(1, 12345);
      Dev dA(A.size() * 8), dI(16);
      dA.up(A);
      dI.up(info);
      HIP(ef::launch_cholesky(g_stream, dA.as<double>(), m, m, kCholTol, dI.as<int>()));
      dI.down(info);
      Stat st;
      st.exact(info[0] == -(jb + 1));
      char extra[32];
      std::snprintf(extra, sizeof extra, "info=%d", info[0]);
      report_exact(idb, st, extra);
    }
  for (int m : {1, 3, 64, 65, 257, 512}) {
    char idb[64];
    std::snprintf(idb, sizeof idb, "chol/tri_inv/m%d", m);
    if (g_list) { std::printf("%s\n", idb); continue; }
    if (!wanted(idb)) continue;
    std::vector<double> L, Li((size_t)m * m, -777.25);
    if (!chol_host(spd_matrix(m, 1e2, 500 + m), m, L)) {
      std::printf("case=%s worst=inf rms=0 FAIL (host factor)\n", idb);
      ++g_fail;
      continue;
    }
    Dev dL(L.size() * 8), dLi(Li.size() * 8);
    dL.up(L);
    dLi.up(Li);
    HIP(ef::launch_tri_inv(g_stream, dL.as<double>(), m, dLi.as<double>()));
    dLi.down(Li);
    report(idb, tri_certificate(L, m, Li));
  }
}

// ------------------------------------------------------------------ jacobi
// Plain cyclic Jacobi on the host (T = double: what double precision reaches; T = long
// double: the reference eigenvalues).  A rotation is skipped when |a_pq| <= tol sqrt(|a_pp
// a_qq|); a sweep without rotations ends it.  Eigenvalues descending, vectors in columns.
template <class T>
static void jacobi_host(const std::vector<double>& A0, int m, T tol, std::vector<T>& lam, std::vector<T>& V) {
  std::vector<T> A((size_t)m * m);
  for (size_t i = 0; i < A.size(); ++i) A[i] = A0[i];
  V.assign((size_t)m * m, 0);
  for (int i = 0; i < m; ++i) V[(size_t)i * m + i] = 1;
  for (int sweep = 0; sweep < 60; ++sweep) {
    int rot = 0;
    for (int p = 0; p < m - 1; ++p)
      for (int q = p + 1; q < m; ++q) {
        const T apq = A[(size_t)p * m + q], app = A[(size_t)p * m + p], aqq = A[(size_t)q * m + q];
        if (apq == 0 || std::fabs(apq) <= tol * std::sqrt(std::fabs(app * aqq))) continue;
        ++rot;
        const T theta = (aqq - app) / (2 * apq);
        T t = 1 / (std::fabs(theta) + std::sqrt(theta * theta + 1));
        if (theta < 0) t = -t;
        const T c = 1 / std::sqrt(t * t + 1), s = t * c;
        for (int k = 0; k < m; ++k) {
          const T kp = A[(size_t)k * m + p], kq = A[(size_t)k * m + q];
          A[(size_t)k * m + p] = c * kp - s * kq;
          A[(size_t)k * m + q] = s * kp + c * kq;
          const T vp = V[(size_t)k * m + p], vq = V[(size_t)k * m + q];
          V[(size_t)k * m + p] = c * vp - s * vq;
          V[(size_t)k * m + q] = s * vp + c * vq;
        }
        for (int k = 0; k < m; ++k) {
          const T pk = A[(size_t)p * m + k], qk = A[(size_t)q * m + k];
          A[(size_t)p * m + k] = c * pk - s * qk;
          A[(size_t)q * m + k] = s * pk + c * qk;
        }
        A[(size_t)p * m + q] = A[(size_t)q * m + p] = 0;
      }
    if (!rot) break;
  }
  std::vector<int> ord(m);
  for (int i = 0; i < m; ++i) ord[i] = i;
  std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return A[(size_t)a * m + a] > A[(size_t)b * m + b]; });
  lam.resize(m);
  std::vector<T> Vs((size_t)m * m);
  for (int j = 0; j < m; ++j) {
    lam[j] = A[(size_t)ord[j] * m + ord[j]];
    for (int k = 0; k < m; ++k) Vs[(size_t)k * m + j] = V[(size_t)k * m + ord[j]];
  }
  V.swap(Vs);
}

struct EigQuality {
  ld resid = 0, orth = 0, orth_diag = 0, trace_err = 0, normF = 0;  // orth_diag: the norms' part of orth
  bool descending = true;
};
// measured in long double; lam, V (columns, stride ldv) of any real type
template <class T>
static EigQuality eig_quality(const std::vector<double>& A, int m, const T* lam, const T* V, int64_t ldv) {
  EigQuality q;
  ld tr = 0, sl = 0;
  for (int i = 0; i < m; ++i) {
    tr += A[(size_t)i * m + i];
    sl += lam[i];
    if (i && !(lam[i - 1] >= lam[i])) q.descending = false;
    for (int j = 0; j < m; ++j) q.normF += (ld)A[(size_t)i * m + j] * A[(size_t)i * m + j];
  }
  q.normF = sqrtl(q.normF);
  q.trace_err = fabsl(sl - tr);
  std::vector<ld> r(m);
  for (int j = 0; j < m; ++j) {
    ld n2 = 0;
    for (int i = 0; i < m; ++i) {
      ld s = 0;
      for (int k = 0; k < m; ++k) s += (ld)A[(size_t)i * m + k] * V[(size_t)k * ldv + j];
      s -= (ld)lam[j] * V[(size_t)i * ldv + j];
      n2 += s * s;
    }
    q.resid = std::max(q.resid, sqrtl(n2));
  }
  for (int a = 0; a < m; ++a)
    for (int b = a; b < m; ++b) {
      ld s = 0;
      for (int k = 0; k < m; ++k) s += (ld)V[(size_t)k * ldv + a] * V[(size_t)k * ldv + b];
      q.orth = std::max(q.orth, fabsl(s - (a == b ? 1 : 0)));
      if (a == b) q.orth_diag = std::max(q.orth_diag, fabsl(s - 1));
    }
  return q;
}

static const char* kJacNames[6] = {"geometric", "clustered", "diagonal", "zero", "rankone", "indefinite"};

static std::vector<double> jacobi_matrix(int m, int type, uint64_t seed) {
  Rng rng(seed);
  std::vector<double> spec(m, 0.0);
  switch (type) {
    case 0:  // random orthogonal x geometric spectrum 1 .. 1e-12
      for (int i = 0; i < m; ++i) spec[i] = m == 1 ? 1.0 : std::pow(1e-12, (double)i / (m - 1));
      return sym_from_spectrum(spec, m, rng);
    case 1:  // eight exactly equal eigenvalues, a pair 1e-14 apart, the rest spread
      for (int i = 0; i < m; ++i) spec[i] = i < 8 ? 0.5 : (i == 8 ? 0.25 : (i == 9 ? 0.25 + 1e-14 : 0.6 + 0.4 * rng.uni()));
      return sym_from_spectrum(spec, m, rng);
    case 2: {  // already diagonal, unsorted, both signs and a repeat
      std::vector<double> A((size_t)m * m, 0.0);
      for (int i = 0; i < m; ++i) A[(size_t)i * m + i] = i == 3 ? 0.75 : (i == 1 ? 0.75 : rng.gauss());
      return A;
    }
    case 3:
      return std::vector<double>((size_t)m * m, 0.0);
    case 4: {  // rank one
      std::vector<double> x(m), A((size_t)m * m);
      for (auto& v : x) v = rng.real();
      for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) A[(size_t)i * m + j] = x[i] * x[j];
      return A;
    }
    default:  // half the spectrum geometric 1 .. 1e-6, the rest +-1e-17 (a Gram of rounded data)
      for (int i = 0; i < m; ++i) {
        const int r = (m + 1) / 2;
        spec[i] = i < r ? std::pow(1e-6, r == 1 ? 0.0 : (double)i / (r - 1)) : ((rng.next() & 1) ? 1e-17 : -1e-17);
      }
      return sym_from_spectrum(spec, m, rng);
  }
}

struct JacHostRef {
  std::vector<double> A;
  ld r_host = 0, o_host = 0, r_ld = 0, norm2 = 0;
  std::vector<ld> lam;
};
static JacHostRef jacobi_host_ref(int m, int type) {
  JacHostRef h;
  h.A = jacobi_matrix(m, type, 7000 + 10 * m + type);
  std::vector<double> lam, V;
  jacobi_host<double>(h.A, m, 1e-15, lam, V);
  const EigQuality q = eig_quality(h.A, m, lam.data(), V.data(), m);
  h.r_host = q.resid;
  h.o_host = q.orth;
  std::vector<ld> Vl;
  jacobi_host<ld>(h.A, m, 1e-19L, h.lam, Vl);
  h.r_ld = eig_quality(h.A, m, h.lam.data(), Vl.data(), m).resid;
  for (ld x : h.lam) h.norm2 = std::max(h.norm2, fabsl(x));
  return h;
}

// Thresholds, computed for the matrix at hand:
//   residual   m tol |A|_F + 4 r_host: every off-diagonal entry left is <= tol |A|_2, and
//              r_host is the residual of the plain double-precision host Jacobi (tol 1e-15);
//   orthogon.  4 o_host, likewise; the 4 covers the block method's other rotation order;
//   eigenvalue |lam - lam_ref| <= residual + |A|_2 orthogonality (Weyl) + the long-double
//              reference's own residual;
//   trace      |sum lam - trace A| <= m times the eigenvalue threshold.
static void jacobi_judge(const std::string& id, const JacHostRef& h, int m, double tol, const std::vector<double>& lam,
                         const std::vector<double>& V, int64_t ldv, bool converged, int sweeps, int max_sweeps) {
  const EigQuality q = eig_quality(h.A, m, lam.data(), V.data(), ldv);
  const ld r_thr = (ld)m * tol * q.normF + 4 * h.r_host, o_thr = 4 * h.o_host;
  ld eig = 0;
  for (int i = 0; i < m; ++i) eig = std::max(eig, fabsl((ld)lam[i] - h.lam[i]));
  const ld e_thr = q.resid + h.norm2 * q.orth + h.r_ld;
  Stat st;
  st.add(q.resid, r_thr);
  st.add(q.orth, o_thr);
  st.add(eig, e_thr);
  st.add(q.trace_err, (ld)m * (r_thr + h.norm2 * o_thr + h.r_ld));
  st.exact(q.descending);
  st.exact(converged && sweeps <= max_sweeps);
  int stray = 0;  // nothing written between the rows of evecs (ldv > m; pre-filled by the caller)
  for (int i = 0; i < m; ++i)
    for (int64_t j = m; j < ldv; ++j) stray += V[(size_t)i * ldv + j] != -777.25;
  st.exact(stray == 0);
  char extra[320];
  std::snprintf(extra, sizeof extra,
                "res=%.3Lg res_host=%.3Lg res_thr=%.3Lg orth=%.3Lg orth_diag=%.3Lg orth_host=%.3Lg eig=%.3Lg eig_thr=%.3Lg trace=%.3Lg "
                "sweeps=%d conv=%d desc=%d stray=%d",
                q.resid, h.r_host, r_thr, q.orth, q.orth_diag, h.o_host, eig, e_thr, q.trace_err, sweeps, (int)converged,
                (int)q.descending, stray);
  report(id, st, extra);
}

static const int kSweeps = 60;  // ef_fit.hip's kMaxSweeps

// The host references of the wanted (order, spectrum) pairs, computed side by side on up to
// 8 threads before the first launch (the long-double Jacobi at the largest order is most of
// the group's time).
typedef std::map<std::pair<int, int>, JacHostRef> JacRefs;
static JacRefs jacobi_host_refs(const std::vector<std::pair<int, int>>& keys) {
  std::vector<JacHostRef> out(keys.size());
  std::atomic<size_t> next{0};
  auto work = [&] {
    for (size_t i; (i = next.fetch_add(1)) < keys.size();) out[i] = jacobi_host_ref(keys[i].first, keys[i].second);
  };
  const unsigned hw = std::thread::hardware_concurrency();
  const size_t nt = std::min<size_t>(std::min<size_t>(8, hw ? hw : 4), keys.size());
  std::vector<std::thread> th;
  for (size_t t = 1; t < nt; ++t) th.emplace_back(work);
  work();
  for (auto& t : th) t.join();
  JacRefs refs;
  for (size_t i = 0; i < keys.size(); ++i) refs[keys[i]] = std::move(out[i]);
  return refs;
}

static void group_jacobi() {
  JacRefs refs;
  if (!g_list) {
    std::vector<std::pair<int, int>> keys;  // the largest orders first
    for (int m : {272, 161, 160, 129, 128, 127, 90, 89, 88, 87, 17, 3, 2, 1})
      for (int type = 0; type < 6; ++type) {
        char pre[64];
        std::snprintf(pre, sizeof pre, "/m%d_%s", m, kJacNames[type]);
        bool any = !g_only;
        for (const char* tail : {"", "_tol1e-12", "_tol1e-06"})
          for (const char* path : {"jacobi/lds", "jacobi/scalar", "jacobi/block"})
            any = any || wanted(std::string(path) + pre + tail);
        if (any) keys.push_back({m, type});
      }
    refs = jacobi_host_refs(keys);
  }
  for (int m : {1, 2, 3, 17, 87, 88})
    for (int type = 0; type < 6; ++type) {
      char idb[96];
      std::snprintf(idb, sizeof idb, "jacobi/lds/m%d_%s", m, kJacNames[type]);
      if (g_list) { std::printf("%s\n", idb); continue; }
      if (!wanted(idb)) continue;
      const JacHostRef& h = refs.at({m, type});
      const int64_t lda = m + 3, ldv = m + 5;
      std::vector<double> hA((size_t)m * lda, 0.0), lam(m, -777.25), V((size_t)m * ldv, -777.25);
      for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) hA[(size_t)i * lda + j] = h.A[(size_t)i * m + j];
      std::vector<int> info(1, 12345);
      Dev dA(hA.size() * 8), dL(lam.size() * 8), dV(V.size() * 8), dI(16);
      dA.up(hA);
      dV.up(V);
      dI.up(info);
      HIP(ef::launch_jacobi(g_stream, dA.as<double>(), m, lda, dL.as<double>(), dV.as<double>(), ldv, kSweeps,
                            dI.as<int>()));
      dL.down(lam);
      dV.down(V);
      dI.down(info);
      // the kernel rotates until |a_pq| is below 2^-53 / 100 of both diagonal entries
      jacobi_judge(idb, h, m, kU64, lam, V, ldv, info[0] >= 1, info[0], kSweeps);
    }
  for (int m : {89, 90, 127, 128, 129, 160, 161, 272}) {
    const bool block = m >= 128;
    bool any = false;
    auto case_id = [&](int type, double tol) {
      char idb[96];
      std::snprintf(idb, sizeof idb, "jacobi/%s/m%d_%s_tol%g", block ? "block" : "scalar", m, kJacNames[type], tol);
      return std::string(idb);
    };
    for (int type = 0; type < 6 && !g_list; ++type) any = any || wanted(case_id(type, 1e-12)) || wanted(case_id(type, 1e-6));
    if (!any && !g_list) continue;
    // one solver object per order: every solve after the first reuses its graphs and buffers
    ef::JacobiBig big;
    const int64_t lda = m + 3, ldv = m + 5;
    std::vector<double> hA((size_t)m * lda, 0.0), lam(m), V((size_t)m * ldv);
    Dev* dW = nullptr;
    Dev* dF = nullptr;
    Dev* dA = nullptr;
    Dev* dL = nullptr;
    Dev* dV = nullptr;
    if (!g_list) {
      dW = new Dev(ef::jacobi_big_work_elems(m) * 8);
      dF = new Dev(64);
      dA = new Dev(hA.size() * 8);
      dL = new Dev(lam.size() * 8);
      dV = new Dev(V.size() * 8);
      HIP(big.init(m, dW->as<double>(), dF->as<int>(), g_stream));
    }
    for (int type = 0; type < 6; ++type) {
      for (double tol : {1e-12, 1e-6}) {
        if (!block && tol != 1e-12) continue;  // the scalar rounds always use 1e-12
        const std::string idb = case_id(type, tol);
        if (g_list) { std::printf("%s\n", idb.c_str()); continue; }
        if (!wanted(idb)) continue;
        const JacHostRef& h = refs.at({m, type});
        for (int i = 0; i < m; ++i)
          for (int j = 0; j < m; ++j) hA[(size_t)i * lda + j] = h.A[(size_t)i * m + j];
        std::fill(V.begin(), V.end(), -777.25);
        dA->up(hA);
        dV->up(V);
        int sweeps = 0;
        hipError_t err = hipSuccess;
        const int rc = big.solve(g_stream, dA->as<double>(), lda, dL->as<double>(), dV->as<double>(), ldv, kSweeps,
                                 &sweeps, &err, tol);
        HIP(err);
        dL->down(lam);
        dV->down(V);
        jacobi_judge(idb, h, m, tol, lam, V, ldv, rc == 0, sweeps, kSweeps);
      }
    }
    if (!g_list) {
      HIP(hipStreamSynchronize(g_stream));
      big.destroy();
      delete dV;
      delete dL;
      delete dA;
      delete dF;
      delete dW;
    }
  }
}

// ------------------------------------------------------------------ host self-checks
// The references against their own thresholds, before any kernel is involved.
static void group_host() {
  for (int med = 0; med < 2; ++med) {  // the product's pair enumeration is the stated pair set, each pair once
    int seen[6][6] = {};
    for (int p = 0; p < ef::oz_pairs(med != 0); ++p) {
      int a = -1, b = -1;
      ef::oz_pair(p, med != 0, a, b);
      if (a >= 0 && a < 6 && b >= 0 && b < 6) ++seen[a][b];
    }
    Stat st;
    st.exact(ef::oz_pairs(med != 0) == (med ? 15 : 21));
    for (int a = 0; a < 6; ++a)
      for (int b = 0; b < 6; ++b) st.exact(seen[a][b] == (cq_kept(med != 0, a, b) ? 1 : 0));
    report_exact(std::string("host/cq/pair_set_") + (med ? "medium" : "full"), st);
  }
  {  // cq: the emulation against the long-double product, inside bound (b), both forms
    const CqData d = cq_data(2048, false);
    const CqRef r = cq_reference(d);
    for (int med = 0; med < 2; ++med) {
      Stat st;
      for (size_t e = 0; e < r.ref.size(); ++e) st.add(fabsl((ld)r.emu[med][e] - r.ref[e]), r.bnd[med][e]);
      report(std::string("host/cq/emulation_") + (med ? "medium" : "full"), st);
    }
    const CqData de = cq_data(2048, true);
    const CqRef re = cq_reference(de);
    for (int med = 0; med < 2; ++med) {
      Stat st;
      for (size_t e = 0; e < re.ref.size(); ++e) st.exact((ld)re.emu[med][e] == re.ref[e]);
      report_exact(std::string("host/cq/integer_") + (med ? "medium" : "full"), st);
    }
  }
  {  // s3: hi.hi' + hi.lo' + lo.hi' in double against the long-double product
    const int64_t M = 64, K = 512;
    Rng rng(5);
    std::vector<double> C((size_t)M * K), Q((size_t)K * 256);
    for (auto& x : C) x = rng.real();
    for (auto& x : Q) x = rng.real();
    Stat st;
    for (int64_t i = 0; i < M; ++i)
      for (int c = 0; c < 256; ++c) {
        ld s = 0, sa = 0;
        for (int64_t k = 0; k < K; ++k) {
          const ld p = (ld)C[i * K + k] * Q[k * 256 + c];
          s += p;
          sa += fabsl(p);
        }
        st.add(fabsl((ld)s3_model(&C[i * K], Q.data(), K, c) - s), s3_bound(K, 1, sa, 0.0, 0.0));
      }
    report("host/s3/split_model", st);
    // split-exact entries: hi = h and lo = l
    Rng r2(6);
    Stat se;
    for (int i = 0; i < 4096; ++i) {
      const double x = s3_entry(r2, S3_E2);
      float hi, lo;
      split_host(x, hi, lo);
      se.exact((double)hi == std::nearbyint(x) && (double)hi + (double)lo == x);
    }
    report_exact("host/s3/split_exact_entries", se);
  }
  for (int m : {33, 257}) {  // Cholesky and inverse references against their certificates
    for (double cond : {1e2, 1e10}) {
      const std::vector<double> A = spd_matrix(m, cond, 900 + m);
      std::vector<double> L, Li;
      char idb[64];
      std::snprintf(idb, sizeof idb, "host/chol/m%d_cond%g", m, cond);
      if (!chol_host(A, m, L)) {
        std::printf("case=%s worst=inf rms=0 FAIL\n", idb);
        ++g_fail;
        continue;
      }
      report(idb, chol_certificate(A, m, L.data(), m));
      tri_inv_host(L, m, Li);
      std::snprintf(idb, sizeof idb, "host/tri_inv/m%d_cond%g", m, cond);
      report(idb, tri_certificate(L, m, Li));
    }
    std::vector<double> L;
    Stat st;
    st.exact(!chol_host(failing_matrix(m, 17, m), m, L));
    report_exact("host/chol/pivot_m" + std::to_string(m), st);
  }
  for (int m : {3, 17, 129})  // the host Jacobi against the thresholds a device result must meet
    for (int type = 0; type < 6; ++type) {
      const JacHostRef h = jacobi_host_ref(m, type);
      std::vector<double> lam, V;
      jacobi_host<double>(h.A, m, 1e-15, lam, V);
      jacobi_judge("host/jacobi/m" + std::to_string(m) + "_" + kJacNames[type], h, m, 1e-15, lam, V, m, true, 1, 1);
    }
}

// ------------------------------------------------------------------ main
int main(int argc, char** argv) {
  const std::string g = argc > 1 ? argv[1] : "";
  g_only = argc > 2 ? argv[2] : nullptr;
  if (g == "--list") {
    g_list = true;
    std::printf("groups: tall s3 cq chol jacobi (and --host)\n");
    group_tall();
    group_s3();
    group_cq();
    group_chol();
    group_jacobi();
    return 0;
  }
  if (g == "--host") {
    group_host();
    std::printf("kernel_units --host: %s\n", g_fail ? "FAILED" : "ok");
    return g_fail ? 1 : 0;
  }
  void (*fn)() = g == "tall" ? group_tall : g == "s3" ? group_s3 : g == "cq" ? group_cq : g == "chol" ? group_chol
                 : g == "jacobi" ? group_jacobi : nullptr;
  if (!fn) {
    std::printf("usage: kernel_units <tall|s3|cq|chol|jacobi> [case] | --list | --host\n");
    return 64;
  }
  HIP(hipSetDevice(0));
  HIP(hipStreamCreate(&g_stream));
  fn();
  HIP(hipStreamSynchronize(g_stream));
  HIP(hipStreamDestroy(g_stream));
  std::printf("kernel_units %s: %s\n", g.c_str(), g_fail ? "FAILED" : "ok");
  return g_fail ? 1 : 0;
}
