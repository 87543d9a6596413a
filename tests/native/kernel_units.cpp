// Kernel-level checks of the fit's matrix-product and eigen-solver kernels (Makefile target
// `kernel_units`, run by tests/test_gpu_kernel_units.py).  The program links the product
// objects, creates one stream and calls the ef:: launchers of csrc/ef_linalg.hpp directly;
// every case has a host reference of its own in plain loops (long double for real-valued
// cases, int64 / __int128 for integer ones).
//
//   kernel_units --list            groups and cases
//   kernel_units <group> [case]    tall | s3 | cq | chol | jacobi | cov | proj  (GPU)
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
  void up_at(size_t off, const std::vector<T>& v) const {  // the same, `off` bytes into the buffer
    HIP(hipMemcpy(static_cast<char*>(p) + off, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  }
  // every byte of the buffer = `byte`, in stream order (0x55: a dirty pool buffer; 0xff: NaN)
  void fill(int byte) const { HIP(hipMemsetAsync(p, byte, bytes, g_stream)); }
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

// f(i) for every i in [0, n), handed out in blocks of `grain` to at most 16 threads
static size_t pool_threads(size_t jobs) {
  const unsigned hw = std::thread::hardware_concurrency();
  return std::max<size_t>(1, std::min<size_t>(std::min<size_t>(16, hw ? hw : 4), jobs));
}
template <class F>
static void parallel_for(size_t n, size_t grain, F f) {
  std::atomic<size_t> next{0};
  auto work = [&] {
    for (size_t b; (b = next.fetch_add(grain)) < n;)
      for (size_t i = b; i < std::min(n, b + grain); ++i) f(i);
  };
  const size_t nt = pool_threads((n + grain - 1) / grain);
  std::vector<std::thread> th;
  for (size_t t = 1; t < nt; ++t) th.emplace_back(work);
  work();
  for (auto& t : th) t.join();
}
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

// ------------------------------------------------------------------ cov
// The exact integer covariance / Gram (ef_cov_i8.hip), driven as ef_fit.hip drives it, with
// the product's allocation sizes (At: dim * kpad + kSyrkPadBytes, order, slabs: no slack of
// the test's own) and every work buffer dirty before each launch: At, slabs, S64, cvec, R
// and Q2 hold 0x55 bytes, C holds NaN, so an entry read before it is written, or never
// written, shows.
//
// Host reference: X' = X - 128 as int8 rows of the operand (dim x K), S' = X'^T X' (or
// X' X'^T) in int64, the column sums c, R_i = X'_i . c in int64, Q = c . c in __int128, the
// numerator  n S'_ij - c_i c_j  (Gram: n^2 S'_ij - n (R_i + R_j) + Q) in __int128 and the
// quotient by n (n - 1) (Gram: n^2 (n - 1)) in long double.
//
// Per case:
//   /pieces  bit-equal: At's bytes against [kb][row][kk] = x ^ 0x80 (zero past K) and the
//            0x55 of the pad behind it; S1 = sum x, S2 = sum x^2 from the fused transpose
//            (where it runs) and from launch_colstats; S64 of launch_cov_i8_cross on the
//            upper 64-blocks (i / 64 <= j / 64; the rest is not part of the contract); the
//            plan's expectations.
//   /C       |C - ref| <= 2 u 1.01 |ref| (the conversion of the numerator and the division;
//            den < 2^53 is exact, asserted), 4 u 1.01 |ref| with w (w_i w_j, and the
//            product with it); ref = 0 gives exactly 0.  AND bit-equal to the host's
//            (double)num / den [* (w_i * w_j)]: int128 -> fp64 and the division are both
//            correctly rounded on either side.
//   /whole   C[j][i] bit-equal to C[i][j] everywhere and no NaN left (the mirror write
//            through LDS on ragged last blocks); launch_cov_from_cross fed the S64 and S1 of
//            the same rows gives a C bit-equal to launch_cov_i8's.
enum CovKind { CK_UNI, CK_EXT, CK_255 };  // uniform 0..255; only {0, 255} (x' = -128 / 127); all 255
static const int64_t kDefaultSlabBytes = (int64_t)8 << 30;  // ef_internal.hpp opt_cov_slab_bytes

struct CovCase {
  const char* tag;
  int64_t n, d;
  bool gram;
  CovKind kind;
  bool stdz;
  int slabs;  // slab budget in slabs of dim x dim int32; 0: the product's default (8 GiB)
  int xoff;   // X starts this many bytes into its allocation
  // what the plan must look like (-1 / false: anything)
  int want_passes = -1, want_splits = -1;
  int64_t want_kps = -1;
  bool must_split = false, short_split = false, short_pass = false;
  std::string id() const {
    char b[160];
    std::snprintf(b, sizeof b, "cov/%s/%s_n%lld_d%lld_%s%s", tag, gram ? "gram" : "cov", (long long)n, (long long)d,
                  kind == CK_UNI ? "uni" : kind == CK_EXT ? "ext" : "255", stdz ? "_std" : "");
    std::string s = b;
    if (slabs) s += "_b" + std::to_string(slabs);
    if (xoff) s += "_off" + std::to_string(xoff);
    return s;
  }
  int64_t dim() const { return gram ? n : d; }
  int64_t K() const { return gram ? d : n; }
  int64_t budget() const { return slabs ? (int64_t)slabs * dim() * dim() * 4 : kDefaultSlabBytes; }
};

static std::vector<CovCase> cov_cases() {
  std::vector<CovCase> v;
  auto add = [&](const char* tag, int64_t n, int64_t d, bool gram, CovKind kind, bool stdz, int slabs,
                 int xoff = 0) -> CovCase& {
    v.push_back(CovCase{tag, n, d, gram, kind, stdz, slabs, xoff});
    return v.back();
  };
  // tile geometry, covariance path: syrk_i8_kernel<256> below order 2048 (one tile, ragged,
  // exact fit, one row / column into the next tile), syrk16_i8_kernel<6> on 256 x 384 tiles
  // from 2048 (exact fit of the rows, two ragged rows, one column into a new 384 tile);
  // d % 4 != 0 ends in cov_finalize_kernel, the others in cov_finalize4_kernel
  for (int64_t d : {1, 3, 63, 64, 65, 255, 256, 257, 513}) {
    add("tile", 100, d, false, CK_UNI, false, 0);
    add("tile", 100, d, false, (d & 1) ? CK_EXT : CK_UNI, true, 1);
  }
  for (int64_t d : {2048, 2050, 2305}) add("tile", 130, d, false, CK_UNI, false, 0);
  add("tile", 130, 2050, false, CK_EXT, true, 1);
  add("tile", 130, 2048, false, CK_EXT, true, 0);
  // K edges: one work item (budget one slab: splits = 1) walks 1..5 stages around the
  // 4-stage LDS ring, zero padding past n inside the last stage; n = 1 has den = 0 on this
  // path and checks the pieces only
  for (int64_t n : {1, 63, 64, 65, 191, 192, 256, 257, 320}) {
    add("kedge", n, 64, false, (n & 1) ? CK_EXT : CK_UNI, false, 1);
    add("kedge", n, 2050, false, CK_UNI, false, 1);
  }
  add("kedge", 320, 64, false, CK_UNI, false, 0);  // the default budget: one stage per split
  // split-K and passes
  add("split", 448, 64, false, CK_UNI, false, 2).short_split = true;  // 7 stages as 4 + 3
  add("split", 448, 64, false, CK_EXT, true, 3).short_split = true;   // 3 + 3 + 1
  {
    CovCase& c = add("split", 131073, 64, false, CK_UNI, false, 1);  // 2049 stages: 1025 + 1024
    c.want_passes = 2, c.short_pass = true;
  }
  {
    CovCase& c = add("split", 262100, 64, false, CK_UNI, false, 1);  // 4096 stages: 1366 + 1366 + 1364
    c.want_passes = 3, c.short_pass = true;
  }
  {
    CovCase& c = add("split", 262200, 8, false, CK_EXT, false, 2);  // 4097 stages: (1025 + 1024) + (1025 + 1023)
    c.want_passes = 2, c.want_splits = 2, c.short_split = true, c.short_pass = true;
  }
  {
    CovCase& c = add("split", 393100, 8, false, CK_UNI, true, 3);  // 6143 stages: 3 x 1024 + (1024 + 1024 + 1023)
    c.want_passes = 2, c.want_splits = 3, c.short_pass = true;
  }
  // the int32 accumulator margin: 131008 samples in one work item, a column of pixels all 0
  // (x' = -128: the diagonal entry is 131008 * 16384 = 2^31 - 1048576); one sample more
  // must split
  {
    CovCase& c = add("margin", 131008, 64, false, CK_EXT, false, 1);
    c.want_passes = 1, c.want_splits = 1, c.want_kps = 2047;
    add("margin", 131009, 64, false, CK_EXT, false, 1).must_split = true;
  }
  // the finalize's int128 branch on the covariance path (n > 2^23) beside the int64 one;
  // d = 6 reaches it in cov_finalize_kernel
  add("wide", (int64_t)1 << 23, 8, false, CK_UNI, false, 0);
  add("wide", ((int64_t)1 << 23) + 1, 8, false, CK_UNI, false, 0);
  add("wide", ((int64_t)1 << 23) + 1, 8, false, CK_EXT, true, 0);
  add("wide", ((int64_t)1 << 23) + 1, 6, false, CK_EXT, false, 0);
  // Gram path (dim = n, K = d): shift_copy_kernel, rowdot_kernel, sumsq128_kernel and the
  // finalize with gram = 1; all-255 pixels: the cancellation n^2 S' - n (R_i + R_j) + Q = 0
  add("gram", 2, 1, true, CK_UNI, false, 0);
  add("gram", 3, 64, true, CK_EXT, false, 0);
  add("gram", 65, 100, true, CK_UNI, false, 0);
  add("gram", 65, 100, true, CK_255, false, 0);
  add("gram", 257, 130, true, CK_EXT, false, 1);
  add("gram", 300, 4097, true, CK_UNI, false, 0);
  add("gram", 300, 4097, true, CK_255, false, 2);
  add("gram", 2050, 70, true, CK_UNI, false, 0);
  // transposes: transpose_stats_lds_kernel (d % 256 == 0), transpose_stats_kernel (d % 4 ==
  // 0), shift_transpose_kernel + launch_colstats (other d, or X not 4-byte aligned: a sliced
  // device tensor); n = 8200 makes workgroups stride over more than one 64-row block
  const int64_t tr[8][4] = {{256, 1, 17, 8200}, {512, 15, 64, 8200}, {4, 1, 17, 8200}, {252, 15, 200, 0},
                            {260, 64, 8200, 0}, {50, 1, 17, 200},    {65, 15, 64, 8200}, {256, 200, 0, 0}};
  for (auto& t : tr)
    for (int a = 1; a < 4; ++a)
      if (t[a]) add("transpose", t[a], t[0], false, (a & 1) ? CK_UNI : CK_EXT, false, 0);
  for (int64_t n : {17, 200, 8200}) add("transpose", n, 256, false, CK_UNI, false, 0, 1);
  return v;
}

struct CovData {
  int64_t n, d, dim, K;
  bool gram;
  std::vector<uint8_t> X;  // n x d pixels
  std::vector<int8_t> Xt;  // dim x K: the operand's rows, x - 128
};

static CovData cov_data(const CovCase& c) {
  CovData D;
  D.n = c.n, D.d = c.d, D.gram = c.gram, D.dim = c.dim(), D.K = c.K();
  const int64_t n = c.n, d = c.d;
  D.X.assign((size_t)n * d, 255);
  if (c.kind != CK_255) {
    Rng rng(77003ull * n + 131ull * d + (int)c.kind);
    for (size_t e = 0; e < D.X.size(); e += 8) {
      const uint64_t r = rng.next();
      for (size_t b = 0; b < 8 && e + b < D.X.size(); ++b) {
        const unsigned v = (unsigned)(r >> (8 * b)) & 255u;
        D.X[e + b] = (uint8_t)(c.kind == CK_UNI ? v : ((v & 1) ? 255 : 0));
      }
    }
    // one all-zero column and one constant column (StandardScaler scale 1, covariance 0)
    for (int64_t i = 0; i < n; ++i) {
      if (d >= 2) D.X[(size_t)i * d + d - 1] = 0;
      if (d >= 3) D.X[(size_t)i * d + 1] = 200;
    }
  }
  D.Xt.resize((size_t)D.dim * D.K);
  if (c.gram) {
    for (size_t e = 0; e < D.X.size(); ++e) D.Xt[e] = (int8_t)(D.X[e] ^ 0x80u);
  } else {
    parallel_for((size_t)d, 1, [&](size_t col) {
      for (int64_t k = 0; k < n; ++k) D.Xt[col * (size_t)n + k] = (int8_t)(D.X[(size_t)k * d + col] ^ 0x80u);
    });
  }
  return D;
}

// sum a_k b_k in int64 (int32 partial sums over 32768 terms: 2^15 2^14 < 2^31); skip: one
// term left out (--host's sensitivity check)
static int64_t dot_i8(const int8_t* a, const int8_t* b, int64_t K, int64_t skip = -1) {
  int64_t s = 0;
  for (int64_t k0 = 0; k0 < K; k0 += 32768) {
    const int64_t k1 = std::min(K, k0 + 32768);
    int32_t t = 0;
    for (int64_t k = k0; k < k1; ++k) t += (int32_t)a[k] * (int32_t)b[k];
    s += t;
  }
  if (skip >= 0 && skip < K) s -= (int64_t)a[skip] * (int64_t)b[skip];
  return s;
}

struct CovRef {
  std::vector<int64_t> rows;     // the rows of the dim x dim result the reference covers
  std::vector<int64_t> S;        // [rows][dim]: S'
  std::vector<uint64_t> s1, s2;  // [d]: sum x, sum x^2
  std::vector<long long> c, R;   // [d]: s1 - 128 n; Gram: [n] X'_i . c
  __int128 Q = 0;                // Gram: c . c
};

static CovRef cov_reference(const CovData& D, int64_t skip = -1) {
  CovRef r;
  r.rows = sample_rows(D.dim);
  r.S.assign(r.rows.size() * (size_t)D.dim, 0);
  parallel_for(r.S.size(), D.K > 4096 ? 1 : 64, [&](size_t e) {
    const int64_t i = r.rows[e / (size_t)D.dim], j = (int64_t)(e % (size_t)D.dim);
    r.S[e] = dot_i8(&D.Xt[(size_t)i * D.K], &D.Xt[(size_t)j * D.K], D.K, skip);
  });
  r.s1.assign((size_t)D.d, 0), r.s2.assign((size_t)D.d, 0), r.c.assign((size_t)D.d, 0);
  for (int64_t i = 0; i < D.n; ++i)
    for (int64_t k = 0; k < D.d; ++k) {
      const uint64_t x = D.X[(size_t)i * D.d + k];
      r.s1[k] += x;
      r.s2[k] += x * x;
    }
  for (int64_t k = 0; k < D.d; ++k) r.c[k] = (long long)r.s1[k] - 128LL * D.n;
  if (D.gram) {
    r.R.assign((size_t)D.n, 0);
    for (int64_t i = 0; i < D.n; ++i) {
      long long s = 0;
      for (int64_t k = 0; k < D.d; ++k) s += (long long)D.Xt[(size_t)i * D.d + k] * r.c[k];
      r.R[i] = s;
    }
    for (int64_t k = 0; k < D.d; ++k) r.Q += (__int128)r.c[k] * r.c[k];
  }
  return r;
}

static __int128 cov_num(const CovData& D, const CovRef& r, size_t ri, int64_t j) {
  const int64_t i = r.rows[ri];
  const __int128 nn = D.n, s = r.S[ri * (size_t)D.dim + j];
  if (D.gram) return nn * nn * s - nn * ((__int128)r.R[i] + r.R[j]) + r.Q;
  return nn * s - (__int128)r.c[i] * r.c[j];
}
// the denominator; exact in fp64 below 2^53 (every case: asserted)
static bool cov_den(const CovData& D, double& den, ld& den_ld) {
  const __int128 nn = D.n, v = D.gram ? nn * nn * (nn - 1) : nn * (nn - 1);
  den = D.gram ? (double)D.n * (double)D.n * (double)(D.n - 1) : (double)D.n * (double)(D.n - 1);
  den_ld = (ld)v;
  return v < ((__int128)1 << 53) && (__int128)den == v;
}

static std::string cov_plan_text(const ef::CovPlan& p) {
  char b[200];
  std::snprintf(b, sizeof b, "tj=%d njb=%d ntiles=%d splits=%d kps=%lld passes=%d nst=%lld spp=%lld", p.tj, p.njb,
                p.ntiles, p.splits, (long long)p.kps, p.passes, (long long)p.nst, (long long)p.stages_per_pass);
  return b;
}
// a split of some pass that has no stages ((splits - 1) kps >= the pass's stages)
static bool cov_plan_has_empty_split(const ef::CovPlan& p) {
  for (int pass = 0; pass < p.passes; ++pass) {
    const int64_t st0 = (int64_t)pass * p.stages_per_pass, st1 = std::min(p.nst, st0 + p.stages_per_pass);
    if ((int64_t)(p.splits - 1) * p.kps >= st1 - st0) return true;
  }
  return false;
}
// the plan against the case's expectations and the planner's own invariants (host only)
static void cov_plan_check(const CovCase& c, const ef::CovPlan& p, Stat& st) {
  st.exact(p.kps >= 1 && p.kps <= 2047);  // int32-exact work items
  st.exact((int64_t)p.splits * p.kps >= p.stages_per_pass && (int64_t)p.passes * p.stages_per_pass >= p.nst);
  st.exact(p.slab_elems == (int64_t)p.splits * c.dim() * c.dim() && p.slab_elems * 4 <= std::max(c.budget(), c.dim() * c.dim() * 4));
  st.exact(p.njb == (c.dim() >= 2048 ? 6 : 0) && p.tj == (c.dim() >= 2048 ? 384 : 256));
  if (c.want_passes >= 0) st.exact(p.passes == c.want_passes);
  if (c.want_splits >= 0) st.exact(p.splits == c.want_splits);
  if (c.want_kps >= 0) st.exact(p.kps == c.want_kps);
  if (c.must_split) st.exact(p.splits * p.passes > 1);
  if (c.short_split) st.exact(p.splits > 1 && p.stages_per_pass - (int64_t)(p.splits - 1) * p.kps < p.kps);
  if (c.short_pass) st.exact(p.passes > 1 && p.nst - (int64_t)(p.passes - 1) * p.stages_per_pass < p.stages_per_pass);
}

static void cov_case(const CovCase& c) {
  const std::string id = c.id();
  if (g_list) { std::printf("%s\n", id.c_str()); return; }
  if (!wanted(id)) return;
  const CovData D = cov_data(c);
  const CovRef r = cov_reference(D);
  const int64_t n = c.n, d = c.d, dim = D.dim, K = D.K, kpad = ef::cov_i8_kpad(K);
  const bool gram = c.gram;
  // the product's allocations, byte for byte (ef_fit.hip)
  Dev dX((size_t)n * d + c.xoff), dAt((size_t)dim * kpad + ef::kSyrkPadBytes, 0), dS1((size_t)d * 8), dS2((size_t)d * 8),
      dS1b((size_t)d * 8), dS2b((size_t)d * 8);
  dX.up_at(c.xoff, D.X);
  const uint8_t* Xd = dX.as<uint8_t>() + c.xoff;
  dAt.fill(0x55);
  const bool fused = !gram && ef::cov_i8_fused_stats(Xd, d);
  HIP(ef::launch_cov_i8_prep(g_stream, Xd, n, d, gram, dAt.as<uint8_t>(), fused ? dS1.as<unsigned long long>() : nullptr,
                             fused ? dS2.as<unsigned long long>() : nullptr));
  HIP(ef::launch_colstats(g_stream, Xd, n, d, dS1b.as<unsigned long long>(), dS2b.as<unsigned long long>()));
  const unsigned long long* S1 = fused ? dS1.as<unsigned long long>() : dS1b.as<unsigned long long>();
  const unsigned long long* S2 = fused ? dS2.as<unsigned long long>() : dS2b.as<unsigned long long>();

  Stat sp;  // the integer pieces
  {
    std::vector<uint8_t> at(dAt.bytes);
    dAt.down(at);
    int64_t bad = 0;
    for (int64_t kb = 0; kb < kpad / 64; ++kb)
      for (int64_t row = 0; row < dim; ++row) {
        const uint8_t* got = &at[((size_t)kb * dim + row) * 64];
        for (int kk = 0; kk < 64; ++kk) {
          const int64_t k = kb * 64 + kk;
          bad += got[kk] != (k < K ? (uint8_t)D.Xt[(size_t)row * K + k] : (uint8_t)0);
        }
      }
    for (size_t e = (size_t)dim * kpad; e < at.size(); ++e) bad += at[e] != 0x55;  // nothing written behind At
    sp.n += (int64_t)at.size(), sp.mism += bad;
    std::vector<uint64_t> a(d), b(d);
    if (fused) {
      dS1.down(a);
      dS2.down(b);
      for (int64_t k = 0; k < d; ++k) sp.exact(a[k] == r.s1[k] && b[k] == r.s2[k]);
    }
    dS1b.down(a);
    dS2b.down(b);
    for (int64_t k = 0; k < d; ++k) sp.exact(a[k] == r.s1[k] && b[k] == r.s2[k]);
  }
  std::vector<double> w;
  Dev dMean((size_t)d * 8), dVar((size_t)d * 8), dScale((size_t)d * 8), dW((size_t)d * 8);
  if (c.stdz) {
    HIP(ef::launch_stats_finalize(g_stream, S1, S2, n, d, 1, dMean.as<double>(), dVar.as<double>(), dScale.as<double>(),
                                  dW.as<double>()));
    w.resize(d);
    dW.down(w);
    // a constant pixel gets scale 1; every other weight is 1 / sqrt(var) to its few roundings
    // (the numerator's conversion, n^2, the division, the root, the reciprocal)
    for (int64_t k = 0; k < d; ++k) {
      const __int128 vn = (__int128)n * r.s2[k] - (__int128)r.s1[k] * r.s1[k];
      if (vn == 0) sp.exact(w[k] == 1.0);
      else sp.exact(fabsl((ld)w[k] - 1 / sqrtl((ld)vn / ((ld)n * n))) <= 5 * (ld)kU64 * w[k]);
    }
  }
  const double* wd = c.stdz ? dW.as<double>() : nullptr;
  const ef::CovPlan plan = ef::cov_i8_plan(dim, K, c.budget());
  cov_plan_check(c, plan, sp);
  sp.exact(!cov_plan_has_empty_split(plan));  // (none is reachable: --host enumerates the planner)
  Dev dSl((size_t)plan.slab_elems * 4, 0), dS64x((size_t)dim * dim * 8), dS64((size_t)dim * dim * 8), dCv((size_t)d * 8),
      dCv2((size_t)d * 8), dR((size_t)(gram ? n : 1) * 8), dQ2(16), dOrd((size_t)ef::cov_i8_order_bytes(dim), 0),
      dC((size_t)dim * dim * 8), dC2((size_t)dim * dim * 8);
  if (!gram) {
    dSl.fill(0x55);
    dS64x.fill(0x55);
    HIP(ef::launch_cov_i8_cross(g_stream, plan, d, dAt.as<uint8_t>(), dSl.as<int>(), dS64x.as<long long>(), dOrd.p));
    std::vector<long long> s64((size_t)dim * dim);
    dS64x.down(s64);
    for (size_t ri = 0; ri < r.rows.size(); ++ri)
      for (int64_t j = 0; j < dim; ++j) {
        const int64_t i = r.rows[ri];
        if (i / 64 <= j / 64) sp.exact(s64[(size_t)i * dim + j] == r.S[ri * (size_t)dim + j]);
      }
  }
  const char* prep = gram ? "shift_copy" : !fused ? "shift_transpose+colstats" : d % 256 == 0 ? "transpose_stats_lds"
                                                                                               : "transpose_stats";
  char path[160];
  std::snprintf(path, sizeof path, " prep=%s finalize=%s/%s rows=%zu", prep, dim % 4 == 0 ? "finalize4" : "finalize",
                gram ? "gram" : n > ((int64_t)1 << 23) ? "int128" : "narrow", r.rows.size());
  report_exact(id + "/pieces", sp, cov_plan_text(plan) + path);
  double den;
  ld den_ld;
  const bool den_exact = cov_den(D, den, den_ld);
  if (n < 2) return;  // den = 0: the pieces only

  dSl.fill(0x55);
  dS64.fill(0x55);
  dCv.fill(0x55);
  dR.fill(0x55);
  dQ2.fill(0x55);
  dC.fill(0xff);
  HIP(ef::launch_cov_i8(g_stream, plan, n, d, gram, S1, wd, dAt.as<uint8_t>(), dSl.as<int>(),
                        plan.passes > 1 ? dS64.as<long long>() : nullptr, dCv.as<long long>(), dR.as<long long>(),
                        dQ2.as<unsigned long long>(), dOrd.p, dC.as<double>()));
  std::vector<double> C((size_t)dim * dim);
  dC.down(C);
  Stat sc;
  sc.exact(den_exact);
  int64_t biteq = 0, total = 0;
  for (size_t ri = 0; ri < r.rows.size(); ++ri)
    for (int64_t j = 0; j < dim; ++j) {
      const int64_t i = r.rows[ri];
      const __int128 num = cov_num(D, r, ri, j);
      ld ref = (ld)num / den_ld;  // (|num| < 2^64: exact in long double)
      double hv = (double)num / den;
      if (c.stdz) ref = ref * (ld)w[i] * (ld)w[j], hv *= w[i] * w[j];
      const double got = C[(size_t)i * dim + j];
      sc.add(fabsl((ld)got - ref), (c.stdz ? 4 : 2) * (ld)kU64 * 1.01L * fabsl(ref));
      const bool same = same_bits(got, hv) || (got == 0.0 && hv == 0.0);
      sc.exact(same);
      biteq += same, ++total;
    }
  report(id + "/C", sc, "biteq=" + std::to_string(biteq) + "/" + std::to_string(total));

  Stat sw;
  for (int64_t i = 0; i < dim; ++i)
    for (int64_t j = i; j < dim; ++j) {
      const double a = C[(size_t)i * dim + j], b = C[(size_t)j * dim + i];
      sw.exact(a == a && same_bits(a, b));
    }
  if (!gram) {
    dCv2.fill(0x55);
    dC2.fill(0xff);
    HIP(ef::launch_cov_from_cross(g_stream, dS64x.as<long long>(), S1, n, d, wd, dCv2.as<long long>(), dC2.as<double>()));
    std::vector<double> C2((size_t)dim * dim);
    dC2.down(C2);
    sw.n += (int64_t)C.size();
    sw.mism += std::memcmp(C.data(), C2.data(), C.size() * 8) ? 1 : 0;
    if (sw.mism) {
      int64_t m = 0;
      for (size_t e = 0; e < C.size(); ++e) m += !same_bits(C[e], C2[e]);
      std::printf("  from_cross: %lld entries differ\n", (long long)m);
    }
  }
  report_exact(id + "/whole", sw);
}

static void group_cov() {
  for (const CovCase& c : cov_cases()) cov_case(c);
}

// ------------------------------------------------------------------ proj
// The training projection F = ((X - mu) w) . E on int8 digits (ef_proj_i8.hip), through
// launch_proj_i8 with a dirty work buffer (0x55) and F pre-filled with NaN.
//   E1  w = null, mu integer-valued (not all 128: cc_kernel counts), E column c = (integers
//       -3..3) 2^e_c with e_c spread over -30..30 and one all-zero column (t_c = 0); pixels
//       uniform with 0 and 255 present.  Every value, each Horner partial included, is an
//       integer below 2^53 times a power of two: bit-equal to 2^e_c sum_k (x - mu) m.
//   E2  all six digits: mu = 128 (cc = 0), at most 64 pixels per row differ from 128, all
//       in {127, 129} and spread over every K stage, E = (random 46-bit integers) 2^e_c with
//       the column's largest in [2^45, 2^46): V is that integer, |sum x' V| < 2^52, every
//       Horner step is exact.  Bit-equal to 2^e_c sum_k x' V.
//   R   real E (column maxima 2^-20..2^20), mu, and w with one entry 1.0; the componentwise
//       bound of proj_bound below against the long-double product with E'' = fl(w E).
enum ProjKind { PJ_E1, PJ_E2, PJ_R };
static const char* kProjNames[3] = {"E1", "E2", "R"};

struct ProjData {
  int64_t n = 0, d = 0;
  int kk = 0;
  ProjKind kind = PJ_R;
  std::vector<uint8_t> X;
  std::vector<double> mu, w, E;  // w empty: null
  std::vector<int64_t> M;        // E kinds: E[k][c] = M[k][c] 2^ec[c]
  std::vector<int> ec;
};

static ProjData proj_data(int64_t n, int64_t d, int kk, ProjKind kind) {
  ProjData p;
  p.n = n, p.d = d, p.kk = kk, p.kind = kind;
  Rng rng(900001ull * n + 7919ull * d + 31ull * kk + (int)kind);
  p.X.resize((size_t)n * d);
  p.mu.resize(d);
  p.E.resize((size_t)d * kk);
  p.ec.resize(kk);
  for (int c = 0; c < kk; ++c) p.ec[c] = kk == 1 ? 7 : -30 + (60 * c) / (kk - 1);
  if (kind == PJ_E2) {
    for (auto& m : p.mu) m = 128.0;
    std::fill(p.X.begin(), p.X.end(), (uint8_t)128);
    const int64_t nstg = d / 64, cnt = d == 64 ? 40 : 64;
    for (int64_t i = 0; i < n; ++i)
      for (int64_t t = 0; t < cnt; ++t) {  // stage t % nstg (first and last included), a distinct offset in it
        const int64_t stage = t % nstg, q = t / nstg;
        const int64_t k = stage * 64 + (q * 7 + i * 13 + stage * 5) % 64;
        p.X[(size_t)i * d + k] = (rng.next() & 1) ? 127 : 129;
      }
  } else {
    for (auto& x : p.X) x = (uint8_t)(rng.next() & 255);
    p.X[0] = 0;
    p.X[p.X.size() - 1] = 255;
    if (p.X.size() == 1) p.X[0] = 255;
  }
  if (kind == PJ_R) {
    p.w.resize(d);
    for (int64_t k = 0; k < d; ++k) {
      p.mu[k] = 255.0 * rng.uni();
      p.w[k] = 1.0 / (2.0 + 62.0 * rng.uni());
    }
    p.mu[d > 3 ? 3 : 0] = 200.0;  // a constant pixel: scale 1
    p.w[d > 3 ? 3 : 0] = 1.0;
    for (int c = 0; c < kk; ++c) p.ec[c] = kk == 1 ? -3 : -20 + (40 * c) / (kk - 1);
    for (int64_t k = 0; k < d; ++k)
      for (int c = 0; c < kk; ++c)  // magnitudes spread over 2^-12..1 of the column's scale
        p.E[(size_t)k * kk + c] = std::ldexp(rng.real64(), p.ec[c] - rng.range(0, 12));
    for (int c = 0; c < kk; ++c) p.E[(size_t)(c % d) * kk + c] = std::ldexp(rng.real64(), p.ec[c] + 6);
    return p;
  }
  p.M.resize((size_t)d * kk);
  if (kind == PJ_E1)
    for (auto& m : p.mu) m = (double)rng.range(0, 255);
  for (int64_t k = 0; k < d; ++k)
    for (int c = 0; c < kk; ++c) {
      int64_t m;
      if (kind == PJ_E1) m = (kk >= 2 && c == 1) ? 0 : rng.range(-3, 3);
      else {
        m = (int64_t)(rng.next() >> 18);  // < 2^46
        if (k == c % d) m |= (int64_t)1 << 45;
        if (rng.next() & 1) m = -m;
      }
      p.M[(size_t)k * kk + c] = m;
      p.E[(size_t)k * kk + c] = std::ldexp((double)m, p.ec[c]);
    }
  return p;
}

// The scheme's per-column state as ef_proj_i8.hip's header states it: E'' = fl(w E), t_c
// with 2^t_c max|E''| in [2^45, 2^46) (0 for a zero column), V = rint(2^t_c E'') in six
// signed base-256 digits, c = sum (128 - mu) w E in a plain fp64 loop.
struct ProjCols {
  std::vector<double> Epp, cc;
  std::vector<int> t;
  std::vector<int8_t> D;    // [6][kk][d]
  std::vector<ld> ccabs;    // sum |128 - mu||E''|
};
static ProjCols proj_cols(const ProjData& p) {
  ProjCols q;
  const int64_t d = p.d;
  const int kk = p.kk;
  q.Epp.resize((size_t)d * kk);
  q.cc.assign(kk, 0.0);
  q.ccabs.assign(kk, 0);
  q.t.resize(kk);
  q.D.assign((size_t)6 * kk * d, 0);
  for (int c = 0; c < kk; ++c) {
    double mx = 0, s = 0;
    for (int64_t k = 0; k < d; ++k) {
      const double wv = p.w.empty() ? 1.0 : p.w[k], e = wv * p.E[(size_t)k * kk + c];
      q.Epp[(size_t)k * kk + c] = e;
      mx = std::fmax(mx, std::fabs(e));
      s += (128.0 - p.mu[k]) * wv * p.E[(size_t)k * kk + c];
      q.ccabs[c] += fabsl((ld)128 - p.mu[k]) * fabsl((ld)e);
    }
    q.cc[c] = s;
    q.t[c] = oz_shift(mx);
    for (int64_t k = 0; k < d; ++k) {
      int32_t dg[6];
      oz_digits_host(q.Epp[(size_t)k * kk + c], q.t[c], dg, 1);
      for (int j = 0; j < 6; ++j) q.D[((size_t)j * kk + c) * d + k] = (int8_t)dg[j];
    }
  }
  return q;
}

// One row of the emulated product: I_j = X' . D_j (exact), the fp64 Horner, ldexp, + c.
// drop_digit / drop_stage leave one digit's product or one 64-pixel K stage out (--host's
// sensitivity check).  T[c] = sum_j 256^j |I_j|, xabs = sum_k |x'|; *partials_exact: every
// Horner partial equalled its exact integer value.
static void proj_emulate_row(const ProjData& p, const ProjCols& q, int64_t i, int drop_digit, int drop_stage, double* F,
                             ld* T, ld* xabs, bool* partials_exact) {
  const int64_t d = p.d;
  std::vector<int8_t> xs(d);
  ld xa = 0;
  for (int64_t k = 0; k < d; ++k) {
    xs[k] = (int8_t)(p.X[(size_t)i * d + k] ^ 0x80u);
    xa += std::abs((int)xs[k]);
  }
  if (xabs) *xabs = xa;
  for (int c = 0; c < p.kk; ++c) {
    int64_t I[6];
    for (int j = 0; j < 6; ++j) {
      const int8_t* dj = &q.D[((size_t)j * p.kk + c) * d];
      I[j] = dot_i8(xs.data(), dj, d);
      if (drop_stage >= 0) I[j] -= dot_i8(xs.data() + 64 * drop_stage, dj + 64 * drop_stage, 64);
      if (j == drop_digit) I[j] = 0;
    }
    double v = (double)I[5];
    __int128 ex = I[5];
    ld t = ldexpl(fabsl((ld)I[5]), 40);
    bool ok = true;
    for (int j = 4; j >= 0; --j) {
      v = std::fma(v, 256.0, (double)I[j]);
      ex = ex * 256 + I[j];
      ok = ok && (__int128)v == ex;
      t += ldexpl(fabsl((ld)I[j]), 8 * j);
    }
    if (partials_exact) *partials_exact = *partials_exact && ok;
    if (T) T[c] = t;
    F[c] = std::ldexp(v, -q.t[c]) + q.cc[c];
  }
}

// E kinds: 2^ec sum_k (x - mu) M in __int128, independent of the digit scheme; *fits: the
// sum is below 2^53 (so the double holds it)
static double proj_int_ref(const ProjData& p, int64_t i, int c, bool* fits) {
  __int128 s = 0;
  for (int64_t k = 0; k < p.d; ++k)
    s += (__int128)((int64_t)p.X[(size_t)i * p.d + k] - (int64_t)p.mu[k]) * p.M[(size_t)k * p.kk + c];
  const __int128 a = s < 0 ? -s : s;
  if (fits) *fits = *fits && a < ((__int128)1 << 53);
  return std::ldexp((double)(int64_t)s, p.ec[c]);
}

// R: long-double reference sum_k (x - mu) E'' and the bound, per entry:
//   quantisation  |V - 2^t E''| <= 1/2 per entry:            2^-t sum_k |x'_k| / 2
//   Horner        five fma, each rounding a partial no larger than T = sum_j 256^j |I_j|:
//                                                             5 1.01 u 2^-t T
//   cc            a length-d fp64 dot of (128 - mu) w E in some order (the products' own
//                 roundings, fl(w E) against fl((128 - mu) w), inside the two extra units):
//                                                             gamma_(d+2) sum |128 - mu||E''|
//   final add                                                 u |F|
// (ldexp is exact; the I_j are exact int32.)
static ld proj_bound(const ProjData& p, const ProjCols& q, int c, ld T, ld xabs, double F) {
  const ld s = ldexpl(1, -q.t[c]);
  return 0.5L * s * xabs + 5 * 1.01L * (ld)kU64 * s * T + gamma_n((int)p.d + 2) * q.ccabs[c] + (ld)kU64 * fabsl((ld)F);
}
static ld proj_real_ref(const ProjData& p, const ProjCols& q, int64_t i, int c) {
  ld s = 0;
  for (int64_t k = 0; k < p.d; ++k) s += ((ld)p.X[(size_t)i * p.d + k] - (ld)p.mu[k]) * (ld)q.Epp[(size_t)k * p.kk + c];
  return s;
}

// digit columns per tile, restating proj_layout's rule (ef_proj_i8.hip): 384 where it pads no
// more than 256, 256 unless it pads > 15 % more than 128
static int proj_tn(int kk) {
  const int64_t p = 6 * (int64_t)kk, n128 = (p + 127) / 128 * 128, n256 = (p + 255) / 256 * 256,
                n384 = (p + 383) / 384 * 384;
  return n384 <= n256 ? 384 : n256 * 100 <= n128 * 115 ? 256 : 128;
}

struct ProjShape {
  int64_t n, d;
  int kk;
};
static std::vector<ProjShape> proj_shapes() {
  // every (d, kk) pair of the lists once, n walking its list beside them (30 of the 150
  // combinations), and the largest of everything
  const int KK[6] = {1, 12, 40, 64, 65, 128}, DD[5] = {64, 128, 256, 320, 1024};
  const int64_t NN[5] = {1, 255, 256, 257, 700};
  std::vector<ProjShape> v;
  for (int i = 0; i < 30; ++i) v.push_back({NN[(i + i / 5) % 5], DD[i % 5], KK[i % 6]});
  v.push_back({700, 1024, 128});
  v.push_back({257, 1024, 65});
  v.push_back({1, 64, 1});
  return v;
}

static void proj_case(const ProjShape& sh, ProjKind kind) {
  char idb[96];
  std::snprintf(idb, sizeof idb, "proj/%s/n%lld_d%lld_kk%d", kProjNames[kind], (long long)sh.n, (long long)sh.d, sh.kk);
  if (g_list) { std::printf("%s\n", idb); return; }
  if (!wanted(idb)) return;
  const ProjData p = proj_data(sh.n, sh.d, sh.kk, kind);
  const int64_t n = p.n, d = p.d;
  const int kk = p.kk;
  Dev dX((size_t)n * d), dMu((size_t)d * 8), dW((size_t)d * 8), dE((size_t)d * kk * 8), dF((size_t)n * kk * 8);
  if (!ef::proj_i8_supported(dX.as<uint8_t>(), n, d, kk)) {
    std::printf("case=%s worst=inf rms=0 FAIL (shape not supported)\n", idb);
    ++g_fail;
    return;
  }
  Dev dWork(ef::proj_i8_work_bytes(n, d, kk), 0);
  dX.up(p.X);
  dMu.up(p.mu);
  if (!p.w.empty()) dW.up(p.w);
  dE.up(p.E);
  dWork.fill(0x55);
  dF.fill(0xff);
  HIP(ef::launch_proj_i8(g_stream, dX.as<uint8_t>(), n, d, dMu.as<double>(), p.w.empty() ? nullptr : dW.as<double>(),
                         dE.as<double>(), kk, dWork.p, dF.as<double>()));
  std::vector<double> F((size_t)n * kk);
  dF.down(F);
  char extra[64];
  std::snprintf(extra, sizeof extra, "tn=%d tiles=%d stages=%lld", proj_tn(kk), (6 * kk + proj_tn(kk) - 1) / proj_tn(kk),
                (long long)(d / 64));
  if (kind != PJ_R) {
    std::vector<char> same((size_t)n * kk);
    std::atomic<bool> fits{true};
    parallel_for((size_t)n, 1, [&](size_t i) {
      bool f = true;
      for (int c = 0; c < kk; ++c) {
        const double want = proj_int_ref(p, (int64_t)i, c, &f), got = F[i * kk + c];
        same[i * kk + c] = same_bits(got, want) || (got == 0.0 && want == 0.0);
      }
      if (!f) fits = false;
    });
    Stat st;
    st.exact(fits);
    for (char s : same) st.exact(s != 0);
    report_exact(idb, st, extra);
    return;
  }
  const ProjCols q = proj_cols(p);
  std::vector<double> ratio((size_t)n * kk);
  parallel_for((size_t)n, 1, [&](size_t i) {
    std::vector<double> emu(kk);
    std::vector<ld> T(kk);
    ld xabs = 0;
    proj_emulate_row(p, q, (int64_t)i, -1, -1, emu.data(), T.data(), &xabs, nullptr);
    for (int c = 0; c < kk; ++c) {
      const double got = F[i * kk + c];
      const ld err = fabsl((ld)got - proj_real_ref(p, q, (int64_t)i, c)), b = proj_bound(p, q, c, T[c], xabs, got);
      ratio[i * kk + c] = !(err == err) ? std::numeric_limits<double>::infinity()
                          : b > 0       ? (double)(err / b)
                                        : (err == 0 ? 0.0 : std::numeric_limits<double>::infinity());
    }
  });
  Stat st;
  for (double rt : ratio) st.add(rt, 1);
  report(idb, st, extra);
}

// shapes launch_proj_i8 must not be given: the caller keeps the fp64 GEMM
static Stat proj_refusals() {
  Stat st;
  const uint8_t* aligned = reinterpret_cast<const uint8_t*>((uintptr_t)1 << 20);
  st.exact(ef::proj_i8_supported(aligned, 10, 128, 4));
  st.exact(!ef::proj_i8_supported(aligned, 10, 100, 4));      // d % 64 != 0
  st.exact(!ef::proj_i8_supported(aligned + 8, 10, 128, 4));  // X not 16-byte aligned
  st.exact(!ef::proj_i8_supported(aligned, 10, 65600, 4));    // d > 65536
  return st;
}

static void group_proj() {
  for (const ProjShape& sh : proj_shapes())
    for (ProjKind kind : {PJ_E1, PJ_E2, PJ_R}) proj_case(sh, kind);
  if (g_list) { std::printf("proj/refusals\n"); return; }
  if (wanted("proj/refusals")) report_exact("proj/refusals", proj_refusals());
}

// ------------------------------------------------------------------ host self-checks
// The references against their own thresholds, before any kernel is involved.
// cov and proj: the planner enumerated, the cases' plans, the integer references against
// their representability conditions, the R bound on the host emulation of the scheme, and
// the sensitivity of the E cases (one sample, one digit, one K stage dropped from the
// emulated product must fail them).
static void host_cov_proj() {
  {  // every plan the planner can return for up to 300 stages and 1..64 slabs of budget
    int64_t plans = 0, empty = 0, broken = 0;
    std::string first;
    for (int64_t dim : {8, 64, 513, 2050, 2305})
      for (int64_t smax = 1; smax <= 64; ++smax)
        for (int64_t nst = 1; nst <= 300; ++nst) {
          const ef::CovPlan p = ef::cov_i8_plan(dim, nst * 64, smax * dim * dim * 4);
          ++plans;
          broken += !(p.nst == nst && p.kps >= 1 && p.kps <= 2047 && p.splits >= 1 && p.splits <= smax &&
                      (int64_t)p.splits * p.kps >= p.stages_per_pass && (int64_t)p.passes * p.stages_per_pass >= nst);
          if (cov_plan_has_empty_split(p)) {
            if (!empty) first = "dim=" + std::to_string(dim) + " smax=" + std::to_string(smax) + " " + cov_plan_text(p);
            ++empty;
          }
        }
    Stat st;
    st.n = plans, st.mism = broken;
    report_exact("host/cov/plan_enumeration", st,
                 empty ? "splits without stages: " + std::to_string(empty) + " plans, first " + first
                       : "no reachable plan has a split without stages");
    // (a plan with an empty split would need a case of its own in cov_cases(): the kernel
    // must then store zeros to that slab)
    Stat se;
    se.exact(empty == 0);
    report_exact("host/cov/no_empty_split_case_needed", se);
  }
  {  // the cases' plans (256 CUs assumed where no device answers)
    Stat st;
    for (const CovCase& c : cov_cases()) {
      const ef::CovPlan p = ef::cov_i8_plan(c.dim(), c.K(), c.budget());
      const int64_t before = st.mism;
      cov_plan_check(c, p, st);
      st.exact(!cov_plan_has_empty_split(p));
      if (st.mism != before) std::printf("  plan of %s: %s\n", c.id().c_str(), cov_plan_text(p).c_str());
    }
    report_exact("host/cov/case_plans", st);
  }
  {  // the reference's pieces against a second, plain evaluation; one sample dropped shows
    CovCase cc{"host", 100, 5, false, CK_UNI, false, 0, 0}, cg{"host", 7, 130, true, CK_EXT, false, 0, 0};
    for (const CovCase& c : {cc, cg}) {
      const CovData D = cov_data(c);
      const CovRef r = cov_reference(D), rd = cov_reference(D, 37);
      double den;
      ld den_ld;
      Stat st, sd;
      st.exact(cov_den(D, den, den_ld));
      int64_t differ = 0;
      for (size_t ri = 0; ri < r.rows.size(); ++ri)
        for (int64_t j = 0; j < D.dim; ++j) {
          // C_ij from centred long-double data: (1 / (n - 1)) sum (x_i - mean_i)(x_j - mean_j)
          const int64_t i = r.rows[ri];
          ld s = 0;
          if (c.gram) {
            for (int64_t k = 0; k < D.d; ++k) {
              const ld mk = (ld)r.s1[k] / D.n;
              s += ((ld)D.X[(size_t)i * D.d + k] - mk) * ((ld)D.X[(size_t)j * D.d + k] - mk);
            }
          } else {
            const ld mi = (ld)r.s1[i] / D.n, mj = (ld)r.s1[j] / D.n;
            for (int64_t k = 0; k < D.n; ++k) s += ((ld)D.X[(size_t)k * D.d + i] - mi) * ((ld)D.X[(size_t)k * D.d + j] - mj);
          }
          s /= (D.n - 1);
          const ld ref = (ld)cov_num(D, r, ri, j) / den_ld;
          st.add(fabsl(ref - s), 1e-15L * (fabsl(s) + 1));
          const double a = (double)cov_num(D, r, ri, j) / den, b = (double)cov_num(D, rd, ri, j) / den;
          differ += !same_bits(a, b);
        }
      report(std::string("host/cov/reference_") + (c.gram ? "gram" : "cov"), st);
      sd.exact(differ > 0);  // the E check (bit-equal C) sees one dropped sample
      report_exact(std::string("host/cov/sensitivity_sample_") + (c.gram ? "gram" : "cov"), sd,
                   std::to_string(differ) + " entries move");
    }
  }
  for (const ProjShape& sh : {ProjShape{3, 320, 12}, ProjShape{2, 64, 65}, ProjShape{2, 1024, 5}}) {
    char tail[64];
    std::snprintf(tail, sizeof tail, "n%lld_d%lld_kk%d", (long long)sh.n, (long long)sh.d, sh.kk);
    for (ProjKind kind : {PJ_E1, PJ_E2}) {
      const ProjData p = proj_data(sh.n, sh.d, sh.kk, kind);
      const ProjCols q = proj_cols(p);
      const int nstg = (int)(sh.d / 64);
      Stat st, sd;
      std::vector<double> F(sh.kk), G(sh.kk);
      bool fits = true, partials = true, digits_used = true;
      int64_t stage_seen = 0, digit_seen[6] = {};
      for (int64_t i = 0; i < sh.n; ++i) {
        proj_emulate_row(p, q, i, -1, -1, F.data(), nullptr, nullptr, &partials);
        for (int c = 0; c < sh.kk; ++c) st.exact(same_bits(F[c], proj_int_ref(p, i, c, &fits)) || (F[c] == 0 && proj_int_ref(p, i, c, nullptr) == 0));
        for (int s : {0, nstg - 1}) {  // one K stage dropped: first and last
          proj_emulate_row(p, q, i, -1, s, G.data(), nullptr, nullptr, nullptr);
          for (int c = 0; c < sh.kk; ++c) stage_seen += !same_bits(F[c], G[c]);
        }
        for (int j = 0; j < 6; ++j) {  // one digit's product dropped
          proj_emulate_row(p, q, i, j, -1, G.data(), nullptr, nullptr, nullptr);
          for (int c = 0; c < sh.kk; ++c) digit_seen[j] += !same_bits(F[c], G[c]);
        }
      }
      for (int j = 0; j < 6; ++j) digits_used = digits_used && digit_seen[j] > 0;
      st.exact(fits);      // |sum (x - mu) M| < 2^53
      st.exact(partials);  // every Horner partial is its exact integer
      report_exact(std::string("host/proj/") + kProjNames[kind] + "_representable_" + tail, st);
      sd.exact(stage_seen > 0);
      if (kind == PJ_E2) sd.exact(digits_used);  // E1 has the top digit only: E2 carries all six
      else sd.exact(digit_seen[5] > 0);
      report_exact(std::string("host/proj/") + kProjNames[kind] + "_sensitivity_" + tail, sd,
                   "entries moved by a dropped stage: " + std::to_string(stage_seen) + ", by digit 0..5: " +
                       std::to_string(digit_seen[0]) + " " + std::to_string(digit_seen[1]) + " " +
                       std::to_string(digit_seen[2]) + " " + std::to_string(digit_seen[3]) + " " +
                       std::to_string(digit_seen[4]) + " " + std::to_string(digit_seen[5]));
    }
    {  // R: the emulation inside the bound
      const ProjData p = proj_data(sh.n, sh.d, sh.kk, PJ_R);
      const ProjCols q = proj_cols(p);
      Stat st;
      std::vector<double> F(sh.kk);
      std::vector<ld> T(sh.kk);
      for (int64_t i = 0; i < sh.n; ++i) {
        ld xabs = 0;
        proj_emulate_row(p, q, i, -1, -1, F.data(), T.data(), &xabs, nullptr);
        for (int c = 0; c < sh.kk; ++c)
          st.add(fabsl((ld)F[c] - proj_real_ref(p, q, i, c)), proj_bound(p, q, c, T[c], xabs, F[c]));
      }
      report(std::string("host/proj/R_emulation_") + tail, st);
    }
  }
  report_exact("host/proj/refusals", proj_refusals());
}

static void group_host() {
  host_cov_proj();
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
    std::printf("groups: tall s3 cq chol jacobi cov proj (and --host)\n");
    group_tall();
    group_s3();
    group_cq();
    group_chol();
    group_jacobi();
    group_cov();
    group_proj();
    return 0;
  }
  if (g == "--host") {
    group_host();
    std::printf("kernel_units --host: %s\n", g_fail ? "FAILED" : "ok");
    return g_fail ? 1 : 0;
  }
  void (*fn)() = g == "tall" ? group_tall : g == "s3" ? group_s3 : g == "cq" ? group_cq : g == "chol" ? group_chol
                 : g == "jacobi" ? group_jacobi : g == "cov" ? group_cov : g == "proj" ? group_proj : nullptr;
  if (!fn) {
    std::printf("usage: kernel_units <tall|s3|cq|chol|jacobi|cov|proj> [case] | --list | --host\n");
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
