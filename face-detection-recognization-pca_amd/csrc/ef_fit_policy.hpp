// The Rayleigh-Ritz policy of the fit's wide-block subspace iteration (ef_fit.hip): when a
// step is due, which Jacobi tolerance it takes, whether it ends the iteration, the next
// shift and where the next step goes.  Pure host arithmetic on at most m Ritz values and kk
// residual norms: no HIP, no context, so tests/native/host_units.cpp drives it directly.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace ef {

// The solver's tuning values.  The product library always runs these defaults; the
// diagnostic build (-DEF_DIAGNOSTICS) fills one from the environment once per eigensolve
// (read_fit_knobs, ef_fit.hip), for the A/B tools under tools/.
struct FitKnobs {
  double rr_loose = 1e-4;     // EF_FIT_RR_LOOSE: the coarse-phase Rayleigh-Ritz tolerance (1e-12 = off)
  double rr_first = 1e-2;     // EF_FIT_RR_FIRST
  double resid_tol = 1e-9;    // EF_FIT_RESID_TOL (0 = off)
  double gap_tol = 1e-5;      // EF_FIT_GAP_TOL (0 = off)
  double coarse_tol = 1e-4;   // EF_FIT_COARSE_TOL
  double coarse_pred = 1e-6;  // EF_FIT_COARSE_PRED
  double gap_margin = 0.0;    // EF_FIT_GAP_MARGIN (> 0: p = log(margin need) / log(rho))
  int early_rule = 0;         // EF_FIT_EARLY (0: steps 1, 2, 4 below order 12288; 1: at any order; n: step n only)
  int m = 0;                  // EF_FIT_M: block width (0 = the solver's own)
  bool tn_tall = true;        // EF_FIT_TN_TALL=0: Y^T.Y and Q^T.Y on gemm64's split-K
  bool shift = true;          // EF_FIT_SHIFT=0: sigma = 0
  bool cq_i8 = true;          // EF_FIT_CQ_I8=0: the fp64 MFMA product
  bool cq_med = true;         // EF_FIT_CQ_MED=0: every fine product in the full form
  bool side = true;           // EF_FIT_SIDE=0: the planes on the main stream at the first fine product
  bool defer = true;          // EF_FIT_DEFER=0: the host check of every CholQR factor
  bool proj_f64 = false;      // EF_FIT_PROJ_F64: the training projection on the fp64 GEMM
  bool debug = false;         // EF_FIT_DEBUG: one line per Rayleigh-Ritz step on stderr
};

// Rayleigh-Ritz period: a grid-Jacobi RR costs ~ a few iterations at dim ~ 16k, ~10 at dim ~ 2k
inline int rr_period(int64_t dim) { return dim >= 12288 ? 8 : 16; }

constexpr double kResidFloor = 1e-12;  // |r_i| / theta_1 always accepted by the gap rule

// What one Rayleigh-Ritz step decided, with the figures the EF_FIT_DEBUG line and the
// non-convergence message print.
struct RitzStep {
  bool diverged = false;  // theta_1 not finite: nothing else is set, no state changed
  bool accepted = false;
  double sigma_next = 0.0;  // the shift of the products from the next iteration on
  double worst = 0.0;       // largest relative change of a kept Ritz value since the previous step
  int worst_i = 0;
  double resid_max = -1.0;  // largest |r_i| / theta_1 (-1: the step had no residuals)
  double gap_worst = 0.0;   // largest |r_i| / gap_i
  int gap_i = -1;
};

// The rules of one wide solve and the state they keep between Rayleigh-Ritz steps.
//
// Spectral shift: the iteration multiplies by C - sigma I.  Convergence of eigenpair i
// goes as max_{j > m} |lambda_j - sigma| / (lambda_i - sigma) per product instead of
// lambda_{m+1} / lambda_i.  sigma = theta_m / 2 (theta_m, the block's smallest Ritz
// value, never exceeds lambda_m) is safe for any PSD C: every unwanted |lambda_j - sigma|
// is at most max(lambda_{m+1} - sigma, sigma) < lambda_k - sigma, so the wanted block
// stays dominant.  Ritz values are reported and tested unshifted.
// Chebyshev acceleration (EF_OPT_FIT_CHEBYSHEV, default on): with [0, theta_m] as the
// interval of the unwanted spectrum (centre = half-width = sigma), the iterates follow
// the three-term recurrence X_{j+1} = 2 A~ X_j - X_{j-1}, A~ = (C - sigma I) / sigma,
// restarted (X_0 = the current block) at every Rayleigh-Ritz step, which refreshes
// sigma.  Eigenpair i then converges per product as 1 / (x + sqrt(x^2 - 1)),
// x = lambda_i / sigma - 1, instead of (lambda_{m+1} - sigma) / (lambda_i - sigma): the
// C3 fit's 40 products drop to ~27 in a model of its spectrum.  Each iterate is
// orthonormalised (Y = Q' L^T); the previous one is carried into the same frame
// (W = Q_old L^-T, one extra tall GEMM), so the recurrence holds exactly for the block's
// span while the columns stay orthonormal (no growth of the dominant components).
struct RitzPolicy {
  int64_t dim;
  int kk, m, max_iters;
  bool cheb_on, shift_on;
  FitKnobs kn;

  // ---- state kept between steps
  bool coarse;                // the products still run in reduced precision
  double sigma = 0.0;         // the shift the products carry
  std::vector<double> prev;   // the previous step's Ritz values of C (unshifted), descending
  bool have_prev = false, prev_fine = false;
  double last_worst = 1.0;
  double prev_resid_max = 0.0;  // largest |r_i| / theta_1 at the previous fp64 step (0: none)
  double rate_prev = 0.0;  // predicted per-product error factor of the products since the last step
  int last_rr_it = 0;
  int next_rr = 8;  // iteration of the next scheduled Rayleigh-Ritz step

  // coarse_phase: the solver has a reduced-precision product for this problem and starts in it
  RitzPolicy(int64_t dim_, int kk_, int m_, int max_iters_, bool cheb_on_, bool shift_on_, bool coarse_phase,
             const FitKnobs& kn_ = FitKnobs())
      : dim(dim_), kk(kk_), m(m_), max_iters(max_iters_), cheb_on(cheb_on_), shift_on(shift_on_),
        kn(kn_), coarse(coarse_phase), prev(m_, 0.0) {}

  // this iteration's product is fp64
  bool fine() const { return !coarse; }

  // Rayleigh-Ritz at iterations 1, 2, 4 (small orders only: there they re-order the block
  // early enough to matter; at order >= 12288 they cost 26 of 62 Jacobi sweeps and change
  // no iteration count), 8, then every rr_period(dim)
  bool rr_due(int it) const {
    const bool early = kn.early_rule == 0   ? dim < 12288 && (it <= 2 || it == 4)
                       : kn.early_rule == 1 ? (it <= 2 || it == 4)
                                            : it == kn.early_rule;
    return early || it == next_rr || it == max_iters;
  }

  // The tolerance this step's Jacobi takes: 1e-12 after an fp64 product, else looser.
  // A Rayleigh-Ritz step after reduced-precision products can never be the converged
  // one (that needs two steps after fp64 products), and its Ritz values only steer the
  // shift, the rate and the switch to fp64 (1e-4 / 1e-6 decisions): its Jacobi stops at
  // off-diagonals of 1e-4 of the diagonal scale (Ritz value error ~1e-8 / relative
  // gap) instead of 1e-12 — the last sweeps of those solves (C3: 1e-4 0.1461 s, 1e-6
  // 0.1467 s, 1e-3 one more iteration; profiles/r04/rr_loose_ab.txt).  The Ritz basis V stays
  // orthogonal to rounding either way (rotations), so the block's span is unchanged.
  // The first Rayleigh-Ritz step's tolerance: its Ritz values only set the first shift and
  // Chebyshev rate (there is no previous step to compare with), and its basis is re-mixed
  // by the products and CholQR factors that follow.  1e-2 takes 2 of the C3 fit's 20 Jacobi
  // sweeps off, ~1.9 ms, same 23 iterations, eigenvalues equal to 3e-15
  // (profiles/r05/rr_first_ab.txt).
  double jacobi_tol() const { return fine() ? 1e-12 : have_prev ? kn.rr_loose : kn.rr_first; }

  // The int8 digit product of iteration `it` takes
  // the medium form (15 digit pairs, ~2^-40) unless a Rayleigh-Ritz step reads this
  // product or the next: the errors of earlier products are damped by the later ones
  // (residual floor 1e-12 theta_1), the accepted step's Ritz pairs come from full ones
  // (iterations <= 4 may hold the small orders' early Rayleigh-Ritz steps)
  bool medium(int it) const { return it >= 5 && it + 1 < next_rr && it + 1 < max_iters && kn.cq_med; }

  // Ritz-residual acceptance: a Rayleigh-Ritz step after an fp64 product also ends the
  // iteration when every kept pair has |C u_i - theta_i u_i| <= 1e-9 theta_1.  Then each
  // theta_i is within |r|^2 / gap of an eigenvalue and u_i within |r| / gap of its vector.
  // The value-change test needs a second fp64 step to compare with.  The residual test
  // decides from one step, so the C3 fit stops after 22 products instead of 23.  Its
  // eigenvalues move by 1.6e-13 and its components by 1.7e-8 against the 23-product fit,
  // 4.7 ms per fit (profiles/r05/resid_ab.txt).  The residuals come from Y.V, the
  // continuation product, and U = Q.V, the result's.
  // wants_resid: this step should come with the kept pairs' residual norms.
  bool wants_resid() const { return fine() && (kn.resid_tol > 0.0 || kn.gap_tol > 0.0 || kn.debug); }

  // The previous step's Ritz values of C (after an accepted step: the result's).
  const std::vector<double>& theta() const { return prev; }

  // One Rayleigh-Ritz step at iteration `it`.  theta: the m Ritz values of H = Q^T (C - sigma I) Q,
  // descending; rnorm: |C u_i - theta_i u_i| of the kk kept pairs, or null (none formed).
  RitzStep step(int it, const double* theta, const double* rnorm) {
    RitzStep r;
    if (!std::isfinite(theta[0])) {
      r.diverged = true;
      return r;
    }
    const bool fine = !coarse;
    const bool resid = rnorm != nullptr;
    const double resid_tol = kn.resid_tol, gap_tol = kn.gap_tol;
    double resid_max = 1.0;
    if (resid) {
      resid_max = 0.0;
      for (int i = 0; i < kk; ++i) resid_max = std::fmax(resid_max, rnorm[i]);
    }
    std::vector<double> th(theta, theta + m);
    for (int i = 0; i < m; ++i) th[i] += sigma;  // Ritz values of C (H = Q^T (C - sigma I) Q)
    // converged when every kept Ritz value moved by <= 1e-13 relative (floor 1e-15 of
    // the largest) since the previous Rayleigh-Ritz step
    bool ok_vals = have_prev && prev_fine && fine;
    for (int i = 0; i < kk && ok_vals; ++i)
      ok_vals = std::fabs(th[i] - prev[i]) <= std::fmax(1e-13 * std::fabs(th[i]), 1e-15 * std::fabs(th[0]));
    const double th1 = std::fabs(th[0]);
    resid_max /= th1;
    bool ok = ok_vals || (resid && resid_tol > 0.0 && resid_max <= resid_tol);
    // Gap-aware acceptance (round 6): the residual bounds the eigenvector error only through
    // |r_i| / gap_i (Davis-Kahan), so EVERY acceptance — residual or value-change — also needs
    // |r_i| <= 1e-5 gap_i for each kept pair, gap_i the distance from theta_i to the nearest
    // other Ritz value of the block (theta_{k+1} included).  On the reference's Dark spectrum
    // (min gap 2.4e-6 lambda_1, models/Joseph_Lai_dark_model_info.json) the absolute test alone
    // guaranteed only 4.2e-4.  Gaps below the fp64 residual floor (1e-12 theta_1 / 1e-5: an
    // exactly or numerically degenerate pair, whose vectors are not unique) are held to that
    // floor instead, and a value-converged step whose residuals stopped shrinking is accepted
    // (the floor of the arithmetic), so a degenerate spectrum still terminates.
    bool ok_gap = true;
    double gap_worst = 0.0;  // max |r_i| / gap_i (diagnostics)
    double gap_need = 0.0;   // max |r_i| / its gap-rule bound (> 1: not yet)
    int gap_wi = -1;
    if (resid && gap_tol > 0.0) {
      for (int i = 0; i < kk; ++i) {
        double g = HUGE_VAL;
        for (int j = 0; j < m; ++j)
          if (j != i) g = std::fmin(g, std::fabs(th[i] - th[j]));
        const double q = rnorm[i] / std::fmax(g, 1e-300);
        if (q > gap_worst) gap_worst = q, gap_wi = i;
        const double need = rnorm[i] / std::fmax(gap_tol * g, kResidFloor * th1);
        gap_need = std::fmax(gap_need, need);
        if (need > 1.0) ok_gap = false;
      }
      // floor of the arithmetic: values converged and the residuals no longer shrinking
      const bool stalled = ok_vals && prev_resid_max > 0.0 && resid_max > 0.5 * prev_resid_max;
      ok = ok && (ok_gap || stalled);
    }
    if (resid) prev_resid_max = resid_max;
    double worst = have_prev ? 0.0 : 1.0;
    int wi = 0;
    for (int i = 0; i < kk && have_prev; ++i) {
      const double d = std::fabs(th[i] - prev[i]) / std::fmax(std::fabs(th[i]), 1e-300);
      if (d > worst) worst = d, wi = i;
    }
    const double coarse_tol = kn.coarse_tol, coarse_pred = kn.coarse_pred;
    // Chebyshev rate: the k-th Ritz value's error shrinks per product by 1 / rho^2,
    // rho = x + sqrt(x^2 - 1), x = theta_k / sigma - 1 on the next interval [0, theta_m]
    const double sig_next = shift_on && th[m - 1] > 0.0 ? 0.5 * th[m - 1] : 0.0;
    double rate_next = 0.0;
    if (cheb_on && sig_next > 0.0) {
      const double x = th[kk - 1] / sig_next - 1.0;
      if (x > 1.0 + 1e-9) {
        const double rho = x + std::sqrt(x * x - 1.0);
        rate_next = 1.0 / (rho * rho);
      }
    }
    // error of this step's Ritz values: the change since the previous step bounds the
    // previous step's error, which the products since then shrank by rate_prev each
    const double e_now = have_prev && rate_prev > 0.0 ? worst * std::pow(rate_prev, it - last_rr_it) : worst;
    // fp64 products from the next iteration on once the fp32 phase has done its part
    if (coarse && (worst < coarse_tol || (rate_prev > 0.0 && e_now < coarse_pred))) coarse = false;
    // Schedule the next Rayleigh-Ritz step.  The test above passes once the PREVIOUS
    // step's Ritz values were already within 1e-13, so with the change per period
    // shrinking geometrically (worst now vs worst at the previous step) the current error
    // is predicted as worst * rate: when that is below the tolerance the next step comes
    // one iteration later (the test then passes instead of waiting out the period); a
    // wrong prediction only costs that one extra Rayleigh-Ritz step.  With the Chebyshev
    // rate known, the next step is placed where the predicted error reaches the
    // tolerance (from the fp32 floor ~3e-7 when the products so far were fp32).
    {
      const int period = rr_period(dim);
      next_rr = (it / period + 1) * period;
      if (it < 8) next_rr = 8;
      if (fine && prev_fine && have_prev && last_worst > 0.0 && worst < last_worst) {
        const double e_pred = worst * (worst / last_worst);
        if (e_pred <= 3e-14) next_rr = it + 1;
      }
      if (rate_next > 0.0 && have_prev && !coarse) {
        const double e_start = fine ? e_now : std::max(e_now, 3e-7);
        // (unchanged values give e_start = 0 and -inf here: the floor of 1 is taken on the
        // double, before the conversion, which is undefined for -inf and NaN)
        const double pd = std::ceil(std::log(e_start / 3e-14) / std::log(1.0 / rate_next));
        const int p = pd >= 1.0 ? (int)pd : 1;
        next_rr = std::min(next_rr, it + p);
      }
      // Gap rule not met yet: no step can accept before it is, so the next one goes where
      // it should be met (an earlier step would also restart the recurrence and lose the
      // acceleration).  p Chebyshev products shrink the slowest kept vector's residual by
      // T_p(x) = cosh(p acosh x), x = theta_k / sigma - 1; a factor 2 of margin.  (C3: the
      // steps at 23 and 24 that the value rule placed are skipped, 22 -> 25.  The
      // asymptotic rate rho^p >= 1.5 need — diagnostic EF_FIT_GAP_MARGIN=1.5 — placed the
      // step at 24, where the residual had shrunk only 5.2x, not rho^2 = 11x, right after
      // the restart: 1.345e-5 of the gap, one more step, 0.1390 vs 0.1378 s;
      // profiles/r06/fit_gap_sched_ab.txt.)
      if (gap_need > 1.0 && rate_next > 0.0 && !coarse) {
        const double x = th[kk - 1] / sig_next - 1.0;
        const double margin = kn.gap_margin;
        int p = margin > 0.0 ? (int)std::ceil(std::log(margin * gap_need) / std::log(x + std::sqrt(x * x - 1.0)))
                             : (int)std::ceil(std::acosh(2.0 * gap_need) / std::acosh(x));
        next_rr = std::max(next_rr, it + std::max(p, 1));
      }
    }
    rate_prev = rate_next;
    last_rr_it = it;
    // the next products use the shift of this step's block (the continuation Y.V
    // still carries the old one: any sequence of shifts is a valid polynomial filter)
    sigma = sig_next;
    prev = th;
    have_prev = true;
    prev_fine = fine;
    last_worst = worst;
    r.accepted = ok;
    r.sigma_next = sig_next;
    r.worst = worst;
    r.worst_i = wi;
    r.resid_max = resid ? resid_max : -1.0;
    r.gap_worst = gap_worst;
    r.gap_i = gap_wi;
    return r;
  }
};

}  // namespace ef
