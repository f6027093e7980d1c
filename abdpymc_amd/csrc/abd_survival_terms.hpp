// abd_survival_terms.hpp -- the closed-form part of the Poisson hazard models: what one unconstrained point gives
// the kernel (lambda_t, a, b), and the combination of the device sums with the priors into logp and gradient.  Plain C++,
// no HIP: one source for the library (abd_eval.hip) and for the native harness (tests/native/survival_harness.cpp).
//
//   theta = a[K], b[K], m, s, z[T]            (PyMC's creation order; sd = e^s)
//   r_t = m + sd z_t, lambda_t = invlogit(r_t)
//   sums = S_t[T], L, W_0, W_k[K]             (abd_survival.hpp)
//   logp = sum_t [Y_t log lambda_t - lambda_t S_t] + L + C + priors
#pragma once

#include <cmath>

namespace abdi {

struct SurvivalPriors {
  double ab_sd;    // a_k, b_k ~ N(0, ab_sd)
  double mu_mean;  // m ~ N(mu_mean, mu_sd)
  double mu_sd;
  double sd_rate;  // sd ~ Exp(sd_rate), with the log-Jacobian + s
  double z_sd;     // z_t ~ N(0, z_sd)
};

inline int survival_dim(int K, int T) { return 2 * K + 2 + T; }

// A sum whose error does not grow with the number of terms (Neumaier's compensated sum): the host's sums run over up to
// N * T cells (the constant C) or T intervals one after the other, where a plain sum loses about sqrt(n) roundings.
struct SurvivalSum {
  double s = 0.0, c = 0.0;
  void add(double v) {
    const double t = s + v;
    c += std::fabs(s) >= std::fabs(v) ? (s - t) + v : (v - t) + s;
    s = t;
  }
  double value() const { return s + c; }
};

// -softplus(-r) = log invlogit(r): finite for every finite r
inline double survival_log_invlogit(double r) { return std::fmin(r, 0.0) - std::log1p(std::exp(-std::fabs(r))); }
// invlogit(r) without an overflowing exponential
inline double survival_invlogit(double r) {
  const double en = std::exp(-std::fabs(r));
  return (r >= 0.0 ? 1.0 : en) / (1.0 + en);
}

// What the kernel reads of one point, par = lambda[T], a[K], b[K]; and what survival_combine needs again:
// work = log lambda[T], (1 - lambda)[T].
inline void survival_prepare(int K, int T, const double* theta, double* par, double* work) {
  const double m = theta[2 * K], sd = std::exp(theta[2 * K + 1]);
  const double* z = theta + 2 * K + 2;
  for (int t = 0; t < T; ++t) {
    const double r = m + sd * z[t];
    par[t] = survival_invlogit(r);
    work[t] = survival_log_invlogit(r);
    work[T + t] = survival_invlogit(-r);
  }
  for (int k = 0; k < 2 * K; ++k) par[T + k] = theta[k];
}

inline double survival_normal_logp(double v, double mean, double sd, double* g) {
  const double zz = (v - mean) / sd;
  *g = -zz / sd;
  return -0.5 * zz * zz - std::log(sd) - 0.9189385332046727;  // log(2 pi) / 2
}

// logp and grad[D] (may be null) from the device sums.  Y[T] = sum_j y_jt and C are constants of the data.
inline double survival_combine(const SurvivalPriors& p, int K, int T, const double* theta, const double* Y, double C,
                               const double* sums, const double* par, const double* work, double* grad) {
  const double* a = theta;
  const double* b = theta + K;
  const double m = theta[2 * K], s = theta[2 * K + 1], sd = std::exp(s);
  const double* z = theta + 2 * K + 2;
  const double* S = sums;
  const double L = sums[T], W0 = sums[T + 1];
  const double* W = sums + T + 2;
  SurvivalSum lp, sum_dr, sum_zdr;
  double g;
  lp.add(C);
  lp.add(L);
  for (int t = 0; t < T; ++t) {
    const double lam = par[t];
    lp.add(Y[t] * work[t]);
    lp.add(-lam * S[t]);
    const double dr = (Y[t] - lam * S[t]) * work[T + t];
    sum_dr.add(dr);
    sum_zdr.add(z[t] * dr);
    lp.add(survival_normal_logp(z[t], 0.0, p.z_sd, &g));
    if (grad) grad[2 * K + 2 + t] = sd * dr + g;
  }
  for (int k = 0; k < K; ++k) {
    lp.add(survival_normal_logp(a[k], 0.0, p.ab_sd, &g));
    if (grad) grad[k] = -b[k] * W0 + g;
    lp.add(survival_normal_logp(b[k], 0.0, p.ab_sd, &g));
    if (grad) grad[K + k] = (W[k] - a[k] * W0) + g;
  }
  lp.add(survival_normal_logp(m, p.mu_mean, p.mu_sd, &g));
  if (grad) grad[2 * K] = sum_dr.value() + g;
  lp.add(std::log(p.sd_rate));
  lp.add(-p.sd_rate * sd);
  lp.add(s);
  if (grad) grad[2 * K + 1] = (sd * sum_zdr.value() - p.sd_rate * sd) + 1.0;
  return lp.value();
}

// One cell as creation takes it: NaN in y or e makes the cell unfollowed (y = e = 0).  Returns a message for a cell that is
// refused, else null.  A cell without follow-up has its titers set to 0: it adds exact zeros to every sum.
inline const char* survival_check_cell(int K, double& y, double& e, double* x) {
  if (std::isnan(y) || std::isnan(e)) y = e = 0.0;
  if (!std::isfinite(y) || !std::isfinite(e)) return "infected and exposure must be finite or NaN";
  if (y < 0.0) return "infected must not be negative";
  if (e < 0.0) return "exposure must not be negative";
  if (y > 0.0 && e == 0.0) return "infected > 0 with exposure 0 (the likelihood is -inf for every theta)";
  if (y == 0.0 && e == 0.0) {
    for (int k = 0; k < K; ++k) x[k] = 0.0;
    return nullptr;
  }
  for (int k = 0; k < K; ++k)
    if (!std::isfinite(x[k])) return "titer of a followed cell must be finite";
  return nullptr;
}

}  // namespace abdi
