// abd_survival_terms.hpp -- the closed-form part of the Poisson hazard models: what one unconstrained point gives
// the kernel (lambda_t, a, b), and the combination of the device sums with the priors into logp and gradient.  Plain C++,
// no HIP: one source for the library (abd_survival.hip) and for the native harness (tests/native/survival_harness.cpp).
// Also what creation makes of the caller's arrays: the rule for one cell and the planes the kernels read (survival_pack).
//
//   theta = a[K], b[K], m, s, z[T]            (PyMC's creation order; sd = e^s)
//   r_t = m + sd z_t, lambda_t = invlogit(r_t)
//   sums = S_t[T], L, W_0, W_k[K]             (abd_survival.hpp)
//   logp = sum_t [Y_t log lambda_t - lambda_t S_t] + L + C + priors
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#define ABD_SURV_NW 4  // L, W_0, W_1, W_2 of one wave (a row of w_part; the last is unused for K = 1)

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

// What creation keeps of the data: the [interval][individual] planes, padded to ld columns with cells that have no follow-up,
// Y_t = sum_j y_jt and C = sum_{y > 0} y log e - sum lgamma(y + 1).
struct SurvivalPlanes {
  std::vector<double> y, e, x0, x1;  // [T][ld]; x1 for K = 2 only
  std::vector<double> Y;             // [T]
  double C = 0.0;
};

struct SurvivalRefusal {
  int j, t;         // the individual and the interval of the refused cell
  const char* msg;  // null: every cell was taken
};

// The one transpose of the caller's arrays [N][T] (infected, exposure, K titers) into planes [T][ld]: individual j goes to
// column slot[j], or to column j where slot is null.  The cells are taken with j ascending, then t ascending -- the order of the
// terms of Y_t and C -- each through survival_check_cell; the first refused cell ends it.
inline SurvivalRefusal survival_pack(int N, int T, int K, const double* infected, const double* exposure, const double* const* titer,
                                     const int32_t* slot, size_t ld, SurvivalPlanes* p) {
  const size_t plane = ld * (size_t)T;
  p->y.assign(plane, 0.0);
  p->e.assign(plane, 0.0);
  p->x0.assign(plane, 0.0);
  p->x1.assign(K == 2 ? plane : 0, 0.0);
  std::vector<SurvivalSum> Ysum((size_t)T);
  SurvivalSum Csum;
  for (int j = 0; j < N; ++j)
    for (int t = 0; t < T; ++t) {
      const size_t src = (size_t)j * T + t, dst = (size_t)t * ld + (slot ? slot[j] : j);
      double yy = infected[src], ee = exposure[src], xx[2] = {titer[0][src], K == 2 ? titer[1][src] : 0.0};
      if (const char* msg = survival_check_cell(K, yy, ee, xx)) return SurvivalRefusal{j, t, msg};
      p->y[dst] = yy;
      p->e[dst] = ee;
      p->x0[dst] = xx[0];
      if (K == 2) p->x1[dst] = xx[1];
      Ysum[t].add(yy);
      if (yy > 0.0) Csum.add(yy * std::log(ee));
      Csum.add(-std::lgamma(yy + 1.0));
    }
  p->Y.resize((size_t)T);
  for (int t = 0; t < T; ++t) p->Y[t] = Ysum[t].value();
  p->C = Csum.value();
  return SurvivalRefusal{-1, -1, nullptr};
}

}  // namespace abdi
