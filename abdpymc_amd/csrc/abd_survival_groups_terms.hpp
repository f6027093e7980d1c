// abd_survival_groups_terms.hpp -- the closed-form part of the Poisson hazard model by group: what one unconstrained
// point gives the kernel (lambda_t, a_g, b), and the combination of the device sums with the priors into logp and gradient.
// Plain C++, no HIP: one source for the library (abd_survival.hip) and for the native harness
// (tests/native/survival_groups_harness.cpp).  At the end, SurvivalForm: which of the three models a handle holds, asked in one place.
//
//   theta = m, s, z[T], a_mu, a_sl, az[Gr], b     (PyMC's creation order for this model; sd = e^s, a_sd = e^a_sl)
//   r_t = m + sd z_t, lambda_t = invlogit(r_t);  a_g = a_mu + a_sd az_g
//   sums = S_t[T], L, W_x, W0_g[Gr]               (abd_survival_groups.hpp)
//   logp = sum_t [Y_t log lambda_t - lambda_t S_t] + L + C + priors
//   d/da_g = -b W0_g;  d/db = W_x - sum_g a_g W0_g;  d/da_mu = sum_g d/da_g;  d/da_sl = a_sd sum_g az_g d/da_g - rate a_sd + 1;
//   d/daz_g = a_sd d/da_g                         (each with its prior's term)
#pragma once

#include <cstdint>
#include <vector>

#include "abd_survival_periods_terms.hpp"  // SurvivalForm, at the end
#include "abd_survival_terms.hpp"

namespace abdi {

struct SurvivalGroupsPriors {
  double mu_mean;    // m ~ N(mu_mean, mu_sd)
  double mu_sd;
  double sd_rate;    // sd ~ Exp(sd_rate), with the log-Jacobian + s
  double z_sd;       // z_t ~ N(0, z_sd)
  double a_mu_sd;    // a_mu ~ N(0, a_mu_sd)
  double a_sd_rate;  // a_sd ~ Exp(a_sd_rate), with the log-Jacobian + a_sl
  double a_z_sd;     // az_g ~ N(0, a_z_sd)
  double b_sd;       // b ~ N(0, b_sd)
};

inline int survival_groups_dim(int T, int Gr) { return T + Gr + 5; }

// What the kernel reads of one point, par = lambda[T], a[Gr], b; and what survival_groups_combine needs again:
// work = log lambda[T], (1 - lambda)[T].
inline void survival_groups_prepare(int T, int Gr, const double* theta, double* par, double* work) {
  const double m = theta[0], sd = std::exp(theta[1]);
  const double* z = theta + 2;
  for (int t = 0; t < T; ++t) {
    const double r = m + sd * z[t];
    par[t] = survival_invlogit(r);
    work[t] = survival_log_invlogit(r);
    work[T + t] = survival_invlogit(-r);
  }
  const double a_mu = theta[T + 2], a_sd = std::exp(theta[T + 3]);
  for (int g = 0; g < Gr; ++g) par[T + g] = a_mu + a_sd * theta[T + 4 + g];
  par[T + Gr] = theta[T + 4 + Gr];
}

// logp and grad[D] (may be null) from the device sums.  Y[T] = sum_j y_jt and C are constants of the data.
inline double survival_groups_combine(const SurvivalGroupsPriors& p, int T, int Gr, const double* theta, const double* Y, double C,
                                      const double* sums, const double* par, const double* work, double* grad) {
  const double m = theta[0], s = theta[1], sd = std::exp(s);
  const double* z = theta + 2;
  const double a_mu = theta[T + 2], a_sl = theta[T + 3], a_sd = std::exp(a_sl);
  const double* az = theta + T + 4;
  const double b = theta[T + 4 + Gr];
  const double* a = par + T;
  const double* S = sums;
  const double L = sums[T], Wx = sums[T + 1];
  const double* W0 = sums + T + 2;
  SurvivalSum lp, sum_dr, sum_zdr, sum_da, sum_zda, sum_aw;
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
    if (grad) grad[2 + t] = sd * dr + g;
  }
  lp.add(survival_normal_logp(m, p.mu_mean, p.mu_sd, &g));
  if (grad) grad[0] = sum_dr.value() + g;
  lp.add(std::log(p.sd_rate));
  lp.add(-p.sd_rate * sd);
  lp.add(s);
  if (grad) grad[1] = (sd * sum_zdr.value() - p.sd_rate * sd) + 1.0;
  for (int k = 0; k < Gr; ++k) {
    const double da = -b * W0[k];
    sum_da.add(da);
    sum_zda.add(az[k] * da);
    sum_aw.add(a[k] * W0[k]);
    lp.add(survival_normal_logp(az[k], 0.0, p.a_z_sd, &g));
    if (grad) grad[T + 4 + k] = a_sd * da + g;
  }
  lp.add(survival_normal_logp(a_mu, 0.0, p.a_mu_sd, &g));
  if (grad) grad[T + 2] = sum_da.value() + g;
  lp.add(std::log(p.a_sd_rate));
  lp.add(-p.a_sd_rate * a_sd);
  lp.add(a_sl);
  if (grad) grad[T + 3] = (a_sd * sum_zda.value() - p.a_sd_rate * a_sd) + 1.0;
  lp.add(survival_normal_logp(b, 0.0, p.b_sd, &g));
  if (grad) grad[T + 4 + Gr] = (Wx - sum_aw.value()) + g;
  return lp.value();
}

// The layout of the individuals on the device: sorted by group (stable), every group padded to whole tiles of 64.  Returns the
// number of tiles; slot[j] = the column of individual j, tile_group[tile], group_tile[Gr + 1].  The labels must lie in [0, Gr).
inline int survival_groups_layout(int N, int Gr, const int32_t* group, int32_t* slot, int32_t* tile_group, int32_t* group_tile) {
  for (int g = 0; g <= Gr; ++g) group_tile[g] = 0;
  for (int j = 0; j < N; ++j) ++group_tile[group[j] + 1];  // sizes
  int tile = 0;
  for (int g = 0; g < Gr; ++g) {
    const int n = group_tile[g + 1];
    group_tile[g] = tile;
    for (int q = 0; q < (n + 63) / 64; ++q) tile_group[tile++] = g;
  }
  group_tile[Gr] = tile;
  std::vector<int32_t> next((size_t)Gr);  // the next free column of each group; j in ascending order: stable
  for (int g = 0; g < Gr; ++g) next[g] = group_tile[g] * 64;
  for (int j = 0; j < N; ++j) slot[j] = next[group[j]]++;
  return tile;
}

// The form of a handle's model: K titers (Gr = 0, no periods; abd_survival_terms.hpp), by group (Gr > 0, K = 1; this file), or by
// period (P > 0, period holds the T labels, K = 1; this file's closed forms around abd_survival_periods_terms.hpp).  Everything
// that differs between the three on the host is answered here: the sizes of a point and of its rows, and which closed forms make
// the parameter row of a point and combine its sums.
struct SurvivalForm {
  int K = 0, Gr = 0, T = 0, P = 0;
  std::vector<int32_t> period{};  // [T], by period only
  bool grouped() const { return Gr > 0; }
  bool by_period() const { return P > 0; }
  int dim() const { return by_period() ? survival_periods_dim(T, P) : grouped() ? survival_groups_dim(T, Gr) : survival_dim(K, T); }
  // a_t[T], b, or a[Gr], b, or a[K], b[K]: what follows lambda[T] in a parameter row
  int n_ab() const { return by_period() ? T + 1 : grouped() ? Gr + 1 : 2 * K; }
  int par_stride() const { return T + n_ab(); }
  int n_sums() const { return by_period() ? 2 * T + 2 : T + 2 + (grouped() ? Gr : K); }  // the sums of a point that mean something
  // the row the finalize kernel of the form writes
  int out_stride() const { return by_period() ? 2 * T + 2 : grouped() ? T + 2 + Gr : T + ABD_SURV_NW; }
  int work_stride() const { return by_period() ? survival_periods_work(T, P) : 2 * T; }  // the host's row of a point in flight
  int mode() const { return by_period() ? 3 : grouped() ? 0 : K; }                        // MODE of abd_survival_individual_kernel
  void prepare(const double* theta, double* par, double* work) const {
    if (by_period()) {  // the grouped row of the point into work, then one a per interval
      double* gpar = survival_periods_gpar(T, work);
      survival_groups_prepare(T, P, theta, gpar, work);
      survival_periods_expand(T, P, period.data(), gpar, par);
    } else if (grouped()) {
      survival_groups_prepare(T, Gr, theta, par, work);
    } else {
      survival_prepare(K, T, theta, par, work);
    }
  }
  // p: the priors of the form with K titers; gp: those of the forms by group and by period.  The other struct is not read.
  // work: the row prepare made of the point (by period, the folded sums are left in it)
  double combine(const SurvivalPriors& p, const SurvivalGroupsPriors& gp, const double* theta, const double* Y, double C,
                 const double* sums, const double* par, double* work, double* grad) const {
    if (by_period()) {  // W0_t into W0_p, then the grouped closed form on (T, P, W0_p, a_p)
      double* gsums = survival_periods_gsums(T, P, work);
      survival_periods_fold(T, P, period.data(), sums, gsums, survival_periods_comp(T, P, work));
      return survival_groups_combine(gp, T, P, theta, Y, C, gsums, survival_periods_gpar(T, work), work, grad);
    }
    return grouped() ? survival_groups_combine(gp, T, Gr, theta, Y, C, sums, par, work, grad)
                     : survival_combine(p, K, T, theta, Y, C, sums, par, work, grad);
  }
};

}  // namespace abdi
