// abd_survival_periods_terms.hpp -- what the host adds for the Poisson hazard model by period: the expansion of a
// point's P midpoints to one per interval for the kernel, and the fold of the kernel's W0_t into W0_p.  Around the two, the closed
// forms are the grouped model's (abd_survival_groups_terms.hpp) with (T, P, W0_p, a_p) in the places of (T, Gr, W0_g, a_g):
// SurvivalForm, at the end of that file, puts them together.  Plain C++, no HIP: one source for the library (abd_survival.hip)
// and for the native harness (tests/native/survival_periods_harness.cpp).
//
//   theta = m, s, z[T], a_mu, a_sl, az[P], b      (the grouped layout with Gr -> P)
//   a_p = a_mu + a_sd az_p;  a_t = a_p(t)          period[t] in [0, P)
//   par  = lambda[T], a_t[T], b                    (what abd_survival_sums_kernel<3, .> reads)
//   sums = S_t[T], L, W_x, W0_t[T]                 (what it returns)
//   W0_p = sum_{t in p} W0_t                       (ascending t, compensated; a period without intervals: exactly 0)
//   d/da_p = -b W0_p;  d/db = W_x - sum_p a_p W0_p (survival_groups_combine)
#pragma once

#include "abd_survival_terms.hpp"  // SurvivalSum

namespace abdi {

inline int survival_periods_dim(int T, int P) { return T + P + 5; }

// The work row of one point: log lambda[T], (1 - lambda)[T] as for the other forms, then what the grouped closed forms read --
// gpar = lambda[T], a_p[P], b and gsums = S_t[T], L, W_x, W0_p[P] -- and the P compensation terms of the fold.
inline int survival_periods_work(int T, int P) { return 2 * T + (T + P + 1) + (T + 2 + P) + P; }
inline double* survival_periods_gpar(int T, double* work) { return work + 2 * T; }
inline double* survival_periods_gsums(int T, int P, double* work) { return work + 2 * T + (T + P + 1); }
inline double* survival_periods_comp(int T, int P, double* work) { return survival_periods_gsums(T, P, work) + T + 2 + P; }

// par = lambda[T], a_t[T], b from gpar = lambda[T], a_p[P], b (what survival_groups_prepare made of the point): copies, so that
// every interval of a period reads the same bits
inline void survival_periods_expand(int T, int P, const int32_t* period, const double* gpar, double* par) {
  for (int t = 0; t < T; ++t) {
    par[t] = gpar[t];
    par[T + t] = gpar[T + period[t]];
  }
  par[2 * T] = gpar[T + P];
}

// gsums = S_t[T], L, W_x, W0_p[P] from the device's sums = S_t[T], L, W_x, W0_t[T]: every W0_p a SurvivalSum of its intervals'
// W0_t in ascending t.  comp: P doubles of scratch.
inline void survival_periods_fold(int T, int P, const int32_t* period, const double* sums, double* gsums, double* comp) {
  for (int k = 0; k < T + 2; ++k) gsums[k] = sums[k];
  double* W0 = gsums + T + 2;
  for (int p = 0; p < P; ++p) W0[p] = comp[p] = 0.0;
  for (int t = 0; t < T; ++t) {
    const int p = period[t];
    SurvivalSum acc{W0[p], comp[p]};
    acc.add(sums[T + 2 + t]);
    W0[p] = acc.s;
    comp[p] = acc.c;
  }
  for (int p = 0; p < P; ++p) W0[p] = SurvivalSum{W0[p], comp[p]}.value();
}

}  // namespace abdi
