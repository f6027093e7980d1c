// abd_survival_pointwise_terms.hpp -- the host half of the per-individual log-likelihood of the survival models: the
// constant of the data C_j and the number of followed cells of every column of the resident planes, and the parameter row one
// point gives abd_survival_individual_kernel and abd_survival_waic_fold.  Plain C++, no HIP: one source for the library
// (abd_survival.hip) and for the native harness (tests/native/survival_pointwise_harness.cpp).
//
//   ll_j = C_j + A_j - B_j
//   A_j  = sum_t [ y > 0 ? y (log lambda_t + log sigma_jt) : 0 ]      B_j = sum_t e lambda_t sigma_jt      (the device, ascending t)
//   C_j  = sum_{t: y > 0} ( y log e - lgamma(y + 1) )                  (here, once at creation)
#pragma once

#include <cstdint>

#include "abd_survival_terms.hpp"

namespace abdi {

// C[ld] and n_cells[ld] of the planes y, e [T][ld] as creation lays them out (cells without follow-up and padding hold
// y = e = 0).  Per column the terms y log e, then -lgamma(y + 1), of the cells with y > 0 in ascending t, by SurvivalSum; a
// column without such a cell gets exactly 0.0.  n_cells counts the cells with e > 0.
inline void survival_pointwise_constants(int T, int ld, const double* y, const double* e, double* C, int32_t* n_cells) {
  for (int j = 0; j < ld; ++j) {
    SurvivalSum sum;
    int32_t n = 0;
    for (int t = 0; t < T; ++t) {
      const double yy = y[(size_t)t * ld + j], ee = e[(size_t)t * ld + j];
      if (ee > 0.0) ++n;
      if (yy > 0.0) {
        sum.add(yy * std::log(ee));
        sum.add(-std::lgamma(yy + 1.0));
      }
    }
    C[j] = sum.value();
    n_cells[j] = n;
  }
}

// The row of one point: lambda[T], log lambda[T], ab[n_ab], 1 / n_draw.  par and work are what survival_prepare /
// survival_groups_prepare made of the point (par = lambda[T], ab[n_ab]; work = log lambda[T], ...): lambda_t is the same bits
// the sums' kernels read.  ab is a[K], b[K], or a[Gr], b.  n_draw: the number of the draw the fold gives this point, >= 1; 0
// where nothing is folded (the row's last entry is 0 then).  The division is the host's, so the accumulators' bits do not
// depend on the device's.
inline int survival_pointwise_stride(int T, int n_ab) { return 2 * T + n_ab + 1; }
inline void survival_pointwise_row(int T, int n_ab, const double* par, const double* work, int64_t n_draw, double* row) {
  for (int t = 0; t < T; ++t) {
    row[t] = par[t];
    row[T + t] = work[t];
  }
  for (int k = 0; k < n_ab; ++k) row[2 * T + k] = par[T + k];
  row[2 * T + n_ab] = n_draw > 0 ? 1.0 / (double)n_draw : 0.0;
}

}  // namespace abdi
