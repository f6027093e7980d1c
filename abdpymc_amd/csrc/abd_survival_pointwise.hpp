// abd_survival_pointwise.hpp -- the per-individual log-likelihood of the Poisson hazard models and its WAIC accumulators
// (DESIGN 21).
//
// Per point (lambda_t, log lambda_t, a, b) and individual j, with the cell of abd_survival.hpp (y, e, x, eta, sigma):
//   ll_j = (C_j + A_j) - B_j
//   A_j  = sum_t [ y > 0 ? y (log lambda_t + log sigma_jt) : 0 ]      log sigma = min(eta, 0) - log1p(e^-|eta|)
//   B_j  = sum_t lambda_t (e sigma_jt)                                 one fma per cell
//   C_j  = sum_{t: y > 0} ( y log e - lgamma(y + 1) )                  from the host, per slot (abd_survival_pointwise_terms.hpp)
// PyMC's Poisson log-probability with fractional y, summed over the individual's intervals; sum_j ll_j is the data part of logp.
//
// Mapping: lane = individual (slot), a wave owns one tile of 64 and walks all T intervals in ascending order, so A_j and B_j
// stay in the lane: no cross-lane operation, no LDS, no barrier, no atomics.  The point is the grid's second dimension.  The
// order of every sum is fixed by T alone: a point's row is the same bits alone, as any row of a full launch and in any split
// of a longer call.  Cells without follow-up and the padding hold y = e = x = 0 and C = 0: sigma is finite, e sigma = 0, and
// the lane writes exactly 0.0.  The grouped form reads its tile's a_g through tile_group as abd_survival_groups_kernel does; the
// form by period reads its interval's a_t inside the loop as abd_survival_periods_kernel does.
// sigma is surv_cell's (surv_sigma); surv_cell itself is not called, it carries the wave sum of S_t.
//
// abd_survival_waic_fold: thread = slot; the launch's n rows go into the handle's accumulators [4][ld] (rows M, S, mean, M2)
// in ascending order by waic_update (abd_readings.hpp), a plain read-modify-write of a column that one thread owns.  Folding
// draws one after the other makes the accumulators independent of how the draws were batched.
#pragma once

#include "abd_readings.hpp"
#include "abd_survival.hpp"

namespace abdi {

struct SurvivalPointArgs {
  const double* y;            // [T][ld]
  const double* e;            // [T][ld]
  const double* x0;           // [T][ld]
  const double* x1;           // [T][ld], K = 2 only
  const double* cj;           // [ld]
  const double* par;          // [points][par_stride]: lambda[T], log lambda[T], ab[n_ab], 1 / n_draw
  const int32_t* tile_group;  // [ntile], the grouped form only
  double* ll;                 // [points][ld]
  int32_t T, ld, ntile, par_stride, n_ab;
};

// MODE 1, 2: K titers, ab = a[K], b[K].  MODE 0: by group, ab = a[Gr], b.  MODE 3: by period, ab = a_t[T], b.
template <int MODE>
__global__ __launch_bounds__(256) void abd_survival_individual_kernel(const SurvivalPointArgs a) {
  const int lane = threadIdx.x & 63;
  const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tile >= a.ntile) return;  // whole waves; no barrier below
  const int point = blockIdx.y;
  const double* lam = a.par + (int64_t)point * a.par_stride;
  const double* loglam = lam + a.T;
  const double* ab = loglam + a.T;
  double a0, b0, a1 = 0.0, b1 = 0.0;
  if (MODE == 0) {
    a0 = ab[a.tile_group[tile]];
    b0 = ab[a.n_ab - 1];
  } else if (MODE == 3) {
    a0 = 0.0;  // per interval, below
    b0 = ab[a.n_ab - 1];
  } else {
    a0 = ab[0];
    b0 = ab[MODE];
    if (MODE == 2) {
      a1 = ab[1];
      b1 = ab[3];
    }
  }
  const int slot = tile * 64 + lane;
  int64_t idx = slot;
  double A = 0.0, B = 0.0;
  for (int t = 0; t < a.T; ++t, idx += a.ld) {
    const double y = a.y[idx], e = a.e[idx];
    if (MODE == 3) a0 = ab[t];
    double eta = b0 * (a.x0[idx] - a0);
    if (MODE == 2) eta = fma(b1, a.x1[idx] - a1, eta);
    const SurvSigma sg = surv_sigma(eta);
    const double ls = fmin(eta, 0.0) - log1p(sg.en);
    A += y > 0.0 ? y * (loglam[t] + ls) : 0.0;
    B = fma(lam[t], e * sg.sig, B);
  }
  a.ll[(int64_t)point * a.ld + slot] = (a.cj[slot] + A) - B;
}

// rows 0 .. n - 1 of ll [n][ld] into acc [4][ld] as draws n0 + 1 .. n0 + n; inv_n of row p at par[p * par_stride + inv_off]
__global__ __launch_bounds__(256) void abd_survival_waic_fold(const double* ll, const double* par, double* acc, int32_t ld,
                                                              int32_t par_stride, int32_t inv_off, int32_t n, int64_t n0) {
  const int slot = blockIdx.x * 256 + threadIdx.x;
  if (slot >= ld) return;
  for (int p = 0; p < n; ++p) waic_update(acc, slot, ld, ll[(int64_t)p * ld + slot], n0 + p + 1, par[(int64_t)p * par_stride + inv_off]);
}

}  // namespace abdi
