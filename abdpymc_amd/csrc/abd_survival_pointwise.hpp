// abd_survival_pointwise.hpp -- the per-individual log-likelihood of the Poisson hazard models and its WAIC accumulators, for a
// handle of resident planes and for an ensemble of per-draw datasets.
//
// Per point (lambda_t, log lambda_t, a, b) and individual j, with the cell of abd_survival.hpp (y, e, x, eta, sigma):
//   ll_j = (C_j + A_j) - B_j
//   A_j  = sum_t [ y > 0 ? y (log lambda_t + log sigma_jt) : 0 ]      log sigma = min(eta, 0) - log1p(e^-|eta|)
//   B_j  = sum_t lambda_t (e sigma_jt)                                 one fma per cell
//   C_j  = sum_{t: y > 0} ( y log e - lgamma(y + 1) )                  from the host, per slot (abd_survival_pointwise_terms.hpp)
// PyMC's Poisson log-probability with fractional y, summed over the individual's intervals; sum_j ll_j is the data part of logp.
// Of an ensemble's event-time datasets C_j is an exact +0 and the kernel writes A_j - B_j (abd_survival.hpp, beside SurvSource,
// point (4)).
//
// Mapping: lane = individual (slot), a wave owns one tile of 64 and walks the intervals in ascending order, so A_j and B_j stay in
// the lane: no cross-lane sum, no LDS, no barrier, no atomics (of an ensemble the one cross-lane operation is the integer maximum
// of n_risk that ends the walk, SurvSource<true, .>).  The point is the grid's second dimension.  The order of every sum is fixed
// by T alone: a point's row is the same bits alone, as any row of a full launch and in any split of a longer call.  Cells
// without follow-up and the padding hold y = e = x = 0 and C = 0: sigma is finite, e sigma = 0, and the lane writes exactly 0.0.
// eta is SurvEta's and the cell SurvSource's, as in the sums kernel; sigma is surv_cell's (surv_sigma), and surv_cell itself is
// not called, it carries the wave sum of S_t.
//
// Row of a point: lambda[T], log lambda[T], ab[n_ab], 1 / n_draw (survival_pointwise_row); of an ensemble then n_draw, the draw's
// number WITHIN ITS DATASET (an int64 in the double's bits), and the dataset (an int32 in the low word): kDrawsRow*.
//
// abd_survival_waic_fold: thread = slot; the launch's n rows go into the handle's accumulators [4][ld] (rows M, S, mean, M2)
// in ascending order by waic_update (abd_readings.hpp), a plain read-modify-write of a column that one thread owns.  Folding
// draws one after the other makes the accumulators independent of how the draws were batched.
// abd_survival_draws_waic_fold: its ensemble form.  Row p goes into the accumulators of its own dataset in acc [M][4][ld]; the
// draw's number within its dataset and its 1 / n come with the row.  A thread owns its column in every dataset.  The statistics of
// dataset m see that dataset's rows in their order and nothing else: they do not depend on how rows were batched or on which other
// datasets' rows stood between them.
#pragma once

#include "abd_readings.hpp"
#include "abd_survival.hpp"

namespace abdi {

struct SurvivalPointArgs {
  SurvivalData data;
  const double* cj;           // [ld], plug-in only
  const double* par;          // [points][par_stride]: the row of a point, above
  const int32_t* tile_group;  // [ntile], the grouped form only
  double* ll;                 // [points][ld]
  int32_t T, ld, ntile, par_stride, n_ab;
};

// entries of an ensemble's row behind ab[n_ab]
constexpr int kDrawsRowInv = 0, kDrawsRowDraw = 1, kDrawsRowDataset = 2, kDrawsRowExtra = 3;

template <int MODE, bool DRAWS>
__global__ __launch_bounds__(256) void abd_survival_individual_kernel(const SurvivalPointArgs a) {
  constexpr bool TWO = MODE == 2;
  const int lane = threadIdx.x & 63;
  const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tile >= a.ntile) return;  // whole waves; no barrier below
  const int point = blockIdx.y;
  const double* lam = a.par + (int64_t)point * a.par_stride;
  const double* loglam = lam + a.T;
  const double* ab = loglam + a.T;
  const SurvEta<MODE> eta_of(ab, a.n_ab, a.tile_group, tile);
  const int slot = tile * 64 + lane;
  const SurvSource<DRAWS, TWO> src(a.data, ab + a.n_ab + kDrawsRowDataset, a.T, a.ld, slot, a.T);
  int64_t idx = slot;
  double A = 0.0, B = 0.0;
  for (int t = 0; t < src.t_end; ++t, idx += a.ld) {
    const SurvIn in = src.cell(t, idx);
    const double eta = eta_of(t, in.x0, in.x1);
    const SurvSigma sg = surv_sigma(eta);
    const double ls = fmin(eta, 0.0) - log1p(sg.en);
    A += in.y > 0.0 ? in.y * (loglam[t] + ls) : 0.0;
    B = fma(lam[t], in.e * sg.sig, B);
  }
  a.ll[(int64_t)point * a.ld + slot] = DRAWS ? A - B : (a.cj[slot] + A) - B;  // of an ensemble C_j = +0
}

// rows 0 .. n - 1 of ll [n][ld] into acc [4][ld] as draws n0 + 1 .. n0 + n; inv_n of row p at par[p * par_stride + inv_off]
__global__ __launch_bounds__(256) void abd_survival_waic_fold(const double* ll, const double* par, double* acc, int32_t ld,
                                                              int32_t par_stride, int32_t inv_off, int32_t n, int64_t n0) {
  const int slot = blockIdx.x * 256 + threadIdx.x;
  if (slot >= ld) return;
  for (int p = 0; p < n; ++p) waic_update(acc, slot, ld, ll[(int64_t)p * ld + slot], n0 + p + 1, par[(int64_t)p * par_stride + inv_off]);
}

// rows 0 .. n - 1 of ll [n][ld] into acc [M][4][ld], row p into its dataset's accumulators as that dataset's draw number n_draw
__global__ __launch_bounds__(256) void abd_survival_draws_waic_fold(const double* ll, const double* par, double* acc, int32_t ld,
                                                                    int32_t par_stride, int32_t inv_off, int32_t n) {
  const int slot = blockIdx.x * 256 + threadIdx.x;
  if (slot >= ld) return;
  for (int p = 0; p < n; ++p) {
    const double* tail = par + (int64_t)p * par_stride + inv_off;
    const int64_t n_draw = *reinterpret_cast<const int64_t*>(tail + kDrawsRowDraw);
    const int64_t ds = *reinterpret_cast<const int32_t*>(tail + kDrawsRowDataset);
    waic_update(acc + ds * 4 * ld, slot, ld, ll[(int64_t)p * ld + slot], n_draw, tail[kDrawsRowInv]);
  }
}

}  // namespace abdi
