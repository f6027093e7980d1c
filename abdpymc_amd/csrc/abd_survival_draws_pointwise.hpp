// abd_survival_draws_pointwise.hpp -- the per-individual log-likelihood of the Poisson hazard models over an ensemble of per-draw
// datasets, and its per-dataset WAIC accumulators: the ensemble form of abd_survival_pointwise.hpp, every point of a
// launch on its OWN dataset.
//
// Mapping: that of abd_survival_individual_kernel<MODE>.  Lane = individual (slot), a wave owns one tile of 64 and walks the
// intervals in ascending order, the point is the grid's second dimension; A_j and B_j stay in the lane: no cross-lane sum, no LDS,
// no barrier, no atomics (the one cross-lane operation is the integer maximum of n_risk that bounds the walk).  By group the
// column layout and tile_group are those of abd_survival_draws_groups_kernel, the same for every dataset.
//
// Data side: that of abd_survival_draws_kernel.  The titer planes [dataset][interval][column] and two int32 per column and
// dataset; e = (t < n_risk) and y = (t == event) are formed in registers, the titer of a cell not at risk is dropped by a select,
// the dataset index is the int32 in the low word of the last double of the point's row, read with the row's other wave-uniform
// values, and a wave ends its walk at the largest n_risk of its 64 lanes (wave_max_uniform).
//
// Row of a point: lambda[T], log lambda[T], ab[n_ab], 1 / n_draw, n_draw (an int64 in the double's bits), dataset (an int32 in
// the low word) -- the row of survival_pointwise_row, then the draw's number WITHIN ITS DATASET and the dataset.
//
// Why a row on dataset m is, bit for bit, what abd_survival_individual_loglik returns on a plug-in handle of the same form made
// of that dataset's (infected, exposure, titer) -- for a finite parameter row, which is what a sampler hands over:
//   (a) the same cell in the same order.  Creation of the plug-in handle makes y = e = x = 0 of a cell not at risk and keeps
//       y in {0, 1}, e = 1 and the titer of a cell at risk; the selects here give the same three doubles.  eta = b (x - a)
//       (K = 2: fma(b1, x1 - a1, .)), surv_sigma(eta), ls = fmin(eta, 0) - log1p(en), A += y > 0 ? y (log lambda_t + ls) : 0 and
//       B = fma(lambda_t, e sigma, B) are the plug-in kernel's expressions, in ascending t, with the same lambda_t and
//       log lambda_t (the host's, from the same prepare of the same form).
//   (b) C_j is an exact +0.  Of an event-time dataset the host's C_j (survival_pointwise_constants) sums, per cell with y > 0,
//       y log e = 1 log 1 = +0 and -lgamma(2) = -0; the compensated sum of those from +0.0 is +0.0, and so is the C_j of a column
//       without an event.  So the plug-in's (C + A) - B is (+0 + A) - B = A - B: +0 + A is A for every A but -0, and (c) excludes
//       that.
//   (c) the skipped cells add nothing.  Behind t_end no lane of the wave is at risk: in the plug-in kernel such a cell has y = 0,
//       which adds +0.0 to A, and e sigma = +0 (e = +0, sigma in [0, 1]), fma(lambda, +0, B) = B + (+0) = B.  Neither accumulator
//       can hold -0: both start at +0.0, and a round-to-nearest sum is -0 only where both terms are.  So A and B behind t_end are
//       what they were at t_end.
//   (d) by group, a padding lane is a lane with n_risk = 0 and event = -1: never at risk, y = e = x = 0 in every interval it
//       walks, A = B = +0.0, and it writes A - B = an exact 0.0 -- what the plug-in handle's padding column holds, whose C is 0.
//       The same holds for the padding behind N of the other forms and for an individual that is never at risk.
//
// abd_survival_draws_waic_fold: thread = slot, the ensemble form of abd_survival_waic_fold.  The launch's n rows go, in ascending
// order, into the accumulators [4][ld] (rows M, S, mean, M2) of their own dataset in acc [M][4][ld] by waic_update; the draw's
// number within its dataset and its 1 / n come with the row.  A thread owns its column in every dataset: a plain
// read-modify-write.  The statistics of dataset m see that dataset's rows in their order and nothing else: they do not depend on
// how rows were batched or on which other datasets' rows stood between them.
#pragma once

#include "abd_readings.hpp"
#include "abd_survival_draws.hpp"  // wave_max_uniform

namespace abdi {

struct SurvivalDrawsPointArgs {
  const double* x0;           // [M][T][ld]
  const double* x1;           // [M][T][ld], K = 2 only
  const int32_t* n_risk;      // [M][ld]; 0 in the padding
  const int32_t* event;       // [M][ld]; -1 in the padding
  const double* par;          // [points][par_stride]: lambda[T], log lambda[T], ab[n_ab], 1 / n_draw, n_draw, dataset
  const int32_t* tile_group;  // [ntile], the grouped form only
  double* ll;                 // [points][ld]
  int32_t T, ld, ntile, par_stride, n_ab;
};

// entries of a row behind ab[n_ab]
constexpr int kDrawsRowInv = 0, kDrawsRowDraw = 1, kDrawsRowDataset = 2, kDrawsRowExtra = 3;

// MODE 1, 2: K titers, ab = a[K], b[K].  MODE 0: by group, ab = a[Gr], b.  MODE 3: by period, ab = a_t[T], b.
template <int MODE>
__global__ __launch_bounds__(256) void abd_survival_draws_individual_kernel(const SurvivalDrawsPointArgs a) {
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
  const int64_t ds = *reinterpret_cast<const int32_t*>(ab + a.n_ab + kDrawsRowDataset);  // wave-uniform, with the point's parameters
  const int slot = tile * 64 + lane;
  const int nr = a.n_risk[ds * a.ld + slot], ev = a.event[ds * a.ld + slot];
  const int t_end = min(a.T, wave_max_uniform(nr));  // behind it no lane of the wave is at risk
  const double* X0 = a.x0 + ds * a.T * a.ld;
  const double* X1 = MODE == 2 ? a.x1 + ds * a.T * a.ld : nullptr;
  int64_t idx = slot;
  double A = 0.0, B = 0.0;
  for (int t = 0; t < t_end; ++t, idx += a.ld) {
    const bool at_risk = t < nr;
    const double y = t == ev ? 1.0 : 0.0, e = at_risk ? 1.0 : 0.0;
    const double x0 = at_risk ? X0[idx] : 0.0;
    if (MODE == 3) a0 = ab[t];
    double eta = b0 * (x0 - a0);
    if (MODE == 2) {
      const double x1 = at_risk ? X1[idx] : 0.0;
      eta = fma(b1, x1 - a1, eta);
    }
    const SurvSigma sg = surv_sigma(eta);
    const double ls = fmin(eta, 0.0) - log1p(sg.en);
    A += y > 0.0 ? y * (loglam[t] + ls) : 0.0;
    B = fma(lam[t], e * sg.sig, B);
  }
  a.ll[(int64_t)point * a.ld + slot] = A - B;  // C_j = +0
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
