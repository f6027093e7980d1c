// abd_survival_draws_forms.hpp -- the data sums of the Poisson hazard models by group and by period over an ensemble of per-draw
// datasets: every point of a launch reads its OWN dataset, as in abd_survival_draws.hpp, for the two forms whose
// midpoint of the titer carries a label (abd_survival_groups.hpp; abd_survival_periods.hpp).
//
// Data side: that of abd_survival_draws_kernel<1>.  One titer plane [dataset][interval][column] and two int32 per column and
// dataset, n_risk and event; e = (t < n_risk) and y = (t == event) are formed in registers, the titer of a cell not at risk is
// dropped by a select, and the dataset index is the int32 in the low word of the last double of the point's parameter row, read
// with the row's other wave-uniform values.  A wave ends its range at the largest n_risk of its 64 lanes.
//
// Mapping: that of the plug-in kernel of the form.
//   by group   columns sorted by group (stable) and every group padded to whole tiles of 64, the same for every dataset (the
//              labels belong to the individuals, not to a draw); tile_group / group_tile as in abd_survival_groups.hpp, so that
//              ntile and ld come from the group sizes; a_g through tile_group[tile], wave-uniform.  Row: lambda[T], a[Gr], b, dataset.
//   by period  the caller's order of individuals; a_t per interval, wave-uniform; W0_t by the butterfly inside the loop.
//              Row: lambda[T], a_t[T], b, dataset.
// The partials go through abd_survival_groups_finalize / abd_survival_periods_finalize as they are.
//
// Why a point on dataset m returns, bit for bit, what the plug-in handle of the form made of that dataset's (infected, exposure,
// titer) returns (abd_survival_create_groups / abd_survival_create_periods):
//   (1) the same cell.  Creation of the plug-in handle makes y = e = x = 0 of a cell not at risk and keeps y in {0, 1}, e = 1 and
//       the titer of a cell at risk; the selects here give the same three doubles, and eta = b (x - a), surv_cell and the
//       updates of L, W0 / W_x are the plug-in kernel's expressions in its order.
//   (2) the same split.  ntile, seg_len and nseg come from the tile count and T alone (SurvivalSums::plan), the tile count from N
//       (by period) or from the group sizes (by group): a wave owns the same tile and the same range in both kernels.
//   (3) the same order of every sum: in a lane over the wave's intervals ascending, the butterfly of wave_sum_uniform over the
//       lanes, and the plug-in form's own finalize kernel over tiles and waves.
//   (4) the skipped cells add nothing.  Behind t_end no lane of the wave is at risk: in the plug-in kernel such a cell has
//       e sigma = +0 (e = +0, sigma in [0, 1]), w = fma(-lambda, +0, +0) (1 - sigma) = +0 and no log term, the butterfly of 64 +0
//       is +0, and an accumulator that started at +0.0 is unchanged by + (+0) and by fma(+0, 0, .) -- it cannot hold -0, since a
//       round-to-nearest sum is -0 only where both terms are.  So the S_t partial of a skipped interval is +0.0, which lane 0
//       writes here, and L, W0, W_x are what they would be.
//   and for these two forms:
//   (5) by group, a padding lane is a lane with n_risk = 0 and event = -1: never at risk, y = e = x = 0 in every interval, which
//       is what the plug-in handle's padding columns hold.  A tile none of whose individuals is ever at risk skips its whole range
//       and writes +0.0 to all of it.
//   (6) by period, the W0_t partial of a skipped interval is the butterfly of 64 w = +0, which is +0: lane 0 writes +0.0 to
//       w0_part as it does to s_part.
// Fixed-order sums only: no floating-point atomics, no LDS in the two kernels.
#pragma once

#include "abd_survival_draws.hpp"  // wave_max_uniform

namespace abdi {

struct SurvivalDrawsFormArgs {
  const double* x;            // [M][T][ld]
  const int32_t* n_risk;      // [M][ld]; 0 in the padding
  const int32_t* event;       // [M][ld]; -1 in the padding
  const double* par;          // [points][par_stride]: the form's row, then the dataset index (an int32 in the last double's low word)
  const int32_t* tile_group;  // [ntile], by group only
  double* s_part;             // [points][ntile][T]
  double* w0_part;            // [points][ntile][T], by period only
  double* w_part;             // [points][ntile * nseg][ABD_SURV_NW]: L, W0 (by group) or 0, W_x, 0
  int32_t T, Gr, ld, ntile, nseg, seg_len, par_stride;
};

__global__ __launch_bounds__(256) void abd_survival_draws_groups_kernel(const SurvivalDrawsFormArgs a) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nw = a.ntile * a.nseg;
  if (w >= nw) return;  // whole waves; no barrier below
  const int point = blockIdx.y;
  const int tile = w % a.ntile, seg = w / a.ntile;
  const int t0 = seg * a.seg_len, t1 = min(t0 + a.seg_len, a.T);
  const double* par = a.par + (int64_t)point * a.par_stride;
  const double ag = par[a.T + a.tile_group[tile]], b = par[a.T + a.Gr];
  const int64_t ds = *reinterpret_cast<const int32_t*>(par + a.T + a.Gr + 1);  // wave-uniform, with the point's parameters
  const int col = tile * 64 + lane;
  const int nr = a.n_risk[ds * a.ld + col], ev = a.event[ds * a.ld + col];
  const int t_end = min(t1, wave_max_uniform(nr));  // behind it no lane of the wave is at risk
  const double* X = a.x + ds * a.T * a.ld;
  double* s_row = a.s_part + ((int64_t)point * a.ntile + tile) * a.T;
  int64_t idx = (int64_t)t0 * a.ld + col;
  double L = 0.0, W0 = 0.0, Wx = 0.0;
  for (int t = t0; t < t_end; ++t, idx += a.ld) {
    const bool at_risk = t < nr;
    const double y = t == ev ? 1.0 : 0.0, e = at_risk ? 1.0 : 0.0;
    const double x = at_risk ? X[idx] : 0.0;
    const SurvCell c = surv_cell(b * (x - ag), y, e, par[t], lane, s_row + t);
    L += c.ly;
    const double wc = c.w;
    W0 += wc;
    Wx = fma(wc, x, Wx);
  }
  if (lane == 0)
    for (int t = max(t_end, t0); t < t1; ++t) s_row[t] = 0.0;
  L = wave_sum_uniform(L);
  W0 = wave_sum_uniform(W0);
  Wx = wave_sum_uniform(Wx);
  if (lane == 0) {
    double* row = a.w_part + ((int64_t)point * nw + w) * ABD_SURV_NW;
    row[0] = L;
    row[1] = W0;
    row[2] = Wx;
    row[3] = 0.0;
  }
}

__global__ __launch_bounds__(256) void abd_survival_draws_periods_kernel(const SurvivalDrawsFormArgs a) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nw = a.ntile * a.nseg;
  if (w >= nw) return;  // whole waves; no barrier below
  const int point = blockIdx.y;
  const int tile = w % a.ntile, seg = w / a.ntile;
  const int t0 = seg * a.seg_len, t1 = min(t0 + a.seg_len, a.T);
  const double* par = a.par + (int64_t)point * a.par_stride;
  const double* at = par + a.T;
  const double b = par[2 * a.T];
  const int64_t ds = *reinterpret_cast<const int32_t*>(par + 2 * a.T + 1);  // wave-uniform, with the point's parameters
  const int col = tile * 64 + lane;
  const int nr = a.n_risk[ds * a.ld + col], ev = a.event[ds * a.ld + col];
  const int t_end = min(t1, wave_max_uniform(nr));  // behind it no lane of the wave is at risk
  const double* X = a.x + ds * a.T * a.ld;
  const int64_t row = ((int64_t)point * a.ntile + tile) * a.T;
  double* s_row = a.s_part + row;
  double* w0_row = a.w0_part + row;
  int64_t idx = (int64_t)t0 * a.ld + col;
  double L = 0.0, Wx = 0.0;
  for (int t = t0; t < t_end; ++t, idx += a.ld) {
    const bool at_risk = t < nr;
    const double y = t == ev ? 1.0 : 0.0, e = at_risk ? 1.0 : 0.0;
    const double x = at_risk ? X[idx] : 0.0;
    const SurvCell c = surv_cell(b * (x - at[t]), y, e, par[t], lane, s_row + t);
    L += c.ly;
    const double wc = c.w;
    Wx = fma(wc, x, Wx);
    const double W0 = wave_sum_uniform(wc);
    if (lane == 0) w0_row[t] = W0;
  }
  if (lane == 0)
    for (int t = max(t_end, t0); t < t1; ++t) {
      s_row[t] = 0.0;
      w0_row[t] = 0.0;
    }
  L = wave_sum_uniform(L);
  Wx = wave_sum_uniform(Wx);
  if (lane == 0) {
    double* r = a.w_part + ((int64_t)point * nw + w) * ABD_SURV_NW;
    r[0] = L;
    r[1] = 0.0;
    r[2] = Wx;
    r[3] = 0.0;
  }
}

}  // namespace abdi
