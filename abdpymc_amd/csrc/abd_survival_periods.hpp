// abd_survival_periods.hpp -- the Poisson hazard model by period: the midpoint of the titer varies with the interval,
// a_t = a_p(t), and the slope b is shared.  The fixed-order sums behind abd_survival_sums_kernel<3, .> (abd_survival.hpp).
//
// Per point (lambda_t, a_t, b) and cell (individual j, interval t), with the cell of abd_survival.hpp (surv_cell):
//   eta = b (x - a_t),  sigma, mu, w as there
//   S_t = sum_j e sigma     W0_t = sum_j w     L = sum_{y > 0} y log sigma     W_x = sum w x
// The host expands the P midpoints of a point to one per interval and folds W0_t into W0_p (abd_survival_periods_terms.hpp): the
// kernels know nothing of periods.
//
// Layout: that of the form with one titer -- the caller's order of individuals, the same planes and the same ntile / seg_len / nseg
// plan from N and T alone.  A point's parameter row is lambda[T], a_t[T], b; a_t is read per interval as a wave-uniform value, as
// lambda_t is (SurvEta<3>).  W0_t goes over the lanes by the butterfly inside the loop, into a second plane of partials, w0_part,
// laid out as s_part; a wave's row of w_part is L, 0, W_x, 0.
//
// Order of the sums over tiles and waves -- fixed by N and T alone; within a wave it is that of abd_survival.hpp:
//   S_t and W0_t over the tiles by surv_finalize_s, once over each of the two partial planes;
//   L and W_x over all waves by surv_finalize_w.
#pragma once

#include "abd_survival.hpp"

namespace abdi {

// The fixed-order sums.  Grid (2 ceil(T / 64) + 1, points), 256 threads.  Workgroup x < ceil(T / 64): S_t of 64 intervals.  The next
// ceil(T / 64): W0_t of 64 intervals, the same sum over the other partial plane.  The last: L and W_x over all waves.
// out: [points][2 T + 2]: S_t[T], L, W_x, W0_t[T].
__global__ __launch_bounds__(256) void abd_survival_periods_finalize(const SurvivalSumsArgs a) {
  __shared__ double sm[64 * ABD_SURV_NW];
  const int tid = threadIdx.x, point = blockIdx.y;
  const int ns = (a.T + 63) / 64;
  double* out = a.out + (int64_t)point * (2 * a.T + 2);
  if ((int)blockIdx.x < ns) {
    surv_finalize_s(a.s_part, point, a.ntile, a.T, blockIdx.x, sm, out);
    return;
  }
  if ((int)blockIdx.x < 2 * ns) {
    surv_finalize_s(a.w0_part, point, a.ntile, a.T, (int)blockIdx.x - ns, sm, out + a.T + 2);
    return;
  }
  const int nw = a.ntile * a.nseg;
  surv_finalize_w(a.w_part + (int64_t)point * nw * ABD_SURV_NW, nw, sm);
  if (tid == 0) out[a.T] = surv_sum_parts(sm, 0);      // L
  if (tid == 1) out[a.T + 1] = surv_sum_parts(sm, 2);  // W_x
}

}  // namespace abdi
