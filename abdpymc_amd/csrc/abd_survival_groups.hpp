// abd_survival_groups.hpp -- the Poisson hazard model by group (reference survival.py:155-174): the layout of its
// columns and the fixed-order sums behind abd_survival_sums_kernel<0, .> (abd_survival.hpp).
//
// Per point (lambda_t, a_g, b) and cell (individual j of group g(j), interval t), with the cell of abd_survival.hpp (surv_cell):
//   eta = b (x - a_g(j)),  sigma, mu, w as there
//   S_t = sum_j e sigma     L = sum_{y > 0} y log sigma     W_x = sum w x     W0_g = sum_{j in g} w
// The host turns the T + 2 + Gr sums into logp and gradient (abd_survival_groups_terms.hpp).
//
// Layout: at creation the individuals are sorted by group (stable) and every group is padded to whole tiles of 64, so that a
// tile belongs to one group: tile_group[tile] names it, and group g owns the tiles [group_tile[g], group_tile[g + 1]).  The layout
// belongs to the individuals: an ensemble of per-draw datasets shares it among its datasets.  A wave reads its a_g from the point's
// parameter row (lambda[T], a[Gr], b) through tile_group as a wave-uniform value (SurvEta<0>); padding lanes hold y = e = x = 0
// and add exact zeros.  A wave's row of w_part is L, W0, W_x, 0.
//
// Order of the sums over tiles and waves -- fixed by N, T and the group sizes alone (they fix the tiles, the ranges and the two
// tables); within a wave it is that of abd_survival.hpp:
//   S_t over all tiles by surv_finalize_s, L and W_x over all waves by surv_finalize_w;
//   W0_g by one wave per group over the waves of the group's tiles only, numbered i = range * n_g + (tile - group_tile[g]) with
//     n_g the group's tile count: lane l adds i = l, l + 64, ... in ascending order to 0.0, then the butterfly of
//     wave_sum_uniform.  A group without tiles adds nothing in any lane: exactly 0.0.
#pragma once

#include "abd_survival.hpp"

namespace abdi {

// The fixed-order sums.  Grid (ceil(T / 64) + 1 + ceil(Gr / 4), points), 256 threads.  Workgroup x < ceil(T / 64): S_t of 64
// intervals.  Workgroup ceil(T / 64): L and W_x over all waves.  The others: W0_g, one wave per group.
// out: [points][T + 2 + Gr]: S_t[T], L, W_x, W0_g[Gr].
__global__ __launch_bounds__(256) void abd_survival_groups_finalize(const SurvivalSumsArgs a) {
  __shared__ double sm[64 * ABD_SURV_NW];
  const int tid = threadIdx.x, point = blockIdx.y;
  const int ns = (a.T + 63) / 64;
  double* out = a.out + (int64_t)point * (a.T + 2 + a.Gr);
  const int nw = a.ntile * a.nseg;
  const double* wp = a.w_part + (int64_t)point * nw * ABD_SURV_NW;
  if ((int)blockIdx.x < ns) {
    surv_finalize_s(a.s_part, point, a.ntile, a.T, blockIdx.x, sm, out);
    return;
  }
  if ((int)blockIdx.x == ns) {
    surv_finalize_w(wp, nw, sm);
    if (tid == 0) out[a.T] = surv_sum_parts(sm, 0);      // L
    if (tid == 1) out[a.T + 1] = surv_sum_parts(sm, 2);  // W_x
    return;
  }
  const int g = ((int)blockIdx.x - ns - 1) * 4 + (tid >> 6), lane = tid & 63;
  if (g >= a.Gr) return;  // whole waves; no barrier below
  const int tile0 = a.group_tile[g], ng = a.group_tile[g + 1] - tile0;
  const int n = ng * a.nseg;  // the waves of this group's tiles
  double v = 0.0;
  for (int i = lane; i < n; i += 64) {
    const int seg = i / ng, tile = tile0 + i % ng;
    v += wp[((int64_t)seg * a.ntile + tile) * ABD_SURV_NW + 1];
  }
  v = wave_sum_uniform(v);
  if (lane == 0) out[a.T + 2 + g] = v;
}

}  // namespace abdi
