// abd_survival_groups.hpp -- the data sums of the Poisson hazard model by group (reference survival.py:155-174).
//
// Per point (lambda_t, a_g, b) and cell (individual j of group g(j), interval t), with the cell of abd_survival.hpp (surv_cell):
//   eta = b (x - a_g(j)),  sigma, mu, w as there
//   S_t = sum_j e sigma     L = sum_{y > 0} y log sigma     W_x = sum w x     W0_g = sum_{j in g} w
// The host turns the T + 2 + Gr sums into logp and gradient (abd_survival_groups_terms.hpp).
//
// Mapping: at creation the individuals are sorted by group (stable) and every group is padded to whole tiles of 64, so that a
// tile belongs to one group: tile_group[tile] names it, and group g owns the tiles [group_tile[g], group_tile[g + 1]).  As in
// abd_survival.hpp a wave owns one tile and one contiguous range of intervals, reads its a_g from the point's parameter row
// (lambda[T], a[Gr], b) as a wave-uniform value and runs surv_cell; padding lanes hold y = e = x = 0 and add exact zeros.
//
// Order of every sum -- fixed by N, T and the group sizes alone (they fix the tiles, the ranges and the two tables):
//   within a wave: L, W_x, W0 over the wave's intervals in ascending order in each lane, then 64 lanes by the DPP butterfly of
//     wave_sum_uniform; e sigma of one interval by the same butterfly;
//   S_t over all tiles as four interleaved partial sums (tiles q, q + 4, ... ascending) added as ((q0 + q1) + q2) + q3
//     (surv_finalize_s);
//   L and W_x over all waves w = range * ntile + tile as 64 interleaved partial sums (waves p, p + 64, ... ascending) and a
//     64-way sum in ascending order (surv_finalize_w);
//   W0_g by one wave per group over the waves of the group's tiles only, numbered i = range * n_g + (tile - group_tile[g]) with
//     n_g the group's tile count: lane l adds i = l, l + 64, ... in ascending order to 0.0, then the butterfly of
//     wave_sum_uniform.  A group without tiles adds nothing in any lane: exactly 0.0.
// The point is the grid's second dimension: a point's sums are the same bits whichever launch carries it.  No floating-point
// atomics.
#pragma once

#include "abd_survival.hpp"

namespace abdi {

struct SurvivalGroupsArgs {
  const double* y;    // [T][ld]
  const double* e;    // [T][ld]
  const double* x;    // [T][ld]
  const double* par;  // [points][par_stride]: lambda[T], a[Gr], b
  const int32_t* tile_group;  // [ntile]
  const int32_t* group_tile;  // [Gr + 1]
  double* s_part;     // [points][ntile][T]
  double* w_part;     // [points][ntile * nseg][ABD_SURV_NW]: L, W0, W_x, 0
  double* out;        // [points][T + 2 + Gr]: S_t[T], L, W_x, W0_g[Gr]
  int32_t T, Gr, ld, ntile, nseg, seg_len, par_stride;
};

__global__ __launch_bounds__(256) void abd_survival_groups_kernel(const SurvivalGroupsArgs a) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nw = a.ntile * a.nseg;
  if (w >= nw) return;  // whole waves; no barrier below
  const int point = blockIdx.y;
  const int tile = w % a.ntile, seg = w / a.ntile;
  const int t0 = seg * a.seg_len, t1 = min(t0 + a.seg_len, a.T);
  const double* par = a.par + (int64_t)point * a.par_stride;
  const double ag = par[a.T + a.tile_group[tile]], b = par[a.T + a.Gr];
  double* s_row = a.s_part + ((int64_t)point * a.ntile + tile) * a.T;
  int64_t idx = (int64_t)t0 * a.ld + tile * 64 + lane;
  double L = 0.0, W0 = 0.0, Wx = 0.0;
  for (int t = t0; t < t1; ++t, idx += a.ld) {
    const double y = a.y[idx], e = a.e[idx], x = a.x[idx];
    const SurvCell c = surv_cell(b * (x - ag), y, e, par[t], lane, s_row + t);
    L += c.ly;
    const double wc = c.w;
    W0 += wc;
    Wx = fma(wc, x, Wx);
  }
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

// The fixed-order sums.  Grid (ceil(T / 64) + 1 + ceil(Gr / 4), points), 256 threads.  Workgroup x < ceil(T / 64): S_t of 64
// intervals.  Workgroup ceil(T / 64): L and W_x over all waves.  The others: W0_g, one wave per group.
__global__ __launch_bounds__(256) void abd_survival_groups_finalize(const SurvivalGroupsArgs a) {
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
