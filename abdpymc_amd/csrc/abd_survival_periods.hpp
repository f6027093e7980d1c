// abd_survival_periods.hpp -- the data sums of the Poisson hazard model by period: the midpoint of the titer varies
// with the interval, a_t = a_p(t), and the slope b is shared.
//
// Per point (lambda_t, a_t, b) and cell (individual j, interval t), with the cell of abd_survival.hpp (surv_cell):
//   eta = b (x - a_t),  sigma, mu, w as there
//   S_t = sum_j e sigma     W0_t = sum_j w     L = sum_{y > 0} y log sigma     W_x = sum w x
// The host expands the P midpoints of a point to one per interval and folds W0_t into W0_p (abd_survival_periods_terms.hpp): the
// kernel knows nothing of periods.
//
// Mapping: that of abd_survival_kernel<1> -- lane = individual in the caller's order, a wave owns one tile of 64 individuals and
// one contiguous range of intervals, the same resident [interval][individual] planes y, e, x and the same ntile / seg_len / nseg
// plan from N and T alone.  A point's parameter row is lambda[T], a_t[T], b; a_t is read per interval as a wave-uniform value,
// as lambda_t is.  Padding lanes hold y = e = x = 0 and add exact zeros.
//
// Order of every sum -- fixed by N and T alone:
//   e sigma and w of one interval over the 64 lanes by the DPP butterfly of wave_sum_uniform, into s_part and w0_part;
//   S_t and W0_t then over the tiles as four interleaved partial sums (tiles q, q + 4, ... ascending) added as
//     ((q0 + q1) + q2) + q3 (surv_finalize_s, once over each of the two partial planes);
//   L and W_x over the wave's intervals in ascending order in each lane, then the butterfly, then over all waves
//     w = range * ntile + tile as 64 interleaved partial sums and a 64-way sum in ascending order (surv_finalize_w).
// The point is the grid's second dimension: a point's sums are the same bits whichever launch carries it.  No floating-point
// atomics, no LDS in the main kernel.
#pragma once

#include "abd_survival.hpp"

namespace abdi {

struct SurvivalPeriodsArgs {
  const double* y;    // [T][ld]
  const double* e;    // [T][ld]
  const double* x;    // [T][ld]
  const double* par;  // [points][par_stride]: lambda[T], a_t[T], b
  double* s_part;     // [points][ntile][T]
  double* w0_part;    // [points][ntile][T]
  double* w_part;     // [points][ntile * nseg][ABD_SURV_NW]: L, 0, W_x, 0 (the grouped kernel's columns)
  double* out;        // [points][2 T + 2]: S_t[T], L, W_x, W0_t[T]
  int32_t T, ld, ntile, nseg, seg_len, par_stride;
};

__global__ __launch_bounds__(256) void abd_survival_periods_kernel(const SurvivalPeriodsArgs a) {
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
  const int64_t row = ((int64_t)point * a.ntile + tile) * a.T;
  double* s_row = a.s_part + row;
  double* w0_row = a.w0_part + row;
  int64_t idx = (int64_t)t0 * a.ld + tile * 64 + lane;
  double L = 0.0, Wx = 0.0;
  for (int t = t0; t < t1; ++t, idx += a.ld) {
    const double y = a.y[idx], e = a.e[idx], x = a.x[idx];
    const SurvCell c = surv_cell(b * (x - at[t]), y, e, par[t], lane, s_row + t);
    L += c.ly;
    const double wc = c.w;
    Wx = fma(wc, x, Wx);
    const double W0 = wave_sum_uniform(wc);
    if (lane == 0) w0_row[t] = W0;
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

// The fixed-order sums.  Grid (2 ceil(T / 64) + 1, points), 256 threads.  Workgroup x < ceil(T / 64): S_t of 64 intervals.  The next
// ceil(T / 64): W0_t of 64 intervals, the same sum over the other partial plane.  The last: L and W_x over all waves.
__global__ __launch_bounds__(256) void abd_survival_periods_finalize(const SurvivalPeriodsArgs a) {
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
