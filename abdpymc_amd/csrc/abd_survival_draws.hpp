// abd_survival_draws.hpp -- the data sums of the Poisson hazard models over an ensemble of per-draw datasets: every
// point of a launch reads its OWN dataset, so that up to ABD_MAX_BATCH chains of different datasets share one launch.
//
// A per-draw dataset (risk.survival_arrays of one draw's binary infections) has event-time form: individual j is at risk in the
// intervals t < n_risk[j] and has its one infection, if any, in interval event[j] = n_risk[j] - 1 (else event[j] = -1).  So
//   e = (t < n_risk),  y = (t == event)
// are formed in registers and the resident data are the titer planes [dataset][interval][individual] and two int32 per
// individual and dataset; no y or e planes.  A cell that is not at risk takes y = e = x = 0, exactly what creation makes of it
// in an abd_survival handle of the same data (survival_check_cell): a titer read there (it may be NaN) is dropped by a select
// and reaches no sum.
//
// Mapping, split (ntile, nseg, seg_len from N and T alone), the cell (surv_cell) and the order of every sum are those of
// abd_survival_kernel<K>, and the partials go through abd_survival_finalize as they are: a point's sums are bit for bit what an
// abd_survival handle of that dataset returns.  One thing is skipped: a wave ends its range at the largest n_risk of its 64
// individuals and writes +0.0 for the S_t partials behind it.  In abd_survival_kernel those cells give e sigma = +0 and w = +0,
// the wave's sum of 64 +0 is +0, and an accumulator that started at +0.0 is unchanged by + (+0) -- it cannot hold -0, since a
// round-to-nearest sum is -0 only where both terms are.  No floating-point atomics.
#pragma once

#include "abd_survival.hpp"

namespace abdi {

struct SurvivalDrawsArgs {
  const double* x0;       // [M][T][ld]
  const double* x1;       // [M][T][ld], K = 2 only
  const int32_t* n_risk;  // [M][ld]; 0 in the padding
  const int32_t* event;   // [M][ld]; -1 in the padding
  const double* par;      // [points][par_stride]: lambda[T], a[K], b[K], then the dataset index (an int32 in the last double's low word)
  double* s_part;         // [points][ntile][T]
  double* w_part;         // [points][ntile * nseg][ABD_SURV_NW]
  int32_t T, ld, ntile, nseg, seg_len, par_stride;
};

// the largest v of the wave, as a scalar
__device__ __forceinline__ int wave_max_uniform(int v) {
  for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
  return __builtin_amdgcn_readfirstlane(v);
}

template <int K>
__global__ __launch_bounds__(256) void abd_survival_draws_kernel(const SurvivalDrawsArgs a) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nw = a.ntile * a.nseg;
  if (w >= nw) return;  // whole waves; no barrier below
  const int point = blockIdx.y;
  const int tile = w % a.ntile, seg = w / a.ntile;
  const int t0 = seg * a.seg_len, t1 = min(t0 + a.seg_len, a.T);
  const double* par = a.par + (int64_t)point * a.par_stride;
  const double a0 = par[a.T], b0 = par[a.T + K];
  const double a1 = K == 2 ? par[a.T + 1] : 0.0, b1 = K == 2 ? par[a.T + K + 1] : 0.0;
  const int64_t ds = *reinterpret_cast<const int32_t*>(par + a.T + 2 * K);  // wave-uniform, with the point's parameters
  const int col = tile * 64 + lane;
  const int nr = a.n_risk[ds * a.ld + col], ev = a.event[ds * a.ld + col];
  const int t_end = min(t1, wave_max_uniform(nr));  // behind it no lane of the wave is at risk
  const double* X0 = a.x0 + ds * a.T * a.ld;
  const double* X1 = K == 2 ? a.x1 + ds * a.T * a.ld : nullptr;
  double* s_row = a.s_part + ((int64_t)point * a.ntile + tile) * a.T;
  int64_t idx = (int64_t)t0 * a.ld + col;
  double L = 0.0, W0 = 0.0, W1 = 0.0, W2 = 0.0;
  for (int t = t0; t < t_end; ++t, idx += a.ld) {
    const bool at_risk = t < nr;
    const double y = t == ev ? 1.0 : 0.0, e = at_risk ? 1.0 : 0.0;
    const double x0 = at_risk ? X0[idx] : 0.0;
    const double lam = par[t];
    double eta = b0 * (x0 - a0);
    double x1 = 0.0;
    if (K == 2) {
      x1 = at_risk ? X1[idx] : 0.0;
      eta = fma(b1, x1 - a1, eta);
    }
    const SurvCell c = surv_cell(eta, y, e, lam, lane, s_row + t);
    L += c.ly;
    const double wc = c.w;
    W0 += wc;
    W1 = fma(wc, x0, W1);
    if (K == 2) W2 = fma(wc, x1, W2);
  }
  if (lane == 0)
    for (int t = max(t_end, t0); t < t1; ++t) s_row[t] = 0.0;
  L = wave_sum_uniform(L);
  W0 = wave_sum_uniform(W0);
  W1 = wave_sum_uniform(W1);
  if (K == 2) W2 = wave_sum_uniform(W2);
  if (lane == 0) {
    double* row = a.w_part + ((int64_t)point * nw + w) * ABD_SURV_NW;
    row[0] = L;
    row[1] = W0;
    row[2] = W1;
    row[3] = W2;
  }
}

}  // namespace abdi
