// abd_survival.hpp -- the data sums of the Poisson hazard models (reference survival.py:116-153).
//
// Per point (lambda_t, a_k, b_k) and cell (individual j, interval t) with y = infected, e = exposure, x_k = titer:
//   eta = sum_k b_k (x_k - a_k),  sigma = 1 / (1 + e^-eta),  mu = e lambda_t sigma,  w = (y - mu)(1 - sigma)
//   S_t = sum_j e sigma     L = sum_{y > 0} y log sigma     W_0 = sum w     W_k = sum w x_k
// The host turns the T + 2 + K sums into logp and gradient (abd_survival_terms.hpp).
//
// Mapping: lane = individual, a wave owns one tile of 64 individuals and one contiguous range of intervals; the data are
// resident as [interval][individual] planes padded to whole tiles, so that a wave's loads are 512 contiguous bytes per plane.
// Cells without follow-up and the padding hold y = e = x = 0 and add exact zeros: no guards in the loop.
// Order of every sum: 64 lanes by the DPP butterfly of wave_sum_uniform; S_t then over the tiles as four interleaved partial
// sums (tiles g, g + 4, ... in ascending order) added as ((g0 + g1) + g2) + g3; L and W_* over the wave's intervals in ascending
// order in each lane, then over the waves as 64 interleaved partial sums and a 64-way sum (finalize_chain's pattern).  The
// split into tiles and ranges is fixed at creation from N and T alone and the point is a grid dimension: a point's sums are
// the same bits whichever launch carries it.  No floating-point atomics.
#pragma once

#include "abd_device.hpp"
#include "abd_survival_terms.hpp"  // ABD_SURV_NW

namespace abdi {

struct SurvivalArgs {
  const double* y;    // [T][ld]
  const double* e;    // [T][ld]
  const double* x0;   // [T][ld]
  const double* x1;   // [T][ld], K = 2 only
  const double* par;  // [points][par_stride]: lambda[T], a[K], b[K]
  double* s_part;     // [points][ntile][T]
  double* w_part;     // [points][ntile * nseg][ABD_SURV_NW]
  double* out;        // [points][T + ABD_SURV_NW]: S_t[T], L, W_0, W_1, W_2
  int32_t T, ld, ntile, nseg, seg_len, par_stride;
};

// e^-|eta|, sigma and 1 - sigma without an overflowing exponential: en = e^-|eta| in (0, 1], d = 1 + en in [1, 2].
// The argument of 2^t is reduced from a two-term product with log2(e), so that en carries the polynomial's error and not
// |eta| roundings of it; the reciprocal takes a second Newton step (abd_device.hpp: 1.1e-16 against 2.2e-15 with one).
__device__ __forceinline__ double surv_exp_neg(double abs_eta) {
  const double hi = -1.4426950408889634, lo = -2.0355273740931033e-17;  // log2(e) = hi + lo
  abs_eta = fmin(abs_eta, 760.0);  // e^-760 < 2^-1074: the result is 0 from here on (and an infinite eta stays out of the fma)
  const double t_hi = abs_eta * hi;
  const double t_lo = fma(abs_eta, hi, -t_hi) + abs_eta * lo;
  const double k = __builtin_rint(t_hi);
  const double f = (t_hi - k) + t_lo;
  return ldexp(exp2_reduced(f), (int)k);
}

// en = e^-|eta|, sigma and 1 - sigma of one cell: the one formation of sigma, for the sums (surv_cell) and for the per-individual
// log-likelihood (abd_survival_pointwise.hpp).
struct SurvSigma {
  double en, sig, oms;
};
__device__ __forceinline__ SurvSigma surv_sigma(double eta) {
  const double en = surv_exp_neg(fabs(eta));
  double r = rcp_newton(1.0 + en);
  r = fma(fma(-(1.0 + en), r, 1.0), r, r);
  const double er = en * r;
  const bool pos = eta >= 0.0;
  return SurvSigma{en, pos ? r : er, pos ? er : r};
}

// One cell given eta: e sigma, summed over the wave into *s_t by lane 0; returns w = (y - mu)(1 - sigma) and the cell's
// y log sigma.  The one statement of the cell: abd_survival_kernel<K> and the grouped kernel (abd_survival_groups.hpp) differ
// in how they form eta.
struct SurvCell {
  double w, ly;
};
__device__ __forceinline__ SurvCell surv_cell(double eta, double y, double e, double lam, int lane, double* s_t) {
  const SurvSigma sg = surv_sigma(eta);
  const double es = e * sg.sig;
  const double S = wave_sum_uniform(es);
  if (lane == 0) *s_t = S;
  // log sigma = min(eta, 0) - log1p(e^-|eta|); a cell with y = 0 has no log term
  const double ls = fmin(eta, 0.0) - log1p(sg.en);
  const double ly = y > 0.0 ? y * ls : 0.0;
  return SurvCell{fma(-lam, es, y) * sg.oms, ly};
}

template <int K>
__global__ __launch_bounds__(256) void abd_survival_kernel(const SurvivalArgs a) {
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
  double* s_row = a.s_part + ((int64_t)point * a.ntile + tile) * a.T;
  int64_t idx = (int64_t)t0 * a.ld + tile * 64 + lane;
  double L = 0.0, W0 = 0.0, W1 = 0.0, W2 = 0.0;
  for (int t = t0; t < t1; ++t, idx += a.ld) {
    const double y = a.y[idx], e = a.e[idx], x0 = a.x0[idx];
    const double lam = par[t];
    double eta = b0 * (x0 - a0);
    double x1 = 0.0;
    if (K == 2) {
      x1 = a.x1[idx];
      eta = fma(b1, x1 - a1, eta);
    }
    const SurvCell c = surv_cell(eta, y, e, lam, lane, s_row + t);
    L += c.ly;
    const double wc = c.w;
    W0 += wc;
    W1 = fma(wc, x0, W1);
    if (K == 2) W2 = fma(wc, x1, W2);
  }
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

// n terms p[0], p[stride], ... added to 0.0 in ascending order, the loads sixteen at a time ahead of the additions
__device__ __forceinline__ double surv_sum_strided(const double* __restrict__ p, int n, int64_t stride) {
  double v = 0.0;
  for (int i0 = 0; i0 < n; i0 += 16) {
    double q[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) q[u] = i0 + u < n ? p[(int64_t)(i0 + u) * stride] : 0.0;
#pragma unroll
    for (int u = 0; u < 16; ++u) v += q[u];
  }
  return v;
}

// S_t of 64 intervals by one workgroup of 256 threads: thread (g, t) adds the tiles g, g + 4, g + 8, ... in ascending order, then
// ((g0 + g1) + g2) + g3.  s_part: [points][ntile][T] partials; sm: 256 doubles.
__device__ __forceinline__ void surv_finalize_s(const double* s_part, int point, int ntile, int T, int block, double* sm, double* out) {
  const int tid = threadIdx.x;
  const int t = block * 64 + (tid & 63), g = tid >> 6;
  const bool live = t < T;
  const double* sp = s_part + (int64_t)point * ntile * T + (int64_t)g * T + (live ? t : 0);
  const int n = (ntile - g + 3) / 4;  // tiles g, g + 4, ... below ntile
  const double v = live ? surv_sum_strided(sp, n, 4 * (int64_t)T) : 0.0;
  sm[tid] = v;
  __syncthreads();
  if (g == 0 && live) out[t] = ((sm[tid] + sm[tid + 64]) + sm[tid + 128]) + sm[tid + 192];
}

// The ABD_SURV_NW columns of the nw rows of wp by one workgroup of 256 threads, as 64 interleaved partial sums (rows part,
// part + 64, ...) left in sm (256 doubles); after it, thread k < ABD_SURV_NW takes column k's sum with surv_sum_parts(sm, k).
__device__ __forceinline__ void surv_finalize_w(const double* wp, int nw, double* sm) {
  const int tid = threadIdx.x;
  const int k = tid % ABD_SURV_NW, part = tid / ABD_SURV_NW;  // 64 parts: waves part, part + 64, ...
  sm[part * ABD_SURV_NW + k] = surv_sum_strided(wp + (int64_t)part * ABD_SURV_NW + k, part < nw ? (nw - part + 63) / 64 : 0, 64 * ABD_SURV_NW);
  __syncthreads();
}

// the 64-way sum of column k's partial sums, in ascending order
__device__ __forceinline__ double surv_sum_parts(const double* sm, int k) {
  double t = 0.0;
#pragma unroll
  for (int q = 0; q < 64; ++q) t += sm[q * ABD_SURV_NW + k];
  return t;
}

// The fixed-order sums over tiles and waves.  Grid (ceil(T / 64) + 1, points), 256 threads.  Workgroup x < ceil(T / 64): S_t of
// 64 intervals (surv_finalize_s).  The last workgroup: L and W_* over the waves (surv_finalize_w).  The order depends on N and T
// alone.
__global__ __launch_bounds__(256) void abd_survival_finalize(const SurvivalArgs a) {
  __shared__ double sm[64 * ABD_SURV_NW];
  const int tid = threadIdx.x, point = blockIdx.y;
  double* out = a.out + (int64_t)point * (a.T + ABD_SURV_NW);
  if (blockIdx.x + 1 < gridDim.x) {
    surv_finalize_s(a.s_part, point, a.ntile, a.T, blockIdx.x, sm, out);
    return;
  }
  const int nw = a.ntile * a.nseg;
  surv_finalize_w(a.w_part + (int64_t)point * nw * ABD_SURV_NW, nw, sm);
  if (tid < ABD_SURV_NW) out[a.T + tid] = surv_sum_parts(sm, tid);
}

}  // namespace abdi
