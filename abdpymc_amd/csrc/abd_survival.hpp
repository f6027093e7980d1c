// abd_survival.hpp -- the data sums of the Poisson hazard models, of every form and of either kind of handle (DESIGN 19, 20, 24,
// 26, 29, 31; reference survival.py:116-174).
//
// Per point (lambda_t, a, b) and cell (individual j, interval t) with y = infected, e = exposure, x_k = titer:
//   eta = sum_k b_k (x_k - a_k),  sigma = 1 / (1 + e^-eta),  mu = e lambda_t sigma,  w = (y - mu)(1 - sigma)
//   S_t = sum_j e sigma     L = sum_{y > 0} y log sigma     W_0 = sum w     W_k = sum w x_k
// The forms differ in the midpoint a of the titer (SurvEta): one per titer (K = 1, 2), one per group of individuals, a_g(j), or one
// per interval, a_t.  By group W_0 is wanted per group, W0_g; by period per interval, W0_t.  The host turns the sums into logp and
// gradient (abd_survival_terms.hpp, abd_survival_groups_terms.hpp, abd_survival_periods_terms.hpp).
//
// Mapping: lane = individual (column), a wave owns one tile of 64 columns and one contiguous range of intervals; the data are
// [interval][column] planes padded to whole tiles, so that a wave's loads are 512 contiguous bytes per plane.  By group the
// columns are sorted by group and every group is padded to whole tiles (abd_survival_groups.hpp); the other forms keep the
// caller's order.  Cells without follow-up and the padding hold y = e = x = 0 and add exact zeros: no guards in the loop.
// Where a cell comes from -- resident planes, or the event-time form of an ensemble of per-draw datasets -- is the business of
// SurvSource.
//
// Order of every sum -- fixed by the tile count and T alone (SurvivalSums::plan), and by the group sizes where there are groups:
//   e sigma of one interval, and by period w of one interval, over the 64 lanes by the DPP butterfly of wave_sum_uniform, into
//     s_part and w0_part;
//   L, W_0 (not by period), W_x = W_1 and W_2 over the wave's intervals in ascending order in each lane, then the butterfly, into
//     the wave's row of w_part;
//   S_t (and W0_t) over the tiles as four interleaved partial sums (tiles g, g + 4, ... ascending) added as ((g0 + g1) + g2) + g3
//     (surv_finalize_s);
//   L and W_* over all waves w = range * ntile + tile as 64 interleaved partial sums (waves p, p + 64, ... ascending) and a 64-way
//     sum in ascending order (surv_finalize_w; finalize_chain's pattern);
//   W0_g over the waves of the group's tiles (abd_survival_groups.hpp).
// The point is the grid's second dimension: a point's sums are the same bits whichever launch carries it.  No floating-point
// atomics, no LDS in the sums kernel.
#pragma once

#include "abd_device.hpp"
#include "abd_survival_terms.hpp"  // ABD_SURV_NW

namespace abdi {

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
// y log sigma.  The one statement of the cell; abd_survival_sums_kernel is its one caller.
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

// ---- the form rule: how a form makes eta of a cell ----
//
// MODE 1, 2: K titers, ab = a[K], b[K].  MODE 0: by group, ab = a[Gr], b, and a_g through tile_group[tile].  MODE 3: by period,
// ab = a_t[T], b, and a_t per interval.  `ab` is what follows lambda[T] (and, in a pointwise row, log lambda[T]) in the point's
// parameter row, n_ab its length (SurvivalForm::n_ab); every value read here is wave-uniform.  The one place that forms eta: the
// sums, the per-individual log-likelihood (abd_survival_pointwise.hpp) and the replicates (abd_survival_predictive.hpp) use it.
template <int MODE>
struct SurvEta {
  const double* ab;
  double a0, b0, a1 = 0.0, b1 = 0.0;
  __device__ __forceinline__ SurvEta(const double* ab_, int n_ab, const int32_t* tile_group, int tile) : ab(ab_) {
    if (MODE == 0) {
      a0 = ab[tile_group[tile]];
      b0 = ab[n_ab - 1];
    } else if (MODE == 3) {
      a0 = 0.0;  // per interval, below
      b0 = ab[n_ab - 1];
    } else {
      a0 = ab[0];
      b0 = ab[MODE];
      if (MODE == 2) {
        a1 = ab[1];
        b1 = ab[3];
      }
    }
  }
  __device__ __forceinline__ double operator()(int t, double x0, double x1) const {
    // t >= 0, and the index says so: with a signed one abd_survival_individual_kernel<3, true> takes 84 VGPRs for 80 and loses
    // its sixth wave per SIMD
    const double eta = b0 * (x0 - (MODE == 3 ? ab[(unsigned)t] : a0));
    return MODE == 2 ? fma(b1, x1 - a1, eta) : eta;
  }
};

// ---- the cell source: where y, e and the titers of a cell come from ----
//
// An abd_survival handle keeps y, e, x0 (and x1) resident as [interval][column] planes.  An abd_survival_draws handle
// keeps M per-draw datasets in event-time form: column j of dataset m is at risk in the intervals t < n_risk[m][j] and has its one
// infection, if any, in interval event[m][j] = n_risk[m][j] - 1 (else -1), so e = (t < n_risk) and y = (t == event) are formed in
// registers and the resident data are the titer planes [dataset][interval][column] and two int32 per column and dataset.  Every
// point of an ensemble launch reads its OWN dataset: the dataset index is the int32 in the low word of the double behind the form's
// part of the point's row, read with the row's other wave-uniform values.
//
// Both sources feed the same kernel body, so the same cell goes through the same expressions, the same split and the same order of
// every sum by construction.  What is left to argue for "a point on dataset m returns, bit for bit, what a plug-in handle of the
// same form made of that dataset's (infected, exposure, titer) returns" (finite parameters, which is what a sampler hands over):
//   (1) the same three doubles.  Creation of the plug-in handle makes y = e = x = 0 of a cell not at risk and keeps y in {0, 1},
//       e = 1 and the titer of a cell at risk (survival_pack).  The selects below give the same: a titer read from a cell not at
//       risk (it may be NaN) is dropped by the select and reaches no sum.
//   (2) cells behind t_end add +0.  A wave ends its range at the largest n_risk of its 64 lanes: behind it no lane is at risk.  In
//       the plug-in kernel such a cell has y = 0 and so no log term, e sigma = +0 (e = +0, sigma in [0, 1]) and
//       w = fma(-lambda, +0, +0) (1 - sigma) = +0; the butterfly of 64 +0 is +0; and an accumulator that started at +0.0 is
//       unchanged by + (+0) and by fma(+0, x, .) or fma(lambda, +0, .) -- it cannot hold -0, since a round-to-nearest sum is -0
//       only where both terms are.  So L, W_*, A_j and B_j are what they would be, and the S_t (by period also the W0_t) partial
//       of a skipped interval is +0.0, which lane 0 writes in the kernel's tail.  A tile none of whose columns is ever at risk
//       skips its whole range and writes +0.0 to all of it.
//   (3) padding lanes.  A padding column (behind N, or behind a group's last individual) has n_risk = 0 and event = -1: never at
//       risk, y = e = x = 0 in every interval, which is what the plug-in handle's padding columns hold.
//   (4) C_j = +0 (the per-individual log-likelihood only).  Of an event-time dataset the host's C_j
//       (survival_pointwise_constants) sums, per cell with y > 0, y log e = 1 log 1 = +0 and -lgamma(2) = -0; the compensated sum
//       of those from +0.0 is +0.0, and so is the C_j of a column without an event.  So the plug-in's (C_j + A) - B is
//       (+0 + A) - B = A - B: +0 + A is A for every A but -0, which (2) excludes.
struct SurvivalData {
  const double* y;        // [T][ld]                       plug-in only
  const double* e;        // [T][ld]                       plug-in only
  const double* x0;       // [T][ld], ensemble [M][T][ld]
  const double* x1;       // as x0, K = 2 only
  const int32_t* n_risk;  // [M][ld]; 0 in the padding     ensemble only
  const int32_t* event;   // [M][ld]; -1 in the padding    ensemble only
};

struct SurvIn {
  double y, e, x0, x1;
};

// the largest v of the wave, as a scalar
__device__ __forceinline__ int wave_max_uniform(int v) {
  for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
  return __builtin_amdgcn_readfirstlane(v);
}

// TWO: the form reads a second titer (K = 2).  col: the lane's column; the wave walks the intervals [., t1) and stops at t_end;
// dataset: the word that holds the dataset index; cell(t, idx) with idx = t * ld + col
template <bool DRAWS, bool TWO>
struct SurvSource;

template <bool TWO>
struct SurvSource<false, TWO> {
  const SurvivalData& d;
  int t_end;
  __device__ __forceinline__ SurvSource(const SurvivalData& d_, const double*, int, int, int, int t1) : d(d_), t_end(t1) {}
  __device__ __forceinline__ SurvIn cell(int, int64_t idx) const {
    return SurvIn{d.y[idx], d.e[idx], d.x0[idx], TWO ? d.x1[idx] : 0.0};
  }
};

template <bool TWO>
struct SurvSource<true, TWO> {
  const double *x0, *x1;
  int nr, ev, t_end;
  __device__ __forceinline__ SurvSource(const SurvivalData& d, const double* dataset, int T, int ld, int col, int t1) {
    const int64_t ds = *reinterpret_cast<const int32_t*>(dataset);  // wave-uniform, with the point's parameters
    nr = d.n_risk[ds * ld + col];
    ev = d.event[ds * ld + col];
    t_end = min(t1, wave_max_uniform(nr));  // behind it no lane of the wave is at risk
    x0 = d.x0 + ds * T * ld;
    x1 = TWO ? d.x1 + ds * T * ld : nullptr;
  }
  __device__ __forceinline__ SurvIn cell(int t, int64_t idx) const {
    const bool at_risk = t < nr;
    return SurvIn{t == ev ? 1.0 : 0.0, at_risk ? 1.0 : 0.0, at_risk ? x0[idx] : 0.0, TWO ? (at_risk ? x1[idx] : 0.0) : 0.0};
  }
};

// ---- the sums kernel, of every form and of either source ----
struct SurvivalSumsArgs {
  SurvivalData data;
  const double* par;          // [points][par_stride]: lambda[T], ab[n_ab]; ensemble: then the dataset index
  const int32_t* tile_group;  // [ntile], by group only
  const int32_t* group_tile;  // [Gr + 1], by group only (the finalize)
  double* s_part;             // [points][ntile][T]
  double* w0_part;            // [points][ntile][T], by period only
  double* w_part;             // [points][ntile * nseg][ABD_SURV_NW]: L, W_0 (by period 0), W_x = W_1, W_2 (K = 2, else 0)
  double* out;                // [points][SurvivalForm::out_stride()]: what the form's finalize kernel writes
  int32_t T, Gr, n_ab, ld, ntile, nseg, seg_len, par_stride;
};

// By period W_0 is wanted per interval: the butterfly runs inside the loop and lane 0 writes W0_t beside S_t; column 1 of the
// wave's row stays 0.
template <int MODE, bool DRAWS>
__global__ __launch_bounds__(256) void abd_survival_sums_kernel(const SurvivalSumsArgs a) {
  constexpr bool TWO = MODE == 2;
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nw = a.ntile * a.nseg;
  if (w >= nw) return;  // whole waves; no barrier below
  const int point = blockIdx.y;
  const int tile = w % a.ntile, seg = w / a.ntile;
  const int t0 = seg * a.seg_len, t1 = min(t0 + a.seg_len, a.T);
  const double* par = a.par + (int64_t)point * a.par_stride;
  const SurvEta<MODE> eta(par + a.T, a.n_ab, a.tile_group, tile);
  const int col = tile * 64 + lane;
  const SurvSource<DRAWS, TWO> src(a.data, par + a.T + a.n_ab, a.T, a.ld, col, t1);
  const int64_t row = ((int64_t)point * a.ntile + tile) * a.T;
  double* s_row = a.s_part + row;
  double* w0_row = a.w0_part + row;  // written by period only
  int64_t idx = (int64_t)t0 * a.ld + col;
  double L = 0.0, W0 = 0.0, W1 = 0.0, W2 = 0.0;
  for (int t = t0; t < src.t_end; ++t, idx += a.ld) {
    const SurvIn in = src.cell(t, idx);
    const SurvCell c = surv_cell(eta(t, in.x0, in.x1), in.y, in.e, par[t], lane, s_row + t);
    L += c.ly;
    const double wc = c.w;
    if (MODE == 3) {
      const double W0t = wave_sum_uniform(wc);
      if (lane == 0) w0_row[t] = W0t;
    } else {
      W0 += wc;
    }
    W1 = fma(wc, in.x0, W1);
    if (TWO) W2 = fma(wc, in.x1, W2);
  }
  if (DRAWS && lane == 0)
    for (int t = max(src.t_end, t0); t < t1; ++t) {
      s_row[t] = 0.0;
      if (MODE == 3) w0_row[t] = 0.0;
    }
  L = wave_sum_uniform(L);
  if (MODE != 3) W0 = wave_sum_uniform(W0);
  W1 = wave_sum_uniform(W1);
  if (TWO) W2 = wave_sum_uniform(W2);
  if (lane == 0) {
    double* r = a.w_part + ((int64_t)point * nw + w) * ABD_SURV_NW;
    r[0] = L;
    r[1] = W0;
    r[2] = W1;
    r[3] = W2;
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

// The fixed-order sums over tiles and waves of the form with K titers.  Grid (ceil(T / 64) + 1, points), 256 threads.  Workgroup
// x < ceil(T / 64): S_t of 64 intervals (surv_finalize_s).  The last workgroup: L and W_* over the waves (surv_finalize_w).  The
// order depends on N and T alone.  out: [points][T + ABD_SURV_NW]: S_t[T], L, W_0, W_1, W_2.
__global__ __launch_bounds__(256) void abd_survival_finalize(const SurvivalSumsArgs a) {
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
