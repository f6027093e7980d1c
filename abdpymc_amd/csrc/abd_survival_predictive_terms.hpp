// abd_survival_predictive_terms.hpp -- what the posterior predictive checks of the survival models state once for the
// kernel (abd_survival_predictive.hpp), the host (abd_survival.hip) and the native harness
// (tests/native/survival_predictive_harness.cpp): the bin of a titer, the keyed uniform of a cell, the Poisson draw, and the
// host's sums of the constants of the data.  Plain C++ with __host__ __device__ functions, no HIP.
//
//   mu_jt(d) = e_jt lambda_t(d) sigma_jt(d)
//   r_jt(d)  = the Poisson(mu) quantile of u(seed, j, t, d): a function of the seed, the CALLER's index j, t and the draw index d
//   bin      = #{edges <= x}: risk.bin_of's rule, at most ABD_SURV_PRED_BINS bins of at most two binning variables
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "abd_survival_terms.hpp"  // SurvivalSum, SurvivalRefusal
#include "abd_types.hpp"           // philox4x32_10, sim_uniform, kSurvReplicate

#define ABD_SURV_PRED_BINS 8     // bins of a variable: up to 7 edges
#define ABD_SURV_PRED_VARS 2     // binning variables
#define ABD_SURV_PRED_MAX_E 4.0  // the largest exposure taken: mu < 4, and the cap of the inversion never binds
#define ABD_SURV_PRED_CAP 32     // P(k > 32 | mu < 4) < 1e-19

namespace abdi {

// #{edges <= x}; a NaN titer (a cell without follow-up) compares false throughout: bin 0
__host__ __device__ inline int surv_pred_bin(double x, const double* edges, int n_edges) {
  int b = 0;
  for (int k = 0; k < n_edges; ++k) b += edges[k] <= x ? 1 : 0;
  return b;
}

// the edges of one variable: null, or why they are refused
inline const char* surv_pred_check_edges(int n_edges, const double* edges) {
  if (n_edges < 0 || n_edges > ABD_SURV_PRED_BINS - 1) return "at most 7 edges (8 bins)";
  for (int k = 0; k < n_edges; ++k) {
    if (!std::isfinite(edges[k])) return "edges must be finite";
    if (k > 0 && !(edges[k] > edges[k - 1])) return "edges must be strictly ascending";
  }
  return nullptr;
}

// The uniform of cell (j, t) at draw d: one Philox call, counter (j, t, low word of d, kSurvReplicate), key (seed lo, seed hi).
// j is the caller's index of the individual, whatever column the handle keeps it in.
__host__ __device__ inline double surv_pred_uniform(uint32_t seed_lo, uint32_t seed_hi, uint32_t j, uint32_t t, uint32_t draw_lo) {
  const Philox4 p = philox4x32_10(j, t, draw_lo, kSurvReplicate, seed_lo, seed_hi);
  return sim_uniform(p.w[0], p.w[1]);
}

// Poisson(mu) at the uniform u in (0, 1) by sequential inversion.  mu = 0 gives 0 with no guard: exp(-0) = 1 > u.
__host__ __device__ inline int surv_pred_poisson(double mu, double u) {
  int k = 0;
  double p = exp(-mu), c = p;
  while (u >= c && k < ABD_SURV_PRED_CAP) {
    ++k;
    p *= mu / k;
    c += p;
  }
  return k;
}

// The constants of the data of one configuration, per (variable, bin) and per individual in the caller's order
struct SurvPredConstants {
  double observed[ABD_SURV_PRED_VARS][ABD_SURV_PRED_BINS];      // O = sum y
  double person_time[ABD_SURV_PRED_VARS][ABD_SURV_PRED_BINS];   // PT = sum e
  int64_t n_cells[ABD_SURV_PRED_VARS][ABD_SURV_PRED_BINS];      // followed cells
  std::vector<double> observed_ind;                             // [N] O_j = sum_t y
};

// What configuration makes of the binning variables.  y, e: the resident planes [T][ld] (cleaned: cells without follow-up and the
// padding hold y = e = 0); column(j) = slot ? slot[j] : j.  titers[v], v < n_var: [N][T] in the caller's order; edges[v] has
// n_edges[v] checked entries.  Writes the byte plane bins[T][ld] (bin of variable 0 in the low nibble, of variable 1 in the high
// one; 0 for cells without follow-up and the padding), slot_j[ld] (the caller's index of a column, -1 for padding) and the
// constants, summed with j ascending, then t ascending, by SurvivalSum.  The first refused cell ends it.
inline SurvivalRefusal surv_pred_pack(int N, int T, size_t ld, const int32_t* slot, const double* y, const double* e, int n_var,
                                      const double* const* titers, const int32_t* n_edges, const double* const* edges, uint8_t* bins,
                                      int32_t* slot_j, SurvPredConstants* c) {
  for (size_t k = 0; k < ld * (size_t)T; ++k) bins[k] = 0;
  for (size_t k = 0; k < ld; ++k) slot_j[k] = -1;
  SurvivalSum O[ABD_SURV_PRED_VARS][ABD_SURV_PRED_BINS], PT[ABD_SURV_PRED_VARS][ABD_SURV_PRED_BINS];
  for (int v = 0; v < ABD_SURV_PRED_VARS; ++v)
    for (int b = 0; b < ABD_SURV_PRED_BINS; ++b) c->n_cells[v][b] = 0;
  c->observed_ind.assign((size_t)N, 0.0);
  for (int j = 0; j < N; ++j) {
    const size_t col = slot ? (size_t)slot[j] : (size_t)j;
    slot_j[col] = j;
    SurvivalSum Oj;
    for (int t = 0; t < T; ++t) {
      const size_t cell = (size_t)t * ld + col;
      const double yy = y[cell], ee = e[cell];
      if (ee > ABD_SURV_PRED_MAX_E) return SurvivalRefusal{j, t, "exposure above 4 (the replicate's inversion is capped for mu < 4)"};
      if (!(ee > 0.0)) continue;
      unsigned byte = 0;
      for (int v = 0; v < n_var; ++v) {
        const double x = titers[v][(size_t)j * T + t];
        if (!std::isfinite(x)) return SurvivalRefusal{j, t, "binning titer of a followed cell must be finite"};
        const int b = surv_pred_bin(x, edges[v], n_edges[v]);
        byte |= (unsigned)b << (4 * v);
        O[v][b].add(yy);
        PT[v][b].add(ee);
        ++c->n_cells[v][b];
      }
      bins[cell] = (uint8_t)byte;
      Oj.add(yy);
    }
    c->observed_ind[(size_t)j] = Oj.value();
  }
  for (int v = 0; v < ABD_SURV_PRED_VARS; ++v)
    for (int b = 0; b < ABD_SURV_PRED_BINS; ++b) {
      c->observed[v][b] = O[v][b].value();
      c->person_time[v][b] = PT[v][b].value();
    }
  return SurvivalRefusal{-1, -1, nullptr};
}

}  // namespace abdi
