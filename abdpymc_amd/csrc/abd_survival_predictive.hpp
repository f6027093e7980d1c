// abd_survival_predictive.hpp -- posterior predictive checks of the Poisson hazard models: per draw and cell the
// expected count mu = e lambda_t sigma and a Poisson replicate of it, reduced over titer bins and over individuals.
//
// abd_survival_replicate_kernel<MODE>: the mapping of abd_survival_individual_kernel (abd_survival_pointwise.hpp) -- lane =
// individual slot, a wave owns one tile of 64 and walks all T intervals in ascending order, the point is the grid's second
// dimension -- with eta formed by the same SurvEta<MODE> (abd_survival.hpp), so E_j = sum_t mu and R_j = sum_t r stay in the lane.
// The bin sums are lane-private columns in LDS, [variable][bin][thread], fp64 for mu and uint32 for r: a thread reads, modifies
// and writes its own column only, so there are no atomics, no barrier, and the order is ascending t.  After the loop a wave sums its columns
// over the lanes (wave_sum_uniform; the counts as doubles, exact below 2^53 in any order) and writes one partial row per (point,
// tile).  The replicate of a cell is surv_pred_poisson at surv_pred_uniform of (seed, caller's index j, t, draw index): the
// kernel reads j of its slot from slot_j, so the grouped layout's reordering does not reach the replicates.  Cells without
// follow-up and the padding hold e = 0: mu = +0.0, replicate 0, bin 0.  No cross-lane step inside the loop; whole waves return
// early and nothing waits on them.
//
// abd_survival_predictive_finalize: per (point, variable, bin) the tile partials as 16 interleaved partial sums (tiles g, g + 16,
// ... ascending), then the 16 in ascending order; the order depends on the tile count alone.  Counts are added as int64.
// abd_survival_predictive_fold: thread = slot; the launch's rows E_j, R_j and R_j >= 1 into the handle's accumulators in
// ascending draw order (abd_survival_waic_fold's pattern): the accumulators do not depend on how the draws were batched.
// No floating-point atomics anywhere.
#pragma once

#include "abd_survival.hpp"
#include "abd_survival_predictive_terms.hpp"

#define ABD_SURV_PRED_COLS (ABD_SURV_PRED_VARS * ABD_SURV_PRED_BINS)  // a partial row: [variable][bin]

namespace abdi {

struct SurvivalReplicateArgs {
  const double* e;            // [T][ld]
  const double* x0;           // [T][ld]
  const double* x1;           // [T][ld], K = 2 only
  const uint8_t* bins;        // [T][ld]: bin of variable 0 | bin of variable 1 << 4
  const int32_t* slot_j;      // [ld]: the caller's index of a column
  const double* par;          // [points][par_stride]: lambda[T], ab[n_ab]
  const int32_t* tile_group;  // [ntile], the grouped form only
  double* e_part;             // [points][ntile][ABD_SURV_PRED_COLS]
  uint32_t* r_part;           // [points][ntile][ABD_SURV_PRED_COLS]
  double* ej;                 // [points][ld]
  int32_t* rj;                // [points][ld]
  int32_t* rep;               // [points][T][ld], or null
  int64_t draw0;              // the draw index of point 0
  uint32_t seed_lo, seed_hi;
  int32_t T, ld, ntile, par_stride, n_ab, n_var;
};

// LDS of a launch: n_var * 8 columns of 256 doubles, then as many of 256 uint32
inline size_t survival_replicate_lds(int n_var) { return (size_t)n_var * ABD_SURV_PRED_BINS * 256 * (sizeof(double) + sizeof(uint32_t)); }

// MODE as SurvEta's (abd_survival.hpp)
template <int MODE>
__global__ __launch_bounds__(256) void abd_survival_replicate_kernel(const SurvivalReplicateArgs a) {
  extern __shared__ double surv_pred_lds[];
  const int lane = threadIdx.x & 63;
  const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tile >= a.ntile) return;  // whole waves; no barrier below
  const int point = blockIdx.y;
  const int ncol = a.n_var * ABD_SURV_PRED_BINS;
  double* Ec = surv_pred_lds + threadIdx.x;                                              // column c at Ec[c * 256]
  uint32_t* Rc = reinterpret_cast<uint32_t*>(surv_pred_lds + ncol * 256) + threadIdx.x;  // ... and at Rc[c * 256]
  for (int c = 0; c < ncol; ++c) {
    Ec[c * 256] = 0.0;
    Rc[c * 256] = 0u;
  }
  const double* lam = a.par + (int64_t)point * a.par_stride;
  const double* ab = lam + a.T;
  const SurvEta<MODE> eta_of(ab, a.n_ab, a.tile_group, tile);
  const int slot = tile * 64 + lane;
  const uint32_t j = (uint32_t)a.slot_j[slot];
  const uint32_t draw_lo = (uint32_t)(a.draw0 + point);
  const bool two = a.n_var == 2;
  int32_t* rep = a.rep ? a.rep + (int64_t)point * a.T * a.ld + slot : nullptr;
  int64_t idx = slot;
  double Ej = 0.0;
  int32_t Rj = 0;
  for (int t = 0; t < a.T; ++t, idx += a.ld) {
    const double e = a.e[idx];
    const unsigned byte = a.bins[idx];
    const double eta = eta_of(t, a.x0[idx], MODE == 2 ? a.x1[idx] : 0.0);
    const double mu = lam[t] * (e * surv_sigma(eta).sig);
    const int r = surv_pred_poisson(mu, surv_pred_uniform(a.seed_lo, a.seed_hi, j, (uint32_t)t, draw_lo));
    const int c0 = (int)(byte & 15u) * 256;
    Ec[c0] += mu;
    Rc[c0] += (uint32_t)r;
    if (two) {
      const int c1 = (ABD_SURV_PRED_BINS + (int)(byte >> 4)) * 256;
      Ec[c1] += mu;
      Rc[c1] += (uint32_t)r;
    }
    Ej += mu;
    Rj += r;
    if (rep) rep[(int64_t)t * a.ld] = r;
  }
  a.ej[(int64_t)point * a.ld + slot] = Ej;
  a.rj[(int64_t)point * a.ld + slot] = Rj;
  double* e_row = a.e_part + ((int64_t)point * a.ntile + tile) * ABD_SURV_PRED_COLS;
  uint32_t* r_row = a.r_part + ((int64_t)point * a.ntile + tile) * ABD_SURV_PRED_COLS;
  for (int c = 0; c < ncol; ++c) {
    const double E = wave_sum_uniform(Ec[c * 256]);
    const double R = wave_sum_uniform((double)Rc[c * 256]);  // integers below 2^53: exact in any order
    if (lane == 0) {
      e_row[c] = E;
      r_row[c] = (uint32_t)R;
    }
  }
}

// Grid (1, points), 256 threads: thread (g, c) = (tid / 16, tid % 16) adds column c of the tiles g, g + 16, ... in ascending
// order; thread c of the first 16 then adds the 16 partial sums in ascending order.  Columns at or past ncol are written as 0.
__global__ __launch_bounds__(256) void abd_survival_predictive_finalize(const double* e_part, const uint32_t* r_part, double* out_e,
                                                                        int64_t* out_r, int32_t ntile, int32_t ncol) {
  __shared__ double sm_e[256];
  __shared__ int64_t sm_r[256];
  const int tid = threadIdx.x, point = blockIdx.y;
  const int c = tid % ABD_SURV_PRED_COLS, g = tid / ABD_SURV_PRED_COLS;
  const int n = c < ncol && g < ntile ? (ntile - g + 15) / 16 : 0;
  const int64_t first = ((int64_t)point * ntile + g) * ABD_SURV_PRED_COLS + c;
  sm_e[tid] = surv_sum_strided(e_part + (n ? first : 0), n, 16 * ABD_SURV_PRED_COLS);
  int64_t r = 0;
  for (int i = 0; i < n; ++i) r += (int64_t)r_part[first + (int64_t)i * 16 * ABD_SURV_PRED_COLS];
  sm_r[tid] = r;
  __syncthreads();
  if (tid < ABD_SURV_PRED_COLS) {
    double E = 0.0;
    int64_t R = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      E += sm_e[q * ABD_SURV_PRED_COLS + tid];
      R += sm_r[q * ABD_SURV_PRED_COLS + tid];
    }
    out_e[(int64_t)point * ABD_SURV_PRED_COLS + tid] = E;
    out_r[(int64_t)point * ABD_SURV_PRED_COLS + tid] = R;
  }
}

// rows 0 .. n - 1 of ej, rj [n][ld] into acc_e, acc_r, acc_pos [ld] as draws n0 .. n0 + n - 1; draw 0 overwrites its column
__global__ __launch_bounds__(256) void abd_survival_predictive_fold(const double* ej, const int32_t* rj, double* acc_e, int64_t* acc_r,
                                                                    int64_t* acc_pos, int32_t ld, int32_t n, int64_t n0) {
  const int slot = blockIdx.x * 256 + threadIdx.x;
  if (slot >= ld) return;
  double E = n0 ? acc_e[slot] : 0.0;
  int64_t R = n0 ? acc_r[slot] : 0, P = n0 ? acc_pos[slot] : 0;
  for (int p = 0; p < n; ++p) {
    const int32_t r = rj[(int64_t)p * ld + slot];
    E += ej[(int64_t)p * ld + slot];
    R += r;
    P += r >= 1 ? 1 : 0;
  }
  acc_e[slot] = E;
  acc_r[slot] = R;
  acc_pos[slot] = P;
}

}  // namespace abdi
