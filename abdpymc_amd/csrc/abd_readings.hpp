// abd_readings.hpp -- per-reading outputs of the two observed Normals "it_s_lik", "it_n_lik" (abd.py:459-469) at one chain
// slot's point, kept on the device while the native sampler draws.  Two walkers over the OD readings (dense panels, observation
// lists) work out each reading's titer response; an op turns it into what is written:
//
//   a_k = titer response at the reading's (gap, ind)   (the arithmetic of abd_deterministics_kernel / abd_obs_kernel)
//   m_k = d s,  s = 1 / (1 + 2^(b log2e (a_k - x_k)))
//
// LogLik: the pointwise log-likelihood, what pm.compute_log_likelihood records per draw, and the per-reading running
// statistics WAIC needs (abdpymc_amd/compare.py):
//   ll_k = -1/2 ((y_k - m_k) / sigma)^2 - log sigma - 1/2 log 2 pi
//   accumulators [4][K_s + K_n] per chain, rows M, S, mean, M2:
//   M   running max of ll                    S  = sum over draws of exp(ll - M), rescaled when M rises
//   mean, M2: Welford's running mean and sum of squared deviations
//
// Predictive: posterior predictive replicates, what pm.sample_posterior_predictive draws per recorded draw, and per-reading
// running statistics of a posterior predictive check (abdpymc_amd/predictive.py):
//   y_rep_k = m_k + sigma z_k,  z_k ~ N(0, 1)
//   The normal z_k comes from a counter-based stream that does not depend on the layout (dense or lists), the storage type,
//   the launch shape, thinning or how chains are sharded over processes:
//   Philox4x32-10, key (seed_lo, seed_hi), counter (r, stream, (uint32)draw, 0x80000000 | antigen << 30 | (draw >> 32) & 0x3FFFFFFF)
//   r: the reading's index in the CALLER's order within its antigen (S = 0, N = 1); stream: the global chain id; draw: a
//   64-bit draw key (the native sampler: the iteration number).  The sweep's counters have c3 = 0: the streams are disjoint.
//   u1 = ((w0 >> 5) 2^26 + (w1 >> 6) + 0.5) 2^-53, u2 the same of w2, w3;  z = sqrt(-2 ln u1) cospi(2 u2)  (Box-Muller)
//   accumulators [3][K_s + K_n] per chain, rows mean, M2, pit:
//   mean, M2: Welford's running mean of m_k and sum of squared deviations from it
//   pit: running mean of Phi((y_k - m_k) / sigma) = P(y_rep_k <= y_k | theta), Phi(t) = erfc(-t / sqrt 2) / 2 -- over the
//        draws the Rao-Blackwellised tail probability P(y_rep_k <= y_k | y); no random numbers
//
// Accumulators are updated by draw n >= 1 with inv_n = 1 / n.  Readings are indexed in the context's sorted order (by
// individual, then gap): for a dense panel reading (g, j) is k = j G + g, the individual-major yxi panel; for observation lists
// the order of the uploaded lists.  A row holds the S readings, then N.  Every reading belongs to exactly one lane and every
// chain has its own rows: a fixed-order read-modify-write, no atomics.
// Included by abd_eval.hip (after abd_eval_kernels.hpp: responses, the power tables, exp2_reduced, rcp_newton); the dense
// walker shares its prologue and its individual's loads with the other cell kernels (abd_cells.hpp).
#pragma once

#include "abd_cells.hpp"
#include "abd_obs.hpp"

enum : int { kAgS = 0, kAgN = 1 };  // antigen index of the per-antigen constants (and of the predictive stream's counter)

// What both walkers read.  A launch's argument block is this and its op's fields, nothing else: a small block keeps the
// kernels' scalar registers for the packed words.  The field order decides how the kernels load the block into scalar
// registers, and with it their SGPR spills: this order spills no more than two blocks of their own did, in any instantiation
// (tools/resource_usage.py).
struct Readings {
  // the readings in sorted order: dense -- y_* the individual-major pair panels yxi (YX<R>), x_* unused; lists -- od,
  // log dilution, gap, individual of every reading
  const void* y_n;
  const void* x_n;
  const void* y_s;
  const void* x_s;
  const uint16_t* g_n;
  const uint16_t* g_s;
  const int32_t* j_n;
  const int32_t* j_s;
  // per antigen (kAgS, kAgN): rho, init, perm, b log2(e), d; temp (N only)
  double rho[2], init[2], perm[2], b2[2], d[2];
  double temp_n;
  const uint64_t* vw;     // [nt][N] packed vaccinations
  const uint64_t* iw;     // [nt][N] the chain slot's constrained infections
  const int8_t* waner;    // [N]
  int64_t K_s, K_n;
  int32_t G, N, nt;
  int32_t bn, bs;         // observation lists: workgroups over the N list, then over the S list
};

template <typename Op>
struct ReadingArgs {
  Readings rd;
  Op op;
};

// ll_k of one reading at titer response a, log dilution x, od y -- the ONE place it is written (LogLik below; the
// per-individual sums of abd_individual.hpp): the residual as obs_term forms it (q = y - d s)
__device__ __forceinline__ double reading_loglik(double b2, double d, double inv_sig, double lnorm, double a, double x, double y) {
  const double t = fmin(b2 * (a - x), 1021.0);
  const double s = rcp_newton(1.0 + exp2_reduced(t));
  const double z = fma(-d, s, y) * inv_sig;
  return fma(-0.5 * z, z, lnorm);
}

// Draw n_draw's value v into column r of a chain's accumulators acc [4][kt] (rows M, S, mean, M2): the one lane that owns
// the column reads, updates and writes it
__device__ __forceinline__ void waic_update(double* acc, int64_t r, int64_t kt, double v, int64_t n_draw, double inv_n) {
  double M, S, mean, M2;
  if (n_draw == 1) {
    M = v;
    S = 1.0;
    mean = v;
    M2 = 0.0;
  } else {
    M = acc[r];
    S = acc[kt + r];
    mean = acc[2 * kt + r];
    M2 = acc[3 * kt + r];
    // e^u for u <= 0 by the same 2^t polynomial as the curve (its constants are already in registers), clamped where
    // e^u is 0 anyway
    if (v > M) {
      S = fma(S, exp2_reduced(fmax((M - v) * 1.4426950408889634074, -1100.0)), 1.0);
      M = v;
    } else {
      S += exp2_reduced(fmax((v - M) * 1.4426950408889634074, -1100.0));
    }
    const double dlt = v - mean;
    mean = fma(dlt, inv_n, mean);
    M2 = fma(dlt, v - mean, M2);
  }
  acc[r] = M;
  acc[kt + r] = S;
  acc[2 * kt + r] = mean;
  acc[3 * kt + r] = M2;
}

// The pointwise log-likelihood: the row and / or the draw's update of the WAIC accumulators
struct LogLik {
  double* ll;             // [K_s + K_n] device row; nullptr: not written
  double* acc;            // [4][K_s + K_n] accumulators of the chain; nullptr: not updated
  int64_t n_draw;         // draw number of the update, >= 1
  double inv_n;           // 1 / n_draw
  double inv_sig[2], lnorm[2];  // per antigen: 1 / sigma, -log sigma - 1/2 log 2 pi
  // one antigen's constants in vector registers (the scalar file holds the individual's packed words)
  struct Side {
    double b2, d, inv_sig, lnorm;
  };
  __device__ __forceinline__ Side side(const Readings& w, int ag) const {
    return {to_vgpr(w.b2[ag]), to_vgpr(w.d[ag]), to_vgpr(inv_sig[ag]), to_vgpr(lnorm[ag])};
  }
  // reading r (column of the S-then-N row of kt readings)
  __device__ __forceinline__ void operator()(const Side& c, int64_t r, int64_t kt, double a, double x, double y) const {
    const double v = reading_loglik(c.b2, c.d, c.inv_sig, c.lnorm, a, x, y);
    if (ll) ll[r] = v;
    if (acc) waic_update(acc, r, kt, v, n_draw, inv_n);
  }
};

// The posterior predictive: the replicate and mean rows and / or the draw's update of the check accumulators
struct Predictive {
  const uint32_t* ord;    // [K_s + K_n] the caller's index of every reading within its antigen (the stream's counter r)
  double* yrep;           // [K_s + K_n] device row; nullptr: not written
  double* mean;           // [K_s + K_n] device row of m_k; nullptr: not written
  double* acc;            // [3][K_s + K_n] accumulators of the chain; nullptr: not updated
  int64_t n_draw;         // draw number of the update, >= 1
  double inv_n;           // 1 / n_draw
  double sig[2], inv_sig[2];  // per antigen: sigma, 1 / sigma
  uint32_t seed_lo, seed_hi, stream, draw_lo;
  uint32_t c3[2];         // per antigen: the fourth counter word
  struct Side {
    double b2, d, sig, inv_sig;
    uint32_t c3;
  };
  __device__ __forceinline__ Side side(const Readings& w, int ag) const {
    return {to_vgpr(w.b2[ag]), to_vgpr(w.d[ag]), to_vgpr(sig[ag]), to_vgpr(inv_sig[ag]), c3[ag]};
  }
  // the standard normal of caller reading r (the stream above)
  __device__ __forceinline__ double z(uint32_t r, uint32_t c3w) const {
    const Philox4 p = philox4x32_10(r, stream, draw_lo, c3w, seed_lo, seed_hi);
    constexpr double kTwo53 = 1.0 / 9007199254740992.0;
    const double u1 = ((double)(((uint64_t)(p.w[0] >> 5) << 26) | (p.w[1] >> 6)) + 0.5) * kTwo53;
    const double u2 = ((double)(((uint64_t)(p.w[2] >> 5) << 26) | (p.w[3] >> 6)) + 0.5) * kTwo53;
    return sqrt(-2.0 * log(u1)) * cospi(2.0 * u2);
  }
  // reading r (column of the S-then-N row of kt readings): the curve, the replicate and / or the accumulator update
  __device__ __forceinline__ void operator()(const Side& c, int64_t r, int64_t kt, double a, double x, double y) const {
    const double t = fmin(c.b2 * (a - x), 1021.0);
    const double m = c.d * rcp_newton(1.0 + exp2_reduced(t));
    if (mean) mean[r] = m;
    if (yrep) yrep[r] = fma(c.sig, z(ord[r], c.c3), m);
    if (!acc) return;
    const double pit = 0.5 * erfc((m - y) * c.inv_sig * 0.70710678118654752440);
    double mu, M2, pm;
    if (n_draw == 1) {
      mu = m;
      M2 = 0.0;
      pm = pit;
    } else {
      mu = acc[r];
      M2 = acc[kt + r];
      pm = acc[2 * kt + r];
      const double dlt = m - mu;
      mu = fma(dlt, inv_n, mu);
      M2 = fma(dlt, m - mu, M2);
      pm = fma(pit - pm, inv_n, pm);
    }
    acc[r] = mu;
    acc[kt + r] = M2;
    acc[2 * kt + r] = pm;
  }
};

// Dense panels: one wave per individual, lanes over gaps (as abd_deterministics_kernel), both antigens of a cell at once;
// the cell's pair is read from the individual-major panel yxi, whose element (g, j) is reading j G + g.
template <typename Op, typename R, int MT>
__global__ __launch_bounds__(ABD_BLOCK) void abd_readings_dense_kernel(const ReadingArgs<Op> a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const Readings& w = a.rd;
  const int G = w.G, N = w.N, nt = w.nt;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const CellTables tabs = cell_tables(smem, w.rho[kAgN], w.rho[kAgS], G, tid);
  const YX<R>* yxn = reinterpret_cast<const YX<R>*>(w.y_n);
  const YX<R>* yxs = reinterpret_cast<const YX<R>*>(w.y_s);
  // the curve constants live in vector registers: the scalar file holds the individual's packed words.  That is why the two
  // titer lines below are cell_titers' (abd_cells.hpp) written out on the VGPR copies and not a call of it
  const double init_n = to_vgpr(w.init[kAgN]), perm_n = to_vgpr(w.perm[kAgN]), temp_n = to_vgpr(w.temp_n);
  const typename Op::Side on = a.op.side(w, kAgN);
  const double init_s = to_vgpr(w.init[kAgS]), perm_s = to_vgpr(w.perm[kAgS]);
  const typename Op::Side os = a.op.side(w, kAgS);
  const int waves_total = gridDim.x * ABD_WAVES_PER_BLOCK;
  for (int j = blockIdx.x * ABD_WAVES_PER_BLOCK + wave; j < N; j += waves_total) {
    uint64_t V[MT], I[MT];
    const double2_t* ts = load_individual<MT>(w.vw, w.iw, w.waner, N, nt, j, tabs, V, I);
    for (int t = 0; t < nt; ++t) {
      const int g = t * 64 + lane;
      if (g < G) {
        const Resp rs = responses<MT>(g, t + 1, I, V, tabs.tab_n, ts);
        const int64_t k = (int64_t)j * G + g;
        const double an = init_n + (rs.cum_i ? perm_n : 0.0) + temp_n * rs.un;
        const double as = init_s + (rs.cum_iv ? perm_s : 0.0) + rs.us;
        const YX<R> cn = yxn[k], cs = yxs[k];
        a.op(os, k, w.K_s + w.K_n, as, (double)cs.x, (double)cs.y);
        a.op(on, w.K_s + k, w.K_s + w.K_n, an, (double)cn.x, (double)cn.y);
      }
    }
  }
}

// Response sums of observation-list reading (gap g, individual j): the exposures at or before g and whether there is one
struct ListSum {
  double u;
  bool cum;
};
// N: the individual's infections
template <int MT>
__device__ __forceinline__ ListSum list_sum_n(const Readings& w, int g, int j, const double2_t* tab) {
  double u = 0.0, d = 0.0;
  bool cum = false;
#pragma unroll
  for (int t = 0; t < MT; ++t)
    if (t < w.nt) {
      const uint64_t I = w.iw[(int64_t)t * w.N + j];
      cum |= any_bits(I, t, g);
      add_bits(I, t, g, tab, u, d);
    }
  return {u, cum};
}
// S: infections, then doses, on the individual's table (waning or not)
template <int MT>
__device__ __forceinline__ ListSum list_sum_s(const Readings& w, int g, int j, const double2_t* ts) {
  double u = 0.0, d = 0.0;
  bool cum = false;
#pragma unroll
  for (int t = 0; t < MT; ++t)
    if (t < w.nt) {
      const uint64_t I = w.iw[(int64_t)t * w.N + j], V = w.vw[(int64_t)t * w.N + j];
      cum |= any_bits(I | V, t, g);
      add_bits(I, t, g, ts, u, d);  // an infection and a dose in the same gap both count (Q5)
      add_bits(V, t, g, ts, u, d);
    }
  return {u, cum};
}

// Observation lists: one lane per reading (as abd_obs_kernel); workgroups [0, bn) take the N list, [bn, bn + bs) the S list.
template <typename Op, typename R, int MT>
__global__ __launch_bounds__(ABD_BLOCK) void abd_readings_lists_kernel(const ReadingArgs<Op> a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const Readings& w = a.rd;
  const int tstride = w.G + 1;
  double2_t* tab = reinterpret_cast<double2_t*>(smem);
  double2_t* tab_ones = tab + tstride;
  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  if (b < w.bn) {
    fill_pow_table(tab, w.rho[kAgN], tstride, tid, ABD_BLOCK);
    __syncthreads();
    const double init = to_vgpr(w.init[kAgN]), perm = to_vgpr(w.perm[kAgN]), temp = to_vgpr(w.temp_n);
    const typename Op::Side c = a.op.side(w, kAgN);
    for (int64_t k = (int64_t)b * ABD_BLOCK + tid; k < w.K_n; k += (int64_t)w.bn * ABD_BLOCK) {
      const int j = w.j_n[k];
      const int g = w.g_n[k];
      const double y = ld<R>(w.y_n, k), x = ld<R>(w.x_n, k);
      const ListSum r = list_sum_n<MT>(w, g, j, tab);
      a.op(c, w.K_s + k, w.K_s + w.K_n, init + (r.cum ? perm : 0.0) + temp * r.u, x, y);
    }
  } else {
    fill_pow_table(tab, w.rho[kAgS], tstride, tid, ABD_BLOCK);
    fill_ones_table(tab_ones, tstride, tid, ABD_BLOCK);
    __syncthreads();
    const double init = to_vgpr(w.init[kAgS]), perm = to_vgpr(w.perm[kAgS]);
    const typename Op::Side c = a.op.side(w, kAgS);
    const int b0 = b - w.bn;
    for (int64_t k = (int64_t)b0 * ABD_BLOCK + tid; k < w.K_s; k += (int64_t)w.bs * ABD_BLOCK) {
      const int j = w.j_s[k];
      const int g = w.g_s[k];
      const double y = ld<R>(w.y_s, k), x = ld<R>(w.x_s, k);
      const ListSum r = list_sum_s<MT>(w, g, j, w.waner[j] != 0 ? tab : tab_ones);
      a.op(c, k, w.K_s + w.K_n, init + (r.cum ? perm : 0.0) + r.u, x, y);
    }
  }
}
