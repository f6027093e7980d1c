// abd_predictive.hpp -- posterior predictive replicates of the two observed Normals "it_s_lik", "it_n_lik" (abd.py:459-469) at
// one chain slot's point, what pm.sample_posterior_predictive draws per recorded draw, and per-reading running statistics of
// a posterior predictive check (abdpymc_amd/predictive.py), kept on the device while the native sampler draws.
//
//   a_k     = titer response at the reading's (gap, ind)   (the arithmetic of abd_pointwise_*_kernel)
//   m_k     = d s,  s = 1 / (1 + 2^(b log2e (a_k - x_k)))  (the noise-free predictive mean, as pointwise_ll forms s)
//   y_rep_k = m_k + sigma z_k,  z_k ~ N(0, 1)
//
// The normal z_k comes from a counter-based stream that does not depend on the layout (dense or lists), the storage type,
// the launch shape, thinning or how chains are sharded over processes:
//   Philox4x32-10, key (seed_lo, seed_hi), counter (r, stream, (uint32)draw, 0x80000000 | antigen << 30 | (draw >> 32) & 0x3FFFFFFF)
//   r: the reading's index in the CALLER's order within its antigen (S = 0, N = 1); stream: the global chain id; draw: a
//   64-bit draw key (the native sampler: the iteration number).  The sweep's counters have c3 = 0: the streams are disjoint.
//   u1 = ((w0 >> 5) 2^26 + (w1 >> 6) + 0.5) 2^-53, u2 the same of w2, w3;  z = sqrt(-2 ln u1) cospi(2 u2)  (Box-Muller)
//
// Readings are indexed in the context's sorted order as in abd_pointwise.hpp (a row holds the S readings, then N).
// Accumulators ([3][K_s + K_n] doubles per chain; rows mean, M2, pit), updated by draw n >= 1, inv_n = 1 / n:
//   mean, M2: Welford's running mean of m_k and sum of squared deviations from it
//   pit: running mean of Phi((y_k - m_k) / sigma) = P(y_rep_k <= y_k | theta), Phi(t) = erfc(-t / sqrt 2) / 2 -- over the
//        draws the Rao-Blackwellised tail probability P(y_rep_k <= y_k | y); no random numbers
// Every reading belongs to exactly one lane and every chain has its own rows: a fixed-order read-modify-write, no atomics.
// Included by abd_eval.hip (after abd_pointwise.hpp: responses, add_bits, any_bits, the power tables, exp2_reduced, rcp_newton).
#pragma once

#include "abd_obs.hpp"

// Everything a launch reads, and nothing else (abd_pointwise.hpp: PointwiseArgs)
struct PredictiveArgs {
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
  const uint64_t* vw;     // [nt][N] packed vaccinations
  const uint64_t* iw;     // [nt][N] the chain slot's constrained infections
  const int8_t* waner;    // [N]
  const uint32_t* ord;    // [K_s + K_n] the caller's index of every reading within its antigen (the stream's counter r)
  double* yrep;           // [K_s + K_n] device row (S readings, then N); nullptr: not written
  double* mean;           // [K_s + K_n] device row of m_k; nullptr: not written
  double* acc;            // [3][K_s + K_n] accumulators of the chain; nullptr: not updated
  double rho_n, rho_s;
  // per antigen: init, perm, temp (N only), b log2(e), d, sigma, 1 / sigma
  double init_n, perm_n, temp_n, b2_n, d_n, sig_n, inv_sig_n;
  double init_s, perm_s, b2_s, d_s, sig_s, inv_sig_s;
  int64_t K_s, K_n;
  int64_t n_draw;         // draw number of the update, >= 1
  double inv_n;           // 1 / n_draw
  uint32_t seed_lo, seed_hi, stream, draw_lo;
  uint32_t c3_s, c3_n;    // fourth counter word of each antigen
  int32_t G, N, nt;
  int32_t bn, bs;         // observation lists: workgroups over the N list, then over the S list
};

// the standard normal of caller reading r (the stream above)
__device__ __forceinline__ double predictive_z(const PredictiveArgs& w, uint32_t r, uint32_t c3) {
  const Philox4 p = philox4x32_10(r, w.stream, w.draw_lo, c3, w.seed_lo, w.seed_hi);
  constexpr double kTwo53 = 1.0 / 9007199254740992.0;
  const double u1 = ((double)(((uint64_t)(p.w[0] >> 5) << 26) | (p.w[1] >> 6)) + 0.5) * kTwo53;
  const double u2 = ((double)(((uint64_t)(p.w[2] >> 5) << 26) | (p.w[3] >> 6)) + 0.5) * kTwo53;
  return sqrt(-2.0 * log(u1)) * cospi(2.0 * u2);
}

// reading r (column of the S-then-N row) of one antigen: the curve, the replicate and / or the accumulator update
__device__ __forceinline__ void predictive_out(const PredictiveArgs& w, int64_t r, uint32_t c3, double a, double x, double y,
                                               double b2, double d, double sig, double inv_sig) {
  const double t = fmin(b2 * (a - x), 1021.0);
  const double m = d * rcp_newton(1.0 + exp2_reduced(t));
  if (w.mean) w.mean[r] = m;
  if (w.yrep) w.yrep[r] = fma(sig, predictive_z(w, w.ord[r], c3), m);
  if (!w.acc) return;
  const int64_t stride = w.K_s + w.K_n;
  const double pit = 0.5 * erfc((m - y) * inv_sig * 0.70710678118654752440);
  double mean, M2, pm;
  if (w.n_draw == 1) {
    mean = m;
    M2 = 0.0;
    pm = pit;
  } else {
    mean = w.acc[r];
    M2 = w.acc[stride + r];
    pm = w.acc[2 * stride + r];
    const double dlt = m - mean;
    mean = fma(dlt, w.inv_n, mean);
    M2 = fma(dlt, m - mean, M2);
    pm = fma(pit - pm, w.inv_n, pm);
  }
  w.acc[r] = mean;
  w.acc[stride + r] = M2;
  w.acc[2 * stride + r] = pm;
}

// Dense panels: one wave per individual, lanes over gaps (as abd_pointwise_dense_kernel), both antigens of a cell at once
template <typename R, int MT>
__global__ __launch_bounds__(ABD_BLOCK) void abd_predictive_dense_kernel(const PredictiveArgs w) {
  extern __shared__ __align__(16) unsigned char smem[];
  double2_t* tabs = reinterpret_cast<double2_t*>(smem);
  const int G = w.G, N = w.N, nt = w.nt, tstride = G + 1;
  double2_t* tab_ones = tabs + 2 * tstride;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  fill_pow_table(tabs, w.rho_n, tstride, tid, ABD_BLOCK);
  fill_pow_table(tabs + tstride, w.rho_s, tstride, tid, ABD_BLOCK);
  fill_ones_table(tab_ones, tstride, tid, ABD_BLOCK);
  __syncthreads();
  const YX<R>* yxn = reinterpret_cast<const YX<R>*>(w.y_n);
  const YX<R>* yxs = reinterpret_cast<const YX<R>*>(w.y_s);
  const double init_n = to_vgpr(w.init_n), perm_n = to_vgpr(w.perm_n), temp_n = to_vgpr(w.temp_n);
  const double b2_n = to_vgpr(w.b2_n), d_n = to_vgpr(w.d_n), sg_n = to_vgpr(w.sig_n), is_n = to_vgpr(w.inv_sig_n);
  const double init_s = to_vgpr(w.init_s), perm_s = to_vgpr(w.perm_s);
  const double b2_s = to_vgpr(w.b2_s), d_s = to_vgpr(w.d_s), sg_s = to_vgpr(w.sig_s), is_s = to_vgpr(w.inv_sig_s);
  const int waves_total = gridDim.x * ABD_WAVES_PER_BLOCK;
  for (int j = blockIdx.x * ABD_WAVES_PER_BLOCK + wave; j < N; j += waves_total) {
    uint64_t V[MT], I[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      V[t] = I[t] = 0;
      if (t < nt) {
        V[t] = uniform_word(w.vw, (int64_t)t * N + j);
        I[t] = uniform_word(w.iw, (int64_t)t * N + j);
      }
    }
    const bool wj = __builtin_amdgcn_readfirstlane((int)w.waner[j]) != 0;
    const double2_t* ts = wj ? tabs + tstride : tab_ones;
    for (int t = 0; t < nt; ++t) {
      const int g = t * 64 + lane;
      if (g < G) {
        const Resp rs = responses<MT>(g, t + 1, I, V, tabs, ts);
        const int64_t k = (int64_t)j * G + g;
        const double an = init_n + (rs.cum_i ? perm_n : 0.0) + temp_n * rs.un;
        const double as = init_s + (rs.cum_iv ? perm_s : 0.0) + rs.us;
        const YX<R> cn = yxn[k], cs = yxs[k];
        predictive_out(w, k, w.c3_s, as, (double)cs.x, (double)cs.y, b2_s, d_s, sg_s, is_s);
        predictive_out(w, w.K_s + k, w.c3_n, an, (double)cn.x, (double)cn.y, b2_n, d_n, sg_n, is_n);
      }
    }
  }
}

// Observation lists: one lane per reading (as abd_pointwise_obs_kernel); workgroups [0, bn) take the N list, [bn, bn + bs) the S list.
template <typename R, int MT>
__global__ __launch_bounds__(ABD_BLOCK) void abd_predictive_obs_kernel(const PredictiveArgs w) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int N = w.N, nt = w.nt, tstride = w.G + 1;
  double2_t* tab = reinterpret_cast<double2_t*>(smem);
  double2_t* tab_ones = tab + tstride;
  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  if (b < w.bn) {
    fill_pow_table(tab, w.rho_n, tstride, tid, ABD_BLOCK);
    __syncthreads();
    const double init = to_vgpr(w.init_n), perm = to_vgpr(w.perm_n), temp = to_vgpr(w.temp_n);
    const double b2 = to_vgpr(w.b2_n), d = to_vgpr(w.d_n), sg = to_vgpr(w.sig_n), is = to_vgpr(w.inv_sig_n);
    for (int64_t k = (int64_t)b * ABD_BLOCK + tid; k < w.K_n; k += (int64_t)w.bn * ABD_BLOCK) {
      const int j = w.j_n[k];
      const int g = w.g_n[k];
      const double y = ld<R>(w.y_n, k), x = ld<R>(w.x_n, k);
      double un = 0.0, dn = 0.0;
      bool cum = false;
#pragma unroll
      for (int t = 0; t < MT; ++t)
        if (t < nt) {
          const uint64_t I = w.iw[(int64_t)t * N + j];
          cum |= any_bits(I, t, g);
          add_bits(I, t, g, tab, un, dn);
        }
      const double an = init + (cum ? perm : 0.0) + temp * un;
      predictive_out(w, w.K_s + k, w.c3_n, an, x, y, b2, d, sg, is);
    }
  } else {
    fill_pow_table(tab, w.rho_s, tstride, tid, ABD_BLOCK);
    fill_ones_table(tab_ones, tstride, tid, ABD_BLOCK);
    __syncthreads();
    const double init = to_vgpr(w.init_s), perm = to_vgpr(w.perm_s);
    const double b2 = to_vgpr(w.b2_s), d = to_vgpr(w.d_s), sg = to_vgpr(w.sig_s), is = to_vgpr(w.inv_sig_s);
    const int b0 = b - w.bn;
    for (int64_t k = (int64_t)b0 * ABD_BLOCK + tid; k < w.K_s; k += (int64_t)w.bs * ABD_BLOCK) {
      const int j = w.j_s[k];
      const int g = w.g_s[k];
      const double y = ld<R>(w.y_s, k), x = ld<R>(w.x_s, k);
      const double2_t* ts = w.waner[j] != 0 ? tab : tab_ones;
      double us = 0.0, ds = 0.0;
      bool cum = false;
#pragma unroll
      for (int t = 0; t < MT; ++t)
        if (t < nt) {
          const uint64_t I = w.iw[(int64_t)t * N + j], V = w.vw[(int64_t)t * N + j];
          cum |= any_bits(I | V, t, g);
          add_bits(I, t, g, ts, us, ds);  // an infection and a dose in the same gap both count (Q5)
          add_bits(V, t, g, ts, us, ds);
        }
      const double as = init + (cum ? perm : 0.0) + us;
      predictive_out(w, k, w.c3_s, as, x, y, b2, d, sg, is);
    }
  }
}
