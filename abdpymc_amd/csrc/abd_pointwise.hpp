// abd_pointwise.hpp -- the pointwise log-likelihood of the two observed Normals "it_s_lik", "it_n_lik" (abd.py:459-469):
// one value per OD reading at one chain slot's point, what pm.compute_log_likelihood records per draw, and the per-reading
// running statistics WAIC needs (abdpymc_amd/compare.py), kept on the device while the native sampler draws.
//
//   a_k  = titer response at the reading's (gap, ind)   (the arithmetic of abd_deterministics_kernel / abd_obs_kernel)
//   m_k  = d / (1 + exp(-b (x_k - a_k)))
//   ll_k = -1/2 ((y_k - m_k) / sigma)^2 - log sigma - 1/2 log 2 pi
//
// Readings are indexed in the context's sorted order (by individual, then gap): for a dense panel reading (g, j) is k = j G + g,
// the individual-major yxi panel; for observation lists the order of the uploaded lists.  A row holds the S readings, then N.
//
// Accumulators ([4][K_s + K_n] doubles per chain, columns as a row; rows M, S, mean, M2), updated by draw n >= 1, inv_n = 1 / n:
//   M   running max of ll                    S  = sum over draws of exp(ll - M), rescaled when M rises
//   mean, M2: Welford's running mean and sum of squared deviations
// Every reading belongs to exactly one lane and every chain has its own rows: a fixed-order read-modify-write, no atomics.
// Included by abd_eval.hip (after abd_eval_kernels.hpp: responses, add_bits, any_bits, the power tables).
#pragma once

#include "abd_obs.hpp"

// Everything a launch reads, and nothing else: a small argument block keeps the kernels' scalar registers for the packed words
struct PointwiseArgs {
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
  double* ll;             // [K_s + K_n] device row (S readings, then N); nullptr: not written
  double* acc;            // [4][K_s + K_n] accumulators of the chain; nullptr: not updated
  double rho_n, rho_s;
  // per antigen: init, perm, temp (N only), b log2(e), d, 1 / sigma, -log sigma - 1/2 log 2 pi
  double init_n, perm_n, temp_n, b2_n, d_n, inv_sig_n, lnorm_n;
  double init_s, perm_s, b2_s, d_s, inv_sig_s, lnorm_s;
  int64_t K_s, K_n;
  int64_t n_draw;         // draw number of the update, >= 1
  double inv_n;           // 1 / n_draw
  int32_t G, N, nt;
  int32_t bn, bs;         // observation lists: workgroups over the N list, then over the S list
};

// one reading's log-density: the residual as obs_term forms it (q = y - d s, s = 1 / (1 + e^(b (a - x))))
__device__ __forceinline__ double pointwise_ll(double a, double x, double y, double b2, double d, double inv_sig, double lnorm) {
  const double t = fmin(b2 * (a - x), 1021.0);
  const double s = rcp_newton(1.0 + exp2_reduced(t));
  const double z = fma(-d, s, y) * inv_sig;
  return fma(-0.5 * z, z, lnorm);
}

// draw n_draw of reading k into its accumulator column
__device__ __forceinline__ void pointwise_update(double* __restrict__ acc, int64_t stride, int64_t k, double ll, int64_t n_draw,
                                                 double inv_n) {
  double M, S, mean, M2;
  if (n_draw == 1) {
    M = ll;
    S = 1.0;
    mean = ll;
    M2 = 0.0;
  } else {
    M = acc[k];
    S = acc[stride + k];
    mean = acc[2 * stride + k];
    M2 = acc[3 * stride + k];
    // e^u for u <= 0 by the same 2^t polynomial as the curve (its constants are already in registers), clamped where
    // e^u is 0 anyway
    if (ll > M) {
      S = fma(S, exp2_reduced(fmax((M - ll) * 1.4426950408889634074, -1100.0)), 1.0);
      M = ll;
    } else {
      S += exp2_reduced(fmax((ll - M) * 1.4426950408889634074, -1100.0));
    }
    const double dlt = ll - mean;
    mean = fma(dlt, inv_n, mean);
    M2 = fma(dlt, ll - mean, M2);
  }
  acc[k] = M;
  acc[stride + k] = S;
  acc[2 * stride + k] = mean;
  acc[3 * stride + k] = M2;
}

// reading r (column of the S-then-N row) gets its value
__device__ __forceinline__ void pointwise_out(const PointwiseArgs& w, int64_t r, double ll) {
  if (w.ll) w.ll[r] = ll;
  if (w.acc) pointwise_update(w.acc, w.K_s + w.K_n, r, ll, w.n_draw, w.inv_n);
}

// Dense panels: one wave per individual, lanes over gaps (as abd_deterministics_kernel), both antigens of a cell at once;
// the cell's pair is read from the individual-major panel yxi, whose element (g, j) is reading j G + g.
template <typename R, int MT>
__global__ __launch_bounds__(ABD_BLOCK) void abd_pointwise_dense_kernel(const PointwiseArgs w) {
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
  // the curve constants live in vector registers: the scalar file holds the individual's packed words
  const double init_n = to_vgpr(w.init_n), perm_n = to_vgpr(w.perm_n), temp_n = to_vgpr(w.temp_n);
  const double b2_n = to_vgpr(w.b2_n), d_n = to_vgpr(w.d_n), is_n = to_vgpr(w.inv_sig_n), ln_n = to_vgpr(w.lnorm_n);
  const double init_s = to_vgpr(w.init_s), perm_s = to_vgpr(w.perm_s);
  const double b2_s = to_vgpr(w.b2_s), d_s = to_vgpr(w.d_s), is_s = to_vgpr(w.inv_sig_s), ln_s = to_vgpr(w.lnorm_s);
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
        pointwise_out(w, k, pointwise_ll(as, (double)cs.x, (double)cs.y, b2_s, d_s, is_s, ln_s));
        pointwise_out(w, w.K_s + k, pointwise_ll(an, (double)cn.x, (double)cn.y, b2_n, d_n, is_n, ln_n));
      }
    }
  }
}

// Observation lists: one lane per reading (as abd_obs_kernel); workgroups [0, bn) take the N list, [bn, bn + bs) the S list.
template <typename R, int MT>
__global__ __launch_bounds__(ABD_BLOCK) void abd_pointwise_obs_kernel(const PointwiseArgs w) {
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
    const double b2 = to_vgpr(w.b2_n), d = to_vgpr(w.d_n), is = to_vgpr(w.inv_sig_n), ln = to_vgpr(w.lnorm_n);
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
      pointwise_out(w, w.K_s + k, pointwise_ll(an, x, y, b2, d, is, ln));
    }
  } else {
    fill_pow_table(tab, w.rho_s, tstride, tid, ABD_BLOCK);
    fill_ones_table(tab_ones, tstride, tid, ABD_BLOCK);
    __syncthreads();
    const double init = to_vgpr(w.init_s), perm = to_vgpr(w.perm_s);
    const double b2 = to_vgpr(w.b2_s), d = to_vgpr(w.d_s), is = to_vgpr(w.inv_sig_s), ln = to_vgpr(w.lnorm_s);
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
      pointwise_out(w, k, pointwise_ll(as, x, y, b2, d, is, ln));
    }
  }
}
