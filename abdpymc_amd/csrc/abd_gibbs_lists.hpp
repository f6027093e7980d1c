// abd_gibbs_lists.hpp -- the binary Gibbs-Metropolis sweep on OBSERVATION LISTS (abd_gibbs.hpp: what the sweep is, why one
// individual's proposals can run on their own, the random stream and everything the two sweep kernels share).
//
// Wave = individual, one proposal at a time in the individual's random order, LANES = the individual's OBSERVATIONS: every
// proposal constrains the flipped row on the scalar unit, evaluates one response and one logistic term per lane, and pays a
// wave-wide sum.  The packed rows live in scalar registers: with one 64-bit word per row (<= 64 gaps; the reference's own
// cohorts have 26 and 31) they fit, with 4 or 8 words they spill (profiles/r04).  The same mapping on dense panels (lanes =
// the 64 gaps of a round, per-round early rejection) took 3.9 ms per sweep at config 3 against the lane-per-proposal kernel's
// 1.67 ms (abd_gibbs_dense.hpp) and was dropped.
#pragma once

#include "abd_gibbs.hpp"

// per-wave LDS of abd_gibbs_kernel: sort keys u32[G+1] + order u16[G+1] + transit u8[G+1] + log u f64[G+1]
__host__ __device__ constexpr size_t abd_gibbs_wave_lds(int G) {
  const size_t n = (size_t)G + 1;
  return abd_gibbs_pad16(4 * n) + abd_gibbs_pad16(2 * n) + abd_gibbs_pad16(n) + abd_gibbs_pad16(8 * n);
}
// LDS of a workgroup: [2][G+1] power tables of the block's chain, [G+1] ones, then the waves' regions
__host__ __device__ constexpr size_t abd_gibbs_lds(int G) {
  return (size_t)3 * (G + 1) * sizeof(double2_t) + (size_t)ABD_WAVES_PER_BLOCK * abd_gibbs_wave_lds(G);
}

// This lane's share of -1/2 sum (q / sigma)^2 over the individual's observations for the given masks (terms
// that do not depend on the discrete state are left out: they cancel in every difference).
// The individual's observations of BOTH antigens form one combined list (N first, then S), 64 per
// pass, one per lane.  The first pass -- the only one for the reference's cohorts (~12 + 12 observations per
// individual) -- is kept in registers for the whole sweep together with the lane's antigen-specific constants, so
// a proposal costs one response + one logistic term per lane and no memory traffic.
template <typename R>
struct ObsLane {
  int g;              // gap of the observation
  double y, x;        // od, log dilution
  double guard;       // 1 for a real observation, 0 for a padding lane
  bool is_s;          // S antigen (else N)
  double init, perm, temp, b, d, nh_is2;  // the antigen's constants: a = init + [exposed] perm + temp u ; -1/2 sigma^-2
};

template <typename R>
__device__ __forceinline__ ObsLane<R> load_obs_lane(const EvalArgs& a, const ChainPar& p, int j, int idx, double is2_n,
                                                    double is2_s) {
  ObsLane<R> o;
  const int kn0 = a.ptr_n[j], cnt_n = a.ptr_n[j + 1] - kn0;
  const int ks0 = a.ptr_s[j], cnt_s = a.ptr_s[j + 1] - ks0;
  o.is_s = idx >= cnt_n;
  const bool valid = idx < cnt_n + cnt_s;
  o.guard = valid ? 1.0 : 0.0;
  o.g = 0;
  o.y = o.x = 0.0;
  if (valid) {
    if (o.is_s) {
      const int k = ks0 + idx - cnt_n;
      o.g = a.g_s[k];
      o.y = ld<R>(a.y_s, k);
      o.x = ld<R>(a.x_s, k);
    } else {
      const int k = kn0 + idx;
      o.g = a.g_n[k];
      o.y = ld<R>(a.y_n, k);
      o.x = ld<R>(a.x_n, k);
    }
  }
  o.init = o.is_s ? p.init_s : p.init_n;
  o.perm = o.is_s ? p.perm_s : p.perm_n;
  o.temp = o.is_s ? 1.0 : p.temp_n;  // unit S boosts (Q1)
  o.b = o.is_s ? p.b_s : p.b_n;
  o.d = o.is_s ? p.d_s : p.d_n;
  o.nh_is2 = -0.5 * (o.is_s ? is2_s : is2_n);
  return o;
}

template <typename R, int MT>
__device__ __forceinline__ double obs_lane_term(const EvalArgs& a, const ObsLane<R>& o, const uint64_t I[MT],
                                                const uint64_t V[MT], const double2_t* tab_n, const double2_t* tab_s) {
  const double2_t* tb = o.is_s ? tab_s : tab_n;
  double u = 0.0;
  bool cum = false;
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    if (t < a.nt) {
      const int rel = o.g - t * 64;  // bits <= rel of word t are exposures at or before the observation's gap
      const uint64_t le = rel >= 63 ? ~0ull : (rel < 0 ? 0ull : ((2ull << rel) - 1ull));
      cum |= ((o.is_s ? (I[t] | V[t]) : I[t]) & le) != 0;
      uint64_t m = I[t];
      while (m) {  // wave-uniform loops over the set bits; table entry 0 is "in the future" = 0
        const int bpos = __builtin_ctzll(m);
        m &= m - 1;
        u += tb[max(rel - bpos + 1, 0)].x;
      }
      m = V[t];
      while (m) {
        const int bpos = __builtin_ctzll(m);
        m &= m - 1;
        const double v = tb[max(rel - bpos + 1, 0)].x;
        u += o.is_s ? v : 0.0;  // doses boost S only
      }
    }
  }
  const double resp = o.init + (cum ? o.perm : 0.0) + o.temp * u;
  double q2 = 0.0, d0 = 0.0, d1 = 0.0, d2 = 0.0, d3 = 0.0;
  obs_term<false>(resp, o.x, o.y, o.b, o.d, o.guard, q2, d0, d1, d2, d3);
  return o.nh_is2 * q2;
}

template <typename R, int MT>
__device__ __forceinline__ double sparse_terms(const EvalArgs& a, const ChainPar& p, int j, int lane, const uint64_t I[MT],
                                               const uint64_t V[MT], const double2_t* tab_n, const double2_t* tab_s,
                                               double is2_n, double is2_s, const ObsLane<R>& first, int n_obs) {
  double acc = obs_lane_term<R, MT>(a, first, I, V, tab_n, tab_s);
  for (int base = 64; base < n_obs; base += 64) {  // individuals with more than 64 observations: the rest from memory
    const ObsLane<R> o = load_obs_lane<R>(a, p, j, base + lane, is2_n, is2_s);
    acc += obs_lane_term<R, MT>(a, o, I, V, tab_n, tab_s);
  }
  return acc;
}

// word `lane` of a wave-uniform row (lanes >= MT: 0)
template <int MT>
__device__ __forceinline__ uint64_t gibbs_lane_word(const uint64_t (&w)[MT], int lane) {
  uint64_t v = 0;
#pragma unroll
  for (int t = 0; t < MT; ++t) v = lane == t ? w[t] : v;
  return v;
}

// LOG: the decision log of abd_gibbs_sweep_log (ga.log: one GibbsRecord per proposal, abd_types.hpp).  The shipped sweep is LOG = false.
template <typename R, int MT, bool LOG = false>
__global__ __launch_bounds__(ABD_BLOCK) void abd_gibbs_kernel(const GibbsArgs ga) {
  extern __shared__ __align__(16) unsigned char smem[];  // abd_gibbs_lds(G)
  const EvalArgs& a = ga.e;
  const int G = a.G, N = a.N, nt0 = a.nt;
  const int tstride = G + 1;
  double2_t* tabs = reinterpret_cast<double2_t*>(smem);
  double2_t* tab_ones = tabs + 2 * tstride;
  const int tid = threadIdx.x, lane0 = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const size_t nd = (size_t)G + 1;
  unsigned char* wbase = reinterpret_cast<unsigned char*>(tab_ones + tstride) + (size_t)wave * abd_gibbs_wave_lds(G);
  uint32_t* keyv = reinterpret_cast<uint32_t*>(wbase);                                    // [G+1] sort key by dim
  uint16_t* order = reinterpret_cast<uint16_t*>(wbase + abd_gibbs_pad16(4 * nd));         // [G+1] dim by rank
  unsigned char* transit = wbase + abd_gibbs_pad16(4 * nd) + abd_gibbs_pad16(2 * nd);     // [G+1] 1 = propose, by dim
  double* logu = reinterpret_cast<double*>(transit + abd_gibbs_pad16(nd));                // [G+1] log of the acceptance uniform, by dim

  const int c = blockIdx.y;  // one chain per block row
  const ChainPar& p = a.ch[c];
  fill_pow_table(tabs, p.rho_n, tstride, tid, ABD_BLOCK);
  fill_pow_table(tabs + tstride, p.rho_s, tstride, tid, ABD_BLOCK);
  fill_ones_table(tab_ones, tstride, tid, ABD_BLOCK);
  __syncthreads();
  const double theta0 = ga.theta0[c], theta7 = ga.theta7[c], is2_n = ga.is2_n[c], is2_s = ga.is2_s[c];
  const uint32_t k0_0 = gibbs_key_lo(ga), k1_0 = ga.seed_hi;
  const uint32_t cs = ga.stream[c];
  const GibbsSlot slot = gibbs_slot(p);
  long long d_n1 = 0, d_m1 = 0;  // changes of sum(i_raw), sum(ab_s_waner) over this wave's individuals
  const int n_dims = G + 1;  // dims 0..G-1: i_raw[g, j]; dim G: ab_s_waner[j]
  unsigned long long n_acc = 0, n_prop = 0;

  const int waves_total = gridDim.x * ABD_WAVES_PER_BLOCK;
  for (int j = blockIdx.x * ABD_WAVES_PER_BLOCK + wave; j < N; j += waves_total) {
    int lane = lane0;
    asm volatile("" : "+v"(lane));
    const int nt = gibbs_opaque_uniform(nt0);
    const uint32_t k0 = (uint32_t)gibbs_opaque_uniform((int)k0_0), k1 = (uint32_t)gibbs_opaque_uniform((int)k1_0);
    // ---- this individual's discrete state ----
    uint64_t V[MT], P[MT], Rw[MT], I[MT];
    gibbs_load_rows<MT>(a, slot, j, nt, V, P, Rw);
    bool wj = __builtin_amdgcn_readfirstlane((int)slot.waner[j]) != 0;
    constrain_masks<MT>(Rw, P, a, I);
    const int pc0 = gibbs_state_counts<MT>(Rw, wj);

    // ---- random order and transit flags of this individual's dims ----
    for (int d = lane; d < n_dims; d += 64) {
      const GibbsDraw r = gibbs_draw(ga, d, j, cs, k0, k1);
      keyv[d] = r.key;
      transit[d] = r.proposed ? 1 : 0;
      logu[d] = log(((double)r.accept + 0.5) * (1.0 / 4294967296.0));  // one log per lane and dim, not one per proposal
    }
    __builtin_amdgcn_wave_barrier();
    for (int d = lane; d < n_dims; d += 64) {  // rank = number of dims with a smaller key; order[rank] = dim
      const uint32_t mine = keyv[d];
      int rank = 0;
      for (int e = 0; e < n_dims; ++e) rank += keyv[e] < mine ? 1 : 0;
      order[rank] = (uint16_t)d;
    }
    __builtin_amdgcn_wave_barrier();

    // this lane's observation of the first pass, the individual's observation count, and the lane's terms at the current state
    const ObsLane<R> first = load_obs_lane<R>(a, p, j, lane, is2_n, is2_s);
    const int n_obs = __builtin_amdgcn_readfirstlane((a.ptr_n[j + 1] - a.ptr_n[j]) + (a.ptr_s[j + 1] - a.ptr_s[j]));
    double cur = sparse_terms<R, MT>(a, p, j, lane, I, V, tabs, wj ? tabs + tstride : tab_ones, is2_n, is2_s, first, n_obs);

    // ---- the sweep ----
    GibbsRecord* const lrec = LOG ? gibbs_log_rows(ga, c, j) : nullptr;
    int n_rec = 0;
    for (int k = 0; k < n_dims; ++k) {
      const int d = __builtin_amdgcn_readfirstlane((int)order[k]);
      if (!__builtin_amdgcn_readfirstlane((int)transit[d])) continue;  // same value proposed: nothing to do
      ++n_prop;
      double delta;
      uint64_t In[MT];
      bool wn = wj;
      const uint64_t bit = d < G ? 1ull << (d & 63) : 0ull;  // the proposed flip of i_raw, in word d >> 6
      if (d < G) {
        uint64_t Rn[MT];
        bool was_one = false;
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          Rn[t] = Rw[t];
          if (t == (d >> 6)) {
            was_one = (Rw[t] & bit) != 0;
            Rn[t] ^= bit;
          }
        }
        delta = gibbs_prior_delta(!was_one, theta0);
        constrain_masks<MT>(Rn, P, a, In);
      } else {
        wn = !wj;
        delta = gibbs_prior_delta(wn, theta7);
#pragma unroll
        for (int t = 0; t < MT; ++t) In[t] = I[t];
      }
      bool changed = wn != wj;  // a flip that leaves the constrained infections as they were moves the prior term only
#pragma unroll
      for (int t = 0; t < MT; ++t) changed |= In[t] != I[t];
      double nxt = cur;
      if (changed) {
        nxt = sparse_terms<R, MT>(a, p, j, lane, In, V, tabs, wn ? tabs + tstride : tab_ones, is2_n, is2_s, first, n_obs);
        delta += wave_sum_uniform(nxt - cur);
      }
      const double log_u = readfirstlane_f64(logu[d]);
      const bool accepted = gibbs_accept(delta, log_u);
      if (LOG) {
        if (lane == 0) {
          gibbs_log_how(lrec, n_rec, d, changed ? ABD_GLOG_LIST : ABD_GLOG_LIST_PRIOR, -1, -1);
          gibbs_log_outcome(lrec, n_rec, delta, log_u, accepted);
        }
        ++n_rec;
      }
      if (accepted) {
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          if (t == (d >> 6)) Rw[t] ^= bit;
          I[t] = In[t];
        }
        cur = nxt;
        wj = wn;
        ++n_acc;
      }
    }

    gibbs_store_state(slot, N, j, nt, lane, gibbs_lane_word<MT>(Rw, lane), gibbs_lane_word<MT>(I, lane), wj, pc0,
                      gibbs_state_counts<MT>(Rw, wj), d_n1, d_m1);
    if (LOG && ga.log_n && lane == 0) ga.log_n[(int64_t)c * N + j] = n_rec;
  }
  gibbs_finish(ga, p, c, lane0, d_n1, d_m1, n_acc, n_prop);
}
