// abd_simulate.hpp -- the forward simulator of a cohort (reference abdpymc/simulation.py:222-279, 328-353): infections under
// titer-mediated protection, the S and N titers they and the vaccinations raise, and OD readings of those titers.
//
// The walk.  Replicate rho, individual j, gaps t = 0 .. G-1 in sequence, s_temp = n_temp = 0 before gap 0:
//   s_prev, n_prev   the titers of gap t - 1 (the bare init values at t = 0)
//   exposed          u_e < lam0[t]
//   p_x              1 / (1 + exp(-b_x (x_prev - a_x)))                      x in {s, n}: the protection curves
//   protected        u_s < p_s or u_n < p_n
//   infected         pcrpos[j, t] == 1 or (exposed and not protected)
//   s_temp           s_temp wane_s + infected rise_i_s + vacs[j, t] rise_v_s
//   n_temp           n_temp wane_n + infected rise_i_n                       (N's temp_rise_v is unused)
//   s_perm           perm_rise_s once any infection or vaccination has occurred in gaps 0 .. t, else 0
//   n_perm           perm_rise_n once any infection has
//   s[t], n[t]       init_x + x_temp + x_perm
// There is no three-gap mask: the reference's simulator has none.
// A reading k of antigen x at (gap, ind, log_dilution):  od = d_x / (1 + exp(-b_x (log_dilution - x[ind, gap]))) + sd_x z_k
//
// Random numbers: Philox4x32-10, key (seed lo, seed hi), counters
//   exposure       (ind_offset + j, rho, t, 0x40000000)            u_e from words 0, 1
//   protection     (ind_offset + j, rho, t, 0x40000001)            u_s from words 0, 1; u_n from words 2, 3
//   reading noise  (r, rho, 0, 0x40000010 | antigen)               z the first Box-Muller value of the four words
//   r: the reading's index in the CALLER's order within its antigen (S = 0, N = 1).  Uniforms and Box-Muller as the
//   predictive stream forms them (abd_readings.hpp): u = ((a >> 5) 2^26 + (b >> 6) + 0.5) 2^-53.  The sweep's counters have
//   c3 = 0 and the predictive stream sets c3's top bit: none of the three streams meet.
// So a replicate depends on (seed, rho) only -- not on how many replicates a call asks for, nor on dense panels or lists -- and
// an individual's infection process depends on its GLOBAL index: it is the same on a cohort sharded by individual
// (abd_set_individual_offset).  The reading noise is keyed by the local reading index and is not.
// A draw is a pure function of its counter, so the walk makes the protection draw only where its outcome matters (exposed
// and no PCR+): the infections are the same as if every gap had made all three.
//
// The step function is plain C++ shared with the CPU harness (tests/native/simulate_harness.cpp); the kernels follow it.
// Included by abd_eval.hip (the host side: abd_simulate).
#pragma once

#include <math.h>

#include "abd_types.hpp"

namespace abdi {

// c3 of the streams (kSimExposure, kSimProtection, kSimNoise) and sim_uniform: abd_types.hpp, beside philox4x32_10

// what the walk reads of one antigen's parameters
struct SimWalkAb {
  double protect_a, protect_b, init, perm_rise, temp_rise_i, temp_rise_v, temp_wane;
};
struct SimWalkPar {
  SimWalkAb s, n;
};

// an individual between two gaps
struct SimState {
  double s_prev, n_prev;  // titers of the gap before
  double s_temp, n_temp;
  bool any_i, any_v;      // an infection / a vaccination has occurred so far
};

__host__ __device__ inline SimState sim_start(const SimWalkPar& p) { return {p.s.init, p.n.init, 0.0, 0.0, false, false}; }

__host__ __device__ inline double sim_p_protection(const SimWalkAb& ab, double titer) {
  return 1.0 / (1.0 + exp(-ab.protect_b * (titer - ab.protect_a)));
}

// The keyed draws of one (individual, replicate)
struct SimKeyed {
  uint32_t seed_lo, seed_hi;
  uint32_t ind;  // global index of the individual
  uint32_t rho;
  __host__ __device__ double exposure(uint32_t t) const {
    const Philox4 p = philox4x32_10(ind, rho, t, kSimExposure, seed_lo, seed_hi);
    return sim_uniform(p.w[0], p.w[1]);
  }
  __host__ __device__ void protection(uint32_t t, double& u_s, double& u_n) const {
    const Philox4 p = philox4x32_10(ind, rho, t, kSimProtection, seed_lo, seed_hi);
    u_s = sim_uniform(p.w[0], p.w[1]);
    u_n = sim_uniform(p.w[2], p.w[3]);
  }
};

// One gap of the walk: is the individual infected in gap t, and the state moved on to it (st.s_prev / n_prev: the titers of t).
// Draws: exposure(t) -> u_e; protection(t, u_s, u_n).
template <typename Draws>
__host__ __device__ inline bool sim_step(const SimWalkPar& p, SimState& st, double lam, bool pcrpos, bool vac, const Draws& dr,
                                         uint32_t t) {
  bool infected = pcrpos;
  if (!pcrpos && dr.exposure(t) < lam) {
    double u_s, u_n;
    dr.protection(t, u_s, u_n);
    infected = !(u_s < sim_p_protection(p.s, st.s_prev) || u_n < sim_p_protection(p.n, st.n_prev));
  }
  st.s_temp = st.s_temp * p.s.temp_wane + (infected ? p.s.temp_rise_i : 0.0) + (vac ? p.s.temp_rise_v : 0.0);
  st.n_temp = st.n_temp * p.n.temp_wane + (infected ? p.n.temp_rise_i : 0.0);
  st.any_i |= infected;
  st.any_v |= vac;
  st.s_prev = p.s.init + st.s_temp + ((st.any_i || st.any_v) ? p.s.perm_rise : 0.0);
  st.n_prev = p.n.init + st.n_temp + (st.any_i ? p.n.perm_rise : 0.0);
  return infected;
}

// The noise-free OD of a reading (abd.logistic) plus sd z
__host__ __device__ inline double sim_od(double b, double d, double sd, double log_dilution, double titer, double z) {
  return d / (1.0 + exp(-b * (log_dilution - titer))) + sd * z;
}

#if defined(__HIPCC__)

// ---- the walk: one lane per (replicate, individual), a workgroup = one wave = 64 consecutive individuals of a replicate ----
constexpr int kSimTile = 16;            // gaps per staged tile: a row of a tile is one 128-byte line of the titer output
constexpr int kSimRow = kSimTile + 1;   // ... padded by one double: lanes that write a column land 2-way on the LDS banks, not 32-way

struct SimWalkArgs {
  SimWalkPar par;
  const double* lam0;        // [G] (device)
  const uint64_t* vw;        // [nt][N] packed vaccinations
  const uint64_t* pw;        // [nt][N] packed PCR positives; nullptr: none are forced
  // the chunk's outputs, replicate-major; nullptr: not written
  int8_t* inf;               // [Rc][N][G]
  double* st;                // [Rc][N][G]
  double* nt;                // [Rc][N][G]
  unsigned long long* cnt;   // [Rc][G], zeroed: infections per gap (integer atomics: order-free)
  uint32_t seed_lo, seed_hi, ind_offset, rho0;  // rho0: the chunk's first replicate
  int32_t G, N;
};

// grid (lane groups, replicates of the chunk).  The outputs are (N, G) row-major per replicate, so a lane storing its own row
// would write with stride G: the titers of 16 gaps are staged through LDS and stored 16 lanes to a row (128 contiguous
// bytes), the infections are collected in one 64-bit word per 64 gaps and stored 64 lanes to a row.
__global__ __launch_bounds__(64) void abd_sim_walk_kernel(const SimWalkArgs a) {
  __shared__ double tile_s[64 * kSimRow];
  __shared__ double tile_n[64 * kSimRow];
  __shared__ uint64_t words[64];
  const int lane = threadIdx.x;
  const int rl = blockIdx.y;
  const int j0 = blockIdx.x * 64;
  const int rows = min(64, a.N - j0);      // individuals of this lane group
  const bool valid = lane < rows;
  const int j = j0 + (valid ? lane : rows - 1);  // (a lane beyond the cohort walks the last individual and stores nothing)
  const SimKeyed dr{a.seed_lo, a.seed_hi, a.ind_offset + (uint32_t)j, a.rho0 + (uint32_t)rl};
  SimState state = sim_start(a.par);
  const int64_t base = ((int64_t)rl * a.N + j0) * a.G;  // the group's first row in a [Rc][N][G] output
  const bool titers = a.st || a.nt;
  const int n_words = (a.G + 63) >> 6;
  for (int t = 0; t < n_words; ++t) {
    const uint64_t V = a.vw[(int64_t)t * a.N + j];
    const uint64_t P = a.pw ? a.pw[(int64_t)t * a.N + j] : 0ull;
    uint64_t I = 0;
    const int gw = min(64, a.G - t * 64);  // gaps of this word
    for (int g0 = 0; g0 < gw; g0 += kSimTile) {
      const int gt = min(kSimTile, gw - g0);
      for (int q = 0; q < gt; ++q) {
        const int b = g0 + q, g = t * 64 + b;
        const bool inf = sim_step(a.par, state, a.lam0[g], (P >> b) & 1ull, (V >> b) & 1ull, dr, (uint32_t)g);
        I |= (uint64_t)inf << b;
        if (a.st) tile_s[lane * kSimRow + q] = state.s_prev;
        if (a.nt) tile_n[lane * kSimRow + q] = state.n_prev;
      }
      if (titers) {
        __syncthreads();
        const int c = lane & 15;
        if (c < gt)
          for (int r = lane >> 4; r < rows; r += 4) {
            const int64_t o = base + (int64_t)r * a.G + t * 64 + g0 + c;
            if (a.st) a.st[o] = tile_s[r * kSimRow + c];
            if (a.nt) a.nt[o] = tile_n[r * kSimRow + c];
          }
        __syncthreads();
      }
    }
    if (a.inf || a.cnt) {
      words[lane] = valid ? I : 0ull;
      __syncthreads();
      unsigned int n_inf = 0;  // of gap t * 64 + lane over the group's individuals
      if (lane < gw) {
        for (int r = 0; r < rows; ++r) {
          const unsigned int bit = (unsigned int)(words[r] >> lane) & 1u;
          n_inf += bit;
          if (a.inf) a.inf[base + (int64_t)r * a.G + t * 64 + lane] = (int8_t)bit;
        }
        if (a.cnt && n_inf) atomicAdd(&a.cnt[(int64_t)rl * a.G + t * 64 + lane], (unsigned long long)n_inf);
      }
      __syncthreads();
    }
  }
}

// ---- the readings: one lane per (reading, replicate) in the context's sorted order, written in the caller's order ----
struct SimReadArgs {
  const void* yx;        // dense: the individual-major pair panel yxi (YX<R>): reading k is cell (k / G, k % G)
  const void* x;         // lists: log dilution, gap, individual of every reading
  const uint16_t* g;
  const int32_t* j;
  const uint32_t* ord;   // [K] the caller's index of every sorted reading within its antigen
  const double* titer;   // [Rc][N][G] the walk's staged titers of this antigen
  double* od;            // [Rc][K], caller's order
  double b, d, sd;
  int64_t K;
  int32_t G, N;
  uint32_t seed_lo, seed_hi, rho0, c3;
};

// grid (ceil(K / 256), replicates of the chunk)
template <typename R, bool Dense>
__global__ __launch_bounds__(256) void abd_sim_read_kernel(const SimReadArgs a) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= a.K) return;
  const int rl = blockIdx.y;
  int j, g;
  double x;
  if (Dense) {
    j = (int)(k / a.G);
    g = (int)(k - (int64_t)j * a.G);
    x = (double)reinterpret_cast<const YX<R>*>(a.yx)[k].x;
  } else {
    j = a.j[k];
    g = a.g[k];
    x = (double)reinterpret_cast<const R*>(a.x)[k];
  }
  const double titer = a.titer[((int64_t)rl * a.N + j) * a.G + g];
  const uint32_t r = a.ord[k];
  const Philox4 p = philox4x32_10(r, a.rho0 + (uint32_t)rl, 0u, a.c3, a.seed_lo, a.seed_hi);
  const double z = sqrt(-2.0 * log(sim_uniform(p.w[0], p.w[1]))) * cospi(2.0 * sim_uniform(p.w[2], p.w[3]));
  a.od[(int64_t)rl * a.K + r] = sim_od(a.b, a.d, a.sd, x, titer, z);
}

#endif  // __HIPCC__

}  // namespace abdi
