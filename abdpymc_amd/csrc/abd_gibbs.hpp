// abd_gibbs.hpp -- one binary Gibbs-Metropolis sweep over [i_raw, ab_s_waner] on the device: what its two kernels share
// (abd_gibbs_lists.hpp: observation lists; abd_gibbs_dense.hpp: dense panels; both included by abd_gibbs.hip).
//
// What it replaces: PyMC's BinaryGibbsMetropolis.astep on the two discrete variables of the model
// (reference abd.py:427, 373; step assignment made by pm.sample, abd.py:922): shuffle all G*N + N binary
// dims, and for each, with probability transit_p = 0.8, flip it, evaluate the JOINT logp and keep the flip
// with probability min(1, exp(delta)).  That is ~0.8 (G N + N) full-graph evaluations per draw.
//
// Why it factorises: flipping a bit of individual j changes (a) that individual's own likelihood terms and
// (b) a prior term whose change does not depend on any other bit: Bernoulli(i_raw | p) moves by
// +-(log p - log(1 - p)) = +-theta_0, Bernoulli(waner | p_waner) by +-theta_7.  So the sweeps of different
// individuals commute exactly, the relative order of one individual's dims under a uniform global shuffle is
// uniform, and the cross-individual order is irrelevant: one wave per (individual, chain) running that
// individual's G + 1 proposals in a uniformly random order IS the reference's sweep, at O(G) instead of
// O(G N) work per proposal.
//
// Randomness: Philox4x32-10, counter (dim, individual, chain slot id + offset, 0), key (seed_lo ^ sweep * 0x9E3779B9, seed_hi):
// word 0 orders the dims (low 9 bits replaced by the dim index, so keys are unique), word 1 is the transit
// draw, word 2 the acceptance draw.  oracle/abd_oracle.c restates the same stream, so whole trajectories can
// be compared bit for bit.
//
// Both kernels make the same decisions bit for bit.  Written once, here: the draw of a dim, the load of an individual's packed
// rows, the prior's share of a flip, the acceptance rule, the write-back of an individual with the bookkeeping of
// sum(i_raw) / sum(ab_s_waner), and the closing atomics.  Each kernel keeps its own arithmetic for the likelihood term and for
// log u (library log / log_uniform_u32): those differ in the last bits and are compared with the oracle per kernel.
#pragma once

#include "abd_device.hpp"

__host__ __device__ constexpr size_t abd_gibbs_pad16(size_t b) { return (b + 15) / 16 * 16; }  // LDS regions start on 16 bytes

// a wave-uniform value the compiler cannot see through (nor hoist what is computed from it out of the loop it is made in).
// Wave-uniform, loop-invariant values that the compiler would otherwise derive masks and key schedules from in front of the
// individual loop and keep, spilled, for the whole kernel are re-made opaque per individual (abd_gibbs_dense.hpp has the account)
__device__ __forceinline__ int gibbs_opaque_uniform(int x) {
  asm volatile("" : "+v"(x));
  return __builtin_amdgcn_readfirstlane(x);
}

// ---- the random stream ----
// low key word of the sweep (the high one is seed_hi)
__device__ __forceinline__ uint32_t gibbs_key_lo(const GibbsArgs& ga) { return ga.seed_lo ^ (ga.sweep * 0x9E3779B9u); }

struct GibbsDraw {
  uint32_t key;     // orders the individual's dims: ascending key = the sweep's order
  bool proposed;    // transit: the flip is proposed (else the same value is, and nothing happens)
  uint32_t accept;  // the acceptance uniform is (accept + 1/2) / 2^32
};
// dim d of individual j on chain stream cs: dims 0 .. G-1 are i_raw[g, j], dim G is ab_s_waner[j]
__device__ __forceinline__ GibbsDraw gibbs_draw(const GibbsArgs& ga, int d, int j, uint32_t cs, uint32_t k0, uint32_t k1) {
  const Philox4 r = philox4x32_10((uint32_t)d, (uint32_t)j + ga.ind_offset, cs, 0u, k0, k1);
  GibbsDraw o;
  o.key = (r.w[0] & ~0x1FFu) | (uint32_t)d;
  o.proposed = r.w[1] < ABD_TRANSIT_P_U32;
  o.accept = r.w[2];
  return o;
}

// ---- the decision ----
// the prior's share of the log-ratio when a bit becomes `one`: Bernoulli(i_raw | p) on the RAW matrix with logodds theta_0
// (abd.py:427), Bernoulli(ab_s_waner | p_waner) with theta_7 (abd.py:373)
__device__ __forceinline__ double gibbs_prior_delta(bool one, double logodds) { return one ? logodds : -logodds; }
// metrop_select: keep the flip if delta > 0 or delta > log(u)
__device__ __forceinline__ bool gibbs_accept(double delta, double log_u) { return delta > 0.0 || delta > log_u; }

// ---- the decision log (abd_gibbs_sweep_log; the logging instantiations only) ----
// the records of individual j of the launch's chain c: one per position in the individual's order, G + 1 at most
__device__ __forceinline__ GibbsRecord* gibbs_log_rows(const GibbsArgs& ga, int c, int j) {
  return ga.log ? ga.log + (int64_t)c * ga.log_cap + (int64_t)j * (ga.e.G + 1) : nullptr;
}
// the record of position pos, in two halves: how the proposal is evaluated, and what came out.  A lane-owned evaluation
// writes both at once; a whole-wave one gets the first from the lane that classified it, the second from lane 0 at the frontier.
// An evaluation redone after an acceptance overwrites its position.
__device__ __forceinline__ void gibbs_log_how(GibbsRecord* rows, int pos, int dim, int path, int gf, int stop) {
  if (!rows) return;
  rows[pos].dim = (int16_t)dim;
  rows[pos].gf = (int16_t)gf;
  rows[pos].stop = (int16_t)stop;
  rows[pos].path = (uint8_t)path;
}
__device__ __forceinline__ void gibbs_log_outcome(GibbsRecord* rows, int pos, double value, double log_u, bool accepted) {
  if (!rows) return;
  rows[pos].value = value;
  rows[pos].log_u = log_u;
  rows[pos].accepted = accepted ? 1 : 0;
}

// ---- an individual's state in its chain's slot ----
struct GibbsSlot {
  uint64_t* rw;   // [nt][N] raw bits, updated in place
  uint64_t* iw;   // [nt][N] the constrained words the evaluation kernels read
  int8_t* waner;  // [N]
};
__device__ __forceinline__ GibbsSlot gibbs_slot(const ChainPar& p) {
  GibbsSlot s;
  s.rw = const_cast<uint64_t*>(p.rw);
  s.iw = const_cast<uint64_t*>(p.iw);
  s.waner = const_cast<int8_t*>(p.waner);
  return s;
}

// the packed rows of individual j, wave-uniform: vaccinations, PCR+ (none: zeros), raw infections
template <int MT>
__device__ __forceinline__ void gibbs_load_rows(const EvalArgs& a, const GibbsSlot& s, int j, int nt, uint64_t (&V)[MT],
                                                uint64_t (&P)[MT], uint64_t (&Rw)[MT]) {
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    V[t] = P[t] = Rw[t] = 0;
    if (t < nt) {
      V[t] = uniform_word(a.vw, (int64_t)t * a.N + j);
      if (a.pw) P[t] = uniform_word(a.pw, (int64_t)t * a.N + j);
      Rw[t] = uniform_word(s.rw, (int64_t)t * a.N + j);
    }
  }
}

// sum(i_raw) of the individual (low 16 bits) and its ab_s_waner (bit 16)
template <int MT>
__device__ __forceinline__ int gibbs_state_counts(const uint64_t (&Rw)[MT], bool wj) {
  int pc = wj ? (1 << 16) : 0;
#pragma unroll
  for (int t = 0; t < MT; ++t) pc += __builtin_popcountll(Rw[t]);
  return pc;
}

// Write the individual's state back: raw bits, waning flag, and what the slot keeps beside them (the constrained words, and --
// added to the wave's running d_n1 / d_m1 -- the changes of sum(i_raw) and sum(ab_s_waner): pc0 / pc1 = gibbs_state_counts
// before / after the sweep).  Lane t < nt brings word t of the raw and of the constrained row.
template <typename T>
__device__ __forceinline__ void gibbs_store_state(const GibbsSlot& s, int N, int j, int nt, int lane, uint64_t raw_word,
                                                  uint64_t kept_word, bool wj, int pc0, int pc1, T& d_n1, T& d_m1) {
  if (lane < nt) {
    s.rw[(int64_t)lane * N + j] = raw_word;
    s.iw[(int64_t)lane * N + j] = kept_word;
  }
  if (lane == 0) s.waner[j] = wj ? 1 : 0;
  d_n1 += (pc1 & 0xFFFF) - (pc0 & 0xFFFF);
  d_m1 += (pc1 >> 16) - (pc0 >> 16);
}

// ---- the end of a wave: its share of the slot's sums (p.cnt: sum(i_raw), sum(ab_s_waner)) and of the sweep's accepted /
// proposed counts (integer atomics: order-free) ----
template <typename TD, typename TN>
__device__ __forceinline__ void gibbs_finish(const GibbsArgs& ga, const ChainPar& p, int c, int lane, TD d_n1, TD d_m1, TN n_acc, TN n_prop) {
  if (lane == 0 && (d_n1 | d_m1)) {
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(const_cast<long long*>(p.cnt));  // (read here: not held for the whole kernel)
    atomicAdd(cnt + 0, (unsigned long long)(long long)d_n1);  // two's complement: a negative change wraps to the right sum
    atomicAdd(cnt + 1, (unsigned long long)(long long)d_m1);
  }
  if (lane == 0 && (n_acc | n_prop)) {
    atomicAdd(ga.counts + 2 * c + 0, (unsigned long long)n_acc);
    atomicAdd(ga.counts + 2 * c + 1, (unsigned long long)n_prop);
  }
}
