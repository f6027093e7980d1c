// abd_individual.hpp -- the joint log-likelihood of every individual's OD readings at one chain slot's point:
//
//   S_j = sum of ll_k over j's S readings,  N_j = the same over its N readings,  T_j = S_j + N_j
//
// ll_k is reading_loglik (abd_readings.hpp), the value LogLik writes per reading.  An individual without readings of an
// antigen gets 0.0 for it.  The running statistics of T_j over the draws are LogLik's (waic_update): accumulators [4][N]
// per chain, rows M, S, mean, M2.
//
// One wave per individual in both kernels.  The order of every sum is fixed, so a row is bit-reproducible:
//   1. a lane adds its readings' terms to its own partial of the antigen, starting from 0.0:
//        dense panels: cells g = 64 t + lane in ascending t, one S and one N reading per cell, each to its antigen's partial
//        observation lists: readings k = seg[j] + lane, + 64, ... of the individual's segment in ascending k (sorted by gap);
//                           the whole S segment, then the whole N segment
//   2. wave_sum per antigen: partials exchanged by lane xor 32, 16, 8, 4, 2, 1 (abd_device.hpp), no LDS round trip
//   3. lane 0 forms T_j = S_j + N_j, writes the rows and updates column j: a plain read-modify-write, no atomics
// Separate kernels, not an op of the per-reading walkers: those keep their registers and spills (tools/resource_usage.py), and
// a lane-per-reading list walk cannot sum by individual without atomics.  They share the walkers' pieces: cell_tables,
// load_individual, responses (dense), list_sum_n / list_sum_s and the power tables (lists).
// Included by abd_eval.hip behind abd_readings.hpp.
#pragma once

#include "abd_readings.hpp"

// The per-individual op of a ReadingArgs block: behind Readings, so that block's field order stays what it is
struct IndLogLik {
  double* ll_s;           // [N] device row of S_j; nullptr: not written
  double* ll_n;           // [N] device row of N_j; nullptr: not written
  double* acc;            // [4][N] accumulators of the chain over T_j; nullptr: not updated
  const int32_t* seg_s;   // observation lists: [N + 1] offset of every individual's first S reading (sorted order)
  const int32_t* seg_n;   // ... and N reading
  int64_t n_draw;         // draw number of the update, >= 1
  double inv_n;           // 1 / n_draw
  double inv_sig[2], lnorm[2];  // per antigen: 1 / sigma, -log sigma - 1/2 log 2 pi
  // step 3 above, by the lane that owns individual j
  __device__ __forceinline__ void put(int j, int N, double s, double n) const {
    if (ll_s) ll_s[j] = s;
    if (ll_n) ll_n[j] = n;
    if (acc) waic_update(acc, j, N, s + n, n_draw, inv_n);
  }
};

// Dense panels: the walk of abd_readings_dense_kernel, the cell's two values summed instead of stored
template <typename R, int MT>
__global__ __launch_bounds__(ABD_BLOCK) void abd_individual_dense_kernel(const ReadingArgs<IndLogLik> a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const Readings& w = a.rd;
  const int G = w.G, N = w.N, nt = w.nt;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const CellTables tabs = cell_tables(smem, w.rho[kAgN], w.rho[kAgS], G, tid);
  const YX<R>* yxn = reinterpret_cast<const YX<R>*>(w.y_n);
  const YX<R>* yxs = reinterpret_cast<const YX<R>*>(w.y_s);
  // the constants in vector registers, as in abd_readings_dense_kernel: the scalar file holds the individual's packed words
  const double init_n = to_vgpr(w.init[kAgN]), perm_n = to_vgpr(w.perm[kAgN]), temp_n = to_vgpr(w.temp_n);
  const double b2_n = to_vgpr(w.b2[kAgN]), d_n = to_vgpr(w.d[kAgN]);
  const double is_n = to_vgpr(a.op.inv_sig[kAgN]), ln_n = to_vgpr(a.op.lnorm[kAgN]);
  const double init_s = to_vgpr(w.init[kAgS]), perm_s = to_vgpr(w.perm[kAgS]);
  const double b2_s = to_vgpr(w.b2[kAgS]), d_s = to_vgpr(w.d[kAgS]);
  const double is_s = to_vgpr(a.op.inv_sig[kAgS]), ln_s = to_vgpr(a.op.lnorm[kAgS]);
  const int waves_total = gridDim.x * ABD_WAVES_PER_BLOCK;
  for (int j = blockIdx.x * ABD_WAVES_PER_BLOCK + wave; j < N; j += waves_total) {
    uint64_t V[MT], I[MT];
    const double2_t* ts = load_individual<MT>(w.vw, w.iw, w.waner, N, nt, j, tabs, V, I);
    double sum_s = 0.0, sum_n = 0.0;
    for (int t = 0; t < nt; ++t) {
      const int g = t * 64 + lane;
      if (g < G) {
        const Resp rs = responses<MT>(g, t + 1, I, V, tabs.tab_n, ts);
        const int64_t k = (int64_t)j * G + g;
        const double an = init_n + (rs.cum_i ? perm_n : 0.0) + temp_n * rs.un;
        const double as = init_s + (rs.cum_iv ? perm_s : 0.0) + rs.us;
        const YX<R> cn = yxn[k], cs = yxs[k];
        sum_s += reading_loglik(b2_s, d_s, is_s, ln_s, as, (double)cs.x, (double)cs.y);
        sum_n += reading_loglik(b2_n, d_n, is_n, ln_n, an, (double)cn.x, (double)cn.y);
      }
    }
    sum_s = wave_sum(sum_s);
    sum_n = wave_sum(sum_n);
    if (lane == 0) a.op.put(j, N, sum_s, sum_n);
  }
}

// Observation lists: the lanes stride over the individual's segment of each list
template <typename R, int MT>
__global__ __launch_bounds__(ABD_BLOCK) void abd_individual_lists_kernel(const ReadingArgs<IndLogLik> a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const Readings& w = a.rd;
  const int N = w.N;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const CellTables tabs = cell_tables(smem, w.rho[kAgN], w.rho[kAgS], w.G, tid);
  const double init_n = to_vgpr(w.init[kAgN]), perm_n = to_vgpr(w.perm[kAgN]), temp_n = to_vgpr(w.temp_n);
  const double b2_n = to_vgpr(w.b2[kAgN]), d_n = to_vgpr(w.d[kAgN]);
  const double is_n = to_vgpr(a.op.inv_sig[kAgN]), ln_n = to_vgpr(a.op.lnorm[kAgN]);
  const double init_s = to_vgpr(w.init[kAgS]), perm_s = to_vgpr(w.perm[kAgS]);
  const double b2_s = to_vgpr(w.b2[kAgS]), d_s = to_vgpr(w.d[kAgS]);
  const double is_s = to_vgpr(a.op.inv_sig[kAgS]), ln_s = to_vgpr(a.op.lnorm[kAgS]);
  const int waves_total = gridDim.x * ABD_WAVES_PER_BLOCK;
  for (int j = blockIdx.x * ABD_WAVES_PER_BLOCK + wave; j < N; j += waves_total) {
    const double2_t* ts = __builtin_amdgcn_readfirstlane((int)w.waner[j]) != 0 ? tabs.tab_s : tabs.tab_ones;
    double sum_s = 0.0, sum_n = 0.0;
    const int s0 = __builtin_amdgcn_readfirstlane(a.op.seg_s[j]), s1 = __builtin_amdgcn_readfirstlane(a.op.seg_s[j + 1]);
    for (int k = s0 + lane; k < s1; k += 64) {
      const double y = ld<R>(w.y_s, k), x = ld<R>(w.x_s, k);
      const ListSum r = list_sum_s<MT>(w, w.g_s[k], j, ts);
      sum_s += reading_loglik(b2_s, d_s, is_s, ln_s, init_s + (r.cum ? perm_s : 0.0) + r.u, x, y);
    }
    const int n0 = __builtin_amdgcn_readfirstlane(a.op.seg_n[j]), n1 = __builtin_amdgcn_readfirstlane(a.op.seg_n[j + 1]);
    for (int k = n0 + lane; k < n1; k += 64) {
      const double y = ld<R>(w.y_n, k), x = ld<R>(w.x_n, k);
      const ListSum r = list_sum_n<MT>(w, w.g_n[k], j, tabs.tab_n);
      sum_n += reading_loglik(b2_n, d_n, is_n, ln_n, init_n + (r.cum ? perm_n : 0.0) + temp_n * r.u, x, y);
    }
    sum_s = wave_sum(sum_s);
    sum_n = wave_sum(sum_n);
    if (lane == 0) a.op.put(j, N, sum_s, sum_n);
  }
}
