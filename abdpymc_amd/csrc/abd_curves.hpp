// abd_curves.hpp -- the epidemic curves of one draw (abd_curves, abd_sampler_enable_curves; include/abd_hip.h): what a user
// would reduce from the recorded Deterministics "i", "ab_s_mu", "ab_n_mu" of a draw, reduced on the device over the
// individuals so that a draw is a row of 6 G + 8 numbers instead of three (G, N) arrays.
//
// With last[j] the end of individual j's follow-up (-1: never followed; no array: G - 1 for everyone) and cell (g, j)
// FOLLOWED iff g <= last[j], a row is
//   int64 counts[4][G]   infected       #{j followed at g: i[g, j] = 1}
//                        ever_infected  #{j followed at g: i[g', j] = 1 for some g' <= g}      (Resp::cum_i)
//                        seropos_s      #{j followed at g: ab_s_mu[g, j] >= thr_s}
//                        seropos_n      #{j followed at g: ab_n_mu[g, j] >= thr_n}
//   int64 n_infections[8]  individuals with last[j] >= 0 by their number of infections in gaps 0 .. last[j]; [7]: 7 or more
//   double titer_sums[2][G]  sums over the followed j of ab_s_mu[g, j], of ab_n_mu[g, j]
// The titers are cell_titers (abd_cells.hpp), what abd_deterministics_kernel records: not a second formula.
//
// Reproducibility rule: a row depends on (N, G, last, the slot's state, theta, the thresholds) and on nothing else -- not on
// the grid, the number of CUs, what else runs, or timing.  The individuals are cut into SLABS of ABD_CURVES_SLAB consecutive
// indices.  A workgroup takes whole slabs; inside one, wave w takes individuals w, w + 4, ... in index order and a lane adds
// its gaps' values in registers; the four waves' partials are added in wave order through LDS and the slab's row goes to a
// scratch buffer.  abd_curves_sum_kernel then adds the slab rows: part p of ABD_CURVES_SUM_PARTS adds slabs p, p + PARTS,
// ... in order, and the parts are added in order.  Every addition has its place; there are no atomics of any kind.
#pragma once

#include "abd_cells.hpp"

#define ABD_CURVES_SLAB 64       // individuals per slab: 16 per wave (the power tables' fill is shared by the workgroup's slabs)
#define ABD_CURVES_SUM_PARTS 16  // abd_curves_sum_kernel: partial sums per column ...
#define ABD_CURVES_SUM_COLS 16   // ... and columns per 256-thread workgroup (16 doubles: one 128-byte line per part)
#define ABD_CURVES_NBIN 8        // bins of n_infections

// columns of a row, all 8 bytes wide: the integers first
__host__ __device__ inline int64_t abd_curves_int_cols(int G) { return (int64_t)4 * G + ABD_CURVES_NBIN; }
__host__ __device__ inline int64_t abd_curves_row_cols(int G) { return (int64_t)6 * G + ABD_CURVES_NBIN; }
__host__ __device__ inline int abd_curves_slabs(int N) { return (N + ABD_CURVES_SLAB - 1) / ABD_CURVES_SLAB; }

// The launch's argument block: the walk and the curves' own fields (in this order the kernels spill fewer scalar registers
// than with the pointer first; tools/resource_usage.py)
struct CurvesArgs {
  CellWalk w;
  double thr_s, thr_n;
  unsigned long long* slab_rows;  // [slabs][6 G + 8] scratch, one row per slab
  int32_t n_slabs;
};

// dynamic LDS behind the power tables, the slab's row: [2][G] doubles, [4][G] + 8 ints (41 KB with the tables at 512 gaps)
__host__ __device__ inline size_t abd_curves_lds_bytes(int G) {
  return (size_t)2 * G * sizeof(double) + ((size_t)4 * G + ABD_CURVES_NBIN) * sizeof(int);
}

template <int MT>
__global__ __launch_bounds__(ABD_BLOCK) void abd_curves_kernel(const CurvesArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const CellWalk& w = a.w;
  const int G = w.G, N = w.N, nt = w.nt;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const CellTables tabs = cell_tables(smem, w, tid);
  double* red_d = reinterpret_cast<double*>(tabs.behind);  // [2][G]: ab_s_mu, ab_n_mu
  int* red_c = reinterpret_cast<int*>(red_d + 2 * G);       // [4][G] counts, then [8] bins
  const int64_t n_int = abd_curves_int_cols(G), n_row = abd_curves_row_cols(G);
  for (int slab = blockIdx.x; slab < a.n_slabs; slab += gridDim.x) {
    // the lane's partials of gap 64 t + lane over its wave's individuals of this slab
    int c_inf[MT], c_ever[MT], c_ps[MT], c_pn[MT];
    double s_s[MT], s_n[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      c_inf[t] = c_ever[t] = c_ps[t] = c_pn[t] = 0;
      s_s[t] = s_n[t] = 0.0;
    }
    int bins = 0;  // lane k < 8: individuals of this wave with k infections
    const int j_end = min(N, (slab + 1) * ABD_CURVES_SLAB);
    for (int j = slab * ABD_CURVES_SLAB + wave; j < j_end; j += ABD_WAVES_PER_BLOCK) {
      const int last = last_gap(w, j);
      if (last < 0) continue;  // never followed (wave-uniform)
      uint64_t V[MT], I[MT];
      const double2_t* ts = load_individual<MT>(w, j, tabs, V, I);
      bins += lane == min(followed_infections<MT>(I, last, nt), ABD_CURVES_NBIN - 1);
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        const int g = t * 64 + lane;
        if (t < nt && t * 64 <= last && g < G) {
          const CellTiters c = cell_titers<MT>(w, V, I, tabs.tab_n, ts, g, t + 1);
          const int bit = (int)((I[t] >> lane) & 1ull);
          if (g <= last) {
            c_inf[t] += bit;
            c_ever[t] += c.cum_i ? 1 : 0;
            c_ps[t] += c.mus >= a.thr_s ? 1 : 0;
            c_pn[t] += c.mun >= a.thr_n ? 1 : 0;
            s_s[t] += c.mus;
            s_n[t] += c.mun;
          }
        }
      }
    }
    slab_reduce<MT>(
        wave, lane, G, nt,
        [&](bool first, int t, int g) {
          slab_put(first, red_c[g], c_inf[t]);
          slab_put(first, red_c[G + g], c_ever[t]);
          slab_put(first, red_c[2 * G + g], c_ps[t]);
          slab_put(first, red_c[3 * G + g], c_pn[t]);
          slab_put(first, red_d[g], s_s[t]);
          slab_put(first, red_d[G + g], s_n[t]);
        },
        [&](bool first) {
          if (lane < ABD_CURVES_NBIN) slab_put(first, red_c[4 * G + lane], bins);
        });
    unsigned long long* row = a.slab_rows + (int64_t)slab * n_row;
    for (int e = tid; e < (int)n_int; e += ABD_BLOCK) row[e] = (unsigned long long)(long long)red_c[e];
    for (int e = tid; e < 2 * G; e += ABD_BLOCK) row[n_int + e] = (unsigned long long)__double_as_longlong(red_d[e]);
    __syncthreads();  // (the next slab's wave 0 stores over red_*)
  }
}

// out[c] = sum over the slabs of column c of their rows, in the fixed order described above: integer columns first
__global__ __launch_bounds__(ABD_CURVES_SUM_PARTS* ABD_CURVES_SUM_COLS) void abd_curves_sum_kernel(
    const unsigned long long* __restrict__ slab_rows, int n_slabs, int G, unsigned long long* __restrict__ out) {
  __shared__ unsigned long long part[ABD_CURVES_SUM_PARTS][ABD_CURVES_SUM_COLS];
  const int64_t n_int = abd_curves_int_cols(G), n_row = abd_curves_row_cols(G);
  const int cl = threadIdx.x % ABD_CURVES_SUM_COLS, p = threadIdx.x / ABD_CURVES_SUM_COLS;
  const int64_t col = (int64_t)blockIdx.x * ABD_CURVES_SUM_COLS + cl;
  const bool is_int = col < n_int;
  if (col < n_row) {
    if (is_int) {
      long long acc = 0;
      for (int s = p; s < n_slabs; s += ABD_CURVES_SUM_PARTS) acc += (long long)slab_rows[(int64_t)s * n_row + col];
      part[p][cl] = (unsigned long long)acc;
    } else {
      double acc = 0.0;
      for (int s = p; s < n_slabs; s += ABD_CURVES_SUM_PARTS) acc += __longlong_as_double((long long)slab_rows[(int64_t)s * n_row + col]);
      part[p][cl] = (unsigned long long)__double_as_longlong(acc);
    }
  }
  __syncthreads();
  if (p == 0 && col < n_row) {
    if (is_int) {
      long long acc = 0;
      for (int q = 0; q < ABD_CURVES_SUM_PARTS; ++q) acc += (long long)part[q][cl];
      out[col] = (unsigned long long)acc;
    } else {
      double acc = 0.0;
      for (int q = 0; q < ABD_CURVES_SUM_PARTS; ++q) acc += __longlong_as_double((long long)part[q][cl]);
      out[col] = (unsigned long long)__double_as_longlong(acc);
    }
  }
}
