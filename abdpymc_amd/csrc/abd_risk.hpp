// abd_risk.hpp -- infection risk by titer of one draw (abd_risk, abd_sampler_enable_risk; include/abd_hip.h): the person-time
// table a Poisson / Cox-type model of "infection in gap g given the titer of gap g - 1" with a piecewise-constant titer effect
// needs of a binary draw, reduced on the device over the individuals.
//
// With (start, end) the window, last[j] the follow-up of the curves (abd_curves.hpp) and edges_s / edges_n up to 7 ascending
// bin edges per antigen, cell (g, j) is AT RISK iff start < g < end, g <= last[j] and, under first_only, i[g', j] = 0 for
// every start < g' < g; it is an EVENT iff it is at risk and i[g, j] = 1.  The table is
//   int64 table[2][2][G][8]   antigen (S, N) x (at risk, events) x gap x bin
// where the bin of a cell is #{e in edges: x >= e} of the titer of the PREVIOUS gap, x = ab_s_mu[g - 1, j] or
// ab_n_mu[g - 1, j]: cell_titers (abd_cells.hpp) at g - 1, what abd_deterministics_kernel records, not a second formula.  A NaN titer fails
// every comparison: bin 0.
//
// The kernel pair has the shape of the curves': slabs of ABD_CURVES_SLAB individuals, a wave per individual, a lane per gap of
// each 64-gap word; the table depends on (N, G, last, the slot's state, theta, the spec) and on nothing else.  A wave sees at
// most 16 individuals of a slab and a slab holds 64, so the 8 bins of one (antigen, kind, gap) are 8-bit counters packed
// into one 64-bit word -- in the lane's registers, in LDS where the four waves are added, and in the slab's row.
// abd_risk_sum_kernel unpacks the slab rows and adds them, slab p, p + PARTS, ... per part and then the parts, into 32-bit
// counts (a count is at most N < 2^31).  Integers only; no atomics of any kind.
#pragma once

#include "abd_curves.hpp"

#define ABD_RISK_NBIN 8        // titer bins per antigen
#define ABD_RISK_MAX_EDGES 7   // ... and the edges between them
#define ABD_RISK_SUM_PARTS 16  // abd_risk_sum_kernel: partial sums per packed column ...
#define ABD_RISK_SUM_COLS 16   // ... and packed columns per 256-thread workgroup
static_assert(ABD_CURVES_SLAB <= 255, "a slab's count must fit an 8-bit counter");
static_assert(ABD_RISK_NBIN * 8 == 64, "eight 8-bit counters per packed word");

// packed columns of a slab row: [antigen][kind][G]; counts of a table: [antigen][kind][G][8]
__host__ __device__ inline int64_t abd_risk_packed_cols(int G) { return (int64_t)4 * G; }
__host__ __device__ inline int64_t abd_risk_table_cols(int G) { return (int64_t)4 * G * ABD_RISK_NBIN; }

struct RiskArgs {
  CellWalk w;
  unsigned long long* slab_rows;  // [slabs][4 G] packed scratch, one row per slab
  double edges_s[ABD_RISK_MAX_EDGES], edges_n[ABD_RISK_MAX_EDGES];  // unused edges are +inf: never reached
  int32_t n_slabs;
  int32_t start, end, first_only;
};

// dynamic LDS behind the power tables: the slab's packed row [4][G], then the edges (41 KB with the tables at 512 gaps)
__host__ __device__ inline size_t abd_risk_lds_bytes(int G) {
  return (size_t)abd_risk_packed_cols(G) * sizeof(unsigned long long) + (size_t)2 * ABD_RISK_MAX_EDGES * sizeof(double);
}

template <int MT>
__global__ __launch_bounds__(ABD_BLOCK) void abd_risk_kernel(const RiskArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const CellWalk& w = a.w;
  const int G = w.G, N = w.N, nt = w.nt;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  unsigned long long* red = reinterpret_cast<unsigned long long*>(smem + cell_tables_bytes(G));  // [4][G] packed
  const int n_row = (int)abd_risk_packed_cols(G);
  // the edges live in LDS (every lane reads the same address: a broadcast), not in 28 scalar registers beside the packed words;
  // stored in front of the prologue's barrier
  double* edges = reinterpret_cast<double*>(red + n_row);  // [2][ABD_RISK_MAX_EDGES]
  if (tid == 0) {
#pragma unroll
    for (int e = 0; e < ABD_RISK_MAX_EDGES; ++e) {
      edges[e] = a.edges_s[e];
      edges[ABD_RISK_MAX_EDGES + e] = a.edges_n[e];
    }
  }
  const CellTables tabs = cell_tables(smem, w, tid);
  for (int slab = blockIdx.x; slab < a.n_slabs; slab += gridDim.x) {
    // the lane's packed counters of gap 64 t + lane over its wave's individuals of this slab
    unsigned long long r_s[MT], e_s[MT], r_n[MT], e_n[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) r_s[t] = e_s[t] = r_n[t] = e_n[t] = 0ull;
    const int j_end = min(N, (slab + 1) * ABD_CURVES_SLAB);
    for (int j = slab * ABD_CURVES_SLAB + wave; j < j_end; j += ABD_WAVES_PER_BLOCK) {
      const int last = last_gap(w, j);  // (read first: one vector register less, a wave more per SIMD)
      uint64_t V[MT], I[MT];
      const double2_t* ts = load_individual<MT>(w, j, tabs, V, I);
      // the last gap at risk (wave-uniform): the end of the window, of the follow-up and, under first_only, the first
      // infection after `start`
      int limit = min(last, a.end - 1);
      if (a.first_only) {
        int first = G;
#pragma unroll
        for (int t = MT - 1; t >= 0; --t) {
          const uint64_t after = I[t] & ~bits_upto(a.start - t * 64);  // gaps of this word behind `start`
          if (after) first = t * 64 + __builtin_ctzll(after);
        }
        limit = min(limit, first);
      }
      if (limit <= a.start) continue;  // nothing at risk (wave-uniform)
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        const int g = t * 64 + lane;
        if (t < nt && t * 64 <= limit && t * 64 + 63 > a.start && g > a.start && g <= limit) {
          const CellTiters c = cell_titers<MT>(w, V, I, tabs.tab_n, ts, g - 1, t + 1);  // the predecessor's titers
          int bs = 0, bn = 0;
#pragma unroll
          for (int e = 0; e < ABD_RISK_MAX_EDGES; ++e) {
            bs += c.mus >= edges[e] ? 1 : 0;
            bn += c.mun >= edges[ABD_RISK_MAX_EDGES + e] ? 1 : 0;
          }
          const unsigned long long bit = (I[t] >> lane) & 1ull;
          r_s[t] += 1ull << (8 * bs);
          e_s[t] += bit << (8 * bs);
          r_n[t] += 1ull << (8 * bn);
          e_n[t] += bit << (8 * bn);
        }
      }
    }
    // (no byte passes 64)
    slab_reduce<MT>(
        wave, lane, G, nt,
        [&](bool first, int t, int g) {
          slab_put(first, red[g], r_s[t]);
          slab_put(first, red[G + g], e_s[t]);
          slab_put(first, red[2 * G + g], r_n[t]);
          slab_put(first, red[3 * G + g], e_n[t]);
        },
        [](bool) {});
    unsigned long long* row = a.slab_rows + (int64_t)slab * n_row;
    for (int e = tid; e < n_row; e += ABD_BLOCK) row[e] = red[e];
    __syncthreads();  // (the next slab's wave 0 stores over red)
  }
}

// out[col][b] = sum over the slabs of byte b of packed column col of their rows
__global__ __launch_bounds__(ABD_RISK_SUM_PARTS* ABD_RISK_SUM_COLS) void abd_risk_sum_kernel(
    const unsigned long long* __restrict__ slab_rows, int n_slabs, int G, uint32_t* __restrict__ out) {
  __shared__ uint32_t part[ABD_RISK_SUM_PARTS][ABD_RISK_SUM_COLS][ABD_RISK_NBIN];
  const int64_t n_row = abd_risk_packed_cols(G);
  const int cl = threadIdx.x % ABD_RISK_SUM_COLS, p = threadIdx.x / ABD_RISK_SUM_COLS;
  const int64_t col = (int64_t)blockIdx.x * ABD_RISK_SUM_COLS + cl;
  uint32_t acc[ABD_RISK_NBIN];
#pragma unroll
  for (int b = 0; b < ABD_RISK_NBIN; ++b) acc[b] = 0u;
  if (col < n_row)
    for (int s = p; s < n_slabs; s += ABD_RISK_SUM_PARTS) {
      const unsigned long long w = slab_rows[(int64_t)s * n_row + col];
#pragma unroll
      for (int b = 0; b < ABD_RISK_NBIN; ++b) acc[b] += (uint32_t)(w >> (8 * b)) & 0xffu;
    }
#pragma unroll
  for (int b = 0; b < ABD_RISK_NBIN; ++b) part[p][cl][b] = acc[b];
  __syncthreads();
  // thread (cl2, b) of the first 128 adds the parts of one count
  if (threadIdx.x < ABD_RISK_SUM_COLS * ABD_RISK_NBIN) {
    const int cl2 = threadIdx.x / ABD_RISK_NBIN, b = threadIdx.x % ABD_RISK_NBIN;
    const int64_t col2 = (int64_t)blockIdx.x * ABD_RISK_SUM_COLS + cl2;
    if (col2 < n_row) {
      uint32_t sum = 0u;
      for (int q = 0; q < ABD_RISK_SUM_PARTS; ++q) sum += part[q][cl2][b];
      out[col2 * ABD_RISK_NBIN + b] = sum;
    }
  }
}
