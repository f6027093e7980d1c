// abd_cells.hpp -- the cell walk that the per-draw kernels share: abd_deterministics_kernel (abd_small.hpp),
// abd_readings_dense_kernel (abd_readings.hpp), abd_curves_kernel, abd_risk_kernel, abd_diag_kernel, abd_timeline_kernel.
// One wave per individual, the lanes over the gaps of each 64-gap word; the power tables in LDS; the titers of a cell from
// responses<MT> (abd_device.hpp) and the two expressions of cell_titers below -- the ONE place they are written.  A kernel
// keeps its own loop over individuals and words and its own per-cell body: what it does with (mun, mus) and the bit.
#pragma once

#include "abd_device.hpp"

// What the walk reads.  A kernel's argument block is { CellWalk w; its own fields }: a small block keeps the scalar registers
// for the packed words (a 2 KB EvalArgs would take them).
struct CellWalk {
  const uint64_t* vw;      // [nt][N] packed vaccinations
  const uint64_t* iw;      // [nt][N] the chain slot's constrained infections
  const int8_t* waner;     // [N]
  const int32_t* last;     // [N] end of follow-up; nullptr: G - 1 for everyone (read by the kernels that know of follow-up)
  double rho_n, rho_s, init_n, perm_n, temp_n, init_s, perm_s;
  int32_t G, N, nt;
};

// dynamic LDS of the three power tables (rho_n, rho_s, ones), G + 1 entries each: a kernel's own LDS lies behind them
__host__ __device__ inline size_t cell_tables_bytes(int G) { return (size_t)3 * (G + 1) * sizeof(double2_t); }

struct CellTables {
  const double2_t* tab_n;     // powers of rho_n
  const double2_t* tab_s;     // powers of rho_s: a waner's S table
  const double2_t* tab_ones;  // a non-waner's
  unsigned char* behind;      // the first byte behind the tables
};

// The prologue: the workgroup fills the tables and waits for them
__device__ __forceinline__ CellTables cell_tables(unsigned char* smem, double rho_n, double rho_s, int G, int tid) {
  double2_t* tabs = reinterpret_cast<double2_t*>(smem);
  const int tstride = G + 1;
  fill_pow_table(tabs, rho_n, tstride, tid, ABD_BLOCK);
  fill_pow_table(tabs + tstride, rho_s, tstride, tid, ABD_BLOCK);
  fill_ones_table(tabs + 2 * tstride, tstride, tid, ABD_BLOCK);
  __syncthreads();
  return {tabs, tabs + tstride, tabs + 2 * tstride, smem + cell_tables_bytes(G)};
}
__device__ __forceinline__ CellTables cell_tables(unsigned char* smem, const CellWalk& w, int tid) {
  return cell_tables(smem, w.rho_n, w.rho_s, w.G, tid);
}

// An individual's packed words V, I (wave-uniform: scalar registers) and its S table, chosen by waner[j].  V and I are the
// caller's plain arrays: a kernel that indexes them by a loop variable keeps them in registers only as such.
template <int MT>
__device__ __forceinline__ const double2_t* load_individual(const uint64_t* vw, const uint64_t* iw, const int8_t* waner, int N, int nt,
                                                            int j, const CellTables& tabs, uint64_t (&V)[MT], uint64_t (&I)[MT]) {
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    V[t] = I[t] = 0;
    if (t < nt) {
      V[t] = uniform_word(vw, (int64_t)t * N + j);
      I[t] = uniform_word(iw, (int64_t)t * N + j);
    }
  }
  const bool wj = __builtin_amdgcn_readfirstlane((int)waner[j]) != 0;
  return wj ? tabs.tab_s : tabs.tab_ones;
}
template <int MT>
__device__ __forceinline__ const double2_t* load_individual(const CellWalk& w, int j, const CellTables& tabs, uint64_t (&V)[MT],
                                                            uint64_t (&I)[MT]) {
  return load_individual<MT>(w.vw, w.iw, w.waner, w.N, w.nt, j, tabs, V, I);
}

// the end of individual j's follow-up (wave-uniform); -1: never followed
__device__ __forceinline__ int last_gap(const CellWalk& w, int j) { return w.last ? __builtin_amdgcn_readfirstlane(w.last[j]) : w.G - 1; }

// bits 0 .. rel of a word (none for rel < 0, all from 63 on)
__device__ __forceinline__ uint64_t bits_upto(int rel) { return rel >= 63 ? ~0ull : (rel < 0 ? 0ull : ((2ull << rel) - 1ull)); }

// infections at gaps 0 .. last
template <int MT>
__device__ __forceinline__ int followed_infections(const uint64_t (&I)[MT], int last, int nt) {
  int n_inf = 0;
#pragma unroll
  for (int t = 0; t < MT; ++t)
    if (t < nt) n_inf += __builtin_popcountll(I[t] & bits_upto(last - t * 64));
  return n_inf;
}

// The titers of cell (g, j): ab_n_mu, ab_s_mu (abd.py:341, 389-391) from the responses to the exposures in words 0 .. n_words - 1
// at or before g, and whether there was an infection at or before g.  Every kernel above records, sums, bins or accumulates
// THESE values.
struct CellTiters {
  double mun, mus;
  bool cum_i;
};

template <int MT>
__device__ __forceinline__ CellTiters cell_titers(const CellWalk& w, const uint64_t (&V)[MT], const uint64_t (&I)[MT], const double2_t* tn,
                                                   const double2_t* ts, int g, int n_words) {
  const Resp rs = responses<MT>(g, n_words, I, V, tn, ts);
  CellTiters c;
  c.mun = w.init_n + (rs.cum_i ? w.perm_n : 0.0) + w.temp_n * rs.un;
  c.mus = w.init_s + (rs.cum_iv ? w.perm_s : 0.0) + rs.us;
  c.cum_i = rs.cum_i;
  return c;
}

// A slab's row in LDS from the four waves' lane partials, in wave order: wave 0 stores, waves 1, 2, 3 add in turn.
// cols(first, t, g) moves the lane's columns of gap g = 64 t + lane with slab_put; tail(first) what is not per gap.
template <typename T>
__device__ __forceinline__ void slab_put(bool first, T& at, T v) {
  if (first)
    at = v;
  else
    at += v;
}

template <int MT, typename Cols, typename Tail>
__device__ __forceinline__ void slab_reduce(int wave, int lane, int G, int nt, Cols cols, Tail tail) {
  for (int w = 0; w < ABD_WAVES_PER_BLOCK; ++w) {
    if (wave == w) {
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        const int g = t * 64 + lane;
        if (t < nt && g < G) cols(w == 0, t, g);
      }
      tail(w == 0);
    }
    __syncthreads();
  }
}
