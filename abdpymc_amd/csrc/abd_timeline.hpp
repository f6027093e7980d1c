// abd_timeline.hpp -- per-individual timelines over ALL draws of a chain (abd_sampler_enable_timelines, abd_sampler_timelines,
// abd_sampler_timeline_quantiles; include/abd_hip.h has the definition in full): what the reference's per-individual figure
// reads from the (draw, gap, ind) arrays of the whole posterior -- the spread of the two titers of a cell, which is bimodal
// (infected before that gap or not) so that mean and sd are the wrong summary, the infection probability, and the probability
// of at least one infection so far inside the cell's time chunk -- kept on the device because a run at full size never keeps
// its draws.
//
// Per chain and cell (g, j): a histogram of 64 counters of 16 bits for ab_n_mu and one for ab_s_mu (bin 0 underflow, 1 .. 62
// interior, 63 overflow and NaN; timeline_bin), and two uint32: `inf`, the draws with i[g, j] = 1, and `cum`, the draws with
// i[g', j] = 1 for some g' <= g of g's chunk (timeline_cum: a mask over the packed words).  Per chain and individual `ninf[8]`,
// uint32: the draws by the number of infections at gaps <= last[j], [7] pooling 7 and more.  264 bytes per cell.
// A cell and all its counters belong to one lane, an individual's ninf row to one lane, a chain has its own planes, the update
// is a plain read-modify-write: no atomics of any kind, bit-reproducible whatever the launch shape.
//
// Layout.  The planes are internal and INDIVIDUAL-major like the diagnostics' (abd_diag.hpp), cell j G + g.  A cell's 64
// counters are one aligned 128-byte line, so a draw touches one 32-byte sector of the cell's line per antigen, and no line is
// ever shared by two lanes.  The lane increments the 32-bit word that holds its counter (by 1 or by 1 << 16): the words of a
// line are the lane's own, and a counter stops at planned_draws <= 65535, so nothing carries into its neighbour.  inf and cum
// are one 8-byte element.
//
// The bin rule, the chunk's mask and the cumulative bit are plain C++ shared with the CPU harness
// (tests/native/timeline_harness.cpp); the quantile of a pooled histogram is shared with the read-out kernel.
#pragma once

#include <math.h>

#include "abd_types.hpp"

#define ABD_TL_BINS 64           // counters per histogram: underflow, 62 interior bins, overflow
#define ABD_TL_MAX_DRAWS 65535   // what a 16-bit counter holds
#define ABD_TL_MAX_Q 8           // quantiles per read-out
#define ABD_TL_NINF 8            // bins of the number of infections

namespace abdi {

// a titer range [lo, hi) as the kernels take it: inv_w = 62 / (hi - lo) and w = (hi - lo) / 62, computed once by the host
struct TimelineRange {
  double lo, hi, inv_w, w;
};

__host__ __device__ inline TimelineRange timeline_range(double lo, double hi) {
  TimelineRange r;
  r.lo = lo, r.hi = hi;
  r.inv_w = (double)(ABD_TL_BINS - 2) / (hi - lo);
  r.w = (hi - lo) / (double)(ABD_TL_BINS - 2);
  return r;
}

// the bin of titer x: 0 below lo, 63 from hi on and for NaN, else 1 + min(61, floor((x - lo) * inv_w))
__host__ __device__ inline int timeline_bin(double x, double lo, double hi, double inv_w) {
  if (x < lo) return 0;
  if (!(x < hi)) return ABD_TL_BINS - 1;
  const double k = floor((x - lo) * inv_w);  // in [0, 62] up to rounding: lo <= x < hi
  return 1 + (k < (double)(ABD_TL_BINS - 3) ? (int)k : ABD_TL_BINS - 3);
}

// The first gap of g's chunk: chunk borders 0, splits..., G (n_splits <= 2 ascending splits s0, s1), so the largest of 0 and
// the splits that is <= g.
__host__ __device__ inline int timeline_chunk_start(int g, int n_splits, int s0, int s1) {
  int lo = 0;
  if (n_splits > 0 && g >= s0) lo = s0;
  if (n_splits > 1 && g >= s1) lo = s1;
  return lo;
}

// the gaps lo .. g (lo <= g) as a mask over packed word t (gaps 64 t .. 64 t + 63)
__host__ __device__ inline uint64_t timeline_span_mask(int t, int lo, int g) {
  const int rel = g - t * 64;  // bits <= rel of this word are gaps at or before g
  const uint64_t le = rel >= 63 ? ~0ull : (rel < 0 ? 0ull : ((2ull << rel) - 1ull));
  const int a = lo - t * 64;   // bits < a of this word are gaps before lo
  const uint64_t below = a <= 0 ? 0ull : (a >= 64 ? ~0ull : ((1ull << a) - 1ull));
  return le & ~below;
}

// 1 iff some bit of the individual's packed infections I is set at a gap g' <= g of g's chunk (0 <= g < 64 MT)
template <int MT>
__host__ __device__ inline uint32_t timeline_cum(int g, const uint64_t (&I)[MT], int n_splits, int s0, int s1) {
  const int lo = timeline_chunk_start(g, n_splits, s0, s1);
  bool hit = false;
#pragma unroll
  for (int t = 0; t < MT; ++t) hit |= (I[t] & timeline_span_mask(t, lo, g)) != 0;
  return hit ? 1u : 0u;
}

// The quantile q of a pooled histogram c[0..63] over [lo, hi) with bin width w: NaN for an empty one; with t = q n and b the
// smallest bin with c[b] > 0 and C[b] >= t (C the inclusive cumulative sums): lo for b = 0, hi for b = 63, else
// lo + w ((b - 1) + (t - C[b-1]) / c[b]).  timelines.quantiles is the same definition as NumPy.
__host__ __device__ inline double timeline_quantile(const uint32_t (&c)[ABD_TL_BINS], double q, double lo, double hi, double w) {
  uint32_t n = 0;
#pragma unroll
  for (int b = 0; b < ABD_TL_BINS; ++b) n += c[b];
  if (n == 0) return NAN;
  const double t = q * (double)n;
  int at = -1;
  uint32_t C = 0, before = 0, here = 0;
#pragma unroll
  for (int b = 0; b < ABD_TL_BINS; ++b) {
    const uint32_t Cb = C + c[b];
    if (at < 0 && c[b] > 0 && (double)Cb >= t) at = b, before = C, here = c[b];
    C = Cb;
  }
  // (t <= n = C[last populated bin]: a bin is always found)
  if (at == 0) return lo;
  if (at == ABD_TL_BINS - 1) return hi;
  return lo + w * ((double)(at - 1) + (t - (double)before) / (double)here);
}

struct alignas(8) TimelineCell {  // a cell of i
  uint32_t inf, cum;
};

}  // namespace abdi

#if defined(__HIPCC__)

#include "abd_cells.hpp"

// The launch's argument block: the walk and the timelines' own fields
struct TimelineArgs {
  CellWalk w;
  uint32_t* hist_n;       // the chain's [N * G][32] words = [N * G][64] 16-bit counters of ab_n_mu
  uint32_t* hist_s;       // ... of ab_s_mu
  abdi::TimelineCell* cell;  // [N * G]
  uint32_t* ninf;         // [N][8]
  abdi::TimelineRange rn, rs;
  int32_t n_splits, s0, s1;  // the chunks' inner borders
};

// One draw of one chain into its timeline counters.  The walk is abd_diag_kernel's and the titers are cell_titers
// (abd_cells.hpp), what abd_deterministics_kernel records: not a third formula.  Reads the slot's state and indicator words
// only: dense and list cohorts run the same code.
template <int MT>
__global__ __launch_bounds__(ABD_BLOCK) void abd_timeline_kernel(const TimelineArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const CellWalk& w = a.w;
  const int G = w.G, N = w.N, nt = w.nt;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const CellTables tabs = cell_tables(smem, w, tid);
  const int waves_total = gridDim.x * ABD_WAVES_PER_BLOCK;
  for (int j = blockIdx.x * ABD_WAVES_PER_BLOCK + wave; j < N; j += waves_total) {
    const int last = last_gap(w, j);
    uint64_t V[MT], I[MT];
    const double2_t* ts = load_individual<MT>(w, j, tabs, V, I);
    const int n_inf = followed_infections<MT>(I, last, nt);
    // the individual's row of ninf: one counter moves, its lane's (a never-followed individual's row stays 0)
    if (last >= 0 && lane == min(n_inf, ABD_TL_NINF - 1)) a.ninf[(int64_t)j * ABD_TL_NINF + lane] += 1u;
    for (int t = 0; t < nt; ++t) {
      const int g = t * 64 + lane;
      if (g < G) {
        const int64_t o = (int64_t)j * G + g;  // individual-major: the cell's own line in either histogram
        abdi::TimelineCell ci = a.cell[o];  // (in flight while the responses are summed)
        const CellTiters c = cell_titers<MT>(w, V, I, tabs.tab_n, ts, g, t + 1);
        const int bn = abdi::timeline_bin(c.mun, a.rn.lo, a.rn.hi, a.rn.inv_w);
        const int bs = abdi::timeline_bin(c.mus, a.rs.lo, a.rs.hi, a.rs.inv_w);
        uint32_t* wn = a.hist_n + o * (ABD_TL_BINS / 2) + (bn >> 1);
        uint32_t* ws = a.hist_s + o * (ABD_TL_BINS / 2) + (bs >> 1);
        const uint32_t hn = *wn, hs = *ws;
        ci.inf += (uint32_t)((I[t] >> lane) & 1ull);
        ci.cum += abdi::timeline_cum<MT>(g, I, a.n_splits, a.s0, a.s1);
        *wn = hn + (1u << ((bn & 1) * 16));
        *ws = hs + (1u << ((bs & 1) * 16));
        a.cell[o] = ci;
      }
    }
  }
}

// Gap rows [g0, g0 + n_g) of one individual-major histogram plane -> dst [n_g][N][64] 16-bit counters, the caller's gap-major
// order.  A cell's histogram is one 128-byte line on either side, so there is nothing to transpose inside it: eight lanes move
// a line, 16 bytes each, and both sides see whole lines.
__global__ __launch_bounds__(256) void abd_timeline_hist_export_kernel(const uint4* __restrict__ src, int G, int N, int g0, int n_g,
                                                                       uint4* __restrict__ dst) {
  const int64_t cells = (int64_t)n_g * N;
  const int part = threadIdx.x & 7;
  for (int64_t e = (int64_t)blockIdx.x * 32 + (threadIdx.x >> 3); e < cells; e += (int64_t)gridDim.x * 32) {
    const int gr = (int)(e / N), j = (int)(e - (int64_t)gr * N);
    dst[e * 8 + part] = src[((int64_t)j * G + g0 + gr) * 8 + part];
  }
}

#define ABD_TL_QTILE 16  // abd_timeline_quantile_kernel: a 16 x 16 tile of cells per 256-thread workgroup, one cell per thread

// Quantiles of the histograms pooled over the sampler's n chains (32-bit sums), per cell: out [n_q][G][N] doubles, gap-major.
// hist: chain k's plane at hist + k * chain_stride words.  A thread sums its cell's 64 counters over the chains in registers
// and evaluates timeline_quantile per q; the values go through an LDS tile so that reads run along g (the planes' order) and
// writes along j (the output's), as abd_diag_export_kernel does.  Rows are padded to 17 doubles = 34 banks.
__global__ __launch_bounds__(256) void abd_timeline_quantile_kernel(const uint32_t* __restrict__ hist, int64_t chain_stride, int n_chains,
                                                                    int G, int N, abdi::TimelineRange r, int n_q, const double* __restrict__ q,
                                                                    double* __restrict__ out) {
  __shared__ double tile[ABD_TL_QTILE][ABD_TL_QTILE + 1];
  const int tiles_g = (G + ABD_TL_QTILE - 1) / ABD_TL_QTILE;
  const int g0 = (int)(blockIdx.x % tiles_g) * ABD_TL_QTILE, j0 = (int)(blockIdx.x / tiles_g) * ABD_TL_QTILE;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int g = g0 + tx, j = j0 + ty;
  const bool have = g < G && j < N;
  uint32_t c[ABD_TL_BINS];
#pragma unroll
  for (int b = 0; b < ABD_TL_BINS; ++b) c[b] = 0u;
  if (have) {
    for (int k = 0; k < n_chains; ++k) {
      const uint4* line = reinterpret_cast<const uint4*>(hist + (int64_t)k * chain_stride + ((int64_t)j * G + g) * (ABD_TL_BINS / 2));
#pragma unroll
      for (int v = 0; v < ABD_TL_BINS / 8; ++v) {
        const uint4 w = line[v];
        const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          c[8 * v + 2 * e] += ws[e] & 0xffffu;
          c[8 * v + 2 * e + 1] += ws[e] >> 16;
        }
      }
    }
  }
  const int go = g0 + ty, jo = j0 + tx;  // the cell this thread writes
  for (int iq = 0; iq < n_q; ++iq) {
    if (have) tile[ty][tx] = abdi::timeline_quantile(c, q[iq], r.lo, r.hi, r.w);
    __syncthreads();
    if (go < G && jo < N) out[((int64_t)iq * G + go) * N + jo] = tile[tx][ty];
    __syncthreads();
  }
}

#endif  // __HIPCC__
