// abd_diag.hpp -- per-cell convergence accumulators over ALL draws of a chain (abd_sampler_enable_diagnostics,
// abd_sampler_diagnostics; include/abd_hip.h has the definition in full): what split R-hat and a batch-means ESS of
// "i", "ab_n_mu", "ab_s_mu" need -- second moments per half-chain and the moments of the batch means -- kept on the device,
// because at the sizes this project is for a run never keeps its draws.
//
// Per chain and cell, for each of the two titers seven doubles (Welford mean and M2 of either half; the running batch sum
// `cur`; Welford mean and M2 of the closed batches' means) and for i, whose moments are functions of counts, four uint32 (ones
// in either half, the running batch count, the sum of the closed batches' counts) and a uint64 (the sum of their squares):
// 136 bytes.  A cell belongs to one lane, a chain has its own planes, the update is a fixed-order read-modify-write: no
// atomics of any kind, bit-reproducible whatever the launch shape.
//
// Layout.  The planes are internal, so they are laid out for the hardware: INDIVIDUAL-major, cell j G + g, one plane per
// quantity.  abd_diag_kernel has the shape of abd_deterministics_kernel (one wave per individual, lanes over gaps), so a wave's
// 64 lanes touch 512 contiguous bytes of a plane (the running sums' gap-major planes put N doubles between two lanes).  The
// four uint32 of i are one 16-byte element.  abd_diag_export_kernel turns a plane into the caller's (G, N) order at read-out.
//
// The per-cell update and the draw's flags are plain C++ shared with the CPU harness (tests/native/diag_harness.cpp).
#pragma once

#include "abd_types.hpp"

namespace abdi {

// planes of one titer, in the order they are stored
enum { kDiagMean0 = 0, kDiagM20, kDiagMean1, kDiagM21, kDiagCur, kDiagBmMean, kDiagBmM2, kDiagTiterPlanes };

// What a draw is to the accumulators: a function of its index d = iteration - tune, the half length H and the batch length L
// alone, so that cutting a run into several calls changes nothing.
struct DiagDraw {
  double inv_n;    // 1 / (the draw's 1-based place in its half)
  double inv_L;    // 1 / L
  double inv_b;    // 1 / (batches closed so far in this chain, both halves pooled, this draw's included)
  int32_t half;    // 0, 1
  int32_t in_batch;        // the draw belongs to one of the half's B = H / L whole batches (the trailing H % L draws do not)
  int32_t first_of_batch;  // cur = x, not cur += x
  int32_t close_batch;     // the batch's mean enters bm_mean / bm_M2
};

// d in [0, 2 H), H >= 1, L >= 1
__host__ __device__ inline DiagDraw diag_draw(int64_t d, int64_t H, int64_t L) {
  DiagDraw w;
  const int64_t B = H / L;
  w.half = d >= H ? 1 : 0;
  const int64_t p = d - (w.half ? H : 0);
  w.inv_n = 1.0 / (double)(p + 1);
  w.inv_L = 1.0 / (double)L;
  w.in_batch = p < B * L ? 1 : 0;
  w.first_of_batch = (w.in_batch && p % L == 0) ? 1 : 0;
  w.close_batch = (w.in_batch && p % L == L - 1) ? 1 : 0;
  w.inv_b = 1.0 / (double)((w.half ? B : 0) + p / L + 1);
  return w;
}

struct DiagTiter {  // a cell of one titer: mean, M2 of the draw's half; what the draw does not touch is neither read nor written
  double mean, M2, cur, bm_mean, bm_M2;
};

__host__ __device__ inline void diag_update_titer(DiagTiter& c, double x, const DiagDraw& w) {
  const double d = x - c.mean;
  c.mean += d * w.inv_n;
  c.M2 += d * (x - c.mean);
  if (!w.in_batch) return;
  c.cur = w.first_of_batch ? x : c.cur + x;
  if (!w.close_batch) return;
  const double bm = c.cur * w.inv_L;
  const double e = bm - c.bm_mean;
  c.bm_mean += e * w.inv_b;
  c.bm_M2 += e * (bm - c.bm_mean);
}

struct alignas(16) DiagInf {  // a cell of i
  uint32_t c_h0, c_h1, cur, sum_cb;
};

__host__ __device__ inline void diag_update_inf(DiagInf& c, unsigned long long& sum_cb2, uint32_t bit, const DiagDraw& w) {
  if (w.half)
    c.c_h1 += bit;
  else
    c.c_h0 += bit;
  if (!w.in_batch) return;
  c.cur = w.first_of_batch ? bit : c.cur + bit;
  if (!w.close_batch) return;
  c.sum_cb += c.cur;
  sum_cb2 += (unsigned long long)c.cur * c.cur;
}

}  // namespace abdi

#if defined(__HIPCC__)

#include "abd_cells.hpp"

// The launch's argument block: the walk and the accumulators' own fields (the draw in front of the pointers: fewer scalar
// spills; tools/resource_usage.py)
struct DiagArgs {
  CellWalk w;
  abdi::DiagDraw d;
  double* tit;            // the chain's [2][kDiagTiterPlanes][N * G] planes: ab_n_mu, then ab_s_mu
  abdi::DiagInf* inf;     // [N * G]
  unsigned long long* cb2;  // [N * G]
};

// One draw of one chain into its accumulators.  The titers are cell_titers (abd_cells.hpp), what abd_deterministics_kernel
// records: not a second formula.  Reads the slot's state and indicator words only: dense and list cohorts run the same code.
template <int MT>
__global__ __launch_bounds__(ABD_BLOCK) void abd_diag_kernel(const DiagArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const CellWalk& cw = a.w;
  const int G = cw.G, N = cw.N, nt = cw.nt;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const CellTables tabs = cell_tables(smem, cw, tid);
  const abdi::DiagDraw w = a.d;
  const int64_t cells = (int64_t)G * N;
  const int half_at = w.half ? abdi::kDiagMean1 : abdi::kDiagMean0;
  const int waves_total = gridDim.x * ABD_WAVES_PER_BLOCK;
  for (int j = blockIdx.x * ABD_WAVES_PER_BLOCK + wave; j < N; j += waves_total) {
    uint64_t V[MT], I[MT];
    const double2_t* ts = load_individual<MT>(cw, j, tabs, V, I);
    for (int t = 0; t < nt; ++t) {
      const int g = t * 64 + lane;
      if (g < G) {
        const int64_t o = (int64_t)j * G + g;  // individual-major: the wave's lanes are neighbours in every plane
        // the loads first, so that they are in flight while the responses are summed
        abdi::DiagTiter c[2] = {};
        for (int v = 0; v < 2; ++v) {
          double* pl = a.tit + (int64_t)v * abdi::kDiagTiterPlanes * cells + o;
          c[v].mean = pl[(half_at + 0) * cells];
          c[v].M2 = pl[(half_at + 1) * cells];
          if (w.in_batch && !w.first_of_batch) c[v].cur = pl[abdi::kDiagCur * cells];
          if (w.close_batch) {
            c[v].bm_mean = pl[abdi::kDiagBmMean * cells];
            c[v].bm_M2 = pl[abdi::kDiagBmM2 * cells];
          }
        }
        abdi::DiagInf ci = a.inf[o];
        unsigned long long cb2 = w.close_batch ? a.cb2[o] : 0ull;
        const CellTiters ct = cell_titers<MT>(cw, V, I, tabs.tab_n, ts, g, t + 1);
        const uint32_t bit = (uint32_t)((I[t] >> lane) & 1ull);
        const double x[2] = {ct.mun, ct.mus};
        for (int v = 0; v < 2; ++v) {
          abdi::diag_update_titer(c[v], x[v], w);
          double* pl = a.tit + (int64_t)v * abdi::kDiagTiterPlanes * cells + o;
          pl[(half_at + 0) * cells] = c[v].mean;
          pl[(half_at + 1) * cells] = c[v].M2;
          if (w.in_batch) pl[abdi::kDiagCur * cells] = c[v].cur;
          if (w.close_batch) {
            pl[abdi::kDiagBmMean * cells] = c[v].bm_mean;
            pl[abdi::kDiagBmM2 * cells] = c[v].bm_M2;
          }
        }
        abdi::diag_update_inf(ci, cb2, bit, w);
        a.inf[o] = ci;
        if (w.close_batch) a.cb2[o] = cb2;
      }
    }
  }
}

#define ABD_DIAG_TILE 32  // abd_diag_export_kernel: a 32 x 32 tile per 256-thread workgroup, eight rows per pass

// One individual-major plane -> the caller's (G, N) gap-major order, 8 bytes per cell, through an LDS tile: rows of the tile
// are read along g (contiguous in the plane) and written along j (contiguous in the output).  The tile's rows are padded to 33
// elements = 66 banks of 4 bytes: the 32 lanes that read a column hit banks 2 tx + 2 c (+ 1), all different.
// src: the plane's first element; elements `stride` bytes apart; width 8: copied as they are; width 4: a uint32, widened.
__global__ __launch_bounds__(256) void abd_diag_export_kernel(const unsigned char* __restrict__ src, int stride, int width, int G, int N,
                                                              unsigned long long* __restrict__ dst) {
  __shared__ unsigned long long tile[ABD_DIAG_TILE][ABD_DIAG_TILE + 1];
  const int tiles_g = (G + ABD_DIAG_TILE - 1) / ABD_DIAG_TILE;
  const int g0 = (int)(blockIdx.x % tiles_g) * ABD_DIAG_TILE, j0 = (int)(blockIdx.x / tiles_g) * ABD_DIAG_TILE;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < ABD_DIAG_TILE; r += 8) {
    const int j = j0 + r, g = g0 + tx;
    if (j < N && g < G) {
      const unsigned char* p = src + ((int64_t)j * G + g) * stride;
      tile[r][tx] = width == 8 ? *reinterpret_cast<const unsigned long long*>(p) : (unsigned long long)*reinterpret_cast<const uint32_t*>(p);
    }
  }
  __syncthreads();
  for (int r = ty; r < ABD_DIAG_TILE; r += 8) {
    const int g = g0 + r, j = j0 + tx;
    if (g < G && j < N) dst[(int64_t)g * N + j] = tile[tx][r];
  }
}

#endif  // __HIPCC__
