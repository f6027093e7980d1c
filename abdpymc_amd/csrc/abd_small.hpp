// abd_small.hpp -- the small kernels of the context: packing / unpacking / flipping the discrete state, the recorded
// Deterministics (abd.py:649/667, 341, 389-391), the hardware-queue probe.
#pragma once

#include "abd_cells.hpp"
#include "abd_planes.hpp"

// One wave that stays on the device for `ticks` of the 100 MHz s_memrealtime counter and says when (abd_context.hip:
// probe_stream_queues -- which of the context's HIP streams can have kernels on the device at the same time)
__global__ void abd_spin_kernel(unsigned long long* out, unsigned long long ticks) {
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  unsigned long long t = t0;
  while (t - t0 < ticks) {
    __builtin_amdgcn_s_sleep(16);
    t = __builtin_amdgcn_s_memrealtime();
  }
  if (threadIdx.x == 0) {
    out[0] = t0;
    out[1] = t;
  }
}

// (G, N) gap-major int8 (PyMC's i_raw, or vacs.T / pcrpos.T) -> packed words [nt][N]
__global__ __launch_bounds__(256) void abd_pack_bits_kernel(const int8_t* __restrict__ src, uint64_t* __restrict__ dst,
                                                            int G, int N, int nt) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const int t = blockIdx.y;
  if (j >= N || t >= nt) return;
  uint64_t w = 0;
  const int g_end = min(64, G - t * 64);
  for (int b = 0; b < g_end; ++b) w |= (uint64_t)(src[(int64_t)(t * 64 + b) * N + j] != 0) << b;  // coalesced over j
  dst[(int64_t)t * N + j] = w;
}

// What the integer pre-pass needs besides the words (a 2 KB EvalArgs is not passed for it)
struct ConstrainArgs {
  const uint64_t* pw;  // [nt][N] packed pcrpos, nullptr = ignore_pcrpos
  int32_t N, nt, n_chunks, pad_;
  uint64_t chunk_mask[3][ABD_MAXT_MAX];
};

// Refresh a chain slot's cached state from its raw discrete state: iw = constrain(rw, pcrpos) (abd.py:640-667) for every
// individual, cnt[0] += sum(i_raw), cnt[1] += sum(ab_s_waner) (the caller zeroes cnt; integer adds: order-free).
template <int MT>
__global__ __launch_bounds__(256) void abd_constrain_kernel(const ConstrainArgs a, const uint64_t* __restrict__ rw,
                                                            const int8_t* __restrict__ waner, uint64_t* __restrict__ iw,
                                                            unsigned long long* cnt) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  int n1 = 0, m1 = 0;
  if (j < a.N) {
    uint64_t P[MT], Rw[MT], I[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      P[t] = Rw[t] = 0;
      if (t < a.nt) {
        Rw[t] = rw[(int64_t)t * a.N + j];
        if (a.pw) P[t] = a.pw[(int64_t)t * a.N + j];
        n1 += __builtin_popcountll(Rw[t]);
      }
    }
    constrain_masks<MT>(Rw, P, a, I);
#pragma unroll
    for (int t = 0; t < MT; ++t)
      if (t < a.nt) iw[(int64_t)t * a.N + j] = I[t];
    m1 = waner[j] != 0;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    n1 += __shfl_xor(n1, off, 64);
    m1 += __shfl_xor(m1, off, 64);
  }
  if ((threadIdx.x & 63) == 0 && (n1 | m1)) {
    atomicAdd(cnt + 0, (unsigned long long)n1);
    atomicAdd(cnt + 1, (unsigned long long)m1);
  }
}

// One proposed flip of the resident state (abd_flip_discrete): the bit, its individual's constrained words, the counters
template <int MT>
__global__ void abd_flip_kernel(const ConstrainArgs a, uint64_t* rw, int8_t* waner, uint64_t* iw, unsigned long long* cnt, int G,
                                int64_t flat) {
  const int N = a.N;
  const int64_t gn = (int64_t)G * N;
  if (flat < gn) {
    const int64_t g = flat / N, j = flat % N;
    const uint64_t bit = 1ull << (g & 63);
    const uint64_t w = rw[(g >> 6) * N + j] ^ bit;
    rw[(g >> 6) * N + j] = w;
    cnt[0] += (w & bit) ? 1ull : ~0ull;  // +1 / -1
    uint64_t P[MT], Rw[MT], I[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      P[t] = Rw[t] = 0;
      if (t < a.nt) {
        Rw[t] = rw[(int64_t)t * N + j];
        if (a.pw) P[t] = a.pw[(int64_t)t * N + j];
      }
    }
    constrain_masks<MT>(Rw, P, a, I);
#pragma unroll
    for (int t = 0; t < MT; ++t)
      if (t < a.nt) iw[(int64_t)t * N + j] = I[t];
  } else {
    const int8_t w = waner[flat - gn] ^ 1;
    waner[flat - gn] = w;
    cnt[1] += w ? 1ull : ~0ull;
  }
}

// Exposure planes (abd_planes.hpp) of up to ABD_MAX_BATCH_K slots from their packed words: 64 x 64-bit tiles transposed with
// ballots, one wave per (lane group, 64-gap word, slot) -- grid (lane groups from lg0 on, nt, slots).  Launched stream-ordered
// behind every writer of iw: a writer cannot update the planes itself, since neighbouring individuals share a 64-bit mask
// and per-individual writers would race.  which = 0: src = iw, the infection masks; 1: src = vw, the vaccination masks.
struct PlaneArgs {
  const uint64_t* src[ABD_MAX_BATCH_K];  // [nt][N]
  uint64_t* dst[ABD_MAX_BATCH_K];        // [n_lg][abd_plane_gaps(G)][2]
  int32_t N, G, which, lg0;
};
__global__ __launch_bounds__(64) void abd_planes_kernel(const PlaneArgs a) {
  const int lane = threadIdx.x, lg = a.lg0 + (int)blockIdx.x, t = blockIdx.y, k = blockIdx.z;
  const int j = lg * 64 + lane;
  const uint64_t w = j < a.N ? a.src[k][(int64_t)t * a.N + j] : 0ull;  // lane = individual
  uint64_t mine = 0;
  for (int b = 0; b < 64; ++b) {
    const uint64_t m = __builtin_amdgcn_ballot_w64(((w >> b) & 1ull) != 0);
    if (lane == b) mine = m;  // lane = gap
  }
  const int g = t * 64 + lane;
  if (g < a.G) a.dst[k][abd_plane_index(lg, g, a.G, a.which)] = mine;
}

// Deterministics "i", "ab_n_mu", "ab_s_mu" for one chain, written (G, N) gap-major as PyMC records them;
// with `sums` ([3][G*N]: i, ab_n_mu, ab_s_mu) they are also added to running sums (posterior means on device).
// The titers are cell_titers (abd_cells.hpp): the per-draw summaries reduce the same values.
template <int MT>
__global__ __launch_bounds__(ABD_BLOCK) void abd_deterministics_kernel(const CellWalk w, int8_t* __restrict__ out_i,
                                                                       double* __restrict__ out_mun,
                                                                       double* __restrict__ out_mus,
                                                                       double* __restrict__ sums) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int G = w.G, N = w.N, nt = w.nt;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const CellTables tabs = cell_tables(smem, w, tid);
  const int waves_total = gridDim.x * ABD_WAVES_PER_BLOCK;
  for (int j = blockIdx.x * ABD_WAVES_PER_BLOCK + wave; j < N; j += waves_total) {
    uint64_t V[MT], I[MT];
    const double2_t* ts = load_individual<MT>(w, j, tabs, V, I);
    for (int t = 0; t < nt; ++t) {
      const int g = t * 64 + lane;
      if (g < G) {
        const CellTiters c = cell_titers<MT>(w, V, I, tabs.tab_n, ts, g, t + 1);
        const int64_t o = (int64_t)g * N + j;
        const int bit = (int)((I[t] >> lane) & 1ull);
        if (out_i) out_i[o] = (int8_t)bit;
        if (out_mun) out_mun[o] = c.mun;
        if (out_mus) out_mus[o] = c.mus;
        if (sums) {
          const int64_t cells = (int64_t)G * N;
          sums[o] += (double)bit;
          sums[cells + o] += c.mun;
          sums[2 * cells + o] += c.mus;
        }
      }
    }
  }
}

// packed words [nt][N] -> (G, N) gap-major int8, for reading a chain's i_raw back
__global__ __launch_bounds__(256) void abd_unpack_bits_kernel(const uint64_t* __restrict__ src, int8_t* __restrict__ dst,
                                                              int G, int N) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const int g = blockIdx.y;
  if (j < N && g < G) dst[(int64_t)g * N + j] = (int8_t)((src[(int64_t)(g >> 6) * N + j] >> (g & 63)) & 1ull);
}

