// abd_planes.hpp -- exposure planes: a chain slot's discrete state transposed for the dense gap loop (host + device).
//
// The gap loop of abd_dense.hpp walks one gap row of 64 individuals (a lane group) per step.  What it needs of the discrete
// state in that step is, per lane, one bit of the constrained infections and one of the vaccinations -- and whether the lane's
// individual has been exposed before (abd.py:306).  All of that is a function of the chain's discrete state alone, which
// changes once per sweep and not once per evaluation, so it is kept TRANSPOSED beside `iw`: for every (lane group, gap) one
// 64-bit lane mask of the constrained infections and one of the vaccinations (abd_types.hpp: PlaneGap).  A wave fetches the
// masks of a gap with one 16-byte scalar load, a pair of gaps ahead, and keeps "exposed so far" as two lane masks in scalar
// registers.
//
// Here: the layout's index functions, the tile transpose as a reference loop (the device does it with ballots:
// abd_small.hpp: abd_planes_kernel), the exposure bookkeeping of one gap and the steps that turn the running H sums into
// the perm sums and the loop's scalar index steps in plain C++ -- the same functions run in the kernel and in
// tests/native/planes_harness.cpp, hc_sum_harness.cpp, plane_fetch_harness.cpp.
#pragma once

#include "abd_types.hpp"

// gaps per lane group in a plane: G rounded up to even (a pair of gaps is 32 aligned bytes) plus one pair of zeros
// (the loop fetches one pair ahead: the last fetch of a row reads gaps <= G + 1)
__host__ __device__ inline int abd_plane_gaps(int G) { return ((G + 1) & ~1) + 2; }
// 64-bit words of one slot's planes
__host__ __device__ inline size_t abd_plane_words(int n_lg, int G) { return (size_t)n_lg * (size_t)abd_plane_gaps(G) * 2; }
// index of the lane mask of (lane group lg, gap g): which = 0 the constrained infections, 1 the vaccinations
__host__ __device__ inline size_t abd_plane_index(int lg, int g, int G, int which) {
  return ((size_t)lg * (size_t)abd_plane_gaps(G) + (size_t)g) * 2 + (size_t)which;
}

// ---- the scalar bookkeeping of the plane form's gap loop (abd_dense.hpp: dense_walk_planes) ----
// The loop walks a piece [g0, g1) of a row a pair of gaps at a time and refills its row buffers two gaps ahead, so near the
// piece's end it asks for rows past the last one; those loads are aimed at the last row instead (they are never used).  The
// offset of the row to load is kept running and clamped, one add and one min per row, instead of being worked out from the
// gap index (add, min, multiply, shift): `off` is the offset of row min(r, last) in any unit, `step` one row in that unit,
// `last_off` = last * step.  A clamped offset stays clamped: min(min(u, L) + s, L) = min(u + s, L) for s >= 0.
__host__ __device__ inline uint32_t abd_row_off_next(uint32_t off, uint32_t step, uint32_t last_off) {
  const uint32_t n = off + step;
  return n < last_off ? n : last_off;
}
// The masks of a pair of gaps are fetched one pair ahead, from a pointer that advances by a pair: the first fetch of a piece is
// the pair that holds its first even gap, and the last one reads the pair after the last pair it walks -- at most gaps G and
// G + 1, inside the row's padding (abd_plane_gaps).
__host__ __device__ inline int abd_plane_first_pair(int g0) { return (g0 + 1) & ~1; }

// Reference transpose: words [nt][N] (word t of individual j: gaps 64 t .. 64 t + 63, as rw / iw / vw) -> the `which` masks
// of planes [n_lg][abd_plane_gaps(G)] (everything else is left as it is).  Bit l of the mask of (lg, g) = bit g of
// individual 64 lg + l; lanes past the last individual and gaps past G - 1 stay zero.
inline void abd_plane_transpose_ref(const uint64_t* words, int N, int G, int which, uint64_t* planes) {
  const int n_lg = (N + 63) / 64;
  for (int lg = 0; lg < n_lg; ++lg)
    for (int g = 0; g < G; ++g) {
      uint64_t m = 0;
      for (int l = 0; l < 64; ++l) {
        const int j = lg * 64 + l;
        if (j < N) m |= ((words[(size_t)(g >> 6) * N + j] >> (g & 63)) & 1ull) << l;
      }
      planes[abd_plane_index(lg, g, G, which)] = m;
    }
}

// ---- exposure bookkeeping of one gap (abd.py:306: perm_response) ----
// seen.n: lanes whose individual has had an infection in a gap walked so far; seen.s: an infection or a vaccination (a
// vaccination exposes S but not N).  The gap of the first exposure itself already counts: the flags are updated BEFORE the
// gap's titers are formed.
struct ExposureSeen {
  uint64_t n, s;
};
// how a piece's start state seeds them: lanes with an infection / a vaccination in a gap before the piece's first
// (abd_dense.hpp: dense_start_state; a piece that starts at gap 0 of a lane group starts from {0, 0})
__host__ __device__ inline ExposureSeen abd_exposure_start(uint64_t infected_before, uint64_t vaccinated_before) {
  ExposureSeen s;
  s.n = infected_before;
  s.s = infected_before | vaccinated_before;
  return s;
}
// the lanes that gap's masks expose for the FIRST time (n: N antigen, s: S antigen); both zero in most gaps
__host__ __device__ inline ExposureSeen abd_exposure_new(const ExposureSeen& seen, uint64_t m_i, uint64_t m_v) {
  ExposureSeen nw;
  nw.n = m_i & ~seen.n;
  nw.s = (m_i | m_v) & ~seen.s;
  return nw;
}
__host__ __device__ inline void abd_exposure_mark(ExposureSeen& seen, uint64_t m_i, uint64_t m_v) {
  seen.n |= m_i;
  seen.s |= m_i | m_v;
}

// ---- the perm sums from the H sums (abd_terms.hpp: A_N_HC, A_S_HC) ----
// sum over a piece's gaps of h cf, cf = "exposed so far" in {0, 1}, is per lane the lane's H sum over the gaps from its first
// exposure on: H at the piece's end minus H just before the first-exposure gap's h was added.  The difference is taken in the
// HC accumulator itself, with H the running accumulator (it goes on across the pieces of a range), in three steps:
//   1. piece start:  a lane exposed before the piece            HC <- HC - H      (abd_hc_open)
//   2. the gap of a lane's first exposure inside the piece,
//      before that gap's h is added                              HC <- HC - H      (abd_hc_open)
//   3. piece end:    a lane exposed by then                      HC <- HC + H      (abd_hc_close)
// Each is one rounded fp64 add under a lane select; a lane that is never exposed keeps HC as it was (exactly 0.0 from zero).
// Both forms of the gap loop and tests/native/hc_sum_harness.cpp call these.
__host__ __device__ inline double abd_hc_open(double hc, double H, bool lane_on) {
  const double d = hc - H;
  return lane_on ? d : hc;
}
__host__ __device__ inline double abd_hc_close(double hc, double H, bool lane_on) {
  const double d = hc + H;
  return lane_on ? d : hc;
}

// High word of the S boost e_i + e_v in {0.0, 1.0, 2.0} (unit boosts, abd.py:272) from "either" and "both" of the gap's
// infection and vaccination indicators (the low word is zero): two selects instead of an fp64 add, the same double bit for bit.
__host__ __device__ inline uint32_t abd_s_boost_hi(bool either, bool both) {
  const uint32_t one = either ? 0x3FF00000u : 0u;
  return both ? 0x40000000u : one;
}
