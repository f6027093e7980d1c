// plane_fetch_harness.cpp -- the scalar side of the plane form of the dense gap loop (abd_dense.hpp: dense_walk_planes) on the
// CPU (tests/test_plane_fetch.py): where it fetches its lane masks and which rows it loads.  The loop keeps one set of masks for
// the even and one for the odd gap of a pair, refills each for the next pair right behind its use from a running pointer, and
// refills its row buffers two gaps ahead from a running, clamped offset (abd_planes.hpp: abd_plane_first_pair,
// abd_row_off_next).  The walk below is the kernel's, fetch for fetch and load for load, on a row buffer of exactly
// abd_plane_gaps(G) gaps.  Checked: every gap a fetch touches lies inside the row; the masks handed to gap g are those a direct
// read of gap g gives; the row loaded for gap g + 2 is row min(g + 2, g1 - 1) of the piece, by offset.  With
// -DPLANE_FETCH_HARNESS_MAIN a stand-alone program (built with host ASan + UBSan: the row is a heap block of its exact size).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "abd_planes.hpp"

namespace {

struct Gap {
  uint64_t i, v;
};

// the masks of gap g of the test row: distinct for every (gap, which), never zero inside the row
inline uint64_t mask_of(int g, int which) { return 0x9E3779B97F4A7C15ull * (uint64_t)(2 * g + which + 1) | 1ull; }

struct Walk {
  const Gap* row;  // [abd_plane_gaps(G)]
  int G, gaps;
  uint32_t row_step;  // one row, in the offset's unit
  long long bad = 0, fetches = 0, loads = 0, clamped = 0;
  int max_gap = -1;      // the last gap any fetch touched
  int* trace = nullptr;  // (optional) the gap of every fetch, in order
  int n_trace = 0;
  int g0 = 0, g1 = 0;

  Gap fetch(int g) {
    if (g > max_gap) max_gap = g;
    if (trace) trace[n_trace++] = g;
    ++fetches;
    if (g < 0 || g >= gaps) {
      ++bad;
      return Gap{0, 0};  // (counted; not read)
    }
    return row[g];
  }
  // a gap of the walk gets these masks
  void step(int g, const Gap& m) {
    if (g < g0 || g >= g1 || g >= G) {
      ++bad;
      return;
    }
    if (m.i != row[g].i || m.v != row[g].v) ++bad;
    if (m.i != mask_of(g, 0) || m.v != mask_of(g, 1)) ++bad;
  }
  // a row buffer is refilled for gap g_for from offset off
  void load(int g_for, uint32_t off) {
    const int last = g1 - 1 - g0;
    const int want = g_for - g0 < last ? g_for - g0 : last;
    if (off != (uint32_t)want * row_step) ++bad;
    clamped += g_for - g0 > last;
    ++loads;
  }
  // dense_walk_planes, the scalar side of it
  int walk(int a, int b) {
    g0 = a;
    g1 = b;
    const uint32_t row_last = (uint32_t)(g1 - 1 - g0) * row_step;
    uint32_t off = 2u * row_step < row_last ? 2u * row_step : row_last;
    int f = abd_plane_first_pair(g0);  // the fetch pointer, as a gap
    Gap me = fetch(f), mo = fetch(f + 1);
    int left = g1 - g0, g = g0, steps = 0;
    if (g0 & 1) {
      step(g, fetch(g0));
      load(g + 2, off);
      off = abd_row_off_next(off, row_step, row_last);
      --left;
      ++g;
      ++steps;
    }
    for (int pairs = left >> 1; pairs > 0; --pairs) {
      step(g, me);
      me = fetch(f + 2);
      load(g + 2, off);
      off = abd_row_off_next(off, row_step, row_last);
      step(g + 1, mo);
      mo = fetch(f + 3);
      load(g + 3, off);
      off = abd_row_off_next(off, row_step, row_last);
      f += 2;
      g += 2;
      steps += 2;
    }
    if (left & 1) {
      step(g, me);
      ++steps;
    }
    return steps;
  }
};

// a row of exactly abd_plane_gaps(G) gaps on the heap: gaps < G distinct, the padding zero (as a slot's planes have it)
std::vector<Gap> make_row(int G) {
  std::vector<Gap> row((size_t)abd_plane_gaps(G));
  for (int g = 0; g < (int)row.size(); ++g) row[(size_t)g] = g < G ? Gap{mask_of(g, 0), mask_of(g, 1)} : Gap{0, 0};
  return row;
}

Walk make_walk(const std::vector<Gap>& row, int G, uint32_t row_step) {
  Walk w;
  w.row = row.data();
  w.G = G;
  w.gaps = (int)row.size();
  w.row_step = row_step;
  return w;
}

}  // namespace

extern "C" {

int plane_fetch_gaps(int G) { return abd_plane_gaps(G); }
int plane_fetch_first_pair(int g0) { return abd_plane_first_pair(g0); }
unsigned plane_fetch_row_off_next(unsigned off, unsigned step, unsigned last_off) { return abd_row_off_next(off, step, last_off); }

// One piece [g0, g1) of a row of G gaps, rows row_step apart.  trace (may be NULL; room for g1 - g0 + 5 entries): the gap of
// every fetch in order.  out[0] = fetches, out[1] = the last gap a fetch touched, out[2] = gaps walked, out[3] = row loads.
// Returns the number of violations: a fetch outside the row, masks that are not the gap's, a row load from another offset.
long long plane_fetch_piece(int G, int g0, int g1, unsigned row_step, int* trace, long long* out) {
  const std::vector<Gap> row = make_row(G);
  Walk w = make_walk(row, G, row_step);
  w.trace = trace;
  const int steps = w.walk(g0, g1);
  out[0] = w.fetches;
  out[1] = w.max_gap;
  out[2] = steps;
  out[3] = w.loads;
  return w.bad + (steps != g1 - g0);
}

// Every piece [g0, g1) with 0 <= g0 < g1 <= G.  out[0] = pieces, out[1] = fetches, out[2] = the last gap any fetch touched,
// out[3] = row loads that were aimed at the piece's last row instead of a row past it.  Returns the violations over all.
long long plane_fetch_all_pieces(int G, unsigned row_step, long long* out) {
  const std::vector<Gap> row = make_row(G);
  long long bad = 0, pieces = 0, fetches = 0, clamped = 0;
  int max_gap = -1;
  for (int g0 = 0; g0 < G; ++g0)
    for (int g1 = g0 + 1; g1 <= G; ++g1) {
      Walk w = make_walk(row, G, row_step);
      const int steps = w.walk(g0, g1);
      bad += w.bad + (steps != g1 - g0);
      ++pieces;
      fetches += w.fetches;
      clamped += w.clamped;
      if (w.max_gap > max_gap) max_gap = w.max_gap;
    }
  out[0] = pieces;
  out[1] = fetches;
  out[2] = max_gap;
  out[3] = clamped;
  return bad;
}

}  // extern "C"

#ifdef PLANE_FETCH_HARNESS_MAIN
int main() {
  long long bad = 0, pieces = 0;
  for (int G = 1; G <= 70; ++G)
    for (unsigned row_step : {64u, 70u * 16u, 10000u * 16u}) {
      long long out[4];
      bad += plane_fetch_all_pieces(G, row_step, out);
      bad += out[0] != (long long)G * (G + 1) / 2;
      bad += out[2] >= abd_plane_gaps(G);
      pieces += out[0];
    }
  std::printf(bad ? "plane fetch harness: %lld violations\n" : "plane fetch harness ok (%lld pieces)\n", bad ? bad : pieces);
  return bad ? 1 : 0;
}
#endif
