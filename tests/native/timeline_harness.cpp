// CPU harness for the shared rules of abd_timeline.hpp (tests/test_timelines_cpu.py): a stand-alone program that checks the
// bin rule, the chunk's mask and the cumulative bit -- the source the kernel compiles -- against brute-force restatements,
// and replays a file of titers and quantile levels through timeline_bin / timeline_quantile for the NumPy side to compare.
// Built with g++, plain and with -fsanitize=address,undefined.
//
//   timeline_harness                 the self-checks only
//   timeline_harness IN OUT          ... and the replay
//   IN:  double lo, hi; int64 D, Q; double x[D]; double q[Q]
//   OUT: int64 bin[D]; int64 hist[64]; double quantile[Q]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "abd_timeline.hpp"

using namespace abdi;

namespace {

int g_failed = 0;

void expect(bool ok, const char* what, double a = 0, double b = 0, double c = 0) {
  if (ok) return;
  if (++g_failed <= 20) std::fprintf(stderr, "FAILED %s (%.17g, %.17g, %.17g)\n", what, a, b, c);
}

// the rule restated without a multiplication by the reciprocal's closed form: a linear search over the interior bins' own
// test floor((x - lo) * inv_w) == k, after the three special cases
int bin_brute(double x, double lo, double hi) {
  if (std::isnan(x)) return 63;
  if (x < lo) return 0;
  if (x >= hi) return 63;
  const double inv_w = 62.0 / (hi - lo);
  const double v = (x - lo) * inv_w;
  for (int k = 0; k < 61; ++k)
    if (v >= (double)k && v < (double)(k + 1)) return 1 + k;
  return 62;  // floor(v) >= 61: the last interior bin
}

void check_bins(double lo, double hi) {
  const TimelineRange r = timeline_range(lo, hi);
  expect(r.inv_w == 62.0 / (hi - lo) && r.w == (hi - lo) / 62.0, "timeline_range", lo, hi);
  const double inf = std::numeric_limits<double>::infinity();
  std::vector<double> xs = {-inf, inf, std::nan(""), lo, hi, 0.0, -0.0, std::numeric_limits<double>::max(), std::numeric_limits<double>::lowest()};
  for (int k = 0; k <= 62; ++k) xs.push_back(lo + r.w * k), xs.push_back(lo + (hi - lo) * k / 62.0), xs.push_back(lo + r.w * (k + 0.5));
  const size_t n = xs.size();
  for (size_t e = 0; e < n; ++e) {
    if (!std::isfinite(xs[e])) continue;
    xs.push_back(std::nextafter(xs[e], -inf));
    xs.push_back(std::nextafter(xs[e], inf));
  }
  for (double x : xs) {
    const int b = timeline_bin(x, r.lo, r.hi, r.inv_w);
    expect(b >= 0 && b <= 63, "bin in range", x, lo, hi);
    expect(b == bin_brute(x, lo, hi), "bin against the brute-force rule", x, lo, hi);
    if (x < lo) expect(b == 0, "underflow", x, lo, hi);
    if (x >= hi || std::isnan(x)) expect(b == 63, "overflow", x, lo, hi);
    if (x >= lo && x < hi) expect(b >= 1 && b <= 62, "interior", x, lo, hi);
  }
  // monotone over a fine sweep
  int prev = 0;
  for (int k = -100; k <= 6300; ++k) {
    const double x = lo + (hi - lo) * k / 6200.0;
    const int b = timeline_bin(x, r.lo, r.hi, r.inv_w);
    expect(b >= prev, "monotone", x, lo, hi);
    prev = b;
  }
}

// every g and every split position (none, one, two) for G gaps, over a few infection patterns
void check_cum(int G) {
  constexpr int MT = ABD_MAXT_MAX;
  const int nt = (G + 63) / 64;
  std::vector<std::vector<int>> patterns;
  patterns.push_back(std::vector<int>((size_t)G, 0));
  patterns.push_back(std::vector<int>((size_t)G, 1));
  for (int g0 = 0; g0 < G; ++g0) {  // one infection at g0; and one at g0 with a repeat 37 gaps on
    if (G > 64 && g0 % 5 != 0 && g0 != 63 && g0 != 64 && g0 != G - 1) continue;  // (thinned at the larger sizes)
    std::vector<int> a((size_t)G, 0);
    a[(size_t)g0] = 1;
    patterns.push_back(a);
    if (g0 + 37 < G) a[(size_t)(g0 + 37)] = 1, patterns.push_back(a);
  }
  std::vector<std::vector<uint64_t>> words;
  for (const auto& bits : patterns) {
    std::vector<uint64_t> I(MT, 0ull);
    for (int g = 0; g < G; ++g)
      if (bits[(size_t)g]) I[(size_t)(g >> 6)] |= 1ull << (g & 63);
    words.push_back(I);
  }
  for (int s0 = -1; s0 <= G; ++s0) {      // -1: no split
    for (int s1 = -1; s1 <= G; ++s1) {    // -1: no second split
      if (s0 < 0 && s1 >= 0) continue;
      if (s1 >= 0 && s1 <= s0) continue;  // ascending, unique (abd_create refuses the rest)
      if (s1 >= 0 && G > 64 && (s1 - s0) % 11 != 1) continue;  // (the pairs thinned at the larger sizes)
      const int n_splits = (s0 >= 0) + (s1 >= 0);
      const int borders[4] = {0, s0 >= 0 ? s0 : G, s1 >= 0 ? s1 : G, G};
      for (int g = 0; g < G; ++g) {
        // brute force: the chunk [a, b) that holds g
        int lo = 0;
        for (int c = 0; c <= n_splits; ++c) {
          const int a = borders[c], b = c == n_splits ? G : borders[c + 1];
          if (g >= a && g < b) lo = a;
        }
        expect(timeline_chunk_start(g, n_splits, s0, s1) == lo, "chunk start", g, s0, s1);
        uint64_t beyond = 0;
        for (int t = 0; t < MT; ++t) {
          const uint64_t m = timeline_span_mask(t, lo, g);
          for (int b = 0; b < 64; ++b) {
            const int k = t * 64 + b;
            expect((int)((m >> b) & 1ull) == (k >= lo && k <= g ? 1 : 0), "span mask bit", k, lo, g);
          }
          beyond |= t >= nt ? m : 0ull;
        }
        expect(beyond == 0, "no bits beyond the words in use", g, s0, s1);
        for (size_t p = 0; p < patterns.size(); ++p) {
          int want = 0;  // ... then a scan of lo .. g
          for (int k = lo; k <= g; ++k) want |= patterns[p][(size_t)k];
          uint64_t I[MT];
          for (int t = 0; t < MT; ++t) I[t] = words[p][(size_t)t];
          expect((int)timeline_cum<MT>(g, I, n_splits, s0, s1) == want, "cumulative bit", g, s0, s1);
        }
      }
    }
  }
}

void check_quantile() {
  uint32_t c[ABD_TL_BINS] = {};
  const TimelineRange r = timeline_range(-4.0, 8.0);
  expect(std::isnan(timeline_quantile(c, 0.5, r.lo, r.hi, r.w)), "empty histogram");
  c[0] = 3, c[63] = 1;
  expect(timeline_quantile(c, 0.5, r.lo, r.hi, r.w) == -4.0, "bin 0 gives lo");
  expect(timeline_quantile(c, 1.0, r.lo, r.hi, r.w) == 8.0, "bin 63 gives hi");
  uint32_t d[ABD_TL_BINS] = {};
  d[10] = 5, d[40] = 5;  // two modes
  expect(timeline_quantile(d, 0.5, r.lo, r.hi, r.w) == r.lo + r.w * (9.0 + 5.0 / 5.0), "median at the end of the lower mode");
  expect(timeline_quantile(d, 0.0, r.lo, r.hi, r.w) == r.lo + r.w * 9.0, "q = 0: the start of the first populated bin");
  expect(timeline_quantile(d, 0.75, r.lo, r.hi, r.w) == r.lo + r.w * (39.0 + 2.5 / 5.0), "inside the upper mode");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 1 && argc != 3) return std::fprintf(stderr, "usage: timeline_harness [IN OUT]\n"), 2;
  const double ranges[][2] = {{-4.0, 8.0}, {0.0, 1.0}, {-1.7, 3.3}, {1e-3, 1.1e-3}, {-1e300, 1e300}, {5.0, 5.0 + 1e-9}, {0.1, 0.7}};
  for (const auto& r : ranges) check_bins(r[0], r[1]);
  const int sizes[] = {1, 63, 64, 65, 130};
  for (int G : sizes) check_cum(G);
  check_quantile();
  if (g_failed) return std::fprintf(stderr, "%d checks failed\n", g_failed), 1;
  if (argc == 3) {
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) return std::fprintf(stderr, "cannot open %s\n", argv[1]), 2;
    double range[2];
    int64_t head[2];
    if (std::fread(range, sizeof(double), 2, in) != 2 || std::fread(head, sizeof(int64_t), 2, in) != 2) return std::fprintf(stderr, "short header\n"), 2;
    const int64_t D = head[0], Q = head[1];
    if (D < 0 || D > ABD_TL_MAX_DRAWS || Q < 0 || Q > 1024) return std::fprintf(stderr, "bad header\n"), 2;
    std::vector<double> x((size_t)D), q((size_t)Q);
    if (std::fread(x.data(), sizeof(double), x.size(), in) != x.size() || std::fread(q.data(), sizeof(double), q.size(), in) != q.size())
      return std::fprintf(stderr, "short input\n"), 2;
    std::fclose(in);
    const TimelineRange r = timeline_range(range[0], range[1]);
    std::vector<int64_t> bin((size_t)D), hist(ABD_TL_BINS, 0);
    uint32_t c[ABD_TL_BINS] = {};
    for (int64_t d = 0; d < D; ++d) {
      const int b = timeline_bin(x[(size_t)d], r.lo, r.hi, r.inv_w);
      bin[(size_t)d] = b;
      c[b] += 1;
    }
    for (int b = 0; b < ABD_TL_BINS; ++b) hist[(size_t)b] = c[b];
    std::vector<double> out((size_t)Q);
    for (int64_t k = 0; k < Q; ++k) out[(size_t)k] = timeline_quantile(c, q[(size_t)k], r.lo, r.hi, r.w);
    std::FILE* of = std::fopen(argv[2], "wb");
    if (!of) return std::fprintf(stderr, "cannot open %s\n", argv[2]), 2;
    std::fwrite(bin.data(), sizeof(int64_t), bin.size(), of);
    std::fwrite(hist.data(), sizeof(int64_t), hist.size(), of);
    std::fwrite(out.data(), sizeof(double), out.size(), of);
    if (std::fclose(of) != 0) return std::fprintf(stderr, "write failed\n"), 2;
  }
  std::printf("timeline ok\n");
  return 0;
}
