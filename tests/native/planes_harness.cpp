// planes_harness.cpp -- abd_planes.hpp on the CPU (tests/test_planes_native.py): the reference transpose against a
// bit-by-bit definition, and the exposure bookkeeping of the plane form of the gap loop stepped against the legacy form's
// per-lane OR chain restated here.  With -DPLANES_HARNESS_MAIN a stand-alone program (built with host ASan + UBSan).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "abd_planes.hpp"

extern "C" {

// words [nt][N] -> planes [n_lg][abd_plane_gaps(G)][2], the `which` masks (the others untouched); returns the words of a plane set
long long planes_transpose(const uint64_t* words, int N, int G, int which, uint64_t* planes) {
  abd_plane_transpose_ref(words, N, G, which, planes);
  return (long long)abd_plane_words((N + 63) / 64, G);
}
int planes_gaps(int G) { return abd_plane_gaps(G); }
long long planes_index(int lg, int g, int G, int which) { return (long long)abd_plane_index(lg, g, G, which); }

// One lane group, gaps [g0, G) walked as one piece after a start state built from the gaps before g0.
//   inf, vac: [G][64] bytes 0/1 (lane l's constrained infection / vaccination in gap g); k = {c perm_n, c init_n, c perm_s, c init_s}
// Plane form: masks of every gap, seen seeded by abd_exposure_start, cf and base rewritten only for the lanes abd_exposure_new
// names, base refreshed as fma(1.0, cp, ci).  Legacy form: per lane, cf_hi |= the gap's bit, addend fma(cf, cp, ci) every gap.
// out (may be NULL): [G - g0][64][4] of {cf_n, cf_s, addend_n, addend_s} of the plane form.  Returns the number of (gap, lane,
// value) triples whose bits differ between the forms.
long long planes_exposure_check(const uint8_t* inf, const uint8_t* vac, int G, int g0, const double* k, double* out) {
  const double cp_n = k[0], ci_n = k[1], cp_s = k[2], ci_s = k[3];
  std::vector<uint64_t> m_i((size_t)G, 0), m_v((size_t)G, 0);
  for (int g = 0; g < G; ++g)
    for (int l = 0; l < 64; ++l) {
      m_i[(size_t)g] |= (uint64_t)(inf[(size_t)g * 64 + l] != 0) << l;
      m_v[(size_t)g] |= (uint64_t)(vac[(size_t)g * 64 + l] != 0) << l;
    }
  // start state
  uint64_t before_i = 0, before_v = 0;
  uint32_t cfn_hi[64], cfs_hi[64];  // legacy: high word of 0.0 / 1.0 per lane
  for (int l = 0; l < 64; ++l) cfn_hi[l] = cfs_hi[l] = 0;
  for (int g = 0; g < g0; ++g) {
    before_i |= m_i[(size_t)g];
    before_v |= m_v[(size_t)g];
    for (int l = 0; l < 64; ++l) {
      const uint32_t ei = inf[(size_t)g * 64 + l] ? 0x3FF00000u : 0u, ev = vac[(size_t)g * 64 + l] ? 0x3FF00000u : 0u;
      cfn_hi[l] |= ei;
      cfs_hi[l] |= ei | ev;
    }
  }
  ExposureSeen seen = abd_exposure_start(before_i, before_v);
  const double b1_n = std::fma(1.0, cp_n, ci_n), b1_s = std::fma(1.0, cp_s, ci_s);
  double cf_n[64], cf_s[64], base_n[64], base_s[64];
  for (int l = 0; l < 64; ++l) {
    cf_n[l] = (seen.n >> l) & 1 ? 1.0 : 0.0;
    cf_s[l] = (seen.s >> l) & 1 ? 1.0 : 0.0;
    base_n[l] = (seen.n >> l) & 1 ? b1_n : std::fma(0.0, cp_n, ci_n);
    base_s[l] = (seen.s >> l) & 1 ? b1_s : std::fma(0.0, cp_s, ci_s);
  }
  auto hi_to_double = [](uint32_t hi) {
    const uint64_t b = (uint64_t)hi << 32;
    double d;
    std::memcpy(&d, &b, sizeof d);
    return d;
  };
  auto differ = [](double a, double b) { return std::memcmp(&a, &b, sizeof a) != 0; };
  long long bad = 0;
  for (int g = g0; g < G; ++g) {
    const ExposureSeen nw = abd_exposure_new(seen, m_i[(size_t)g], m_v[(size_t)g]);
    if ((nw.n | nw.s) != 0) {
      for (int l = 0; l < 64; ++l) {
        if ((nw.n >> l) & 1) {
          cf_n[l] = 1.0;
          base_n[l] = b1_n;
        }
        if ((nw.s >> l) & 1) {
          cf_s[l] = 1.0;
          base_s[l] = b1_s;
        }
      }
      abd_exposure_mark(seen, m_i[(size_t)g], m_v[(size_t)g]);
    }
    for (int l = 0; l < 64; ++l) {
      const uint32_t ei = inf[(size_t)g * 64 + l] ? 0x3FF00000u : 0u, ev = vac[(size_t)g * 64 + l] ? 0x3FF00000u : 0u;
      cfn_hi[l] |= ei;
      cfs_hi[l] |= ei | ev;
      const double lcf_n = hi_to_double(cfn_hi[l]), lcf_s = hi_to_double(cfs_hi[l]);
      const double lad_n = std::fma(lcf_n, cp_n, ci_n), lad_s = std::fma(lcf_s, cp_s, ci_s);
      bad += differ(lcf_n, cf_n[l]) + differ(lcf_s, cf_s[l]) + differ(lad_n, base_n[l]) + differ(lad_s, base_s[l]);
      if (out) {
        double* o = out + ((size_t)(g - g0) * 64 + l) * 4;
        o[0] = cf_n[l];
        o[1] = cf_s[l];
        o[2] = base_n[l];
        o[3] = base_s[l];
      }
    }
  }
  return bad;
}

}  // extern "C"

#ifdef PLANES_HARNESS_MAIN
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}
int main() {
  long long bad = 0;
  // transpose: full, empty, random tiles; ragged last lane group (N % 64 in {1, 63}) and last word (G % 64 in {1, 33})
  const int shapes[][2] = {{64, 64}, {65, 65}, {127, 97}, {1, 1}, {129, 33}, {191, 257}};
  for (const auto& sh : shapes)
    for (int fill = 0; fill < 3; ++fill) {
      const int N = sh[0], G = sh[1], nt = (G + 63) / 64, n_lg = (N + 63) / 64;
      std::vector<uint64_t> w((size_t)nt * N);
      for (int t = 0; t < nt; ++t)
        for (int j = 0; j < N; ++j) {
          uint64_t v = fill == 0 ? 0 : fill == 1 ? ~0ull : rnd();
          const int g_end = G - t * 64;
          if (g_end < 64) v &= (1ull << g_end) - 1;
          w[(size_t)t * N + j] = v;
        }
      for (int which = 0; which < 2; ++which) {
        std::vector<uint64_t> pl(abd_plane_words(n_lg, G), 0xA5A5A5A5A5A5A5A5ull);
        planes_transpose(w.data(), N, G, which, pl.data());
        for (int lg = 0; lg < n_lg; ++lg)
          for (int g = 0; g < abd_plane_gaps(G); ++g)
            for (int l = 0; l < 64; ++l) {
              const int j = lg * 64 + l;
              const uint64_t got = (pl[abd_plane_index(lg, g, G, which)] >> l) & 1, other = pl[abd_plane_index(lg, g, G, which ^ 1)];
              if (g < G) {
                const uint64_t want = j < N ? (w[(size_t)(g >> 6) * N + j] >> (g & 63)) & 1 : 0;
                bad += got != want;
              } else {
                bad += pl[abd_plane_index(lg, g, G, which)] != 0xA5A5A5A5A5A5A5A5ull;  // padding gaps are not the transpose's
              }
              bad += other != 0xA5A5A5A5A5A5A5A5ull;
            }
      }
    }
  // exposure bookkeeping: random histories at several densities and start gaps
  const double k[4] = {0x1.23456789abcdep+9, -0x1.fedcba9876543p+10, 0x1.0f0f0f0f0f0f1p+8, -0.0};
  for (int G : {1, 2, 33, 65, 130})
    for (int dens = 0; dens < 4; ++dens)
      for (int g0 : {0, 1, 31, 32, 63, 64, G - 1}) {
        if (g0 >= G) continue;
        std::vector<uint8_t> inf((size_t)G * 64), vac((size_t)G * 64);
        for (auto& b : inf) b = dens == 3 ? 1 : (rnd() % 200) < (uint64_t)dens * 3;
        for (auto& b : vac) b = (rnd() % 200) < (uint64_t)dens * 2;
        bad += planes_exposure_check(inf.data(), vac.data(), G, g0, k, nullptr);
      }
  std::printf(bad ? "planes harness: %lld mismatches\n" : "planes harness ok\n", bad);
  return bad ? 1 : 0;
}
#endif
