// hc_sum_harness.cpp -- the perm sums of the dense gap loop as differences of the H sums (abd_planes.hpp: abd_hc_open /
// abd_hc_close) and the S boost by selects (abd_s_boost_hi) on the CPU (tests/test_hc_sum_native.py).  One lane group of 64
// lanes walks a range of rows cut into pieces, as a wave of abd_dense.hpp does: the H sums run on across the pieces, every
// piece has its own exposure history (a piece is another individual, or the rest of one whose earlier gaps are summarised
// by "exposed before").  The plane form's bookkeeping (lane masks) and the legacy form's (per-lane OR chain) are both
// stepped and must give the same bits; the reference is the cf-weighted sum in long double.
// With -DHC_SUM_HARNESS_MAIN a stand-alone program (built with host ASan + UBSan).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "abd_planes.hpp"

extern "C" {

// h_n, h_s: [n][64] doubles; inf, vac: [n][64] bytes 0/1; bounds: [P + 1] row bounds of the pieces (bounds[0] = 0,
// bounds[P] = n); before_i, before_v: [P][64] bytes: the lane had an infection / a vaccination before piece p.
// out: [64][8] = {HC_n, HC_s (difference form), err_n, err_s (difference form - long double reference), sum |h_n|, sum |h_s|,
// err_n, err_s of the gap-by-gap fma form}.  Returns the number of lanes whose plane-form and legacy-form bits differ.
long long hc_sum_run(const double* h_n, const double* h_s, const uint8_t* inf, const uint8_t* vac, int n, const int* bounds, int P,
                     const uint8_t* before_i, const uint8_t* before_v, double* out) {
  double H_n[64], H_s[64], hc_n[64], hc_s[64];     // plane form
  double L_n[64], L_s[64], lc_n[64], lc_s[64];     // legacy form
  double fm_n[64], fm_s[64];                       // gap by gap: fma(h, cf, .)
  long double ref_n[64], ref_s[64], abs_n[64], abs_s[64];
  for (int l = 0; l < 64; ++l) {
    H_n[l] = H_s[l] = hc_n[l] = hc_s[l] = L_n[l] = L_s[l] = lc_n[l] = lc_s[l] = fm_n[l] = fm_s[l] = 0.0;
    ref_n[l] = ref_s[l] = abs_n[l] = abs_s[l] = 0.0L;
  }
  for (int p = 0; p < P; ++p) {
    uint64_t bi = 0, bv = 0;
    uint32_t cfn_hi[64], cfs_hi[64];
    for (int l = 0; l < 64; ++l) {
      bi |= (uint64_t)(before_i[(size_t)p * 64 + l] != 0) << l;
      bv |= (uint64_t)(before_v[(size_t)p * 64 + l] != 0) << l;
      cfn_hi[l] = before_i[(size_t)p * 64 + l] ? 0x3FF00000u : 0u;
      cfs_hi[l] = (before_i[(size_t)p * 64 + l] || before_v[(size_t)p * 64 + l]) ? 0x3FF00000u : 0u;
    }
    ExposureSeen seen = abd_exposure_start(bi, bv);
    for (int l = 0; l < 64; ++l) {  // step 1
      hc_n[l] = abd_hc_open(hc_n[l], H_n[l], (seen.n >> l) & 1);
      hc_s[l] = abd_hc_open(hc_s[l], H_s[l], (seen.s >> l) & 1);
      lc_n[l] = abd_hc_open(lc_n[l], L_n[l], cfn_hi[l] != 0);
      lc_s[l] = abd_hc_open(lc_s[l], L_s[l], cfs_hi[l] != 0);
    }
    for (int g = bounds[p]; g < bounds[p + 1]; ++g) {
      uint64_t m_i = 0, m_v = 0;
      for (int l = 0; l < 64; ++l) {
        m_i |= (uint64_t)(inf[(size_t)g * 64 + l] != 0) << l;
        m_v |= (uint64_t)(vac[(size_t)g * 64 + l] != 0) << l;
      }
      // plane form: step 2 in the rare branch, before the gap's h is added
      const ExposureSeen nw = abd_exposure_new(seen, m_i, m_v);
      if ((nw.n | nw.s) != 0) {
        for (int l = 0; l < 64; ++l) {
          hc_n[l] = abd_hc_open(hc_n[l], H_n[l], (nw.n >> l) & 1);
          hc_s[l] = abd_hc_open(hc_s[l], H_s[l], (nw.s >> l) & 1);
        }
        abd_exposure_mark(seen, m_i, m_v);
      }
      for (int l = 0; l < 64; ++l) {
        const double hn = h_n[(size_t)g * 64 + l], hs = h_s[(size_t)g * 64 + l];
        // legacy form: per-lane first-exposure test on the high words, then the OR chain
        const uint32_t ei = inf[(size_t)g * 64 + l] ? 0x3FF00000u : 0u, ev = vac[(size_t)g * 64 + l] ? 0x3FF00000u : 0u;
        const bool first_n = (ei & ~cfn_hi[l]) != 0, first_s = ((ei | ev) & ~cfs_hi[l]) != 0;
        lc_n[l] = abd_hc_open(lc_n[l], L_n[l], first_n);
        lc_s[l] = abd_hc_open(lc_s[l], L_s[l], first_s);
        cfn_hi[l] |= ei;
        cfs_hi[l] |= ei | ev;
        H_n[l] += hn;
        H_s[l] += hs;
        L_n[l] += hn;
        L_s[l] += hs;
        const bool cn = cfn_hi[l] != 0, cs = cfs_hi[l] != 0;  // the gap of the first exposure already counts
        fm_n[l] = std::fma(hn, cn ? 1.0 : 0.0, fm_n[l]);
        fm_s[l] = std::fma(hs, cs ? 1.0 : 0.0, fm_s[l]);
        if (cn) ref_n[l] += (long double)hn;
        if (cs) ref_s[l] += (long double)hs;
        abs_n[l] += std::fabs((long double)hn);
        abs_s[l] += std::fabs((long double)hs);
      }
    }
    for (int l = 0; l < 64; ++l) {  // step 3
      hc_n[l] = abd_hc_close(hc_n[l], H_n[l], (seen.n >> l) & 1);
      hc_s[l] = abd_hc_close(hc_s[l], H_s[l], (seen.s >> l) & 1);
      lc_n[l] = abd_hc_close(lc_n[l], L_n[l], cfn_hi[l] != 0);
      lc_s[l] = abd_hc_close(lc_s[l], L_s[l], cfs_hi[l] != 0);
    }
  }
  long long bad = 0;
  for (int l = 0; l < 64; ++l) {
    bad += std::memcmp(&hc_n[l], &lc_n[l], sizeof(double)) != 0;
    bad += std::memcmp(&hc_s[l], &lc_s[l], sizeof(double)) != 0;
    double* o = out + (size_t)l * 8;
    o[0] = hc_n[l];
    o[1] = hc_s[l];
    o[2] = (double)((long double)hc_n[l] - ref_n[l]);
    o[3] = (double)((long double)hc_s[l] - ref_s[l]);
    o[4] = (double)abs_n[l];
    o[5] = (double)abs_s[l];
    o[6] = (double)((long double)fm_n[l] - ref_n[l]);
    o[7] = (double)((long double)fm_s[l] - ref_s[l]);
  }
  return bad;
}

// the S boost by selects against the fp64 add, all four combinations of the two indicators: the number whose bits differ
int hc_boost_check(void) {
  int bad = 0;
  for (int i = 0; i < 2; ++i)
    for (int v = 0; v < 2; ++v) {
      const double e_i = i ? 1.0 : 0.0, e_v = v ? 1.0 : 0.0, sum = e_i + e_v;
      const uint64_t bits = (uint64_t)abd_s_boost_hi(i || v, i && v) << 32;
      bad += std::memcmp(&bits, &sum, sizeof sum) != 0;
    }
  return bad;
}

}  // extern "C"

#ifdef HC_SUM_HARNESS_MAIN
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}
static double unif() { return (double)(rnd() >> 11) * 0x1p-53; }
int main() {
  long long bad = hc_boost_check();
  double worst = 0.0;
  for (int rep = 0; rep < 200; ++rep) {
    const int n = 1 + (int)(rnd() % 500), P = 1 + (int)(rnd() % 4);
    const int Pn = P > n ? n : P;  // every piece has at least one row
    std::vector<int> bounds((size_t)Pn + 1, 0);
    bounds[(size_t)Pn] = n;
    for (int p = 1; p < Pn; ++p) bounds[(size_t)p] = bounds[(size_t)p - 1] + 1 + (int)(rnd() % (uint64_t)(n - bounds[(size_t)p - 1] - (Pn - p)));
    std::vector<double> hn((size_t)n * 64), hs((size_t)n * 64), out(64 * 8);
    std::vector<uint8_t> inf((size_t)n * 64), vac((size_t)n * 64), bi((size_t)Pn * 64), bv((size_t)Pn * 64);
    const uint64_t dens = rnd() % 4;  // 0: nobody is ever exposed inside a piece
    for (auto& x : hn) x = (unif() - 0.5) * std::exp(4.0 * unif() - 2.0);
    for (auto& x : hs) x = (unif() - 0.5) * std::exp(4.0 * unif() - 2.0);
    for (auto& b : inf) b = (rnd() % 400) < dens * 3;
    for (auto& b : vac) b = (rnd() % 400) < dens * 2;
    for (auto& b : bi) b = rnd() % 4 == 0;
    for (auto& b : bv) b = rnd() % 4 == 0;
    bad += hc_sum_run(hn.data(), hs.data(), inf.data(), vac.data(), n, bounds.data(), Pn, bi.data(), bv.data(), out.data());
    const double bound = (2.0 * n + 3.0) * 0x1p-53;
    for (int l = 0; l < 64; ++l) {
      const double* o = out.data() + (size_t)l * 8;
      bad += !(std::fabs(o[2]) <= bound * o[4]) + !(std::fabs(o[3]) <= bound * o[5]);
      if (o[4] > 0.0) worst = std::fmax(worst, std::fabs(o[2]) / (0x1p-53 * o[4]));
      if (o[5] > 0.0) worst = std::fmax(worst, std::fabs(o[3]) / (0x1p-53 * o[5]));
    }
  }
  std::printf("worst error %.2f u sum|h|\n", worst);
  std::printf(bad ? "hc sum harness: %lld failures\n" : "hc sum harness ok\n", bad);
  return bad ? 1 : 0;
}
#endif
