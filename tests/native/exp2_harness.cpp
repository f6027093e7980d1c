// CPU harness for the pre-biased 2^(j/1024) table of the dense kernels (abd_types.hpp: abd_exp2_prebias, abd_exp2_clamp,
// abd_exp2_scaled_hi; used by abd_dense.hpp: one_plus_exp2_pair and abd_device.hpp: one_plus_exp2_tab).
#include <cmath>
#include <cstring>

#include "abd_types.hpp"

static uint64_t plain_bits(int j) {  // 2^(j/1024) as abd_create rounds it
  const double t = (double)exp2l((long double)j / (long double)ABD_EXP2_TAB);
  uint64_t b;
  std::memcpy(&b, &t, sizeof b);
  return b;
}

// high word of 2^(j/1024) 2^e the way the kernels formed it before the table was pre-biased: e = clamp(k >> 10), j = k & 1023
extern "C" uint32_t exp2_hi_plain(int k) {
  int e = k >> 10;
  e = e < -1022 ? -1022 : e > 510 ? 510 : e;
  return (uint32_t)(plain_bits(k & (ABD_EXP2_TAB - 1)) >> 32) + ((uint32_t)e << 20);
}
// ... and from the pre-biased table
extern "C" uint32_t exp2_hi_prebiased(int k) {
  const int kc = abd_exp2_clamp(k);
  const int j = kc & (ABD_EXP2_TAB - 1);
  return abd_exp2_scaled_hi((uint32_t)(abd_exp2_prebias(plain_bits(j), j) >> 32), kc);
}
extern "C" int exp2_low_words_kept() {  // the bias touches the high word only
  for (int j = 0; j < ABD_EXP2_TAB; ++j)
    if ((uint32_t)abd_exp2_prebias(plain_bits(j), j) != (uint32_t)plain_bits(j)) return 0;
  return 1;
}
// first k of [k0, k1] at which the two high words differ (k1 + 1: none)
extern "C" long long exp2_first_difference(int k0, int k1) {
  for (long long k = k0; k <= k1; ++k)
    if (exp2_hi_plain((int)k) != exp2_hi_prebiased((int)k)) return k;
  return (long long)k1 + 1;
}
// 2^(-j/1024), j in [0, 1024], as the sweep's log of the acceptance uniform reads it (abd_gibbs_dense.hpp: log_uniform_u32):
// the entry of k = -j scaled, against T[1024 - j] / 2 (and 1 for j = 0); bits of the double
extern "C" uint64_t exp2_inverse_prebiased(int j) {
  const int idx = -j & (ABD_EXP2_TAB - 1);
  const uint64_t e = abd_exp2_prebias(plain_bits(idx), idx);
  return ((uint64_t)abd_exp2_scaled_hi((uint32_t)(e >> 32), -j) << 32) | (e & 0xFFFFFFFFull);
}
extern "C" uint64_t exp2_inverse_plain(int j) {
  uint64_t b = plain_bits(0);
  if (j != 0) {
    double t;
    b = plain_bits((1024 - j) & (ABD_EXP2_TAB - 1));
    std::memcpy(&t, &b, sizeof t);
    t *= 0.5;
    std::memcpy(&b, &t, sizeof b);
  }
  return b;
}
