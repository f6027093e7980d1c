// CPU harness for abd_survival_groups_terms.hpp (tests/test_survival_groups_terms_native.py): what the library makes of one
// point (lambda_t, a_g, b for the kernel) and of the device sums (logp, gradient), and the layout of the individuals by group,
// as plain functions.
#include "abd_survival_groups_terms.hpp"

extern "C" int survival_groups_terms(int T, int Gr, const double* priors, const double* theta, const double* Y, double C,
                                     const double* sums, double* par, double* logp, double* grad) {
  using namespace abdi;
  const SurvivalGroupsPriors p{priors[0], priors[1], priors[2], priors[3], priors[4], priors[5], priors[6], priors[7]};
  double* work = new double[2 * T];
  survival_groups_prepare(T, Gr, theta, par, work);
  *logp = survival_groups_combine(p, T, Gr, theta, Y, C, sums, par, work, grad);
  delete[] work;
  return survival_groups_dim(T, Gr);
}

// slot[N], tile_group[ceil(N / 64) + Gr], group_tile[Gr + 1]; returns the number of tiles
extern "C" int survival_groups_layout(int N, int Gr, const int32_t* group, int32_t* slot, int32_t* tile_group, int32_t* group_tile) {
  return abdi::survival_groups_layout(N, Gr, group, slot, tile_group, group_tile);
}
