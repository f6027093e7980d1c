// CPU harness for abd_survival_periods_terms.hpp (tests/test_survival_periods_terms_native.py): what the library makes of one
// point (lambda_t, a_t, b for the kernel) and of the device sums (the fold of W0_t into W0_p, then logp and gradient), through
// SurvivalForm as the library asks for them.
#include "abd_survival_groups_terms.hpp"  // SurvivalForm
#include "abd_survival_periods_terms.hpp"

// par[2 T + 1], gsums[T + 2 + P] (the folded sums), grad[D]; returns D
extern "C" int survival_periods_terms(int T, int P, const int32_t* period, const double* priors, const double* theta, const double* Y,
                                      double C, const double* sums, double* par, double* gsums, double* logp, double* grad) {
  using namespace abdi;
  const SurvivalGroupsPriors gp{priors[0], priors[1], priors[2], priors[3], priors[4], priors[5], priors[6], priors[7]};
  const SurvivalForm form{1, 0, T, P, std::vector<int32_t>(period, period + T)};
  std::vector<double> work((size_t)form.work_stride());
  form.prepare(theta, par, work.data());
  *logp = form.combine(SurvivalPriors{}, gp, theta, Y, C, sums, par, work.data(), grad);
  const double* folded = survival_periods_gsums(T, P, work.data());
  for (int k = 0; k < T + 2 + P; ++k) gsums[k] = folded[k];
  return form.dim();
}

// the sizes of the form: dim, n_ab, par_stride, n_sums, out_stride, mode
extern "C" void survival_periods_sizes(int T, int P, int32_t* out) {
  const abdi::SurvivalForm form{1, 0, T, P, std::vector<int32_t>((size_t)T, 0)};
  const int v[6] = {form.dim(), form.n_ab(), form.par_stride(), form.n_sums(), form.out_stride(), form.mode()};
  for (int k = 0; k < 6; ++k) out[k] = v[k];
}
