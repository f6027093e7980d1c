// CPU harness for abd_survival_terms.hpp (tests/test_survival_terms_native.py): what the library makes of one point (lambda_t, a,
// b for the kernel) and of the device sums (logp, gradient), and its verdict on one cell, as plain functions.
#include <cstring>

#include "abd_survival_terms.hpp"

extern "C" int survival_terms(int K, int T, const double* priors, const double* theta, const double* Y, double C, const double* sums,
                              double* par, double* logp, double* grad) {
  using namespace abdi;
  const SurvivalPriors p{priors[0], priors[1], priors[2], priors[3], priors[4]};
  double* work = new double[2 * T];
  survival_prepare(K, T, theta, par, work);
  *logp = survival_combine(p, K, T, theta, Y, C, sums, par, work, grad);
  delete[] work;
  return survival_dim(K, T);
}

// cell = y, e, x[K], rewritten as creation keeps it; msg: the refusal (empty if none)
extern "C" int survival_cell(int K, double* cell, char* msg, int msg_len) {
  const char* m = abdi::survival_check_cell(K, cell[0], cell[1], cell + 2);
  std::strncpy(msg, m ? m : "", (size_t)msg_len - 1);
  msg[msg_len - 1] = 0;
  return m ? 1 : 0;
}
