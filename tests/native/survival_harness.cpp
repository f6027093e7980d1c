// CPU harness for abd_survival_terms.hpp (tests/test_survival_terms_native.py): what the library makes of one point (lambda_t, a,
// b for the kernel) and of the device sums (logp, gradient), its verdict on one cell, and the planes creation makes of the
// caller's arrays, as plain functions.
#include <cstring>

#include "abd_survival_groups_terms.hpp"
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

// survival_pack as creation calls it.  group null: individual j in column j; else the columns of survival_groups_layout of the
// labels group[N] in [0, Gr).  Returns ld (at most ld_cap, else -1) with planes = y, e, x0, x1 [4][T][ld] (x1 untouched for
// K = 1), Y[T], *C and slot[N]; or 0 for a refused cell, with bad = j, t and its message.
extern "C" int survival_planes(int N, int T, int K, const double* infected, const double* exposure, const double* x0, const double* x1,
                               const int32_t* group, int Gr, int ld_cap, double* planes, double* Y, double* C, int32_t* slot, int* bad,
                               char* msg, int msg_len) {
  using namespace abdi;
  int ntile = (N + 63) / 64;
  if (group) {
    std::vector<int32_t> tile_group((size_t)ntile + Gr), group_tile((size_t)Gr + 1);
    ntile = survival_groups_layout(N, Gr, group, slot, tile_group.data(), group_tile.data());
  } else {
    for (int j = 0; j < N; ++j) slot[j] = j;
  }
  const size_t ld = (size_t)ntile * 64, plane = ld * T;
  if (ld > (size_t)ld_cap) return -1;
  const double* titer[2] = {x0, x1};
  SurvivalPlanes p;
  const SurvivalRefusal r = survival_pack(N, T, K, infected, exposure, titer, group ? slot : nullptr, ld, &p);
  std::strncpy(msg, r.msg ? r.msg : "", (size_t)msg_len - 1);
  msg[msg_len - 1] = 0;
  if (r.msg) {
    bad[0] = r.j;
    bad[1] = r.t;
    return 0;
  }
  const std::vector<double>* src[4] = {&p.y, &p.e, &p.x0, &p.x1};
  for (int k = 0; k < 4; ++k)
    if (!src[k]->empty()) std::memcpy(planes + k * plane, src[k]->data(), plane * sizeof(double));
  std::memcpy(Y, p.Y.data(), (size_t)T * sizeof(double));
  *C = p.C;
  return (int)ld;
}
