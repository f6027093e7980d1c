// CPU harness for abd_survival_predictive_terms.hpp (tests/test_survival_predictive_cpu.py): a stand-alone program, built plain and
// under the sanitizers.
//   survival_predictive_harness IN OUT
// IN:  int64 N, T, ld, n_var, n_edges[2], seed, draw, has_slot, n_grid;
//      double y[T][ld], e[T][ld]                 the planes as creation lays them out (cleaned, padded)
//      double mu[N][T]                           the expected count of every cell, caller's order
//      double titers[n_var][N][T], edges[n_var][7]
//      int64 slot[N]                             (has_slot: the column of individual j)
//      double grid_mu[n_grid], grid_u[n_grid]    pairs for the inversion alone
// OUT: double refusal (0: none, else 1 + the refused individual); then, where none,
//      bins[n_var][N][T] (caller's order, read back from the byte plane through slot), u[N][T], r[N][T], observed[2][8],
//      person_time[2][8], n_cells[2][8], observed_ind[N], slot_j[ld], grid_k[n_grid]
// the bin planes and constants as configuration makes them, and the keyed uniform and the replicate of every cell as the kernel
// forms them from mu.
#include <cstdio>
#include <vector>

#include "abd_survival_predictive_terms.hpp"

namespace {
template <typename T>
bool read(std::FILE* in, std::vector<T>& v) {
  return v.empty() || std::fread(v.data(), sizeof(T), v.size(), in) == v.size();
}
void put(std::FILE* out, const std::vector<double>& v) {
  if (!v.empty()) std::fwrite(v.data(), sizeof(double), v.size(), out);
}
}  // namespace

int main(int argc, char** argv) {
  using namespace abdi;
  if (argc != 3) return 2;
  std::FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 3;
  int64_t h[10];
  if (std::fread(h, sizeof(int64_t), 10, in) != 10) return 4;
  const int N = (int)h[0], T = (int)h[1], n_var = (int)h[3];
  const size_t ld = (size_t)h[2], n_grid = (size_t)h[9];
  const int32_t n_edges[2] = {(int32_t)h[4], (int32_t)h[5]};
  const uint64_t seed = (uint64_t)h[6];
  const uint32_t draw_lo = (uint32_t)(uint64_t)h[7];
  if (N < 1 || T < 1 || ld < (size_t)N || n_var < 1 || n_var > ABD_SURV_PRED_VARS) return 5;
  const size_t plane = ld * T, cells = (size_t)N * T;
  std::vector<double> y(plane), e(plane), mu(cells), titers(n_var * cells), edges((size_t)n_var * 7), grid_mu(n_grid), grid_u(n_grid);
  std::vector<int64_t> slot64(h[8] ? (size_t)N : 0);
  if (!read(in, y) || !read(in, e) || !read(in, mu) || !read(in, titers) || !read(in, edges) || !read(in, slot64) || !read(in, grid_mu) ||
      !read(in, grid_u))
    return 4;
  std::fclose(in);
  std::vector<int32_t> slot(slot64.begin(), slot64.end());
  const double* tp[2] = {titers.data(), titers.data() + (n_var - 1) * cells};
  const double* ep[2] = {edges.data(), edges.data() + (size_t)(n_var - 1) * 7};
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 3;
  for (int v = 0; v < n_var; ++v)
    if (surv_pred_check_edges(n_edges[v], ep[v])) {
      put(out, {-1.0});
      return std::fclose(out) ? 6 : 0;
    }
  std::vector<uint8_t> bins(plane);
  std::vector<int32_t> slot_j(ld);
  SurvPredConstants c;
  const SurvivalRefusal bad = surv_pred_pack(N, T, ld, slot.empty() ? nullptr : slot.data(), y.data(), e.data(), n_var, tp, n_edges, ep,
                                             bins.data(), slot_j.data(), &c);
  put(out, {bad.msg ? 1.0 + bad.j : 0.0});
  if (bad.msg) return std::fclose(out) ? 6 : 0;
  std::vector<double> ob((size_t)n_var * cells), u(cells), r(cells), consts, sj(ld), gk(n_grid);
  for (int j = 0; j < N; ++j)
    for (int t = 0; t < T; ++t) {
      const size_t col = slot.empty() ? (size_t)j : (size_t)slot[j], k = (size_t)j * T + t;
      const unsigned byte = bins[(size_t)t * ld + col];
      ob[k] = byte & 15u;
      if (n_var == 2) ob[cells + k] = byte >> 4;
      // as the kernel: the caller's index of the column, read back from slot_j
      u[k] = surv_pred_uniform((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)slot_j[col], (uint32_t)t, draw_lo);
      r[k] = surv_pred_poisson(mu[k], u[k]);
    }
  for (int v = 0; v < ABD_SURV_PRED_VARS; ++v)
    for (int b = 0; b < ABD_SURV_PRED_BINS; ++b) consts.push_back(c.observed[v][b]);
  for (int v = 0; v < ABD_SURV_PRED_VARS; ++v)
    for (int b = 0; b < ABD_SURV_PRED_BINS; ++b) consts.push_back(c.person_time[v][b]);
  for (int v = 0; v < ABD_SURV_PRED_VARS; ++v)
    for (int b = 0; b < ABD_SURV_PRED_BINS; ++b) consts.push_back((double)c.n_cells[v][b]);
  for (size_t k = 0; k < ld; ++k) sj[k] = slot_j[k];
  for (size_t k = 0; k < n_grid; ++k) gk[k] = surv_pred_poisson(grid_mu[k], grid_u[k]);
  put(out, ob);
  put(out, u);
  put(out, r);
  put(out, consts);
  put(out, c.observed_ind);
  put(out, sj);
  put(out, gk);
  return std::fclose(out) ? 6 : 0;
}
