// CPU harness for abd_survival_pointwise_terms.hpp (tests/test_survival_pointwise_cpu.py): a stand-alone program.
//   survival_pointwise_harness IN OUT
// IN:  int64 T, ld, K, Gr, n_draw; double y[T][ld], e[T][ld], theta[D]   (Gr > 0: the model by group, K = 1)
// OUT: double C[ld], n_cells[ld], row[2 T + n_ab + 1]                     (n_ab = 2 K, or Gr + 1)
// what creation makes of the planes and what one point gives the kernels, as the library forms them.
#include <cstdio>
#include <vector>

#include "abd_survival_groups_terms.hpp"
#include "abd_survival_pointwise_terms.hpp"

int main(int argc, char** argv) {
  using namespace abdi;
  if (argc != 3) return 2;
  std::FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 3;
  int64_t h[5];
  if (std::fread(h, sizeof(int64_t), 5, in) != 5) return 4;
  const int T = (int)h[0], ld = (int)h[1], K = (int)h[2], Gr = (int)h[3];
  if (T < 1 || ld < 1 || (Gr == 0 && K != 1 && K != 2) || Gr < 0) return 5;
  const SurvivalForm form{K, Gr, T};
  const int D = form.dim(), n_ab = form.n_ab();
  const size_t plane = (size_t)T * ld;
  std::vector<double> y(plane), e(plane), theta((size_t)D);
  if (std::fread(y.data(), sizeof(double), plane, in) != plane) return 4;
  if (std::fread(e.data(), sizeof(double), plane, in) != plane) return 4;
  if (std::fread(theta.data(), sizeof(double), (size_t)D, in) != (size_t)D) return 4;
  std::fclose(in);
  std::vector<double> C((size_t)ld), cells_d((size_t)ld), par((size_t)T + n_ab), work((size_t)2 * T);
  std::vector<int32_t> cells((size_t)ld);
  survival_pointwise_constants(T, ld, y.data(), e.data(), C.data(), cells.data());
  for (int j = 0; j < ld; ++j) cells_d[j] = cells[j];
  form.prepare(theta.data(), par.data(), work.data());
  std::vector<double> row((size_t)survival_pointwise_stride(T, n_ab));
  survival_pointwise_row(T, n_ab, par.data(), work.data(), h[4], row.data());
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 3;
  std::fwrite(C.data(), sizeof(double), C.size(), out);
  std::fwrite(cells_d.data(), sizeof(double), cells_d.size(), out);
  std::fwrite(row.data(), sizeof(double), row.size(), out);
  return std::fclose(out) ? 6 : 0;
}
