// CPU harness for the per-cell update of abd_diag.hpp (tests/test_diagnostics_cpu.py): a stand-alone program that replays a
// sequence of draws from a file through diag_draw / diag_update_titer / diag_update_inf, the source the kernel compiles, and
// writes the accumulators.  Built with g++, plain and with -fsanitize=address,undefined.
//
//   diag_harness IN OUT
//   IN:  int64 D, L, C; then double x[D][C]; then uint8 bit[D][C]
//   OUT: double moments[6][C] (mean_h0, M2_h0, mean_h1, M2_h1, bm_mean, bm_M2); then int64 counts[4][C] (c_h0, c_h1, sum_cb,
//        sum_cb2); then int64 info[4] (draws in half 0, in half 1, batches closed, L)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "abd_diag.hpp"

using namespace abdi;

int main(int argc, char** argv) {
  if (argc != 3) return std::fprintf(stderr, "usage: diag_harness IN OUT\n"), 2;
  std::FILE* in = std::fopen(argv[1], "rb");
  if (!in) return std::fprintf(stderr, "cannot open %s\n", argv[1]), 2;
  int64_t head[3];
  if (std::fread(head, sizeof(int64_t), 3, in) != 3) return std::fprintf(stderr, "short header\n"), 2;
  const int64_t D = head[0], L = head[1], C = head[2];
  if (D < 2 || L < 1 || C < 0) return std::fprintf(stderr, "bad header\n"), 2;
  std::vector<double> x((size_t)(D * C));
  std::vector<uint8_t> bit((size_t)(D * C));
  if (std::fread(x.data(), sizeof(double), x.size(), in) != x.size() || std::fread(bit.data(), 1, bit.size(), in) != bit.size())
    return std::fprintf(stderr, "short input\n"), 2;
  std::fclose(in);
  const int64_t H = D / 2;
  // the planes as the device keeps them: per cell both halves' mean and M2, cur, bm_mean, bm_M2; the element of i and its squares
  std::vector<double> pl((size_t)(kDiagTiterPlanes * C), 0.0);
  std::vector<DiagInf> inf((size_t)C, DiagInf{0, 0, 0, 0});
  std::vector<unsigned long long> cb2((size_t)C, 0ull);
  int64_t closed = 0;
  for (int64_t d = 0; d < 2 * H; ++d) {
    const DiagDraw w = diag_draw(d, H, L);
    closed += w.close_batch;
    const int at = w.half ? kDiagMean1 : kDiagMean0;
    for (int64_t c = 0; c < C; ++c) {
      DiagTiter t{pl[(size_t)(at * C + c)], pl[(size_t)((at + 1) * C + c)], pl[(size_t)(kDiagCur * C + c)], pl[(size_t)(kDiagBmMean * C + c)],
                  pl[(size_t)(kDiagBmM2 * C + c)]};
      diag_update_titer(t, x[(size_t)(d * C + c)], w);
      pl[(size_t)(at * C + c)] = t.mean;
      pl[(size_t)((at + 1) * C + c)] = t.M2;
      if (w.in_batch) pl[(size_t)(kDiagCur * C + c)] = t.cur;
      if (w.close_batch) {
        pl[(size_t)(kDiagBmMean * C + c)] = t.bm_mean;
        pl[(size_t)(kDiagBmM2 * C + c)] = t.bm_M2;
      }
      diag_update_inf(inf[(size_t)c], cb2[(size_t)c], bit[(size_t)(d * C + c)], w);
    }
  }
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!out) return std::fprintf(stderr, "cannot open %s\n", argv[2]), 2;
  const int planes[6] = {kDiagMean0, kDiagM20, kDiagMean1, kDiagM21, kDiagBmMean, kDiagBmM2};
  for (int v = 0; v < 6; ++v) std::fwrite(pl.data() + (size_t)(planes[v] * C), sizeof(double), (size_t)C, out);
  std::vector<int64_t> cnt((size_t)(4 * C));
  for (int64_t c = 0; c < C; ++c) {
    cnt[(size_t)c] = inf[(size_t)c].c_h0;
    cnt[(size_t)(C + c)] = inf[(size_t)c].c_h1;
    cnt[(size_t)(2 * C + c)] = inf[(size_t)c].sum_cb;
    cnt[(size_t)(3 * C + c)] = (int64_t)cb2[(size_t)c];
  }
  std::fwrite(cnt.data(), sizeof(int64_t), cnt.size(), out);
  const int64_t info[4] = {H, H, closed, L};
  std::fwrite(info, sizeof(int64_t), 4, out);
  if (std::fclose(out) != 0) return std::fprintf(stderr, "write failed\n"), 2;
  std::printf("diag ok: %lld draws, %lld cells, %lld batches\n", (long long)(2 * H), (long long)C, (long long)closed);
  return 0;
}
