// abd_loo.hpp -- PSIS-LOO by individual for the titer model: the sampler-side storage of T_j = S_j + N_j of every
// kept draw into abd_psis.hpp's resident matrix, and the launch of its estimator over it (abd_sampler.hpp: LooSummary).
//
// The per-individual kernels (abd_individual.hpp) write a draw's S_j and N_j rows into the chain's staging block; one launch per
// draw and chain serves the WAIC accumulators as well.  abd_loo_store is abd_psis_store with the add: thread = slot, it reads
// the n <= 16 staged (S_j, N_j) pairs, forms T_j = S_j + N_j -- the single fp64 add IndLogLik::put does for the accumulators, so
// both see the same bits -- and writes n consecutive doubles of its row, with 16 rows one whole 128-byte line per individual.
// Slots >= N (the padding) write 0.  No atomics, no cross-lane step.
// Included by abd_sampler.hip alone: this unit and abd_survival.hip each compile abd_psis.hpp's kernels.
#pragma once

#include "abd_psis.hpp"
#include "abd_sampler.hpp"

static_assert(ABD_SAMPLER_LOO_MAX_DRAWS == abdi::kPsisMaxDraws, "header / kernel draw cap mismatch");

namespace abdi {

// rows 0 .. n - 1 of ll_s, ll_n [n][ld] to the draws n0 .. n0 + n - 1 of mat [ld][capacity]
__global__ __launch_bounds__(256) void abd_loo_store(const double* ll_s, const double* ll_n, double* mat, int32_t N, int32_t ld, int64_t capacity,
                                                     int32_t n, int64_t n0) {
  const int unit = blockIdx.x * 256 + threadIdx.x;
  if (unit >= ld) return;
  double* row = mat + (int64_t)unit * capacity + n0;
  for (int p = 0; p < n; ++p) row[p] = unit < N ? ll_s[(int64_t)p * ld + unit] + ll_n[(int64_t)p * ld + unit] : 0.0;
}

}  // namespace abdi

int LooSummary::launch(abd_ctx* c, int j, int chain, const double* q, int64_t d, bool last, double* acc, hipStream_t st) {
  if (d < 0) return ABD_OK;  // tuning (nothing is staged: the run call before flushed at its end)
  if (!on()) return launch_individual_loglik(c, chain, q, st, nullptr, nullptr, acc, d + 1);
  const bool keep = d % thin == 0;
  int64_t& sg = staged[(size_t)j];
  if (int rc = launch_individual_loglik(c, chain, q, st, keep ? stage_at(j, 0, sg) : nullptr, keep ? stage_at(j, 1, sg) : nullptr, acc, d + 1))
    return rc;
  if (keep) sg += 1;
  if (sg == kStage || (last && sg > 0)) {
    int64_t& have = stored[(size_t)j];
    if (have + sg > C) return abdi::fail(ABD_ERR_STATE, "loo: chain %d would hold %lld rows of %lld", j, (long long)(have + sg), (long long)C);
    HIP_TRY(launch_kernel(abdi::abd_loo_store, dim3((unsigned)((ld + 255) / 256)), dim3(256), 0, st, (const double*)stage_at(j, 0, 0),
                          (const double*)stage_at(j, 1, 0), (double*)mat, (int32_t)c->N, (int32_t)ld, capacity(), (int32_t)sg,
                          (int64_t)j * C + have));
    have += sg;
    sg = 0;
  }
  return ABD_OK;
}

int LooSummary::stats(abd_ctx* c) {
  const abdi::PsisLaunch p = abdi::psis_launch(mat, cells, out, tail, ld, capacity(), capacity());
  HIP_TRY(launch_kernel(p.kernel, dim3((unsigned)ld), dim3(abdi::kPsisThreads), 0, c->stream, p.args));
  return ABD_OK;
}
