// abd_gibbs.hip -- the device Gibbs sweep of the C ABI (abd_gibbs_sweep; include/abd_hip.h): what PyMC's
// BinaryGibbsMetropolis does to [i_raw, ab_s_waner] inside pm.sample (abd.py:922).
#include "abd_host.hpp"
#include "abd_gibbs_lists.hpp"
#include "abd_gibbs_dense.hpp"

namespace abdi {

using GibbsKernel = void (*)(const GibbsArgs);
// dense panels: lanes = proposals (abd_gibbs_dense.hpp; `stats`: the variant with the scheduler's development counters and the
// decision log; for lists it selects the logging instantiation);
// observation lists: lanes = observations (abd_gibbs_lists.hpp).  Both for 4 or 8 words per individual (<= 256 / <= 512 gaps);
// lists of at most 64 gaps -- the reference's own cohorts have 26 and 31 -- get a one-word instantiation: it holds the
// individual's packed rows in scalar registers, and with one word instead of four they fit (profiles/r04)
template <typename R>
GibbsKernel gibbs_kernel(const abd_ctx* c, bool stats) {
  const bool wide = c->nt > ABD_MAXT;
  if (c->dense && stats) return wide ? abd_gibbs_dense_kernel<R, true, ABD_MAXT_MAX> : abd_gibbs_dense_kernel<R, true, ABD_MAXT>;
  if (c->dense) return wide ? abd_gibbs_dense_kernel<R, false, ABD_MAXT_MAX> : abd_gibbs_dense_kernel<R, false, ABD_MAXT>;
  if (stats && c->nt == 1) return abd_gibbs_kernel<R, 1, true>;
  if (stats) return wide ? abd_gibbs_kernel<R, ABD_MAXT_MAX, true> : abd_gibbs_kernel<R, ABD_MAXT, true>;
  if (c->nt == 1) return abd_gibbs_kernel<R, 1>;
  return wide ? abd_gibbs_kernel<R, ABD_MAXT_MAX> : abd_gibbs_kernel<R, ABD_MAXT>;
}

int enqueue_gibbs(abd_ctx* c, int m, const int32_t* chains, const double* theta, uint64_t seed, uint32_t sweep,
                         uint32_t stream_offset, hipStream_t st, unsigned long long* counts_dev, unsigned int* work_dev,
                         unsigned long long* stats_dev, const GibbsLogDev& log) {
  GibbsArgs ga;
  base_args(c, ga.e);
  ga.e.n_chains = m;
  ga.seed_lo = (uint32_t)seed;
  ga.seed_hi = (uint32_t)(seed >> 32);
  ga.sweep = sweep;
  ga.ind_offset = c->ind_offset;
  ga.counts = counts_dev;
  for (int k = 0; k < m; ++k) {
    const double* t = theta + (size_t)k * ABD_N_THETA;
    ga.e.ch[k] = chain_par(c, chains[k], t);
    const Transformed tr = transform(t);
    ga.stream[k] = (uint32_t)chains[k] + stream_offset;
    ga.theta0[k] = t[0];
    ga.theta7[k] = t[7];
    ga.is2_n[k] = 1.0 / (tr.sig_n * tr.sig_n);
    ga.is2_s[k] = 1.0 / (tr.sig_s * tr.sig_s);
  }
  HIP_TRY(hipMemsetAsync(counts_dev, 0, (size_t)m * 2 * sizeof(unsigned long long), st));
  ga.work = work_dev;
  ga.refill_min = c->g2_refill_min;
  ga.tail_lanes = c->g2_tail_lanes;
  ga.tail_age = c->g2_tail_age;
  ga.stats = stats_dev;
  ga.log = log.rec;
  ga.log_n = log.n;
  ga.log_cap = log.cap;
  if (stats_dev) HIP_TRY(hipMemsetAsync(stats_dev, 0, 8 * sizeof(unsigned long long), st));
  dim3 grid, block(ABD_BLOCK);
  size_t lds;
  if (c->dense) {
    const int rbytes = c->storage == ABD_STORE_F32 ? 4 : 8;
    int nw2 = abd_g2_waves(c->G, rbytes);  // waves of a workgroup = of a CU: as many as its LDS holds, 4 .. 12
    // a one-chain sweep is a sampler unit's: with 8 waves per CU (2 per SIMD) the other units' evaluation kernels find room
    // beside it (12 waves x 168 registers fill the CU's register file); the sweep itself 0.39 -> 0.41 ms, the compound
    // iteration of 4 chains at config 3 6.17 -> 5.90 ms.  Trajectories do not depend on the launch shape.
    if (m == 1) nw2 = std::max(ABD_G2_MIN_WAVES, std::min(nw2, tune_int("ABD_G2_WAVES_ONE", 8)));
    // one workgroup per CU, the individuals of a chain handed out from one queue per chain
    lds = abd_g2_lds(c->G, rbytes, nw2);
    HIP_TRY(hipMemsetAsync(work_dev, 0, (size_t)m * sizeof(unsigned int), st));
    grid = dim3(std::max(1, std::min(c->n_cu / m, (c->N + nw2 - 1) / nw2)), m);
    block = dim3(64 * nw2);
  } else {
    grid = dim3(std::max(1, std::min((c->N + ABD_WAVES_PER_BLOCK - 1) / ABD_WAVES_PER_BLOCK, c->n_cu * 8)), m);
    lds = abd_gibbs_lds(c->G);
  }
  const bool stats = (c->dense && stats_dev != nullptr) || log.rec != nullptr;  // ABD_GIBBS_STATS=1, abd_gibbs_sweep_log
  const GibbsKernel k = c->storage == ABD_STORE_F32 ? gibbs_kernel<float>(c, stats) : gibbs_kernel<double>(c, stats);
  HIP_TRY(launch_kernel(k, grid, block, lds, st, ga));
  // the sweep rewrote iw (abd_gibbs.hpp: gibbs_store_state): the exposure planes of its chains follow on the same stream
  return enqueue_planes(c, m, chains, st);
}

}  // namespace abdi

static_assert(sizeof(abd_gibbs_record) == sizeof(GibbsRecord) && offsetof(abd_gibbs_record, log_u) == offsetof(GibbsRecord, log_u) &&
                  offsetof(abd_gibbs_record, dim) == offsetof(GibbsRecord, dim) && offsetof(abd_gibbs_record, gf) == offsetof(GibbsRecord, gf) &&
                  offsetof(abd_gibbs_record, stop) == offsetof(GibbsRecord, stop) && offsetof(abd_gibbs_record, path) == offsetof(GibbsRecord, path) &&
                  offsetof(abd_gibbs_record, accepted) == offsetof(GibbsRecord, accepted),
              "header / kernel record layout mismatch");
static_assert(ABD_GIBBS_PATH_PRIOR == ABD_GLOG_PRIOR && ABD_GIBBS_PATH_EARLY == ABD_GLOG_EARLY && ABD_GIBBS_PATH_WALK == ABD_GLOG_WALK &&
                  ABD_GIBBS_PATH_TAIL == ABD_GLOG_TAIL && ABD_GIBBS_PATH_WAVE_WANER == ABD_GLOG_WAVE_WANER &&
                  ABD_GIBBS_PATH_WAVE_OVERFLOW == ABD_GLOG_WAVE_OVERFLOW && ABD_GIBBS_PATH_LIST == ABD_GLOG_LIST &&
                  ABD_GIBBS_PATH_LIST_PRIOR == ABD_GLOG_LIST_PRIOR,
              "header / kernel path codes mismatch");

// the sweep of abd_gibbs_sweep; with `records`, logged (abd_gibbs_sweep_log)
static int gibbs_sweep(abd_ctx* c, int32_t n, const int32_t* chains, const double* theta, uint64_t seed, uint32_t sweep,
                       int64_t* accepted, int64_t* proposed, abd_gibbs_record* records, int64_t capacity, int32_t* n_records) {
  if (!c || !chains || !theta) return fail(ABD_ERR_ARG, "NULL argument");
  int rc = check_chains(c, n, chains);
  if (rc) return rc;
  for (int a = 0; a < n; ++a)
    for (int b = a + 1; b < n; ++b)
      if (chains[a] == chains[b]) return fail(ABD_ERR_ARG, "chain %d listed twice: a sweep updates its state in place", chains[a]);
  HIP_TRY(hipSetDevice(c->device));
  if (int frc = flush_ring(c)) return frc;
  std::vector<unsigned long long> counts((size_t)n * 2, 0);
  // the log of one launch's chains: device memory of this call alone
  DevBuf<GibbsRecord> d_rec;
  DevBuf<int32_t> d_nrec;
  const int m_max = std::min<int>(ABD_MAX_BATCH, n);
  if (records) {
    HIP_TRY(d_rec.alloc((size_t)m_max * (size_t)capacity));
    HIP_TRY(d_nrec.alloc((size_t)m_max * c->N));
  }
  static const bool want_stats = env_int("ABD_GIBBS_STATS", 0) != 0;
  for (int k0 = 0; k0 < n; k0 += ABD_MAX_BATCH) {
    const int m = std::min(ABD_MAX_BATCH, n - k0);
    unsigned long long* stats_dev = want_stats ? c->d_counts + (size_t)c->n_slots * 2 : nullptr;
    GibbsLogDev log;
    if (records) {
      log.rec = d_rec;
      log.n = d_nrec;
      log.cap = capacity;
      HIP_TRY(hipMemsetAsync(d_rec, 0, (size_t)m * (size_t)capacity * sizeof(GibbsRecord), c->stream));
      HIP_TRY(hipMemsetAsync(d_nrec, 0, (size_t)m * c->N * sizeof(int32_t), c->stream));
    }
    rc = enqueue_gibbs(c, m, chains + k0, theta + (size_t)k0 * ABD_N_THETA, seed, sweep, 0u, c->stream, c->d_counts,
                       c->d_work, stats_dev, log);
    if (rc) return rc;
    if (records) {
      HIP_TRY(hipMemcpyAsync(records + (size_t)k0 * (size_t)capacity, d_rec, (size_t)m * (size_t)capacity * sizeof(GibbsRecord),
                             hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipMemcpyAsync(n_records + (size_t)k0 * c->N, d_nrec, (size_t)m * c->N * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipMemcpyAsync(counts.data() + (size_t)k0 * 2, c->d_counts, (size_t)m * 2 * sizeof(unsigned long long),
                           hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (stats_dev) {
      unsigned long long st[8];
      HIP_TRY(hipMemcpy(st, stats_dev, sizeof st, hipMemcpyDeviceToHost));
      const double ni = (double)std::max<unsigned long long>(1, st[0]);
      std::fprintf(stderr, "[abd gibbs stats] individuals x chains %llu; per individual: iterations %.1f, refills %.1f, walk steps %.1f "
                   "(lanes busy %.1f of 64), tail finishes %.1f, commit scans %.1f, acceptances %.2f\n",
                   st[0], st[1] / ni, st[2] / ni, st[3] / ni, st[3] ? (double)st[4] / (double)st[3] : 0.0, st[5] / ni, st[6] / ni, st[7] / ni);
    }
  }
  for (int k = 0; k < n; ++k) {
    if (accepted) accepted[k] = (int64_t)counts[(size_t)k * 2];
    if (proposed) proposed[k] = (int64_t)counts[(size_t)k * 2 + 1];
  }
  return ABD_OK;
}

extern "C" {

int abd_gibbs_sweep(abd_ctx* c, int32_t n, const int32_t* chains, const double* theta, uint64_t seed, uint32_t sweep,
                    int64_t* accepted, int64_t* proposed) {
  return gibbs_sweep(c, n, chains, theta, seed, sweep, accepted, proposed, nullptr, 0, nullptr);
}

int abd_gibbs_sweep_log(abd_ctx* c, int32_t n, const int32_t* chains, const double* theta, uint64_t seed, uint32_t sweep,
                        int64_t* accepted, int64_t* proposed, abd_gibbs_record* records, int64_t capacity, int32_t* n_records) {
  if (!c || !records || !n_records) return fail(ABD_ERR_ARG, "NULL argument");
  if (capacity < (int64_t)c->N * (c->G + 1))
    return fail(ABD_ERR_ARG, "capacity %lld: a chain's log takes n_inds * (n_gaps + 1) = %lld records", (long long)capacity,
                (long long)c->N * (c->G + 1));
  return gibbs_sweep(c, n, chains, theta, seed, sweep, accepted, proposed, records, capacity, n_records);
}

}  // extern "C"
