// abd_sampler_summaries.hip -- what a caller of the native sampler (abd_sampler.hip) uses before the first run or after a run:
// switching on and reading the running sums, the accumulators, the per-draw summaries (abd_sampler.hpp) and the leapfrog log,
// and the adaptation.  No kernel is defined here; the launches of a draw are queue_draw's (abd_sampler.hip).
#include "abd_sampler.hpp"

namespace {

// ABD_OK, or what the error e of a device allocation becomes: out of memory names the `bytes` of `name``of` (`tail` closes it)
int alloc_rc(hipError_t e, const char* name, const char* of, size_t bytes, const char* tail = "") {
  if (e == hipSuccess) return ABD_OK;
  if (e != hipErrorOutOfMemory) return fail(ABD_ERR_HIP, "%s%s: %s", name, of, hipGetErrorString(e));
  (void)hipGetLastError();
  return fail(ABD_ERR_NOMEM, "%s%s: %zu bytes of device memory%s", name, of, bytes, tail);
}

// What every read-out begins with: the sampler is there, k is one of its chains, what is read is on() -- else ABD_ERR_STATE
// with the text `off`, which may name `arg` -- the device is set and every stream that may still write the buffers is drained:
// the context's, which a run call joins every pipe into, and the dense chains' side streams (which sampler_run_trains has
// synchronised before a run call returns: DESIGN 23)
template <typename On>
int readout(abd_sampler* s, int32_t k, On on, const char* off, const char* arg = "") {
  if (!s) return fail(ABD_ERR_ARG, "sampler is NULL");
  if (k < 0 || k >= s->n) return fail(ABD_ERR_ARG, "k=%d outside [0, %d)", k, s->n);
  if (!on()) return fail(ABD_ERR_STATE, off, arg, arg);
  HIP_TRY(hipSetDevice(s->c->device));
  HIP_TRY(hipStreamSynchronize(s->c->stream));
  for (const auto& d : s->dc)
    if (d.side) HIP_TRY(hipStreamSynchronize(d.side));
  return ABD_OK;
}

// entries [first, first + count) of the `have` a chain has: `what` is "<summary>: <entries>", `verb` what the chain does to them
int check_window(const char* what, const char* verb, int64_t first, int64_t count, int64_t have) {
  if (first < 0 || count < 0 || first > have || count > have - first)
    return fail(ABD_ERR_ARG, "%s [%lld, %lld) are beyond the %lld the chain %s", what, (long long)first, (long long)(first + count),
                (long long)have, verb);
  return ABD_OK;
}

// A per-chain block of `rows` x `cols` accumulators (abd_sampler_enable_pointwise / _predictive: K_s + K_n columns;
// _individual_loglik: N): the old one freed, a new one allocated and zeroed if `accumulate` (after the upload of the reading
// order if the launches read it: `order`)
int enable_acc(abd_sampler* s, DevBuf<double>& acc, int rows, size_t cols, int32_t accumulate, bool order, const char* what) {
  if (s->ran) return fail(ABD_ERR_STATE, "%s accumulation must be enabled before the first abd_sampler_run call", what);
  abd_ctx* c = s->c;
  HIP_TRY(hipSetDevice(c->device));
  if (acc) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    acc.reset();
  }
  if (!accumulate) return ABD_OK;
  if (order)
    if (int rc = upload_order(c)) return rc;
  const size_t n_acc = std::max<size_t>(1, (size_t)s->n * rows * cols);
  DevBuf<double> fresh;  // (acc stays empty unless the block is there and zeroed)
  if (int rc = alloc_rc(fresh.alloc_zero(n_acc, c->stream), what, " accumulators", n_acc * sizeof(double))) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  acc = std::move(fresh);
  return ABD_OK;
}

// Chain k's block of `rows` x `cols` accumulators, once every update has landed, as three rows of `cols` values: row v of
// column r is at(h, v, r) of the host copy h, and `place` puts it where it belongs in the caller's array; n_draws: the draws
// the block holds
template <typename At, typename Place>
int read_acc(abd_sampler* s, const double* acc, int32_t k, int rows, size_t cols, const char* what, int64_t* n_draws, At at, Place place) {
  if (int rc = readout(s, k, [&] { return acc != nullptr; }, "%s accumulation is not enabled (abd_sampler_enable_%s)", what)) return rc;
  std::vector<double> h((size_t)rows * cols);
  if (cols) HIP_TRY(hipMemcpy(h.data(), acc + (size_t)k * rows * cols, h.size() * sizeof(double), hipMemcpyDeviceToHost));
  place([hp = h.data(), at](int v, size_t r) { return at(hp, v, r); });
  if (n_draws) *n_draws = abdi::n_draws(s);
  return ABD_OK;
}

// where read_acc's three rows go: columns that are sorted readings back to the caller's reading order (S readings, then N) ...
auto by_reading(const abd_ctx* c, double* out) {
  return [c, out](auto value) {
    const size_t Ks = (size_t)c->s.K, Kt = Ks + (size_t)c->n.K;
    const ReadingOut o[3] = {{out, out + Ks}, {out + Kt, out + Kt + Ks}, {out + 2 * Kt, out + 2 * Kt + Ks}};
    scatter_readings(c, o, value);
  };
}
// ... and columns that are in the caller's order already
auto as_they_are(size_t cols, double* out) {
  return [cols, out](auto value) {
    for (int v = 0; v < 3; ++v)
      for (size_t r = 0; r < cols; ++r) out[v * cols + r] = value(v, r);
  };
}
// rows M, S, mean, M2 of `cols` columns -> M + log S = log sum exp(ll) (-inf before the first draw), mean, M2
auto lse_mean_m2(size_t cols) {
  return [cols](const double* h, int v, size_t r) { return v == 0 ? h[r] + std::log(h[cols + r]) : h[(v + 1) * cols + r]; };
}

// What the four abd_sampler_enable_* do alike once their arguments are good: refuse after the first run call, drop what the
// summary holds (nothing has been launched on it: the sampler has not run) and -- want -- let `alloc` fill a fresh one (its
// buffers on the context's stream, its parameters; returns the hipError_t), which the sampler takes whole or not at all.
// bytes: what an out-of-memory message names.
template <typename S, typename Alloc>
int enable_summary(abd_sampler* s, S& summary, const char* name, bool want, size_t bytes, Alloc alloc) {
  if (s->ran) return fail(ABD_ERR_STATE, "%s must be enabled before the first abd_sampler_run call", name);
  HIP_TRY(hipSetDevice(s->c->device));
  summary = S();
  if (!want) return ABD_OK;
  S fresh;
  if (int rc = alloc_rc(alloc(fresh), name, "", bytes)) return rc;
  HIP_TRY(hipStreamSynchronize(s->c->stream));  // (the buffers' zeroes)
  summary = std::move(fresh);
  return ABD_OK;
}

}  // namespace

extern "C" {

int abd_sampler_means(abd_sampler* s, int32_t k, double* i_mean, double* mu_n_mean, double* mu_s_mean, int64_t* n_draws) {
  if (int rc = readout(s, k, [&] { return s->d_sums != nullptr; }, "the sampler was created without accumulate")) return rc;
  abd_ctx* c = s->c;
  const size_t cells = (size_t)c->G * c->N;
  double* outs[3] = {i_mean, mu_n_mean, mu_s_mean};
  const double inv = s->n_accumulated ? 1.0 / (double)s->n_accumulated : 0.0;
  for (int v = 0; v < 3; ++v) {
    if (!outs[v]) continue;
    HIP_TRY(hipMemcpy(outs[v], s->d_sums + ((size_t)k * 3 + v) * cells, cells * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t e = 0; e < cells; ++e) outs[v][e] *= inv;
  }
  if (n_draws) *n_draws = s->n_accumulated;
  return ABD_OK;
}

static_assert(abdnuts::LOG_COLS == ABD_LEAPFROG_COLS && abdnuts::LOG_INIT == ABD_LEAPFROG_INIT && abdnuts::LOG_START == ABD_LEAPFROG_START &&
                  abdnuts::LOG_LEAF == ABD_LEAPFROG_LEAF && abdnuts::D == ABD_N_THETA,
              "abd_hip.h states the leapfrog log's row as abd_nuts.hpp writes it");

int abd_sampler_enable_leapfrog_log(abd_sampler* s, int64_t capacity_rows_per_chain) {
  if (!s) return fail(ABD_ERR_ARG, "sampler is NULL");
  if (capacity_rows_per_chain < 0) return fail(ABD_ERR_ARG, "capacity=%lld is negative", (long long)capacity_rows_per_chain);
  if (s->ran) return fail(ABD_ERR_STATE, "the leapfrog log must be enabled before the first abd_sampler_run call");
  for (auto& ch : s->ch) ch.nuts.attach_log(nullptr);
  s->lf_log.clear();
  if (capacity_rows_per_chain == 0) return ABD_OK;
  try {
    s->lf_log.assign((size_t)s->n, abdnuts::LeapfrogLog(capacity_rows_per_chain));
  } catch (const std::bad_alloc&) {
    s->lf_log.clear();
    return fail(ABD_ERR_NOMEM, "leapfrog log: %lld rows for each of %d chains", (long long)capacity_rows_per_chain, s->n);
  }
  for (int k = 0; k < s->n; ++k) s->ch[(size_t)k].nuts.attach_log(&s->lf_log[(size_t)k]);  // (row 0: the start point)
  return ABD_OK;
}

int abd_sampler_leapfrog_log(abd_sampler* s, int32_t k, int64_t first, int64_t count, double* rows, int64_t* n_total) {
  if (int rc = readout(s, k, [&] { return !s->lf_log.empty(); }, "the leapfrog log is not enabled (abd_sampler_enable_leapfrog_log)")) return rc;
  const abdnuts::LeapfrogLog& log = s->lf_log[(size_t)k];
  if (n_total) *n_total = log.n_total;
  if (int rc = check_window("leapfrog log: rows", "holds", first, count, log.stored())) return rc;
  if (count && !rows) return fail(ABD_ERR_ARG, "rows is NULL");
  if (count) std::memcpy(rows, log.rows.data() + (size_t)first * abdnuts::LOG_COLS, (size_t)count * abdnuts::LOG_COLS * sizeof(double));
  return ABD_OK;
}

int abd_sampler_enable_pointwise(abd_sampler* s, int32_t accumulate) {
  if (!s) return fail(ABD_ERR_ARG, "sampler is NULL");
  return enable_acc(s, s->d_pw_acc, 4, (size_t)(s->c->s.K + s->c->n.K), accumulate, false, "pointwise");
}

int abd_sampler_pointwise_stats(abd_sampler* s, int32_t k, double* out, int64_t* n_draws) {
  if (!s || !out) return fail(ABD_ERR_ARG, "NULL argument");
  const size_t Kt = (size_t)(s->c->s.K + s->c->n.K);
  return read_acc(s, s->d_pw_acc, k, 4, Kt, "pointwise", n_draws, lse_mean_m2(Kt), by_reading(s->c, out));
}

int abd_sampler_enable_individual_loglik(abd_sampler* s, int32_t accumulate) {
  if (!s) return fail(ABD_ERR_ARG, "sampler is NULL");
  return enable_acc(s, s->d_ind_acc, 4, (size_t)s->c->N, accumulate, false, "individual_loglik");
}

int abd_sampler_individual_loglik_stats(abd_sampler* s, int32_t k, double* out, int64_t* n_draws, int64_t* n_readings) {
  if (!s || !out) return fail(ABD_ERR_ARG, "NULL argument");
  const abd_ctx* c = s->c;
  const size_t N = (size_t)c->N;  // (the individuals are in the caller's order: nothing to scatter)
  if (int rc = read_acc(s, s->d_ind_acc, k, 4, N, "individual_loglik", n_draws, lse_mean_m2(N), as_they_are(N, out))) return rc;
  if (n_readings) {
    for (size_t j = 0; j < N; ++j)
      n_readings[j] = (int64_t)(c->seg_s[j + 1] - c->seg_s[j]) + (int64_t)(c->seg_n[j + 1] - c->seg_n[j]);
  }
  return ABD_OK;
}

int abd_sampler_enable_predictive(abd_sampler* s, int32_t accumulate) {
  if (!s) return fail(ABD_ERR_ARG, "sampler is NULL");
  return enable_acc(s, s->d_pp_acc, 3, (size_t)(s->c->s.K + s->c->n.K), accumulate, true, "predictive");
}

int abd_sampler_predictive_stats(abd_sampler* s, int32_t k, double* out, int64_t* n_draws) {
  if (!s || !out) return fail(ABD_ERR_ARG, "NULL argument");
  const size_t Kt = (size_t)(s->c->s.K + s->c->n.K);
  return read_acc(s, s->d_pp_acc, k, 3, Kt, "predictive", n_draws, [Kt](const double* h, int v, size_t r) { return h[v * Kt + r]; },
                  by_reading(s->c, out));
}

int abd_sampler_enable_curves(abd_sampler* s, int64_t capacity, double thr_s, double thr_n) {
  if (!s) return fail(ABD_ERR_ARG, "sampler is NULL");
  if (capacity < 0) return fail(ABD_ERR_ARG, "capacity=%lld is negative", (long long)capacity);
  const abd_ctx* c = s->c;
  CurvesSummary f;
  f.capacity = capacity, f.thr_s = thr_s, f.thr_n = thr_n;
  return enable_summary(s, s->curves, "curves", capacity > 0, f.row_at(c, s->n, 0) * sizeof(unsigned long long), [&](CurvesSummary& x) {
    x = std::move(f);
    hipError_t e = x.rows.alloc(x.row_at(c, s->n, 0));
    if (e == hipSuccess) e = x.scratch.alloc(x.scratch_at(c, s->n));
    return e;
  });
}

int abd_sampler_curves(abd_sampler* s, int32_t k, int64_t first, int64_t count, int64_t* counts, int64_t* n_infections, double* titer_sums,
                       int64_t* n_draws) {
  if (int rc = readout(s, k, [&] { return s->curves.on(); }, "curves are not enabled (abd_sampler_enable_curves)")) return rc;
  if (n_draws) *n_draws = abdi::n_draws(s);
  if (int rc = check_window("curves: draws", "has", first, count, abdi::n_draws(s))) return rc;
  if (count == 0) return ABD_OK;
  abd_ctx* c = s->c;
  const size_t n_row = curves_row_cols(c), G = (size_t)c->G;
  std::vector<unsigned long long> h((size_t)count * n_row);
  HIP_TRY(hipMemcpy(h.data(), s->curves.rows + s->curves.row_at(c, k, first), h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  for (size_t d = 0; d < (size_t)count; ++d)
    split_curves_row(c, h.data() + d * n_row, counts ? counts + d * 4 * G : nullptr, n_infections ? n_infections + d * 8 : nullptr,
                     titer_sums ? titer_sums + d * 2 * G : nullptr);
  return ABD_OK;
}

int abd_sampler_enable_diagnostics(abd_sampler* s, int64_t planned_draws, int64_t batch_len) {
  if (!s) return fail(ABD_ERR_ARG, "sampler is NULL");
  if (planned_draws < 0 || planned_draws == 1) return fail(ABD_ERR_ARG, "diagnostics: planned_draws=%lld is neither 0 nor >= 2", (long long)planned_draws);
  if (planned_draws && batch_len < 1) return fail(ABD_ERR_ARG, "diagnostics: batch_len=%lld is below 1", (long long)batch_len);
  const abd_ctx* c = s->c;
  DiagSummary f;
  f.draws = planned_draws, f.H = planned_draws / 2, f.L = batch_len;
  const size_t cells = (size_t)c->G * c->N;
  const size_t bytes =
      f.tit_at(c, s->n) * sizeof(double) + f.inf_at(c, s->n) * sizeof(uint32_t) + (f.cb2_at(c, s->n) + cells) * sizeof(unsigned long long);
  return enable_summary(s, s->diag, "diagnostics", planned_draws > 0, bytes, [&](DiagSummary& x) {
    x = std::move(f);
    hipError_t e = x.tit.alloc_zero(std::max<size_t>(1, x.tit_at(c, s->n)), c->stream);
    if (e == hipSuccess) e = x.inf.alloc_zero(std::max<size_t>(1, x.inf_at(c, s->n)), c->stream);
    if (e == hipSuccess) e = x.cb2.alloc_zero(std::max<size_t>(1, x.cb2_at(c, s->n)), c->stream);
    if (e == hipSuccess) e = x.stage.alloc(std::max<size_t>(1, cells));
    return e;
  });
}

int abd_sampler_diagnostics(abd_sampler* s, int32_t k, int64_t* i_counts, double* ab_n_mu, double* ab_s_mu, int64_t* info) {
  if (int rc = readout(s, k, [&] { return s->diag.on(); }, "diagnostics are not enabled (abd_sampler_enable_diagnostics)")) return rc;
  const int64_t H = s->diag.H, L = s->diag.L, B = H / L;
  const int64_t have = abdi::n_draws(s), n0 = std::min(have, H), n1 = std::min(std::max<int64_t>(0, have - H), H);
  if (info) {
    info[0] = n0;
    info[1] = n1;
    info[2] = std::min(n0 / L, B) + std::min(n1 / L, B);
    info[3] = L;
  }
  abd_ctx* c = s->c;
  const size_t cells = (size_t)c->G * c->N;
  if (!cells) return ABD_OK;
  // one plane at a time through the staging plane: transposed on the device, copied out (the copy waits for the kernel and
  // the next kernel for the copy: the context's stream)
  auto plane = [&](const void* src, int stride, int width, void* out) -> int {
    if (int rc = launch_diag_export(c, src, stride, width, s->diag.stage, c->stream)) return rc;
    HIP_TRY(hipMemcpyAsync(out, s->diag.stage, cells * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return ABD_OK;
  };
  if (i_counts) {
    const uint32_t* inf = s->diag.inf + s->diag.inf_at(c, k);
    const int comp[3] = {0, 1, 3};  // c_h0, c_h1, sum_cb of the 16-byte element (cur is not handed out)
    for (int v = 0; v < 3; ++v)
      if (int rc = plane(inf + comp[v], 16, 4, i_counts + (size_t)v * cells)) return rc;
    if (int rc = plane(s->diag.cb2 + s->diag.cb2_at(c, k), 8, 8, i_counts + 3 * cells)) return rc;
  }
  double* outs[2] = {ab_n_mu, ab_s_mu};
  const int planes[6] = {0, 1, 2, 3, 5, 6};  // mean_h0, M2_h0, mean_h1, M2_h1, bm_mean, bm_M2 (cur is not handed out)
  for (int x = 0; x < 2; ++x) {
    if (!outs[x]) continue;
    for (int v = 0; v < 6; ++v)
      if (int rc = plane(s->diag.tit + s->diag.tit_at(c, k, x, planes[v]), 8, 8, outs[x] + (size_t)v * cells)) return rc;
  }
  return ABD_OK;
}

int abd_sampler_enable_timelines(abd_sampler* s, int64_t planned_draws, double lo_n, double hi_n, double lo_s, double hi_s) {
  if (!s) return fail(ABD_ERR_ARG, "sampler is NULL");
  if (planned_draws < 0 || planned_draws > ABD_TIMELINE_MAX_DRAWS)
    return fail(ABD_ERR_ARG, "timelines: planned_draws=%lld outside [0, %d] (16-bit counters)", (long long)planned_draws, ABD_TIMELINE_MAX_DRAWS);
  if (planned_draws) {
    const struct { const char* name; double lo, hi; } ag[2] = {{"ab_n_mu", lo_n, hi_n}, {"ab_s_mu", lo_s, hi_s}};
    for (const auto& x : ag)
      if (!std::isfinite(x.lo) || !std::isfinite(x.hi) || !(x.lo < x.hi) || !std::isfinite(x.hi - x.lo))
        return fail(ABD_ERR_ARG, "timelines: the range [%g, %g) of %s is not finite and ascending", x.lo, x.hi, x.name);
  }
  const abd_ctx* c = s->c;
  TimelineSummary f;
  f.draws = planned_draws;
  f.range_n[0] = lo_n, f.range_n[1] = hi_n, f.range_s[0] = lo_s, f.range_s[1] = hi_s;
  // staging of the read-out: a plane of 8 bytes per cell, and at least one gap's row of histograms
  f.stage_bytes = std::max((size_t)c->G * c->N * sizeof(unsigned long long), (size_t)c->N * ABD_TIMELINE_BINS * sizeof(uint16_t));
  const size_t bytes = (f.hist_at(c, s->n) + f.cell_at(c, s->n) + f.ninf_at(c, s->n)) * sizeof(uint32_t) + f.stage_bytes;
  return enable_summary(s, s->timelines, "timelines", planned_draws > 0, bytes, [&](TimelineSummary& x) {
    x = std::move(f);
    hipError_t e = x.hist.alloc_zero(x.hist_at(c, s->n), c->stream);
    if (e == hipSuccess) e = x.cell.alloc_zero(x.cell_at(c, s->n), c->stream);
    if (e == hipSuccess) e = x.ninf.alloc_zero(x.ninf_at(c, s->n), c->stream);
    if (e == hipSuccess) e = x.stage.alloc(x.stage_bytes / sizeof(unsigned long long));
    return e;
  });
}

int abd_sampler_timelines(abd_sampler* s, int32_t k, uint16_t* hist_n, uint16_t* hist_s, int64_t* inf, int64_t* cum, int64_t* ninf,
                          int64_t* n_draws) {
  if (int rc = readout(s, k, [&] { return s->timelines.on(); }, "timelines are not enabled (abd_sampler_enable_timelines)")) return rc;
  if (n_draws) *n_draws = abdi::n_draws(s);
  if (!hist_n && !hist_s && !inf && !cum && !ninf) return ABD_OK;
  abd_ctx* c = s->c;
  const size_t cells = (size_t)c->G * c->N, N = (size_t)c->N, line = ABD_TIMELINE_BINS * sizeof(uint16_t);
  // through the staging buffer on the context's stream: the copy waits for the kernel and the next kernel for the copy
  int64_t* planes[2] = {inf, cum};
  for (int v = 0; v < 2; ++v) {
    if (!planes[v]) continue;
    if (int rc = launch_diag_export(c, s->timelines.cell + s->timelines.cell_at(c, k) + v, 8, 4, s->timelines.stage, c->stream)) return rc;
    HIP_TRY(hipMemcpyAsync(planes[v], s->timelines.stage, cells * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  uint16_t* hists[2] = {hist_n, hist_s};
  const int rows = (int)std::max<size_t>(1, std::min<size_t>((size_t)c->G, s->timelines.stage_bytes / (N * line)));  // gap rows per pass
  for (int v = 0; v < 2; ++v) {
    if (!hists[v]) continue;
    const uint32_t* src = s->timelines.hist + s->timelines.hist_at(c, k, v);
    for (int g0 = 0; g0 < c->G; g0 += rows) {
      const int n_g = std::min(rows, c->G - g0);
      if (int rc = launch_timeline_hist_export(c, src, g0, n_g, s->timelines.stage, c->stream)) return rc;
      HIP_TRY(hipMemcpyAsync(hists[v] + (size_t)g0 * N * ABD_TIMELINE_BINS, s->timelines.stage, (size_t)n_g * N * line, hipMemcpyDeviceToHost,
                             c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
    }
  }
  if (ninf) {
    std::vector<uint32_t> h(N * ABD_TIMELINE_NINF);
    HIP_TRY(hipMemcpy(h.data(), s->timelines.ninf + s->timelines.ninf_at(c, k), h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (size_t e = 0; e < h.size(); ++e) ninf[e] = (int64_t)h[e];
  }
  return ABD_OK;
}

int abd_sampler_timeline_quantiles(abd_sampler* s, int32_t n_q, const double* q, double* out_n, double* out_s) {
  if (!s) return fail(ABD_ERR_ARG, "sampler is NULL");
  if (n_q < 1 || n_q > ABD_TIMELINE_MAX_Q) return fail(ABD_ERR_ARG, "timelines: n_q=%d outside [1, %d]", n_q, ABD_TIMELINE_MAX_Q);
  if (!q) return fail(ABD_ERR_ARG, "timelines: q is NULL");
  for (int e = 0; e < n_q; ++e)
    if (!(q[e] >= 0.0 && q[e] <= 1.0)) return fail(ABD_ERR_ARG, "timelines: q[%d]=%g outside [0, 1]", e, q[e]);
  // (the histograms are pooled over the chains: there is no k, and chain 0 is always one of them)
  if (int rc = readout(s, 0, [&] { return s->timelines.on(); }, "timelines are not enabled (abd_sampler_enable_timelines)")) return rc;
  if (!out_n && !out_s) return ABD_OK;
  abd_ctx* c = s->c;
  const size_t cells = (size_t)c->G * c->N;
  DevBuf<double> d_q, d_out;  // the read-out's own: n_q planes of 8 bytes per cell
  hipError_t e = d_q.upload(q, (size_t)n_q);
  if (e == hipSuccess) e = d_out.alloc((size_t)n_q * cells);
  if (int rc = alloc_rc(e, "timelines", "", (size_t)n_q * cells * sizeof(double), " for the quantiles")) return rc;
  double* outs[2] = {out_n, out_s};
  const double* ranges[2] = {s->timelines.range_n, s->timelines.range_s};
  for (int v = 0; v < 2; ++v) {
    if (!outs[v]) continue;
    const TimelineSummary& tl = s->timelines;  // (chain 0's plane of titer v; a chain's planes are hist_at(c, 1) words apart)
    if (int rc = launch_timeline_quantiles(c, tl.hist + tl.hist_at(c, 0, v), (int64_t)tl.hist_at(c, 1), s->n, ranges[v], n_q, d_q, d_out,
                                           c->stream))
      return rc;
    HIP_TRY(hipMemcpyAsync(outs[v], d_out, (size_t)n_q * cells * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  return ABD_OK;
}

int abd_sampler_enable_risk(abd_sampler* s, int64_t capacity, const abd_risk_spec* spec) {
  if (!s) return fail(ABD_ERR_ARG, "sampler is NULL");
  if (capacity < 0) return fail(ABD_ERR_ARG, "capacity=%lld is negative", (long long)capacity);
  const abd_ctx* c = s->c;
  if (capacity > 0 && !s->ran)  // (a sampler that has run is refused below, whatever the spec)
    if (int rc = check_risk_spec(c, spec)) return rc;
  RiskSummary f;
  f.capacity = capacity;
  if (capacity > 0 && spec) f.spec = *spec;
  return enable_summary(s, s->risk, "risk", capacity > 0, f.table_at(c, s->n, 0) * sizeof(uint32_t), [&](RiskSummary& x) {
    x = std::move(f);
    hipError_t e = x.tables.alloc(x.table_at(c, s->n, 0));
    if (e == hipSuccess) e = x.scratch.alloc(x.scratch_at(c, s->n));
    return e;
  });
}

int abd_sampler_risk(abd_sampler* s, int32_t k, int64_t first, int64_t count, int64_t* table, int64_t* n_draws) {
  if (int rc = readout(s, k, [&] { return s->risk.on(); }, "risk is not enabled (abd_sampler_enable_risk)")) return rc;
  if (n_draws) *n_draws = abdi::n_draws(s);
  if (int rc = check_window("risk: draws", "has", first, count, abdi::n_draws(s))) return rc;
  if (count == 0 || !table) return ABD_OK;
  abd_ctx* c = s->c;
  const size_t n_tab = risk_table_cols(c);
  std::vector<uint32_t> h((size_t)count * n_tab);
  HIP_TRY(hipMemcpy(h.data(), s->risk.tables + s->risk.table_at(c, k, first), h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  for (size_t e = 0; e < h.size(); ++e) table[e] = (int64_t)h[e];
  return ABD_OK;
}

int abd_sampler_enable_loo(abd_sampler* s, int64_t draws_per_chain, int32_t thin) {
  if (!s) return fail(ABD_ERR_ARG, "sampler is NULL");
  if (draws_per_chain < 0) return fail(ABD_ERR_ARG, "loo: draws_per_chain=%lld is negative", (long long)draws_per_chain);
  if (thin < 1) return fail(ABD_ERR_ARG, "loo: thin=%d is below 1", thin);
  const abd_ctx* c = s->c;
  LooSummary f;
  f.draws = draws_per_chain, f.thin = thin, f.C = (draws_per_chain + thin - 1) / thin;
  f.ld = std::max<size_t>(64, ((size_t)c->N + 63) / 64 * 64);
  if (f.C > ABD_SAMPLER_LOO_MAX_DRAWS || (int64_t)s->n * f.C > ABD_SAMPLER_LOO_MAX_DRAWS)
    return fail(ABD_ERR_ARG, "loo: %d chains x %lld kept draws = %lld pass the cap of %d draws (a larger thin fits)", s->n, (long long)f.C,
                (long long)s->n * (long long)f.C, ABD_SAMPLER_LOO_MAX_DRAWS);
  f.stored.assign((size_t)s->n, 0);
  f.staged.assign((size_t)s->n, 0);
  const size_t n_mat = f.ld * (size_t)f.capacity(), n_stage = (size_t)s->n * 2 * LooSummary::kStage * f.ld;
  const size_t bytes = (n_mat + n_stage + 3 * f.ld) * sizeof(double) + 2 * f.ld * sizeof(int32_t);
  return enable_summary(s, s->loo, "loo", draws_per_chain > 0, bytes, [&](LooSummary& x) {
    x = std::move(f);
    // every individual's readings of both antigens; 0 in the padding
    std::vector<int32_t> cells(x.ld, 0);
    for (size_t j = 0; j < (size_t)c->N; ++j) cells[j] = (c->seg_s[j + 1] - c->seg_s[j]) + (c->seg_n[j + 1] - c->seg_n[j]);
    hipError_t e = x.mat.alloc(std::max<size_t>(1, n_mat));
    if (e == hipSuccess) e = x.stage.alloc_zero(n_stage, c->stream);  // (its padding columns are never written)
    if (e == hipSuccess) e = x.out.alloc(3 * x.ld);
    if (e == hipSuccess) e = x.tail.alloc(x.ld);
    if (e == hipSuccess) e = x.cells.upload(cells.data(), x.ld);
    return e;
  });
}

int abd_sampler_loo_rows(abd_sampler* s, int32_t k, int64_t first, int64_t count, double* ll, int64_t* n_rows) {
  if (int rc = readout(s, k, [&] { return s->loo.on(); }, "loo is not enabled (abd_sampler_enable_loo)")) return rc;
  const LooSummary& x = s->loo;
  const int64_t have = x.stored[(size_t)k];
  if (n_rows) *n_rows = have;
  if (int rc = check_window("loo: rows", "holds", first, count, have)) return rc;
  if (count == 0 || !ll) return ABD_OK;
  // the chain's columns [first, first + count) of every individual's row, then turned to draw-major
  const size_t N = (size_t)s->c->N, n = (size_t)count;
  std::vector<double> h(N * n);
  HIP_TRY(hipMemcpy2D(h.data(), n * sizeof(double), x.mat + (size_t)k * x.C + (size_t)first, (size_t)x.capacity() * sizeof(double),
                      n * sizeof(double), N, hipMemcpyDeviceToHost));
  for (size_t j = 0; j < N; ++j)
    for (size_t d = 0; d < n; ++d) ll[d * N + j] = h[j * n + d];
  return ABD_OK;
}

int abd_sampler_loo_stats(abd_sampler* s, double* elpd_loo, double* pareto_k, double* lppd, int32_t* n_tail, int64_t* n_draws,
                          int64_t* n_readings) {
  if (s && (!elpd_loo || !pareto_k || !lppd || !n_tail)) return fail(ABD_ERR_ARG, "NULL argument");
  if (int rc = readout(s, 0, [&] { return s->loo.on(); }, "loo is not enabled (abd_sampler_enable_loo)")) return rc;
  LooSummary& x = s->loo;
  abd_ctx* c = s->c;
  // (the matrix's rows are contiguous only when every chain's columns are full)
  for (int k = 0; k < s->n; ++k)
    if (x.stored[(size_t)k] != x.C)
      return fail(ABD_ERR_STATE, "loo: chain %d holds %lld of its %lld rows: the statistics are those of a finished run", k,
                  (long long)x.stored[(size_t)k], (long long)x.C);
  if (int rc = x.stats(c)) return rc;
  const size_t N = (size_t)c->N, ld = x.ld;
  std::vector<double> h(3 * ld);
  std::vector<int32_t> ht(ld);
  HIP_TRY(hipMemcpyAsync(h.data(), x.out, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(ht.data(), x.tail, ht.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (size_t j = 0; j < N; ++j) {  // (the individuals are in the caller's order: nothing to scatter)
    elpd_loo[j] = h[j];
    pareto_k[j] = h[ld + j];
    lppd[j] = h[2 * ld + j];
    n_tail[j] = ht[j];
    if (n_readings) n_readings[j] = (int64_t)(c->seg_s[j + 1] - c->seg_s[j]) + (int64_t)(c->seg_n[j + 1] - c->seg_n[j]);
  }
  if (n_draws) *n_draws = x.capacity();
  return ABD_OK;
}

int abd_sampler_adaptation(abd_sampler* s, int32_t k, double* inv_mass, double* step_size, double* metric) {
  if (!s) return fail(ABD_ERR_ARG, "sampler is NULL");
  if (k < 0 || k >= s->n) return fail(ABD_ERR_ARG, "k=%d outside [0, %d)", k, s->n);
  const abdnuts::Nuts& nu = s->ch[(size_t)k].nuts;
  if (inv_mass) std::memcpy(inv_mass, nu.inv_mass, sizeof(double) * ABD_N_THETA);
  if (step_size) *step_size = nu.eps;
  if (metric)
    for (int r = 0; r < ABD_N_THETA; ++r)
      for (int c = 0; c < ABD_N_THETA; ++c)
        metric[r * ABD_N_THETA + c] = nu.dense ? nu.cov[r][c] : (r == c ? nu.inv_mass[r] : 0.0);
  return ABD_OK;
}

int abd_sampler_set_adaptation(abd_sampler* s, int32_t k, const double* inv_mass, double step_size) {
  if (!s) return fail(ABD_ERR_ARG, "sampler is NULL");
  if (k < 0 || k >= s->n) return fail(ABD_ERR_ARG, "k=%d outside [0, %d)", k, s->n);
  abdnuts::AdaptiveNuts& ch = s->ch[(size_t)k];
  if (ch.nuts.dense) return fail(ABD_ERR_STATE, "chain %d runs a dense metric", k);
  if (inv_mass)
    for (int d = 0; d < ABD_N_THETA; ++d)
      if (!(inv_mass[d] > 0.0) || !std::isfinite(inv_mass[d])) return fail(ABD_ERR_ARG, "inv_mass[%d]=%g is not a positive finite number", d, inv_mass[d]);
  if (step_size > 0.0 && !std::isfinite(step_size)) return fail(ABD_ERR_ARG, "step_size is not finite");
  ch.install(inv_mass, step_size);
  return ABD_OK;
}

}  // extern "C"
