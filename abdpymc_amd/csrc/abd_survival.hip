// abd_survival.hip -- the survival models of a finished run (include/abd_hip.h: abd_survival_*): creation of a
// handle of any form, the launches of the data sums and of the per-individual log-likelihood, the WAIC accumulators, PSIS-LOO
// over the resident matrix of those rows (abd_survival_loo_*; abd_psis.hpp), the posterior predictive checks
// (abd_survival_predictive_*, abd_survival_replicate), and at the end the ensemble of per-draw datasets, a handle of its
// own kind and of any form (abd_survival_draws_*), with its own per-individual log-likelihood, WAIC and PSIS-LOO per
// dataset.  Both kinds run their sums on one SurvivalSums through one launcher (survival_sums_launch) and their
// per-individual rows on one SurvivalPointRows through one launcher (survival_pointwise_kernel); what differs between them is the
// preparation of a point's rows and where the per-individual rows go.  A handle shares nothing with an abd_ctx.  The
// kernels are in abd_survival.hpp, abd_survival_groups.hpp, abd_survival_periods.hpp, abd_survival_pointwise.hpp and
// abd_survival_predictive.hpp; the closed forms, the packing of the planes and the form of a model (SurvivalForm) are plain C++ in
// the five *_terms.hpp beside them (SurvivalForm: at the end of abd_survival_groups_terms.hpp).
#include <algorithm>
#include <memory>

#include "abd_host.hpp"
#include "abd_psis.hpp"
#include "abd_survival.hpp"
#include "abd_survival_groups.hpp"
#include "abd_survival_groups_terms.hpp"
#include "abd_survival_periods.hpp"
#include "abd_survival_periods_terms.hpp"
#include "abd_survival_pointwise.hpp"
#include "abd_survival_pointwise_terms.hpp"
#include "abd_survival_predictive.hpp"
#include "abd_survival_predictive_terms.hpp"
#include "abd_survival_terms.hpp"

namespace abdi {
// what a creator decides: the rest of a handle follows from it and from the data
struct SurvivalSpec {
  SurvivalForm form;  // K titers, by group (abd_survival_groups.hpp) or by period (abd_survival_periods.hpp)
  int N = 0, device = 0;
  SurvivalPriors priors{};         // of the form with K titers
  SurvivalGroupsPriors gpriors{};  // of the forms by group and by period
};
constexpr int kSurvRepBatch = 4;  // points per launch of abd_survival_replicate: its per-cell buffer holds this many

// the layout of the grouped form (survival_groups_layout): a tile belongs to one group
struct SurvivalLayout {
  int ntile = 0;
  std::vector<int32_t> slot, tile_group, group_tile;
};

// What a launch of the data sums runs on, for a handle of either kind (abd_survival, abd_survival_draws): the device, the stream,
// the plan of the launch, the buffers of ABD_MAX_BATCH points and the two tables of the grouped layout.  A handle holds it by
// value, ahead of its own buffers: members go in reverse declaration order, so those are freed first, then the buffers here, and
// the stream is the last to go (abd_host.hpp).
struct SurvivalSums {
  int device = 0;
  int T = 0, ld = 0, ntile = 0, nseg = 0, seg_len = 0, nw = 0;
  int par_stride = 0, out_stride = 0;  // the rows of a point in d_par / h_par and in d_out / h_out
  Stream stream;
  DevBuf<double> d_par, d_s_part, d_w_part, d_out;
  DevBuf<double> d_w0_part;                    // by period: the second plane of partials
  DevBuf<int32_t> d_tile_group, d_group_tile;  // by group
  MappedBuf<double> h_par, h_out;  // pinned: the source and the target of the two copies of a launch
  std::vector<double> work;        // [ABD_MAX_BATCH] rows of the caller's: log lambda, 1 - lambda (and a form's own) of the points in flight

  // The one place that splits a launch: ntile tiles of 64 individuals, and ranges of intervals -- enough waves for the chip (about
  // 4096) while a wave keeps at least one interval.  From the tile count and T alone: the partial sums of two handles with the same
  // (ntile, T) are added in the same order, whatever their kind.
  void plan(int ntile_, int T_) {
    T = T_;
    ntile = ntile_;
    ld = ntile * 64;
    const int want_seg = std::max(1, std::min(T, (4096 + ntile - 1) / ntile));
    seg_len = (T + want_seg - 1) / want_seg;
    nseg = (T + seg_len - 1) / seg_len;
    nw = ntile * nseg;
  }
  // after plan(): the device (`dev` < 0: the current one), the stream and the buffers.  A row of par is the form's and
  // par_extra doubles of the handle's own; layout is null for the forms in the caller's order
  int alloc(int dev, const SurvivalForm& form, int par_extra, const SurvivalLayout* layout) {
    device = dev;
    par_stride = form.par_stride() + par_extra;
    out_stride = form.out_stride();
    work.resize((size_t)ABD_MAX_BATCH * form.work_stride());
    if (device < 0) HIP_TRY(hipGetDevice(&device));
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(stream.create());
    HIP_TRY(d_par.alloc((size_t)ABD_MAX_BATCH * par_stride));
    HIP_TRY(d_s_part.alloc((size_t)ABD_MAX_BATCH * ntile * T));
    HIP_TRY(d_w_part.alloc((size_t)ABD_MAX_BATCH * nw * ABD_SURV_NW));
    HIP_TRY(d_out.alloc((size_t)ABD_MAX_BATCH * out_stride));
    HIP_TRY(h_par.alloc_pinned((size_t)ABD_MAX_BATCH * par_stride));
    HIP_TRY(h_out.alloc_pinned((size_t)ABD_MAX_BATCH * out_stride));
    if (form.by_period()) HIP_TRY(d_w0_part.alloc((size_t)ABD_MAX_BATCH * ntile * T));
    if (layout) {
      HIP_TRY(d_tile_group.upload(layout->tile_group.data(), (size_t)ntile));
      HIP_TRY(d_group_tile.upload(layout->group_tile.data(), layout->group_tile.size()));
    }
    return ABD_OK;
  }
  // the rows of n <= ABD_MAX_BATCH points: h_par to the device ahead of the launches, and d_out back to h_out behind them
  int upload(int n) {
    HIP_TRY(hipMemcpyAsync(d_par, h_par.host(), (size_t)n * par_stride * sizeof(double), hipMemcpyHostToDevice, stream));
    return ABD_OK;
  }
  int download(int n) {
    HIP_TRY(hipMemcpyAsync(h_out.host(), d_out, (size_t)n * out_stride * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return ABD_OK;
  }
  dim3 grid(int n) const { return dim3((unsigned)((nw + 3) / 4), (unsigned)n); }  // of a sums kernel: a wave per (tile, range)
  void quiesce() {  // before the handle goes
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
  }
};

// What a launch of the per-individual log-likelihood runs on, for a handle of either kind: the parameter rows and the rows ll of
// ABD_MAX_BATCH points, on the device and pinned (abd_survival_pointwise.hpp).  Allocated at the first pointwise call.
struct SurvivalPointRows {
  int stride = 0;  // the parameter row of a point
  DevBuf<double> d_par, d_ll;     // [ABD_MAX_BATCH][stride], [ABD_MAX_BATCH][ld]
  MappedBuf<double> h_par, h_ll;  // pinned
  int ensure(int ld) {
    if (d_ll) return ABD_OK;
    HIP_TRY(d_par.alloc((size_t)ABD_MAX_BATCH * stride));
    HIP_TRY(h_par.alloc_pinned((size_t)ABD_MAX_BATCH * stride));
    HIP_TRY(h_ll.alloc_pinned((size_t)ABD_MAX_BATCH * ld));
    HIP_TRY(d_ll.alloc((size_t)ABD_MAX_BATCH * ld));
    return ABD_OK;
  }
};
}  // namespace abdi

struct abd_survival : SurvivalSpec {
  SurvivalSums sums;  // first: the last to go
  std::vector<double> Y;  // Y_t = sum_j y_jt
  double C = 0.0;         // sum_{y > 0} y log e - sum lgamma(y + 1)
  DevBuf<double> d_y, d_e, d_x0, d_x1;
  // the per-individual log-likelihood and its WAIC accumulators (abd_survival_pointwise.hpp)
  std::vector<int32_t> slot;       // [N] the column of individual j; empty: j itself (the ungrouped layout)
  std::vector<int32_t> n_cells;    // [N] followed cells (e > 0) of individual j, in the caller's order
  std::vector<double> cj;          // [ld] C_j per slot, uploaded at the first pointwise call
  SurvivalPointRows pw;            // the parameter row: lambda[T], log lambda[T], ab[n_ab], 1 / n_draw
  DevBuf<double> d_cj, d_acc;      // [ld], [4][ld]
  MappedBuf<double> h_acc;         // pinned
  int64_t waic_n = 0;              // draws folded into d_acc
  // PSIS-LOO by individual (abd_psis.hpp): the matrix of the draws' rows, unit = slot
  DevBuf<double> d_loo, d_loo_out;  // [ld][loo_cap]; [3][ld]: elpd_loo, pareto k, lppd
  DevBuf<int32_t> d_loo_cells, d_loo_tail;  // [ld] the followed cells per slot (0: padding); [ld] n_tail
  MappedBuf<double> h_loo_out;      // pinned
  MappedBuf<int32_t> h_loo_tail;
  int64_t loo_cap = 0, loo_n = 0;   // the draws the matrix holds room for, and those it holds
  // the posterior predictive checks (abd_survival_predictive.hpp)
  int pp_nvar = 0;                 // binning variables of the configuration; 0: abd_survival_predictive_configure has not run
  uint32_t pp_seed_lo = 0, pp_seed_hi = 0;
  SurvPredConstants pp_const;      // observed, person-time and followed cells per (variable, bin); O_j in the caller's order
  DevBuf<uint8_t> d_pp_bins;       // [T][ld]
  DevBuf<int32_t> d_pp_slot_j, d_pp_rj, d_pp_rep;  // [ld], [ABD_MAX_BATCH][ld], [kSurvRepBatch][T][ld] (at the first abd_survival_replicate)
  DevBuf<uint32_t> d_pp_r_part;                    // [ABD_MAX_BATCH][ntile][ABD_SURV_PRED_COLS]
  DevBuf<double> d_pp_e_part, d_pp_ej, d_pp_out_e, d_pp_acc_e;  // as d_pp_r_part, [ABD_MAX_BATCH][ld], [ABD_MAX_BATCH][COLS], [ld]
  DevBuf<int64_t> d_pp_out_r, d_pp_acc_r;          // [ABD_MAX_BATCH][COLS]; [2][ld]: sum of R_j, draws with R_j >= 1
  MappedBuf<double> h_pp_out_e, h_pp_acc_e;        // pinned
  MappedBuf<int64_t> h_pp_out_r, h_pp_acc_r;
  MappedBuf<int32_t> h_pp_rep;
  int64_t pp_n = 0;                // draws folded since the last reset

  int column(int j) const { return slot.empty() ? j : slot[j]; }
  SurvivalData data() const { return SurvivalData{d_y, d_e, d_x0, d_x1, nullptr, nullptr}; }
};

namespace abdi {
namespace {

// par and work of n <= ABD_MAX_BATCH points: rows of s->sums.h_par and s->sums.work
void survival_prepare_points(abd_survival* s, int n, const double* theta) {
  const int D = s->form.dim(), stride = s->form.par_stride(), ws = s->form.work_stride();
  for (int q = 0; q < n; ++q) s->form.prepare(theta + (size_t)q * D, s->sums.h_par.host() + (size_t)q * stride, s->sums.work.data() + (size_t)q * ws);
}

// fn(k0, nb) for the points k0 .. k0 + nb - 1 of n, at most `batch` of them at a time, until one fails
template <typename Fn>
int survival_batches(int n, int batch, Fn fn) {
  for (int k0 = 0; k0 < n; k0 += batch)
    if (int rc = fn(k0, std::min(batch, n - k0))) return rc;
  return ABD_OK;
}

template <typename Handle>
int survival_destroy(Handle* s) {
  if (!s) return ABD_OK;
  s->sums.quiesce();
  delete s;
  return ABD_OK;
}

// The sums of n <= ABD_MAX_BATCH points, whose rows stand in c.h_par, into c.h_out (rows of out_stride): for a handle of either
// kind (data.n_risk: an ensemble).  The one place that picks the pair of kernels: the sums kernel of the form and of the source,
// then the finalize kernel of the form.
int survival_sums_launch(SurvivalSums& c, const SurvivalForm& form, const SurvivalData& data, int n) {
  if (int rc = c.upload(n)) return rc;
  SurvivalSumsArgs a;
  std::memset(&a, 0, sizeof a);
  a.data = data;
  a.par = c.d_par;
  a.tile_group = c.d_tile_group;
  a.group_tile = c.d_group_tile;
  a.s_part = c.d_s_part;
  a.w0_part = c.d_w0_part;
  a.w_part = c.d_w_part;
  a.out = c.d_out;
  a.T = c.T;
  a.Gr = form.Gr;
  a.n_ab = form.n_ab();
  a.ld = c.ld;
  a.ntile = c.ntile;
  a.nseg = c.nseg;
  a.seg_len = c.seg_len;
  a.par_stride = c.par_stride;
  using Kernel = void (*)(const SurvivalSumsArgs);
  static const Kernel kernels[4][2] = {{abd_survival_sums_kernel<0, false>, abd_survival_sums_kernel<0, true>},
                                       {abd_survival_sums_kernel<1, false>, abd_survival_sums_kernel<1, true>},
                                       {abd_survival_sums_kernel<2, false>, abd_survival_sums_kernel<2, true>},
                                       {abd_survival_sums_kernel<3, false>, abd_survival_sums_kernel<3, true>}};
  const int ns = (c.T + 63) / 64;  // workgroups of a finalize per plane of S_t partials
  const Kernel finalize = form.by_period() ? abd_survival_periods_finalize : form.grouped() ? abd_survival_groups_finalize : abd_survival_finalize;
  const int nfin = form.by_period() ? 2 * ns + 1 : form.grouped() ? ns + 1 + (form.Gr + 3) / 4 : ns + 1;
  HIP_TRY(launch_kernel(kernels[form.mode()][data.n_risk != nullptr], c.grid(n), dim3(256), 0, c.stream, a));
  HIP_TRY(launch_kernel(finalize, dim3((unsigned)nfin, (unsigned)n), dim3(256), 0, c.stream, a));
  return c.download(n);
}

// the sums of n <= ABD_MAX_BATCH points into s->sums.h_out
int survival_launch(abd_survival* s, int n, const double* theta) {
  survival_prepare_points(s, n, theta);
  return survival_sums_launch(s->sums, s->form, s->data(), n);
}

// ---- the per-individual log-likelihood (abd_survival_pointwise.hpp) ----

// At creation, on the host: C_j per slot and the followed cells per individual from the planes y, e [T][ld]
void survival_pointwise_setup(abd_survival* s, const double* y, const double* e) {
  std::vector<int32_t> cells((size_t)s->sums.ld);
  s->cj.resize((size_t)s->sums.ld);
  survival_pointwise_constants(s->form.T, s->sums.ld, y, e, s->cj.data(), cells.data());
  s->n_cells.resize((size_t)s->N);
  for (int j = 0; j < s->N; ++j) s->n_cells[j] = cells[s->column(j)];
  s->pw.stride = survival_pointwise_stride(s->form.T, s->form.n_ab());
}

// The rows pw.h_par of n <= ABD_MAX_BATCH points to the device and ll[n][ld] of them into pw.d_ll, queued on the stream: for a
// handle of either kind (data.n_risk: an ensemble, which has no cj).  The one place that picks the per-individual kernel.
int survival_pointwise_kernel(const SurvivalSums& c, const SurvivalForm& form, const SurvivalData& data, const double* cj, SurvivalPointRows& pw,
                              int n) {
  HIP_TRY(hipMemcpyAsync(pw.d_par, pw.h_par.host(), (size_t)n * pw.stride * sizeof(double), hipMemcpyHostToDevice, c.stream));
  SurvivalPointArgs a;
  std::memset(&a, 0, sizeof a);
  a.data = data;
  a.cj = cj;
  a.par = pw.d_par;
  a.tile_group = c.d_tile_group;
  a.ll = pw.d_ll;
  a.T = c.T;
  a.ld = c.ld;
  a.ntile = c.ntile;
  a.par_stride = pw.stride;
  a.n_ab = form.n_ab();
  using Kernel = void (*)(const SurvivalPointArgs);
  static const Kernel kernels[4][2] = {{abd_survival_individual_kernel<0, false>, abd_survival_individual_kernel<0, true>},
                                       {abd_survival_individual_kernel<1, false>, abd_survival_individual_kernel<1, true>},
                                       {abd_survival_individual_kernel<2, false>, abd_survival_individual_kernel<2, true>},
                                       {abd_survival_individual_kernel<3, false>, abd_survival_individual_kernel<3, true>}};
  const dim3 grid((unsigned)((c.ntile + 3) / 4), (unsigned)n);
  HIP_TRY(launch_kernel(kernels[form.mode()][data.n_risk != nullptr], grid, dim3(256), 0, c.stream, a));
  return ABD_OK;
}

// the buffers of the pointwise launches, at the first of them
int survival_pointwise_ensure(abd_survival* s) {
  if (!s->d_cj) HIP_TRY(s->d_cj.upload(s->cj.data(), (size_t)s->sums.ld));
  return s->pw.ensure(s->sums.ld);
}

// the rows of s->pw.d_ll [n][ld] into the LOO matrix as draws loo_n .. loo_n + n - 1, queued on the stream (abd_psis.hpp)
int survival_loo_store(abd_survival* s, int n) {
  HIP_TRY(launch_kernel(abd_psis_store, dim3((unsigned)((s->sums.ld + 255) / 256)), dim3(256), 0, s->sums.stream, (const double*)s->pw.d_ll, (double*)s->d_loo,
                        (int32_t)s->sums.ld, (int64_t)s->loo_cap, (int32_t)n, (int64_t)s->loo_n));
  return ABD_OK;
}

// what abd_survival_loo_accumulate and _append_rows check before anything is stored
int survival_loo_room(const abd_survival* s, int32_t n) {
  if (n < 0) return fail(ABD_ERR_ARG, "n=%d is negative", n);
  if (s->loo_cap < 1) return fail(ABD_ERR_STATE, "no matrix reserved (abd_survival_loo_reserve comes first)");
  if (s->loo_n + n > s->loo_cap)
    return fail(ABD_ERR_STATE, "%lld draws held and %d more would pass the capacity of %lld", (long long)s->loo_n, n, (long long)s->loo_cap);
  return ABD_OK;
}

// where the rows of a pointwise launch go: copied to s->pw.h_ll; folded into the WAIC accumulators as draws waic_n + 1 ..
// waic_n + n; or stored in the LOO matrix as draws loo_n .. loo_n + n - 1
enum class PointRows { Copy, Fold, Store };

// ll[n][ld] of n <= ABD_MAX_BATCH points into s->pw.d_ll, and on to `to`
int survival_pointwise_launch(abd_survival* s, int n, const double* theta, PointRows to) {
  const bool fold = to == PointRows::Fold;
  if (int rc = survival_pointwise_ensure(s)) return rc;
  const int T = s->form.T, n_ab = s->form.n_ab(), stride = s->form.par_stride();
  survival_prepare_points(s, n, theta);
  for (int q = 0; q < n; ++q)
    survival_pointwise_row(T, n_ab, s->sums.h_par.host() + (size_t)q * stride, s->sums.work.data() + (size_t)q * s->form.work_stride(), fold ? s->waic_n + q + 1 : 0,
                           s->pw.h_par.host() + (size_t)q * s->pw.stride);
  if (int rc = survival_pointwise_kernel(s->sums, s->form, s->data(), s->d_cj, s->pw, n)) return rc;
  if (fold) {
    if (!s->d_acc) HIP_TRY(s->d_acc.alloc_zero((size_t)4 * s->sums.ld, s->sums.stream));
    HIP_TRY(launch_kernel(abd_survival_waic_fold, dim3((unsigned)((s->sums.ld + 255) / 256)), dim3(256), 0, s->sums.stream, (const double*)s->pw.d_ll,
                          (const double*)s->pw.d_par, (double*)s->d_acc, (int32_t)s->sums.ld, (int32_t)s->pw.stride,
                          (int32_t)(s->pw.stride - 1), (int32_t)n, (int64_t)s->waic_n));
  } else if (to == PointRows::Store) {
    if (int rc = survival_loo_store(s, n)) return rc;
  } else {
    HIP_TRY(hipMemcpyAsync(s->pw.h_ll.host(), s->pw.d_ll, (size_t)n * s->sums.ld * sizeof(double), hipMemcpyDeviceToHost, s->sums.stream));
  }
  HIP_TRY(hipStreamSynchronize(s->sums.stream));
  if (fold) s->waic_n += n;
  if (to == PointRows::Store) s->loo_n += n;
  return ABD_OK;
}

// ---- the posterior predictive checks (abd_survival_predictive.hpp) ----

int survival_predictive_configured(const abd_survival* s) {
  if (s->pp_nvar < 1) return fail(ABD_ERR_ARG, "no binning variables (abd_survival_predictive_configure comes first)");
  return ABD_OK;
}

// the buffers of the predictive launches, at the first of them
int survival_predictive_ensure(abd_survival* s) {
  if (s->d_pp_ej) return ABD_OK;
  const size_t ld = (size_t)s->sums.ld, part = (size_t)ABD_MAX_BATCH * s->sums.ntile * ABD_SURV_PRED_COLS, out = (size_t)ABD_MAX_BATCH * ABD_SURV_PRED_COLS;
  HIP_TRY(s->d_pp_e_part.alloc(part));
  HIP_TRY(s->d_pp_r_part.alloc(part));
  HIP_TRY(s->d_pp_rj.alloc(ABD_MAX_BATCH * ld));
  HIP_TRY(s->d_pp_out_e.alloc(out));
  HIP_TRY(s->d_pp_out_r.alloc(out));
  HIP_TRY(s->h_pp_out_e.alloc_pinned(out));
  HIP_TRY(s->h_pp_out_r.alloc_pinned(out));
  HIP_TRY(s->d_pp_acc_e.alloc(ld));
  HIP_TRY(s->d_pp_acc_r.alloc(2 * ld));
  HIP_TRY(s->d_pp_ej.alloc(ABD_MAX_BATCH * ld));
  return ABD_OK;
}

// The replicates of n <= ABD_MAX_BATCH points (n <= kSurvRepBatch where rep) as draws draw0 .. draw0 + n - 1.  fold: the bin sums
// go to s->h_pp_out_e / h_pp_out_r and the rows E_j, R_j into the accumulators; rep: the per-cell replicates go to s->h_pp_rep.
int survival_predictive_launch(abd_survival* s, int n, const double* theta, int64_t draw0, bool fold, bool rep) {
  if (int rc = survival_predictive_ensure(s)) return rc;
  const int T = s->form.T;
  const size_t cells = (size_t)T * s->sums.ld;
  if (rep && !s->d_pp_rep) {
    HIP_TRY(s->h_pp_rep.alloc_pinned(kSurvRepBatch * cells));
    HIP_TRY(s->d_pp_rep.alloc(kSurvRepBatch * cells));
  }
  survival_prepare_points(s, n, theta);
  if (int rc = s->sums.upload(n)) return rc;
  SurvivalReplicateArgs a;
  std::memset(&a, 0, sizeof a);
  a.e = s->d_e;
  a.x0 = s->d_x0;
  a.x1 = s->d_x1;
  a.bins = s->d_pp_bins;
  a.slot_j = s->d_pp_slot_j;
  a.par = s->sums.d_par;
  a.tile_group = s->sums.d_tile_group;
  a.e_part = s->d_pp_e_part;
  a.r_part = s->d_pp_r_part;
  a.ej = s->d_pp_ej;
  a.rj = s->d_pp_rj;
  a.rep = rep ? (int32_t*)s->d_pp_rep : nullptr;
  a.draw0 = draw0;
  a.seed_lo = s->pp_seed_lo;
  a.seed_hi = s->pp_seed_hi;
  a.T = T;
  a.ld = s->sums.ld;
  a.ntile = s->sums.ntile;
  a.par_stride = s->form.par_stride();
  a.n_ab = s->form.n_ab();
  a.n_var = s->pp_nvar;
  const dim3 grid((unsigned)((s->sums.ntile + 3) / 4), (unsigned)n);
  void (*const kernels[4])(const SurvivalReplicateArgs) = {abd_survival_replicate_kernel<0>, abd_survival_replicate_kernel<1>,
                                                           abd_survival_replicate_kernel<2>, abd_survival_replicate_kernel<3>};
  HIP_TRY(launch_kernel(kernels[s->form.mode()], grid, dim3(256), survival_replicate_lds(s->pp_nvar), s->sums.stream, a));
  if (fold) {
    HIP_TRY(launch_kernel(abd_survival_predictive_finalize, dim3(1, (unsigned)n), dim3(256), 0, s->sums.stream, (const double*)s->d_pp_e_part,
                          (const uint32_t*)s->d_pp_r_part, (double*)s->d_pp_out_e, (int64_t*)s->d_pp_out_r, (int32_t)s->sums.ntile,
                          (int32_t)(s->pp_nvar * ABD_SURV_PRED_BINS)));
    HIP_TRY(launch_kernel(abd_survival_predictive_fold, dim3((unsigned)((s->sums.ld + 255) / 256)), dim3(256), 0, s->sums.stream, (const double*)s->d_pp_ej,
                          (const int32_t*)s->d_pp_rj, (double*)s->d_pp_acc_e, (int64_t*)s->d_pp_acc_r, (int64_t*)s->d_pp_acc_r + s->sums.ld,
                          (int32_t)s->sums.ld, (int32_t)n, draw0));
    const size_t out = (size_t)n * ABD_SURV_PRED_COLS;
    HIP_TRY(hipMemcpyAsync(s->h_pp_out_e.host(), s->d_pp_out_e, out * sizeof(double), hipMemcpyDeviceToHost, s->sums.stream));
    HIP_TRY(hipMemcpyAsync(s->h_pp_out_r.host(), s->d_pp_out_r, out * sizeof(int64_t), hipMemcpyDeviceToHost, s->sums.stream));
  }
  if (rep) HIP_TRY(hipMemcpyAsync(s->h_pp_rep.host(), s->d_pp_rep, (size_t)n * cells * sizeof(int32_t), hipMemcpyDeviceToHost, s->sums.stream));
  HIP_TRY(hipStreamSynchronize(s->sums.stream));
  return ABD_OK;
}

// ---- creation ----

int survival_check_shape(int N, int T) {
  if (N < 1) return fail(ABD_ERR_ARG, "n_inds=%d must be >= 1", N);
  if (T < 1 || T > ABD_MAX_GAPS - 1) return fail(ABD_ERR_ARG, "n_intervals=%d outside [1, %d]", T, ABD_MAX_GAPS - 1);
  return ABD_OK;
}

// the scales and rates of a form's priors (`names` is what the message calls them), then the mean of _lam0_raw_mu
int survival_check_priors(const char* names, std::initializer_list<double> positive, double lam0_mu_mean) {
  for (double v : positive)
    if (!(v > 0.0) || !std::isfinite(v)) return fail(ABD_ERR_ARG, "%s must be positive and finite, got %g", names, v);
  if (!std::isfinite(lam0_mu_mean)) return fail(ABD_ERR_ARG, "lam0_mu_mean must be finite, got %g", lam0_mu_mean);
  return ABD_OK;
}

// what the creators of the forms by group and by period, of either kind of handle, check of their eight priors and make of them
template <typename Desc>
int survival_check_gpriors(const Desc* d) {
  return survival_check_priors("lam0_mu_sd, lam0_sd_rate, lam0_z_sd, a_mu_sd, a_sd_rate, a_z_sd, b_sd",
                               {d->lam0_mu_sd, d->lam0_sd_rate, d->lam0_z_sd, d->a_mu_sd, d->a_sd_rate, d->a_z_sd, d->b_sd}, d->lam0_mu_mean);
}
template <typename Desc>
SurvivalGroupsPriors survival_gpriors(const Desc* d) {
  return SurvivalGroupsPriors{d->lam0_mu_mean, d->lam0_mu_sd, d->lam0_sd_rate, d->lam0_z_sd, d->a_mu_sd, d->a_sd_rate, d->a_z_sd, d->b_sd};
}

// ... and of their counts and labels
int survival_check_n_groups(int Gr) {
  if (Gr < 1 || Gr > ABD_SURVIVAL_MAX_GROUPS) return fail(ABD_ERR_ARG, "n_groups=%d outside [1, %d]", Gr, ABD_SURVIVAL_MAX_GROUPS);
  return ABD_OK;
}
int survival_check_groups(int N, int Gr, const int32_t* group) {
  for (int j = 0; j < N; ++j)
    if (group[j] < 0 || group[j] >= Gr) return fail(ABD_ERR_ARG, "individual %d: group %d outside [0, %d)", j, group[j], Gr);
  return ABD_OK;
}
int survival_check_n_periods(int T, int P) {
  if (P < 1 || P > T) return fail(ABD_ERR_ARG, "n_periods=%d outside [1, %d]", P, T);
  return ABD_OK;
}
int survival_check_periods(int T, int P, const int32_t* period) {
  for (int t = 0; t < T; ++t)
    if (period[t] < 0 || period[t] >= P) return fail(ABD_ERR_ARG, "interval %d: period %d outside [0, %d)", t, period[t], P);
  return ABD_OK;
}

// the individuals sorted by group, every group padded to whole tiles; the labels lie in [0, Gr)
SurvivalLayout survival_layout(int N, int Gr, const int32_t* group) {
  SurvivalLayout lay;
  lay.slot.resize((size_t)N);
  lay.tile_group.resize((size_t)(N + 63) / 64 + Gr);
  lay.group_tile.resize((size_t)Gr + 1);
  lay.ntile = survival_groups_layout(N, Gr, group, lay.slot.data(), lay.tile_group.data(), lay.group_tile.data());
  return lay;
}

// Everything after a creator's own checks: the planes, the plan of the launches, the device and its buffers.  spec.device is
// what the caller asked for (< 0: the current device); layout is null for the ungrouped form (individual j in column j).
int survival_create_common(const SurvivalSpec& spec, const double* infected, const double* exposure, const double* const* titer,
                           const SurvivalLayout* layout, abd_survival** out) {
  const int N = spec.N, T = spec.form.T, K = spec.form.K;
  const int ntile = layout ? layout->ntile : (N + 63) / 64;
  SurvivalPlanes p;  // [interval][individual] planes, padded with cells that have no follow-up
  const SurvivalRefusal bad = survival_pack(N, T, K, infected, exposure, titer, layout ? layout->slot.data() : nullptr, (size_t)ntile * 64, &p);
  if (bad.msg) return fail(ABD_ERR_ARG, "individual %d, interval %d: %s", bad.j, bad.t, bad.msg);
  std::unique_ptr<abd_survival> s(new (std::nothrow) abd_survival);
  if (!s) return fail(ABD_ERR_NOMEM, "out of host memory");
  static_cast<SurvivalSpec&>(*s) = spec;
  s->sums.plan(ntile, T);
  if (layout) s->slot = layout->slot;
  s->Y = std::move(p.Y);
  s->C = p.C;
  survival_pointwise_setup(s.get(), p.y.data(), p.e.data());
  if (int rc = s->sums.alloc(spec.device, s->form, 0, layout)) return rc;
  const size_t plane = (size_t)s->sums.ld * T;
  HIP_TRY(s->d_y.upload(p.y.data(), plane));
  HIP_TRY(s->d_e.upload(p.e.data(), plane));
  HIP_TRY(s->d_x0.upload(p.x0.data(), plane));
  if (K == 2) HIP_TRY(s->d_x1.upload(p.x1.data(), plane));
  *out = s.release();
  return ABD_OK;
}

// what a creator says when the host has no memory for its copies of the data
template <typename Desc>
int survival_no_memory(const Desc* d) {
  return fail(ABD_ERR_NOMEM, "out of host memory for %d x %d cells", d->n_inds, d->n_intervals);
}
int survival_draws_no_memory(int M, int N, int T) { return fail(ABD_ERR_NOMEM, "out of host memory for %d datasets of %d x %d cells", M, N, T); }
int survival_no_memory(const abd_survival_draws_desc* d) { return survival_draws_no_memory(d->n_datasets, d->n_inds, d->n_intervals); }
int survival_no_memory(const abd_survival_draws_groups_desc* d) { return survival_draws_no_memory(d->n_datasets, d->n_inds, d->n_intervals); }
int survival_no_memory(const abd_survival_draws_periods_desc* d) { return survival_draws_no_memory(d->n_datasets, d->n_inds, d->n_intervals); }

// The frame of the creators of both kinds of handle around `create`, the creator's own checks and what it builds: nothing may be
// thrown across the C ABI (the host copies of the planes are the large allocations).
template <typename Desc, typename Handle, typename Create>
int survival_create(const Desc* d, Handle** out, Create create) {
  if (!d || !out) return fail(ABD_ERR_ARG, "NULL argument");
  *out = nullptr;
  try {
    return create();
  } catch (const std::bad_alloc&) {
    return survival_no_memory(d);
  }
}

}  // namespace
}  // namespace abdi

extern "C" {

int abd_survival_create(const abd_survival_desc* d, abd_survival** out) {
  return survival_create(d, out, [&] {
    const int K = d->n_titers;
    if (K != 1 && K != 2) return fail(ABD_ERR_ARG, "n_titers=%d: 1 (alone) or 2 (combined)", K);
    if (int rc = survival_check_shape(d->n_inds, d->n_intervals)) return rc;
    if (!d->infected || !d->exposure || !d->titer[0] || (K == 2 && !d->titer[1])) return fail(ABD_ERR_ARG, "NULL array in the descriptor");
    if (int rc = survival_check_priors("ab_sd, lam0_mu_sd, lam0_sd_rate, lam0_z_sd", {d->ab_sd, d->lam0_mu_sd, d->lam0_sd_rate, d->lam0_z_sd},
                                       d->lam0_mu_mean))
      return rc;
    SurvivalSpec spec{SurvivalForm{K, 0, d->n_intervals}, d->n_inds, d->device};
    spec.priors = SurvivalPriors{d->ab_sd, d->lam0_mu_mean, d->lam0_mu_sd, d->lam0_sd_rate, d->lam0_z_sd};
    return survival_create_common(spec, d->infected, d->exposure, d->titer, nullptr, out);
  });
}

int abd_survival_create_groups(const abd_survival_groups_desc* d, abd_survival** out) {
  return survival_create(d, out, [&] {
    const int N = d->n_inds, Gr = d->n_groups;
    if (int rc = survival_check_shape(N, d->n_intervals)) return rc;
    if (int rc = survival_check_n_groups(Gr)) return rc;
    if (!d->infected || !d->exposure || !d->titer || !d->group) return fail(ABD_ERR_ARG, "NULL array in the descriptor");
    if (int rc = survival_check_gpriors(d)) return rc;
    if (int rc = survival_check_groups(N, Gr, d->group)) return rc;
    const SurvivalLayout lay = survival_layout(N, Gr, d->group);  // a tile belongs to one group
    SurvivalSpec spec{SurvivalForm{1, Gr, d->n_intervals}, N, d->device};
    spec.gpriors = survival_gpriors(d);
    return survival_create_common(spec, d->infected, d->exposure, &d->titer, &lay, out);
  });
}

int abd_survival_create_periods(const abd_survival_periods_desc* d, abd_survival** out) {
  return survival_create(d, out, [&] {
    const int T = d->n_intervals, P = d->n_periods;
    if (int rc = survival_check_shape(d->n_inds, T)) return rc;
    if (int rc = survival_check_n_periods(T, P)) return rc;
    if (!d->infected || !d->exposure || !d->titer || !d->period) return fail(ABD_ERR_ARG, "NULL array in the descriptor");
    if (int rc = survival_check_gpriors(d)) return rc;
    if (int rc = survival_check_periods(T, P, d->period)) return rc;
    SurvivalSpec spec{SurvivalForm{1, 0, T, P, std::vector<int32_t>(d->period, d->period + T)}, d->n_inds, d->device};
    spec.gpriors = survival_gpriors(d);
    return survival_create_common(spec, d->infected, d->exposure, &d->titer, nullptr, out);  // no layout: the caller's order
  });
}

int abd_survival_destroy(abd_survival* s) { return survival_destroy(s); }

int32_t abd_survival_dim(abd_survival* s) { return s ? s->form.dim() : -1; }

int abd_survival_logp_dlogp(abd_survival* s, int32_t n, const double* theta, double* logp, double* grad) {
  if (!s || !theta || !logp || !grad) return fail(ABD_ERR_ARG, "NULL argument");
  if (n < 0) return fail(ABD_ERR_ARG, "n=%d is negative", n);
  HIP_TRY(hipSetDevice(s->sums.device));
  const size_t D = (size_t)s->form.dim(), out_stride = (size_t)s->form.out_stride(), par_stride = (size_t)s->form.par_stride();
  return survival_batches(n, ABD_MAX_BATCH, [&](int k0, int nb) {
    if (int rc = survival_launch(s, nb, theta + k0 * D)) return rc;
    for (int q = 0; q < nb; ++q) {
      const size_t k = (size_t)k0 + q;
      logp[k] = s->form.combine(s->priors, s->gpriors, theta + k * D, s->Y.data(), s->C, s->sums.h_out.host() + q * out_stride,
                                s->sums.h_par.host() + q * par_stride, s->sums.work.data() + (size_t)q * s->form.work_stride(), grad + k * D);
    }
    return (int)ABD_OK;
  });
}

int abd_survival_loglik_sums(abd_survival* s, const double* theta, double* sums) {
  if (!s || !theta || !sums) return fail(ABD_ERR_ARG, "NULL argument");
  HIP_TRY(hipSetDevice(s->sums.device));
  if (int rc = survival_launch(s, 1, theta)) return rc;
  std::memcpy(sums, s->sums.h_out.host(), (size_t)s->form.n_sums() * sizeof(double));
  return ABD_OK;
}

int abd_survival_individual_loglik(abd_survival* s, int32_t n, const double* theta, double* ll) {
  if (!s || !theta || !ll) return fail(ABD_ERR_ARG, "NULL argument");
  if (n < 0) return fail(ABD_ERR_ARG, "n=%d is negative", n);
  HIP_TRY(hipSetDevice(s->sums.device));
  const size_t D = (size_t)s->form.dim();
  return survival_batches(n, ABD_MAX_BATCH, [&](int k0, int nb) {
    if (int rc = survival_pointwise_launch(s, nb, theta + k0 * D, PointRows::Copy)) return rc;
    for (int q = 0; q < nb; ++q) {  // slots to the caller's order
      const double* row = s->pw.h_ll.host() + (size_t)q * s->sums.ld;
      double* out = ll + ((size_t)k0 + q) * s->N;
      for (int j = 0; j < s->N; ++j) out[j] = row[s->column(j)];
    }
    return (int)ABD_OK;
  });
}

int abd_survival_waic_reset(abd_survival* s) {
  if (!s) return fail(ABD_ERR_ARG, "NULL argument");
  s->waic_n = 0;  // the first draw folded overwrites its column: the accumulators need no clearing
  return ABD_OK;
}

int abd_survival_waic_accumulate(abd_survival* s, int32_t n, const double* theta) {
  if (!s || !theta) return fail(ABD_ERR_ARG, "NULL argument");
  if (n < 0) return fail(ABD_ERR_ARG, "n=%d is negative", n);
  HIP_TRY(hipSetDevice(s->sums.device));
  return survival_batches(n, ABD_MAX_BATCH,
                          [&](int k0, int nb) { return survival_pointwise_launch(s, nb, theta + (size_t)k0 * s->form.dim(), PointRows::Fold); });
}

int abd_survival_waic_stats(abd_survival* s, double* lse, double* mean, double* m2, int64_t* n_draws, int32_t* n_cells) {
  if (!s || !lse || !mean || !m2 || !n_draws || !n_cells) return fail(ABD_ERR_ARG, "NULL argument");
  if (s->waic_n < 1) return fail(ABD_ERR_ARG, "no draws accumulated (abd_survival_waic_accumulate comes first)");
  HIP_TRY(hipSetDevice(s->sums.device));
  const size_t ld = (size_t)s->sums.ld;
  if (!s->h_acc.host()) HIP_TRY(s->h_acc.alloc_pinned(4 * ld));
  HIP_TRY(hipMemcpyAsync(s->h_acc.host(), s->d_acc, 4 * ld * sizeof(double), hipMemcpyDeviceToHost, s->sums.stream));
  HIP_TRY(hipStreamSynchronize(s->sums.stream));
  const double* acc = s->h_acc.host();
  for (int j = 0; j < s->N; ++j) {
    const size_t c = (size_t)s->column(j);
    lse[j] = acc[c] + std::log(acc[ld + c]);  // M + log S
    mean[j] = acc[2 * ld + c];
    m2[j] = acc[3 * ld + c];
    n_cells[j] = s->n_cells[j];
  }
  *n_draws = s->waic_n;
  return ABD_OK;
}

// ---- PSIS-LOO by individual (abd_psis.hpp) ----

int abd_survival_loo_reserve(abd_survival* s, int64_t capacity) {
  if (!s) return fail(ABD_ERR_ARG, "NULL argument");
  if (capacity < 0 || capacity > ABD_SURVIVAL_LOO_MAX_DRAWS)
    return fail(ABD_ERR_ARG, "capacity=%lld outside [0, %d]", (long long)capacity, ABD_SURVIVAL_LOO_MAX_DRAWS);
  static_assert(ABD_SURVIVAL_LOO_MAX_DRAWS == kPsisMaxDraws, "header / kernel draw cap mismatch");
  HIP_TRY(hipSetDevice(s->sums.device));
  HIP_TRY(hipStreamSynchronize(s->sums.stream));
  s->d_loo.reset();
  s->loo_cap = s->loo_n = 0;
  if (capacity == 0) return ABD_OK;
  const size_t ld = (size_t)s->sums.ld;
  if (s->d_loo.alloc(ld * (size_t)capacity) != hipSuccess) {
    (void)hipGetLastError();
    return fail(ABD_ERR_NOMEM, "the device cannot hold %zu bytes for %lld draws of %zu slots", ld * (size_t)capacity * sizeof(double), (long long)capacity, ld);
  }
  if (!s->d_loo_cells) {  // the followed cells per slot; the padding has none
    std::vector<int32_t> cells(ld, 0);
    for (int j = 0; j < s->N; ++j) cells[(size_t)s->column(j)] = s->n_cells[j];
    HIP_TRY(s->d_loo_cells.upload(cells.data(), ld));
    HIP_TRY(s->d_loo_out.alloc(3 * ld));
    HIP_TRY(s->d_loo_tail.alloc(ld));
    HIP_TRY(s->h_loo_out.alloc_pinned(3 * ld));
    HIP_TRY(s->h_loo_tail.alloc_pinned(ld));
  }
  s->loo_cap = capacity;
  return ABD_OK;
}

int abd_survival_loo_reset(abd_survival* s) {
  if (!s) return fail(ABD_ERR_ARG, "NULL argument");
  s->loo_n = 0;  // the rows are overwritten
  return ABD_OK;
}

int abd_survival_loo_accumulate(abd_survival* s, int32_t n, const double* theta) {
  if (!s || !theta) return fail(ABD_ERR_ARG, "NULL argument");
  if (int rc = survival_loo_room(s, n)) return rc;
  HIP_TRY(hipSetDevice(s->sums.device));
  return survival_batches(n, ABD_MAX_BATCH,
                          [&](int k0, int nb) { return survival_pointwise_launch(s, nb, theta + (size_t)k0 * s->form.dim(), PointRows::Store); });
}

int abd_survival_loo_append_rows(abd_survival* s, int32_t n, const double* ll) {
  if (!s || !ll) return fail(ABD_ERR_ARG, "NULL argument");
  if (int rc = survival_loo_room(s, n)) return rc;
  HIP_TRY(hipSetDevice(s->sums.device));
  if (int rc = survival_pointwise_ensure(s)) return rc;
  const size_t ld = (size_t)s->sums.ld;
  return survival_batches(n, ABD_MAX_BATCH, [&](int k0, int nb) {
    std::memset(s->pw.h_ll.host(), 0, (size_t)nb * ld * sizeof(double));  // the padding holds 0
    for (int q = 0; q < nb; ++q) {  // the caller's order to slots
      const double* in = ll + ((size_t)k0 + q) * s->N;
      double* row = s->pw.h_ll.host() + (size_t)q * ld;
      for (int j = 0; j < s->N; ++j) row[s->column(j)] = in[j];
    }
    HIP_TRY(hipMemcpyAsync(s->pw.d_ll, s->pw.h_ll.host(), (size_t)nb * ld * sizeof(double), hipMemcpyHostToDevice, s->sums.stream));
    if (int rc = survival_loo_store(s, nb)) return rc;
    HIP_TRY(hipStreamSynchronize(s->sums.stream));
    s->loo_n += nb;
    return (int)ABD_OK;
  });
}

int abd_survival_loo_rows(abd_survival* s, int64_t first, int64_t count, double* ll) {
  if (!s || !ll) return fail(ABD_ERR_ARG, "NULL argument");
  if (first < 0 || count < 0 || first + count > s->loo_n)
    return fail(ABD_ERR_ARG, "rows [%lld, %lld) outside the %lld draws held", (long long)first, (long long)(first + count), (long long)s->loo_n);
  if (count == 0) return ABD_OK;
  HIP_TRY(hipSetDevice(s->sums.device));
  const size_t ld = (size_t)s->sums.ld;
  try {
    std::vector<double> buf(ld * (size_t)count);  // [ld][count]
    HIP_TRY(hipStreamSynchronize(s->sums.stream));
    HIP_TRY(hipMemcpy2D(buf.data(), (size_t)count * sizeof(double), (const double*)s->d_loo + first, (size_t)s->loo_cap * sizeof(double),
                        (size_t)count * sizeof(double), ld, hipMemcpyDeviceToHost));
    for (int j = 0; j < s->N; ++j) {
      const double* col = buf.data() + (size_t)s->column(j) * count;
      for (int64_t p = 0; p < count; ++p) ll[(size_t)p * s->N + j] = col[p];
    }
  } catch (const std::bad_alloc&) {
    return fail(ABD_ERR_NOMEM, "out of host memory for %lld x %zu values", (long long)count, ld);
  }
  return ABD_OK;
}

int abd_survival_loo_stats(abd_survival* s, double* elpd_loo, double* pareto_k, double* lppd, int32_t* n_tail, int64_t* n_draws, int32_t* n_cells) {
  if (!s || !elpd_loo || !pareto_k || !lppd || !n_tail || !n_draws || !n_cells) return fail(ABD_ERR_ARG, "NULL argument");
  if (s->loo_n < 1) return fail(ABD_ERR_ARG, "no draws held (abd_survival_loo_accumulate or abd_survival_loo_append_rows comes first)");
  HIP_TRY(hipSetDevice(s->sums.device));
  const size_t ld = (size_t)s->sums.ld;
  const PsisLaunch p = psis_launch(s->d_loo, s->d_loo_cells, s->d_loo_out, s->d_loo_tail, ld, s->loo_cap, s->loo_n);
  HIP_TRY(launch_kernel(p.kernel, dim3((unsigned)ld), dim3(kPsisThreads), 0, s->sums.stream, p.args));
  HIP_TRY(hipMemcpyAsync(s->h_loo_out.host(), s->d_loo_out, 3 * ld * sizeof(double), hipMemcpyDeviceToHost, s->sums.stream));
  HIP_TRY(hipMemcpyAsync(s->h_loo_tail.host(), s->d_loo_tail, ld * sizeof(int32_t), hipMemcpyDeviceToHost, s->sums.stream));
  HIP_TRY(hipStreamSynchronize(s->sums.stream));
  for (int j = 0; j < s->N; ++j) {
    const size_t c = (size_t)s->column(j);
    elpd_loo[j] = s->h_loo_out.host()[c];
    pareto_k[j] = s->h_loo_out.host()[ld + c];
    lppd[j] = s->h_loo_out.host()[2 * ld + c];
    n_tail[j] = s->h_loo_tail.host()[c];
    n_cells[j] = s->n_cells[j];
  }
  *n_draws = s->loo_n;
  return ABD_OK;
}

int abd_survival_predictive_configure(abd_survival* s, int32_t n_var, const double* const* titers, const int32_t* n_edges,
                                      const double* const* edges, uint64_t seed) {
  if (!s || !titers || !n_edges || !edges) return fail(ABD_ERR_ARG, "NULL argument");
  if (n_var != 1 && n_var != 2) return fail(ABD_ERR_ARG, "n_var=%d: one or two binning variables", n_var);
  for (int v = 0; v < n_var; ++v) {
    if (!titers[v] || (n_edges[v] > 0 && !edges[v])) return fail(ABD_ERR_ARG, "NULL array of binning variable %d", v);
    if (const char* msg = surv_pred_check_edges(n_edges[v], edges[v])) return fail(ABD_ERR_ARG, "binning variable %d: %s", v, msg);
  }
  HIP_TRY(hipSetDevice(s->sums.device));
  try {
    const int T = s->form.T;
    const size_t ld = (size_t)s->sums.ld, plane = ld * T;
    std::vector<double> y(plane), e(plane);
    HIP_TRY(hipStreamSynchronize(s->sums.stream));
    HIP_TRY(hipMemcpy(y.data(), s->d_y, plane * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(e.data(), s->d_e, plane * sizeof(double), hipMemcpyDeviceToHost));
    std::vector<uint8_t> bins(plane);
    std::vector<int32_t> slot_j(ld);
    SurvPredConstants c;
    const SurvivalRefusal bad = surv_pred_pack(s->N, T, ld, s->slot.empty() ? nullptr : s->slot.data(), y.data(), e.data(), n_var, titers,
                                               n_edges, edges, bins.data(), slot_j.data(), &c);
    if (bad.msg) return fail(ABD_ERR_ARG, "individual %d, interval %d: %s", bad.j, bad.t, bad.msg);  // the earlier configuration stands
    HIP_TRY(s->d_pp_bins.upload(bins.data(), plane));
    HIP_TRY(s->d_pp_slot_j.upload(slot_j.data(), ld));
    s->pp_const = std::move(c);
  } catch (const std::bad_alloc&) {
    return fail(ABD_ERR_NOMEM, "out of host memory for %d x %d cells", s->N, s->form.T);
  }
  s->pp_nvar = n_var;
  s->pp_seed_lo = (uint32_t)seed;
  s->pp_seed_hi = (uint32_t)(seed >> 32);
  s->pp_n = 0;  // the first draw folded overwrites its column: the accumulators need no clearing
  return ABD_OK;
}

int abd_survival_predictive_reset(abd_survival* s) {
  if (!s) return fail(ABD_ERR_ARG, "NULL argument");
  s->pp_n = 0;
  return ABD_OK;
}

int abd_survival_predictive_accumulate(abd_survival* s, int32_t n, const double* theta, double* expected, int64_t* replicate) {
  if (!s || !theta || !expected || !replicate) return fail(ABD_ERR_ARG, "NULL argument");
  if (n < 0) return fail(ABD_ERR_ARG, "n=%d is negative", n);
  if (int rc = survival_predictive_configured(s)) return rc;
  HIP_TRY(hipSetDevice(s->sums.device));
  const size_t row = (size_t)s->pp_nvar * ABD_SURV_PRED_BINS;
  return survival_batches(n, ABD_MAX_BATCH, [&](int k0, int nb) {
    if (int rc = survival_predictive_launch(s, nb, theta + (size_t)k0 * s->form.dim(), s->pp_n, true, false)) return rc;
    s->pp_n += nb;
    for (int q = 0; q < nb; ++q) {
      std::memcpy(expected + ((size_t)k0 + q) * row, s->h_pp_out_e.host() + (size_t)q * ABD_SURV_PRED_COLS, row * sizeof(double));
      std::memcpy(replicate + ((size_t)k0 + q) * row, s->h_pp_out_r.host() + (size_t)q * ABD_SURV_PRED_COLS, row * sizeof(int64_t));
    }
    return (int)ABD_OK;
  });
}

int abd_survival_predictive_stats(abd_survival* s, double* sum_e, int64_t* sum_r, int64_t* n_pos, int64_t* n_draws) {
  if (!s || !sum_e || !sum_r || !n_pos || !n_draws) return fail(ABD_ERR_ARG, "NULL argument");
  if (int rc = survival_predictive_configured(s)) return rc;
  if (s->pp_n < 1) return fail(ABD_ERR_ARG, "no draws accumulated (abd_survival_predictive_accumulate comes first)");
  HIP_TRY(hipSetDevice(s->sums.device));
  const size_t ld = (size_t)s->sums.ld;
  if (!s->h_pp_acc_e.host()) {
    HIP_TRY(s->h_pp_acc_e.alloc_pinned(ld));
    HIP_TRY(s->h_pp_acc_r.alloc_pinned(2 * ld));
  }
  HIP_TRY(hipMemcpyAsync(s->h_pp_acc_e.host(), s->d_pp_acc_e, ld * sizeof(double), hipMemcpyDeviceToHost, s->sums.stream));
  HIP_TRY(hipMemcpyAsync(s->h_pp_acc_r.host(), s->d_pp_acc_r, 2 * ld * sizeof(int64_t), hipMemcpyDeviceToHost, s->sums.stream));
  HIP_TRY(hipStreamSynchronize(s->sums.stream));
  for (int j = 0; j < s->N; ++j) {
    const size_t c = (size_t)s->column(j);
    sum_e[j] = s->h_pp_acc_e.host()[c];
    sum_r[j] = s->h_pp_acc_r.host()[c];
    n_pos[j] = s->h_pp_acc_r.host()[ld + c];
  }
  *n_draws = s->pp_n;
  return ABD_OK;
}

int abd_survival_predictive_observed(abd_survival* s, double* observed, double* person_time, int64_t* n_cells, double* observed_ind) {
  if (!s || !observed || !person_time || !n_cells || !observed_ind) return fail(ABD_ERR_ARG, "NULL argument");
  if (int rc = survival_predictive_configured(s)) return rc;
  const size_t row = (size_t)s->pp_nvar * ABD_SURV_PRED_BINS;
  std::memcpy(observed, s->pp_const.observed, row * sizeof(double));
  std::memcpy(person_time, s->pp_const.person_time, row * sizeof(double));
  std::memcpy(n_cells, s->pp_const.n_cells, row * sizeof(int64_t));
  std::memcpy(observed_ind, s->pp_const.observed_ind.data(), (size_t)s->N * sizeof(double));
  return ABD_OK;
}

int abd_survival_replicate(abd_survival* s, int32_t n, const double* theta, int64_t draw0, int32_t* rep) {
  if (!s || !theta || !rep) return fail(ABD_ERR_ARG, "NULL argument");
  if (n < 0) return fail(ABD_ERR_ARG, "n=%d is negative", n);
  if (draw0 < 0) return fail(ABD_ERR_ARG, "draw0=%lld is negative", (long long)draw0);
  if (int rc = survival_predictive_configured(s)) return rc;
  HIP_TRY(hipSetDevice(s->sums.device));
  const int T = s->form.T;
  const size_t ld = (size_t)s->sums.ld;
  return survival_batches(n, kSurvRepBatch, [&](int k0, int nb) {
    if (int rc = survival_predictive_launch(s, nb, theta + (size_t)k0 * s->form.dim(), draw0 + k0, false, true)) return rc;
    for (int q = 0; q < nb; ++q) {  // [T][ld] in slots to [N][T] in the caller's order
      const int32_t* plane = s->h_pp_rep.host() + (size_t)q * T * ld;
      int32_t* out = rep + ((size_t)k0 + q) * s->N * T;
      for (int j = 0; j < s->N; ++j) {
        const size_t c = (size_t)s->column(j);
        for (int t = 0; t < T; ++t) out[(size_t)j * T + t] = plane[(size_t)t * ld + c];
      }
    }
    return (int)ABD_OK;
  });
}

}  // extern "C"

// ---- the ensemble of per-draw datasets (SurvSource<true, .> in abd_survival.hpp) ----

struct abd_survival_draws : SurvivalSpec {  // the form, as an abd_survival knows it: K titers, by group or by period
  int M = 0;
  SurvivalSums sums;      // first: the last to go.  Rows of par: the form's row, then the dataset index; of work: the form's
  std::vector<double> Y;  // [M][T]: the events of dataset m in interval t, an integer
  DevBuf<double> d_x0, d_x1;          // titers [M][T][ld]
  DevBuf<int32_t> d_n_risk, d_event;  // [M][ld]
  // the per-individual log-likelihood, its WAIC accumulators and PSIS-LOO, per dataset (abd_survival_pointwise.hpp)
  std::vector<int32_t> slot;            // [N] the column of individual j; empty: j itself (the ungrouped layout)
  std::vector<int32_t> n_cells;         // [M][N] followed cells of individual j in dataset m: its n_risk, in the caller's order
  SurvivalPointRows pw;                 // the parameter row: survival_pointwise_row's, then the draw's number and the dataset
  DevBuf<double> d_acc;                 // [M][4][ld]
  MappedBuf<double> h_acc;              // pinned
  std::vector<int64_t> waic_n, loo_n;   // [M] draws folded into dataset m's accumulators / held in its block of the matrix
  std::vector<int64_t> pending;         // [M] scratch of a call: the rows it has for dataset m so far
  DevBuf<double> d_loo, d_loo_out;      // [M][ld][loo_cap]; [M][3][ld]: elpd_loo, pareto k, lppd
  DevBuf<int32_t> d_loo_tail;           // [M][ld] n_tail (the followed cells per slot are d_n_risk's rows)
  MappedBuf<double> h_loo_out;          // pinned
  MappedBuf<int32_t> h_loo_tail;
  int64_t loo_cap = 0;                  // the draws every dataset's block holds room for

  int column(int j) const { return slot.empty() ? j : slot[j]; }
  SurvivalData data() const { return SurvivalData{nullptr, nullptr, d_x0, d_x1, d_n_risk, d_event}; }
};

namespace abdi {
namespace {

// the sums of n <= ABD_MAX_BATCH points, point q on dataset[q], into s->sums.h_out (rows of out_stride)
int survival_draws_launch(abd_survival_draws* s, int n, const int32_t* dataset, const double* theta) {
  SurvivalSums& c = s->sums;
  const SurvivalForm& form = s->form;
  const int stride = form.par_stride();  // the dataset index follows the form's row
  const size_t D = (size_t)form.dim();
  for (int q = 0; q < n; ++q) {
    double* par = c.h_par.host() + (size_t)q * c.par_stride;
    form.prepare(theta + q * D, par, c.work.data() + (size_t)q * form.work_stride());
    par[stride] = 0.0;
    std::memcpy(par + stride, dataset + q, sizeof(int32_t));
  }
  return survival_sums_launch(c, form, s->data(), n);
}

int survival_draws_check_datasets(const abd_survival_draws* s, int n, const int32_t* dataset) {
  for (int q = 0; q < n; ++q)
    if (dataset[q] < 0 || dataset[q] >= s->M) return fail(ABD_ERR_ARG, "point %d: dataset %d outside [0, %d)", q, dataset[q], s->M);
  return ABD_OK;
}

// ---- the per-individual log-likelihood of an ensemble (abd_survival_pointwise.hpp) ----

// ll[n][ld] of n <= ABD_MAX_BATCH points, point q on dataset[q], into s->pw.d_ll, and on to `to`: copied to s->pw.h_ll; folded
// into the dataset's WAIC accumulators as its draws waic_n[m] + 1 ...; or stored in the dataset's block of the LOO matrix as its
// draws loo_n[m] ...  The rows of one dataset keep their order, whatever stands between them.
int survival_draws_pointwise_launch(abd_survival_draws* s, int n, const int32_t* dataset, const double* theta, PointRows to) {
  const bool fold = to == PointRows::Fold, store = to == PointRows::Store;
  if (int rc = s->pw.ensure(s->sums.ld)) return rc;
  SurvivalSums& c = s->sums;
  const SurvivalForm& form = s->form;
  const int T = form.T, n_ab = form.n_ab(), inv_off = 2 * T + n_ab;
  const size_t D = (size_t)form.dim(), ld = (size_t)c.ld;
  if (fold || store) std::fill(s->pending.begin(), s->pending.end(), 0);
  for (int q = 0; q < n; ++q) {
    double* par = c.h_par.host() + (size_t)q * c.par_stride;
    double* work = c.work.data() + (size_t)q * form.work_stride();
    double* row = s->pw.h_par.host() + (size_t)q * s->pw.stride;
    form.prepare(theta + q * D, par, work);
    const int64_t n_draw = fold ? s->waic_n[dataset[q]] + ++s->pending[dataset[q]] : 0;
    survival_pointwise_row(T, n_ab, par, work, n_draw, row);
    std::memcpy(row + inv_off + kDrawsRowDraw, &n_draw, sizeof n_draw);
    row[inv_off + kDrawsRowDataset] = 0.0;
    std::memcpy(row + inv_off + kDrawsRowDataset, dataset + q, sizeof(int32_t));
  }
  if (int rc = survival_pointwise_kernel(c, form, s->data(), nullptr, s->pw, n)) return rc;
  if (fold) {
    if (!s->d_acc) HIP_TRY(s->d_acc.alloc_zero((size_t)s->M * 4 * ld, c.stream));
    HIP_TRY(launch_kernel(abd_survival_draws_waic_fold, dim3((unsigned)((ld + 255) / 256)), dim3(256), 0, c.stream, (const double*)s->pw.d_ll,
                          (const double*)s->pw.d_par, (double*)s->d_acc, (int32_t)ld, (int32_t)s->pw.stride, (int32_t)inv_off, (int32_t)n));
  } else if (store) {
    // abd_psis_store as it is, once per run of rows of one dataset, on that dataset's block at its own draw count
    for (int q0 = 0; q0 < n;) {
      const int m = dataset[q0];
      int q1 = q0 + 1;
      while (q1 < n && dataset[q1] == m) ++q1;
      HIP_TRY(launch_kernel(abd_psis_store, dim3((unsigned)((ld + 255) / 256)), dim3(256), 0, c.stream, (const double*)s->pw.d_ll + (size_t)q0 * ld,
                            (double*)s->d_loo + (size_t)m * ld * (size_t)s->loo_cap, (int32_t)ld, (int64_t)s->loo_cap, (int32_t)(q1 - q0),
                            (int64_t)(s->loo_n[m] + s->pending[m])));
      s->pending[m] += q1 - q0;
      q0 = q1;
    }
  } else {
    HIP_TRY(hipMemcpyAsync(s->pw.h_ll.host(), s->pw.d_ll, (size_t)n * ld * sizeof(double), hipMemcpyDeviceToHost, c.stream));
  }
  HIP_TRY(hipStreamSynchronize(c.stream));
  if (fold || store) {
    std::vector<int64_t>& count = fold ? s->waic_n : s->loo_n;
    for (int m = 0; m < s->M; ++m) count[m] += s->pending[m];
  }
  return ABD_OK;
}

// what the per-individual calls of an ensemble check of (n, dataset) before the device is touched
int survival_draws_check_points(const abd_survival_draws* s, int n, const int32_t* dataset) {
  if (n < 0) return fail(ABD_ERR_ARG, "n=%d is negative", n);
  return survival_draws_check_datasets(s, n, dataset);
}

// what the three creators of an ensemble check of its shape
int survival_draws_check_shape(int M, int N, int T) {
  if (M < 1) return fail(ABD_ERR_ARG, "n_datasets=%d must be >= 1", M);
  return survival_check_shape(N, T);
}

// Everything after a creator's own checks: every dataset checked, the padded copies, the plan of the launches, the device and its
// buffers.  spec.device is what the caller asked for (< 0: the current device); layout is null for the forms in the caller's order
// (individual j in column j), else the grouped form's, shared by all datasets.
int survival_draws_create_common(const SurvivalSpec& spec, int M, const int32_t* n_risk_in, const int32_t* event_in, const double* const* titer,
                                 const SurvivalLayout* layout, abd_survival_draws** out) {
  const int N = spec.N, T = spec.form.T, K = spec.form.K;
  std::unique_ptr<abd_survival_draws> s(new (std::nothrow) abd_survival_draws);
  if (!s) return fail(ABD_ERR_NOMEM, "out of host memory");
  static_cast<SurvivalSpec&>(*s) = spec;
  s->M = M;
  s->sums.plan(layout ? layout->ntile : (N + 63) / 64, T);  // the split of an abd_survival of the same form and individuals
  // every dataset, individual after individual: the first offender is named; the padded copies as the kernel reads them
  const size_t ld = (size_t)s->sums.ld, plane = ld * T;
  std::vector<int32_t> n_risk((size_t)M * ld, 0), event((size_t)M * ld, -1);
  std::vector<double> x0((size_t)M * plane, 0.0), x1(K == 2 ? (size_t)M * plane : 0, 0.0);
  s->Y.assign((size_t)M * T, 0.0);
  if (layout) s->slot = layout->slot;
  s->n_cells.assign(n_risk_in, n_risk_in + (size_t)M * N);  // a cell is followed where it is at risk
  s->pw.stride = survival_pointwise_stride(T, s->form.n_ab()) + kDrawsRowExtra - 1;
  s->waic_n.assign((size_t)M, 0);
  s->loo_n.assign((size_t)M, 0);
  s->pending.assign((size_t)M, 0);
  for (int m = 0; m < M; ++m)
    for (int j = 0; j < N; ++j) {
      const int nr = n_risk_in[(size_t)m * N + j], ev = event_in[(size_t)m * N + j];
      if (nr < 0 || nr > T) return fail(ABD_ERR_ARG, "dataset %d, individual %d: n_risk=%d outside [0, %d]", m, j, nr, T);
      if (ev != -1 && ev != nr - 1)
        return fail(ABD_ERR_ARG, "dataset %d, individual %d, interval %d: event must be -1 or n_risk - 1 = %d", m, j, ev, nr - 1);
      const size_t col = layout ? (size_t)layout->slot[j] : (size_t)j;
      n_risk[(size_t)m * ld + col] = nr;
      event[(size_t)m * ld + col] = ev;
      if (ev >= 0) s->Y[(size_t)m * T + ev] += 1.0;
      for (int k = 0; k < K; ++k) {
        const double* src = titer[k] + (size_t)m * T * N + j;
        double* dst = (k ? x1 : x0).data() + (size_t)m * plane + col;
        for (int t = 0; t < T; ++t) dst[(size_t)t * ld] = src[(size_t)t * N];  // cells not at risk as they are: the kernel drops them
        for (int t = 0; t < nr; ++t)
          if (!std::isfinite(src[(size_t)t * N]))
            return fail(ABD_ERR_ARG, "dataset %d, individual %d, interval %d: titer %d of a cell at risk must be finite", m, j, t, k);
      }
    }
  // rows of par (the form's, then the dataset index), out and work
  if (int rc = s->sums.alloc(spec.device, s->form, 1, layout)) return rc;
  HIP_TRY(s->d_x0.upload(x0.data(), x0.size()));
  if (K == 2) HIP_TRY(s->d_x1.upload(x1.data(), x1.size()));
  HIP_TRY(s->d_n_risk.upload(n_risk.data(), n_risk.size()));
  HIP_TRY(s->d_event.upload(event.data(), event.size()));
  *out = s.release();
  return ABD_OK;
}

}  // namespace
}  // namespace abdi

extern "C" {

int abd_survival_draws_create(const abd_survival_draws_desc* d, abd_survival_draws** out) {
  return survival_create(d, out, [&] {
    const int K = d->n_titers;
    if (K != 1 && K != 2) return fail(ABD_ERR_ARG, "n_titers=%d: 1 (alone) or 2 (combined)", K);
    if (int rc = survival_draws_check_shape(d->n_datasets, d->n_inds, d->n_intervals)) return rc;
    if (!d->n_risk || !d->event || !d->titer[0] || (K == 2 && !d->titer[1])) return fail(ABD_ERR_ARG, "NULL array in the descriptor");
    if (int rc = survival_check_priors("ab_sd, lam0_mu_sd, lam0_sd_rate, lam0_z_sd", {d->ab_sd, d->lam0_mu_sd, d->lam0_sd_rate, d->lam0_z_sd},
                                       d->lam0_mu_mean))
      return rc;
    SurvivalSpec spec{SurvivalForm{K, 0, d->n_intervals}, d->n_inds, d->device};
    spec.priors = SurvivalPriors{d->ab_sd, d->lam0_mu_mean, d->lam0_mu_sd, d->lam0_sd_rate, d->lam0_z_sd};
    return survival_draws_create_common(spec, d->n_datasets, d->n_risk, d->event, d->titer, nullptr, out);
  });
}

int abd_survival_draws_create_groups(const abd_survival_draws_groups_desc* d, abd_survival_draws** out) {
  return survival_create(d, out, [&] {
    const int N = d->n_inds, Gr = d->n_groups;
    if (int rc = survival_draws_check_shape(d->n_datasets, N, d->n_intervals)) return rc;
    if (int rc = survival_check_n_groups(Gr)) return rc;
    if (!d->n_risk || !d->event || !d->titer || !d->group) return fail(ABD_ERR_ARG, "NULL array in the descriptor");
    if (int rc = survival_check_gpriors(d)) return rc;
    if (int rc = survival_check_groups(N, Gr, d->group)) return rc;
    const SurvivalLayout lay = survival_layout(N, Gr, d->group);  // a tile belongs to one group, in every dataset
    SurvivalSpec spec{SurvivalForm{1, Gr, d->n_intervals}, N, d->device};
    spec.gpriors = survival_gpriors(d);
    return survival_draws_create_common(spec, d->n_datasets, d->n_risk, d->event, &d->titer, &lay, out);
  });
}

int abd_survival_draws_create_periods(const abd_survival_draws_periods_desc* d, abd_survival_draws** out) {
  return survival_create(d, out, [&] {
    const int T = d->n_intervals, P = d->n_periods;
    if (int rc = survival_draws_check_shape(d->n_datasets, d->n_inds, T)) return rc;
    if (int rc = survival_check_n_periods(T, P)) return rc;
    if (!d->n_risk || !d->event || !d->titer || !d->period) return fail(ABD_ERR_ARG, "NULL array in the descriptor");
    if (int rc = survival_check_gpriors(d)) return rc;
    if (int rc = survival_check_periods(T, P, d->period)) return rc;
    SurvivalSpec spec{SurvivalForm{1, 0, T, P, std::vector<int32_t>(d->period, d->period + T)}, d->n_inds, d->device};
    spec.gpriors = survival_gpriors(d);
    return survival_draws_create_common(spec, d->n_datasets, d->n_risk, d->event, &d->titer, nullptr, out);  // no layout: the caller's order
  });
}

int abd_survival_draws_destroy(abd_survival_draws* s) { return survival_destroy(s); }

int32_t abd_survival_draws_dim(abd_survival_draws* s) { return s ? s->form.dim() : -1; }

int abd_survival_draws_logp_dlogp(abd_survival_draws* s, int32_t n, const int32_t* dataset, const double* theta, double* logp, double* grad) {
  if (!s || !dataset || !theta || !logp || !grad) return fail(ABD_ERR_ARG, "NULL argument");
  if (n < 0) return fail(ABD_ERR_ARG, "n=%d is negative", n);
  if (int rc = survival_draws_check_datasets(s, n, dataset)) return rc;
  HIP_TRY(hipSetDevice(s->sums.device));
  const int T = s->form.T;
  const size_t D = (size_t)s->form.dim();
  return survival_batches(n, ABD_MAX_BATCH, [&](int k0, int nb) {
    if (int rc = survival_draws_launch(s, nb, dataset + k0, theta + k0 * D)) return rc;
    for (int q = 0; q < nb; ++q) {  // the closed form of the handle's form on the dataset's own integer Y_t, C = 0
      const size_t k = (size_t)k0 + q;
      logp[k] = s->form.combine(s->priors, s->gpriors, theta + k * D, s->Y.data() + (size_t)dataset[k] * T, 0.0,
                                s->sums.h_out.host() + (size_t)q * s->sums.out_stride, s->sums.h_par.host() + (size_t)q * s->sums.par_stride,
                                s->sums.work.data() + (size_t)q * s->form.work_stride(), grad + k * D);
    }
    return (int)ABD_OK;
  });
}

int abd_survival_draws_loglik_sums(abd_survival_draws* s, int32_t dataset, const double* theta, double* sums) {
  if (!s || !theta || !sums) return fail(ABD_ERR_ARG, "NULL argument");
  if (int rc = survival_draws_check_datasets(s, 1, &dataset)) return rc;
  HIP_TRY(hipSetDevice(s->sums.device));
  if (int rc = survival_draws_launch(s, 1, &dataset, theta)) return rc;
  std::memcpy(sums, s->sums.h_out.host(), (size_t)s->form.n_sums() * sizeof(double));
  return ABD_OK;
}

// ---- per individual and dataset: log-likelihood, WAIC, PSIS-LOO (abd_survival_pointwise.hpp) ----

int abd_survival_draws_individual_loglik(abd_survival_draws* s, int32_t n, const int32_t* dataset, const double* theta, double* ll) {
  if (!s || !dataset || !theta || !ll) return fail(ABD_ERR_ARG, "NULL argument");
  if (int rc = survival_draws_check_points(s, n, dataset)) return rc;
  HIP_TRY(hipSetDevice(s->sums.device));
  const size_t D = (size_t)s->form.dim();
  return survival_batches(n, ABD_MAX_BATCH, [&](int k0, int nb) {
    if (int rc = survival_draws_pointwise_launch(s, nb, dataset + k0, theta + k0 * D, PointRows::Copy)) return rc;
    for (int q = 0; q < nb; ++q) {  // slots to the caller's order
      const double* row = s->pw.h_ll.host() + (size_t)q * s->sums.ld;
      double* out = ll + ((size_t)k0 + q) * s->N;
      for (int j = 0; j < s->N; ++j) out[j] = row[s->column(j)];
    }
    return (int)ABD_OK;
  });
}

int abd_survival_draws_waic_reset(abd_survival_draws* s) {
  if (!s) return fail(ABD_ERR_ARG, "NULL argument");
  std::fill(s->waic_n.begin(), s->waic_n.end(), 0);  // a dataset's first draw folded overwrites its column: no clearing
  return ABD_OK;
}

int abd_survival_draws_waic_accumulate(abd_survival_draws* s, int32_t n, const int32_t* dataset, const double* theta) {
  if (!s || !dataset || !theta) return fail(ABD_ERR_ARG, "NULL argument");
  if (int rc = survival_draws_check_points(s, n, dataset)) return rc;
  HIP_TRY(hipSetDevice(s->sums.device));
  return survival_batches(n, ABD_MAX_BATCH, [&](int k0, int nb) {
    return survival_draws_pointwise_launch(s, nb, dataset + k0, theta + (size_t)k0 * s->form.dim(), PointRows::Fold);
  });
}

int abd_survival_draws_waic_stats(abd_survival_draws* s, double* lse, double* mean, double* m2, int64_t* n_draws, int32_t* n_cells) {
  if (!s || !lse || !mean || !m2 || !n_draws || !n_cells) return fail(ABD_ERR_ARG, "NULL argument");
  if (!std::any_of(s->waic_n.begin(), s->waic_n.end(), [](int64_t v) { return v > 0; }))
    return fail(ABD_ERR_ARG, "no draws accumulated (abd_survival_draws_waic_accumulate comes first)");
  HIP_TRY(hipSetDevice(s->sums.device));
  const size_t ld = (size_t)s->sums.ld, N = (size_t)s->N, all = (size_t)s->M * 4 * ld;
  if (!s->h_acc.host()) HIP_TRY(s->h_acc.alloc_pinned(all));
  HIP_TRY(hipMemcpyAsync(s->h_acc.host(), s->d_acc, all * sizeof(double), hipMemcpyDeviceToHost, s->sums.stream));
  HIP_TRY(hipStreamSynchronize(s->sums.stream));
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int m = 0; m < s->M; ++m) {
    const double* acc = s->h_acc.host() + (size_t)m * 4 * ld;
    const bool has = s->waic_n[m] > 0;  // a dataset without a draw: NaN and n_draws = 0
    for (size_t j = 0; j < N; ++j) {
      const size_t c = (size_t)s->column((int)j), o = (size_t)m * N + j;
      lse[o] = has ? acc[c] + std::log(acc[ld + c]) : nan;  // M + log S
      mean[o] = has ? acc[2 * ld + c] : nan;
      m2[o] = has ? acc[3 * ld + c] : nan;
      n_cells[o] = s->n_cells[o];
    }
    n_draws[m] = s->waic_n[m];
  }
  return ABD_OK;
}

int abd_survival_draws_loo_reserve(abd_survival_draws* s, int64_t capacity) {
  if (!s) return fail(ABD_ERR_ARG, "NULL argument");
  if (capacity < 0 || capacity > ABD_SURVIVAL_LOO_MAX_DRAWS)
    return fail(ABD_ERR_ARG, "capacity=%lld outside [0, %d]", (long long)capacity, ABD_SURVIVAL_LOO_MAX_DRAWS);
  HIP_TRY(hipSetDevice(s->sums.device));
  HIP_TRY(hipStreamSynchronize(s->sums.stream));
  s->d_loo.reset();
  s->loo_cap = 0;
  std::fill(s->loo_n.begin(), s->loo_n.end(), 0);
  if (capacity == 0) return ABD_OK;
  const size_t ld = (size_t)s->sums.ld, M = (size_t)s->M;
  if (s->d_loo.alloc(M * ld * (size_t)capacity) != hipSuccess) {
    (void)hipGetLastError();
    return fail(ABD_ERR_NOMEM, "the device cannot hold %zu bytes for %lld draws of %zu datasets of %zu slots", M * ld * (size_t)capacity * sizeof(double),
                (long long)capacity, M, ld);
  }
  if (!s->d_loo_out) {
    HIP_TRY(s->d_loo_out.alloc(M * 3 * ld));
    HIP_TRY(s->d_loo_tail.alloc(M * ld));
    HIP_TRY(s->h_loo_out.alloc_pinned(M * 3 * ld));
    HIP_TRY(s->h_loo_tail.alloc_pinned(M * ld));
  }
  s->loo_cap = capacity;
  return ABD_OK;
}

int abd_survival_draws_loo_reset(abd_survival_draws* s) {
  if (!s) return fail(ABD_ERR_ARG, "NULL argument");
  std::fill(s->loo_n.begin(), s->loo_n.end(), 0);  // the rows are overwritten
  return ABD_OK;
}

int abd_survival_draws_loo_accumulate(abd_survival_draws* s, int32_t n, const int32_t* dataset, const double* theta) {
  if (!s || !dataset || !theta) return fail(ABD_ERR_ARG, "NULL argument");
  if (int rc = survival_draws_check_points(s, n, dataset)) return rc;
  if (s->loo_cap < 1) return fail(ABD_ERR_STATE, "no matrix reserved (abd_survival_draws_loo_reserve comes first)");
  std::fill(s->pending.begin(), s->pending.end(), 0);  // every dataset's rows of the whole call, before anything is launched
  for (int q = 0; q < n; ++q) ++s->pending[dataset[q]];
  for (int m = 0; m < s->M; ++m)
    if (s->loo_n[m] + s->pending[m] > s->loo_cap)
      return fail(ABD_ERR_STATE, "dataset %d: %lld draws held and %lld more would pass the capacity of %lld", m, (long long)s->loo_n[m],
                  (long long)s->pending[m], (long long)s->loo_cap);
  HIP_TRY(hipSetDevice(s->sums.device));
  return survival_batches(n, ABD_MAX_BATCH, [&](int k0, int nb) {
    return survival_draws_pointwise_launch(s, nb, dataset + k0, theta + (size_t)k0 * s->form.dim(), PointRows::Store);
  });
}

int abd_survival_draws_loo_stats(abd_survival_draws* s, double* elpd_loo, double* pareto_k, double* lppd, int32_t* n_tail, int64_t* n_draws) {
  if (!s || !elpd_loo || !pareto_k || !lppd || !n_tail || !n_draws) return fail(ABD_ERR_ARG, "NULL argument");
  if (s->loo_cap < 1) return fail(ABD_ERR_STATE, "no matrix reserved (abd_survival_draws_loo_reserve comes first)");
  if (!std::any_of(s->loo_n.begin(), s->loo_n.end(), [](int64_t v) { return v > 0; }))
    return fail(ABD_ERR_ARG, "no draws held (abd_survival_draws_loo_accumulate comes first)");
  HIP_TRY(hipSetDevice(s->sums.device));
  const size_t ld = (size_t)s->sums.ld, N = (size_t)s->N, M = (size_t)s->M;
  // abd_psis_kernel as it is, per dataset on that dataset's block: its S is the dataset's own count, its n_cells the dataset's n_risk
  for (size_t m = 0; m < M; ++m) {
    if (s->loo_n[m] < 1) continue;
    const PsisLaunch p = psis_launch((const double*)s->d_loo + m * ld * (size_t)s->loo_cap, (const int32_t*)s->d_n_risk + m * ld,
                                     (double*)s->d_loo_out + m * 3 * ld, (int32_t*)s->d_loo_tail + m * ld, ld, s->loo_cap, s->loo_n[m]);
    HIP_TRY(launch_kernel(p.kernel, dim3((unsigned)ld), dim3(kPsisThreads), 0, s->sums.stream, p.args));
  }
  HIP_TRY(hipMemcpyAsync(s->h_loo_out.host(), s->d_loo_out, M * 3 * ld * sizeof(double), hipMemcpyDeviceToHost, s->sums.stream));
  HIP_TRY(hipMemcpyAsync(s->h_loo_tail.host(), s->d_loo_tail, M * ld * sizeof(int32_t), hipMemcpyDeviceToHost, s->sums.stream));
  HIP_TRY(hipStreamSynchronize(s->sums.stream));
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (size_t m = 0; m < M; ++m) {
    const double* out = s->h_loo_out.host() + m * 3 * ld;
    const bool has = s->loo_n[m] > 0;  // a dataset without a draw: NaN, n_tail = 0 and n_draws = 0
    for (size_t j = 0; j < N; ++j) {
      const size_t c = (size_t)s->column((int)j), o = m * N + j;
      elpd_loo[o] = has ? out[c] : nan;
      pareto_k[o] = has ? out[ld + c] : nan;
      lppd[o] = has ? out[2 * ld + c] : nan;
      n_tail[o] = has ? s->h_loo_tail.host()[m * ld + c] : 0;
    }
    n_draws[m] = s->loo_n[m];
  }
  return ABD_OK;
}

}  // extern "C"
