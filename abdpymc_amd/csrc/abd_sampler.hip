// abd_sampler.hip -- the native compound sampler of the C ABI (abd_sampler_*; include/abd_hip.h): the step pm.sample
// assigns to this model (abd.py:921-922) -- NUTS on the 17 continuous variables (abd_nuts.hpp), the device Gibbs sweep on
// [i_raw, ab_s_waner], recording of the Deterministics -- run against the evaluation path without leaving the library.
#include "abd_sampler.hpp"

#include "abd_loo.hpp"

#include <deque>
#include <memory>

namespace {

// The end of a chain's sweep as the native sampler's host thread sees it (abd_sampler.hip): the sweep's two counters go to
// mapped host memory and a tag behind them -- polled with a plain memory read (a hipEventQuery per pass of the host's loop
// costs the loop several microseconds for as long as a sweep is running, and every chain's records wait behind it)
__global__ void abd_sweep_done_kernel(const unsigned long long* counts, unsigned long long* host_counts, double* host_tag, double tag) {
  if (threadIdx.x == 0) {
    host_counts[0] = counts[0];
    host_counts[1] = counts[1];
    __threadfence_system();
    __hip_atomic_store(host_tag, tag, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

int train_alloc(abd_sampler* s) {
  s->tu.resize((size_t)s->n);
  for (auto& t : s->tu) {
    HIP_TRY(t.slots.alloc(2));
    HIP_TRY(hipMemset(t.slots, 0, 2 * sizeof(TrainPoint)));
    HIP_TRY(t.rec.alloc(abd_sampler::kTrainRing));
  }
  return ABD_OK;
}

int dtrain_alloc(abd_sampler* s) {
  s->dc.resize((size_t)s->n);
  for (auto& d : s->dc) {
    HIP_TRY(d.st.alloc_zero(1, s->c->stream));  // (waited for below)
    HIP_TRY(d.ring.alloc(ABD_TRAIN_RING));
    HIP_TRY(d.begin.alloc(abd_sampler::kBeginBlocks));
    HIP_TRY(d.side.create());
    HIP_TRY(d.done.alloc(4));
  }
  HIP_TRY(hipDeviceSynchronize());
  return ABD_OK;
}

// Queue one launch of unit u's train: the point staged by the host (theta, p_half: the first leapfrog of a half, or a
// plain evaluation with ve = 0), or -- theta == nullptr -- the successor of the launch queued last.
// own_record: nothing is going to be queued behind this launch that could pass its record on (the last leapfrog of a
// half, a plain evaluation, no look-ahead): it writes the record itself.
int train_launch(abd_sampler* s, int u, const double* theta, const double* p_half, double ve, const double* inv_mass, bool own_record) {
  abd_ctx* c = s->c;
  abd_sampler::TrainUnit& t = s->tu[(size_t)u];
  if (t.prod - t.cons >= (uint64_t)abd_sampler::kTrainRing) return fail(ABD_ERR_STATE, "internal: train record ring of unit %d is full", u);
  TrainArgs ta;
  std::memset(&ta, 0, sizeof ta);
  ta.enabled = 1;
  ta.slots = t.slots;
  ta.rec = t.rec.dev() + (t.prod % abd_sampler::kTrainRing);
  ta.ve = ve;
  ta.prior_const = c->prior_const;
  ta.own_record = own_record ? 1 : 0;
  std::memcpy(ta.inv_mass, inv_mass, sizeof ta.inv_mass);
  HostTerms ht;
  std::memset(&ht, 0, sizeof ht);
  if (theta) {
    ht = prepare(theta);
    ta.use_slot = -1;
    ta.next_slot = 0;
    std::memcpy(ta.first.theta, theta, sizeof ta.first.theta);
    if (p_half) std::memcpy(ta.first.p_half, p_half, sizeof ta.first.p_half);
    std::memcpy(ta.first.tr, &ht.tr, sizeof ta.first.tr);
    std::memcpy(ta.first.L0, ht.L0, sizeof ta.first.L0);
    std::memcpy(ta.first.L1, ht.L1, sizeof ta.first.L1);
  } else {
    ta.use_slot = t.next_slot;
    ta.next_slot = t.next_slot ^ 1;
    if (!t.last_own_record) {  // the predecessor left its record beside the point: this launch passes it on
      const size_t kp = (size_t)((t.prod - 1) % abd_sampler::kTrainRing);
      ta.fwd_rec = t.rec.dev() + kp;
      ta.fwd_tag = t.tags[kp];
    }
  }
  // (units driven by their own host threads tag their launches from their own sequence: abd_host.hpp, unit_seq)
  // (the launch assembles its own result and leaves it in ta.rec under ta.tag, set by enqueue_group: no result rows)
  const Caller who{Caller::Train, unit_pipe(c, u), s->unit_tags ? &c->unit_seq[(size_t)u] : nullptr, &ta};
  if (int rc = enqueue_group(c, who, 1, &s->chains[(size_t)u], &ht, true, nullptr)) return rc;
  t.tags[t.prod % abd_sampler::kTrainRing] = ta.tag;
  t.prod += 1;
  t.next_slot = ta.next_slot;
  t.last_own_record = own_record;
  return ABD_OK;
}

// the first leapfrog of the half chain u's tree is about to build, and as many of its successors as the look-ahead allows
int train_begin(abd_sampler* s, int u) {
  abdnuts::Nuts& nu = s->ch[(size_t)u].nuts;
  abd_sampler::TrainUnit& t = s->tu[(size_t)u];
  // a launch whose successor is certain to be queued (any but the half's last, given a look-ahead) leaves its record to it
  const int n_half = nu.half_remaining() + 1;
  auto own = [&](int j) { return s->lookahead == 0 || j == n_half - 1; };
  if (int rc = train_launch(s, u, nu.request(), nu.staged_momentum(), nu.signed_step(), nu.inv_mass, own(0))) return rc;
  t.queued_in_half = 1;
  const int ahead = std::min(s->lookahead, nu.half_remaining());
  for (int k = 0; k < ahead; ++k) {
    if (int rc = train_launch(s, u, nullptr, nullptr, nu.signed_step(), nu.inv_mass, own(t.queued_in_half))) return rc;
    t.queued_in_half += 1;
  }
  return ABD_OK;
}

// has the oldest outstanding record of unit u landed? (never blocks)
bool train_ready(const abd_sampler* s, int u) {
  const abd_sampler::TrainUnit& t = s->tu[(size_t)u];
  if (t.cons >= t.prod) return false;
  const size_t k = (size_t)(t.cons % abd_sampler::kTrainRing);
  if (*(volatile const double*)&t.rec.host()[k].tag != t.tags[k]) return false;
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  return true;
}

// ---- The two ways a unit of sampler_run_units gets an evaluation (RowEval, TrainEval), with the same four operations ----
//   eval(u, m, ids, th)   evaluate the points th[0 .. m) of the chains with slot ids ids[0 .. m)
//   grow(u, un)           launch the next leapfrog of every tree of the unit that is still growing; un.m: how many are
//   ready(u)              has the oldest outstanding result of the unit landed?  Never blocks.
//   take(u, lp, gr, ...)  that result: logp and gradient per chain evaluated and, from a train, the successor's point
// and for the starting points' blocking wait (wait_eval): kSpins, the polls before it synchronises the unit's stream, and
// never(u), the error of a result that is not there even then.  s->trains is asked where a back-end is chosen, nowhere else.

// One unit of sampler_run_units: chains [lo, hi) of the sampler move through their iterations together
struct Unit {
  int lo = 0, hi = 0, m = 0, state = 0;  // m: chains in the evaluation that is outstanding, who[0 .. m) of the sampler
  int64_t k = 0;                         // iterations completed in this call
  std::chrono::steady_clock::time_point t_queued;  // profile: when its last evaluation was about to be queued
  std::vector<int32_t> ids, who;
  std::vector<double> th, lp, gr;
  Unit(int lo, int hi) : lo(lo), hi(hi), ids(hi - lo), who(hi - lo), th((hi - lo) * ABD_N_THETA), lp(hi - lo), gr((hi - lo) * ABD_N_THETA) {}
  // ids, who, th, m of the next evaluation: `growing` -- the chains whose tree is still growing, at the point it asks for;
  // else all of them, at the point they are at
  void stage(abd_sampler* s, bool growing) {
    m = 0;
    for (int j = lo; j < hi; ++j) {
      abdnuts::Nuts& nu = s->ch[(size_t)j].nuts;
      if (growing && !nu.active) continue;
      ids[(size_t)m] = s->chains[(size_t)j];
      who[(size_t)m] = j;
      std::memcpy(th.data() + (size_t)m * ABD_N_THETA, growing ? nu.request() : nu.q, sizeof(double) * ABD_N_THETA);
      ++m;
    }
  }
};

// Result rows: one evaluation launch for the unit's chains into its private rows (slot kSyncSlot + u), tagged from the unit's
// own sequence when several host threads drive the units, else from the context's
struct RowEval {
  static constexpr long kSpins = 2000000;
  abd_sampler* s;
  bool unit_seq;
  std::vector<std::pair<int, double>> out;  // per unit: the rows of its last launch and their tag
  RowEval(abd_sampler* s, bool unit_seq) : s(s), unit_seq(unit_seq), out((size_t)n_units(s)) {}
  int eval(int u, int m, const int32_t* ids, const double* th) {
    abd_ctx* c = s->c;
    double* seqp = unit_seq ? &c->unit_seq[(size_t)u] : nullptr;
    if (int rc = enqueue_slot(c, Caller{Caller::Unit, unit_pipe(c, u), seqp}, kSyncSlot + u, m, ids, th, true)) return rc;
    out[(size_t)u] = {m, seqp ? *seqp : c->seq};
    return ABD_OK;
  }
  int grow(int u, Unit& un) {
    un.stage(s, true);
    return un.m ? eval(u, un.m, un.ids.data(), un.th.data()) : ABD_OK;
  }
  bool ready(int u) const { return rows_missing(s->c, kSyncSlot + u, 0, out[(size_t)u].first - 1, out[(size_t)u].second) < 0; }
  int take(int u, double* lp, double* gr, const double*&, const double*&) { return fetch_slot(s->c, kSyncSlot + u, lp, gr); }
  int never(int u) const { return rows_never_tagged(s->c, kSyncSlot + u, 0, out[(size_t)u].first, out[(size_t)u].second); }
};

// Observation-list trains (abd_sampler::trains; one chain per unit): every evaluation is a train launch that assembles its
// own result into the unit's record ring, a plain one with ve = 0
struct TrainEval {
  static constexpr long kSpins = 4000000;
  abd_sampler* s;
  const double* metric = nullptr;  // of a plain evaluation (it cannot tell at ve = 0); nullptr: the chain's own
  int eval(int u, int, const int32_t*, const double* th) {
    return train_launch(s, u, th, nullptr, 0.0, metric ? metric : s->ch[(size_t)u].nuts.inv_mass, true);
  }
  int grow(int u, Unit& un) {
    abdnuts::Nuts& nu = s->ch[(size_t)u].nuts;
    abd_sampler::TrainUnit& t = s->tu[(size_t)u];
    un.m = nu.active ? 1 : 0;
    if (!nu.active) {
      t.cons = t.prod;  // what is still queued for a half that ended early is never read
      return ABD_OK;
    }
    un.who[0] = u;
    if (nu.n_leaf == 0) return train_begin(s, u);  // a new half: its first point is staged on the host
    if (t.queued_in_half < nu.n_target) {          // the half goes on: keep the look-ahead full
      t.queued_in_half += 1;
      return train_launch(s, u, nullptr, nullptr, nu.signed_step(), nu.inv_mass, s->lookahead == 0 || t.queued_in_half == nu.n_target);
    }
    return ABD_OK;
  }
  bool ready(int u) const { return train_ready(s, u); }
  int take(int u, double* lp, double* gr, const double*& next_q, const double*& next_p_half) {
    abd_sampler::TrainUnit& t = s->tu[(size_t)u];
    const TrainRecord& r = t.rec.host()[t.cons % abd_sampler::kTrainRing];
    *lp = r.lp;
    std::memcpy(gr, r.g, sizeof(double) * ABD_N_THETA);
    next_q = r.next_theta;  // (the slot is not written again before kTrainRing more launches have been queued)
    next_p_half = r.next_p_half;
    t.cons += 1;
    return ABD_OK;
  }
  int never(int u) const { return fail(ABD_ERR_STATE, "the record of chain %d's starting point never received its tag", s->chains[(size_t)u]); }
};

// Block until unit u's evaluation has landed: polls ready(); a result that has not shown after kSpins polls (tens of ms) is
// waited for with a synchronise of the unit's stream, which is counted (abd_wait_fallbacks), and is an error if it is not there then
template <typename Eval>
int wait_eval(Eval& ev, int u) {
  abd_ctx* c = ev.s->c;
  for (long spin = 0; !ev.ready(u); ++spin) {
    if (spin < Eval::kSpins) {
      __builtin_ia32_pause();
      continue;
    }
    __atomic_fetch_add(&c->wait_fallbacks, (int64_t)1, __ATOMIC_RELAXED);
    HIP_TRY(hipStreamSynchronize(c->pipe[unit_pipe(c, u)].st));
    return ev.ready(u) ? ABD_OK : ev.never(u);
  }
  return ABD_OK;
}

// logp and gradient at the starting points, unit by unit through the launch shape the units will use
template <typename Eval>
int start_points(Eval ev, const double* theta0) {
  abd_sampler* s = ev.s;
  for (int u = 0, lo = 0; lo < s->n; ++u, lo += s->unit) {
    const double *next_q, *next_p_half;
    if (int rc = ev.eval(u, std::min(s->unit, s->n - lo), s->chains.data() + lo, theta0 + (size_t)lo * ABD_N_THETA)) return rc;
    if (int rc = wait_eval(ev, u)) return rc;
    if (int rc = ev.take(u, s->lp.data() + lo, s->gr.data() + (size_t)lo * ABD_N_THETA, next_q, next_p_half)) return rc;
  }
  return ABD_OK;
}

// Record staging, allocated at the first call that records: up to rec_chunk draws per chain of the Deterministics and the
// discrete state, and -- each at the first call that asks for it -- one per-reading row per draw ([n][rec_chunk][K_s + K_n])
// of the pointwise log-likelihood and of the posterior predictive replicates
int alloc_record_staging(abd_sampler* s, bool with_ll, bool with_yrep) {
  abd_ctx* c = s->c;
  const size_t n = (size_t)s->n, cells = (size_t)c->G * c->N, Kt = (size_t)(c->s.K + c->n.K);
  HIP_TRY(hipSetDevice(c->device));
  if (!s->d_rec_mu) {
    const size_t per_draw = n * (cells * 18 + c->N + (with_ll ? Kt * sizeof(double) : 0) +
                                 (with_yrep ? Kt * sizeof(double) : 0));  // bytes staged per draw, all chains
    s->rec_chunk = std::max<int64_t>(1, std::min<int64_t>(256, (int64_t)(((size_t)256 << 20) / per_draw)));
    DevBuf<double> mu;  // (the sampler takes both or neither: d_rec_mu is the "allocated" flag)
    DevBuf<int8_t> i8;
    HIP_TRY(mu.alloc(2 * n * s->rec_chunk * cells));
    HIP_TRY(i8.alloc(2 * n * s->rec_chunk * cells + n * s->rec_chunk * c->N));
    s->d_rec_mu = std::move(mu);
    s->d_rec_i8 = std::move(i8);
  }
  auto rows = [&](DevBuf<double>& d, const char* what) -> int {
    if (d) return ABD_OK;
    if (const hipError_t e = d.alloc(std::max<size_t>(1, n * s->rec_chunk * Kt)))
      return fail(ABD_ERR_HIP, "record staging (%s): %s", what, hipGetErrorString(e));
    return ABD_OK;
  };
  if (with_ll)
    if (int rc = rows(s->d_rec_ll, "pointwise log-likelihood")) return rc;
  if (with_yrep) {
    if (int rc = upload_order(c)) return rc;
    if (int rc = rows(s->d_rec_yrep, "posterior predictive")) return rc;
  }
  return ABD_OK;
}

}  // namespace

// Quiesce: launches of a half that ended early may still be on their way (trains); without trains the members' last users
// are on the context's stream
abd_sampler::~abd_sampler() {
  (void)hipSetDevice(c->device);
  (void)((!tu.empty() || !dc.empty()) ? hipDeviceSynchronize() : hipStreamSynchronize(c->stream));
}

extern "C" {

int abd_sampler_create(abd_ctx* c, int32_t n, const int32_t* chains, const double* theta0, const abd_sampler_opts* opts,
                       abd_sampler** out) {
  if (!c || !chains || !theta0 || !opts || !out) return fail(ABD_ERR_ARG, "NULL argument");
  *out = nullptr;
  if (int rc = check_chains(c, n, chains)) return rc;
  for (int a = 0; a < n; ++a)
    for (int b = a + 1; b < n; ++b)
      if (chains[a] == chains[b]) return fail(ABD_ERR_ARG, "chain %d listed twice", chains[a]);
  if (opts->tune < 0) return fail(ABD_ERR_ARG, "tune=%lld is negative", (long long)opts->tune);
  if (opts->chain_offset < 0) return fail(ABD_ERR_ARG, "chain_offset=%d is negative", opts->chain_offset);
  if (opts->max_treedepth < 1 || opts->max_treedepth > abdnuts::MAX_DEPTH)
    return fail(ABD_ERR_ARG, "max_treedepth=%d outside [1, %d]", opts->max_treedepth, abdnuts::MAX_DEPTH);
  if (!(opts->target_accept > 0.0 && opts->target_accept < 1.0))
    return fail(ABD_ERR_ARG, "target_accept=%g outside (0, 1)", opts->target_accept);
  std::unique_ptr<abd_sampler> sp(new (std::nothrow) abd_sampler());  // every early return releases the half-built sampler
  abd_sampler* const s = sp.get();
  if (!s) return fail(ABD_ERR_NOMEM, "out of host memory");
  s->c = c;
  s->n = n;
  s->o = *opts;
  s->chains.assign(chains, chains + n);
  s->ch.resize((size_t)n);
  s->lp.resize((size_t)n);
  s->gr.resize((size_t)n * ABD_N_THETA);
  // chains per unit: a large dense cohort keeps the chip busy with one chain per launch and gains most from chains
  // that never wait for each other; a small cohort is bound by the host's ~6 us per launch, which a unit's chains share
  // (measured, tools/probe_nuts_rate.py: config 3 -- 8 chains 88 k evals/s with units of 1, 82 k with 4; 16 chains 92 k / 112 k;
  // default cohort, 16 chains -- 152 k with units of 1, 334 k with 4, 359 k with 8)
  // host threads that drive the units: one for dense cohorts (bound by the device), up to four for observation lists
  // (bound by the host's two launches per evaluation)
  s->threads = c->dense ? 1 : 4;
  s->threads = std::max(1, std::min(16, env_int("ABD_SAMPLER_THREADS", s->threads)));
  // With four host threads (observation lists) the best split is four units -- one per thread and per
  // hardware queue: default cohort, evaluations/s seen by NUTS with 4 / 8 / 16 chains 217 k / 339 k / 491 k against
  // 166 k / 253 k / 300-370 k for the best split on one thread.
  // Large dense cohorts (one host thread): at most about four units -- the hardware queues -- of 1, 2, 4 or 8 chains, the
  // sizes the dense kernel has a shape for (config 3, evaluations/s seen by NUTS over 150-300 iterations: 8 chains 79 k
  // with units of 1, 112 k with 2; 12 chains 97 k / 88 k / 83 k with 2 / 3 / 4; 16 chains 91 k / 100 k with 2 / 4;
  // 32 chains 100 k / 134 k with 4 / 8)
  // With leapfrog trains (one chain per unit) and the streams spread evenly over the hardware queues, eight chains run best
  // as eight units, two per queue: 126 k against 121 k as four units of two; sixteen chains: 145 k as eight units of two,
  // 155 k as four units of four
  const bool trains_ok = (c->dense || c->obs_lanes) && c->dense_own_sum && opts->dense_metric == 0 && env_int("ABD_SAMPLER_TRAINS", 1) != 0;
  int dense_unit = 1;
  while (dense_unit < 8 && 2 * dense_unit <= n / 4) dense_unit *= 2;
  // dense trains: units of 1, 2 or 4 chains (abd_sampler::dtrains)
  s->dtrains = trains_ok && c->dense;
  // as few chains per unit as keep the units within the four hardware queues (a queue runs one kernel at a time): measured at
  // config 3, evaluations/s seen by NUTS while all chains are at work, units of 1 / 2 / 4 chains -- 4 chains 139 k / 138 k /
  // 102 k; 8 chains 140 k / 176 k / 183 k; 16 chains - / 149 k / 195 k
  if (s->dtrains) dense_unit = n <= 4 ? 1 : (n < 8 ? 2 : 4);
  s->unit = (c->dense && ((int64_t)c->G * c->N >= 500000 || s->dtrains)) ? dense_unit : std::max(s->threads > 1 ? 1 : 2, std::min(8, (n + 3) / 4));
  s->unit = env_int("ABD_SAMPLER_UNIT", s->unit);
  s->unit = std::max(1, std::min({s->unit, n, (int)ABD_MAX_BATCH}));
  if (s->dtrains && s->unit != 1 && s->unit != 2 && s->unit != 4) s->dtrains = false;  // (a train unit is a workgroup's waves)

  // the starting points through the launch shape the units will use
  if (hipSetDevice(c->device) != hipSuccess) return fail(ABD_ERR_HIP, "hipSetDevice failed");
  if (int rc = flush_ring(c)) return rc;
  if (n_units(s) > 1 && tune_int("ABD_PROBE_QUEUES", 1) != 0)
    if (int rc = probe_stream_queues(c)) return rc;
  s->trains = trains_ok && !c->dense && s->unit == 1;
  if (s->dtrains) {
    // the unit's launch shape: two workgroups per CU, however many units there are (config 3, evaluations/s seen by NUTS over
    // the call with 1 / 2 per CU: 3 chains 78 k / 78 k but 94 k / 106 k while all are at work, 4 chains 128 k / 129 k and the compound
    // iteration 966 / 1 027 per s, 5 chains 85 k / 120 k, 7 chains 106 k / 123 k, 16 chains as units of four 125 k / 136 k; 3 or 4
    // per CU are slower again: profiles/r04/b_train_grid_*.txt): chains finish their trees and iterations at different times, and
    // a unit that is alone for a while gets through its launches faster on the larger grid.  A unit that is alone for the whole run
    // takes four per CU where its ranges are long enough to pay for the set-up (config 5: 77 gap rows per range)
    int per_cu = std::min(2, c->dbpc);
    if (n_units(s) == 1) {
      const int64_t rows = (int64_t)c->n_lg * c->G, nsub = ABD_WAVES_PER_BLOCK / std::max(1, s->unit);
      if (rows / ((int64_t)c->n_cu * c->dbpc * nsub) >= 32) per_cu = c->dbpc;
    }
    s->dtrain_blocks = dense_blocks(c, s->unit, 0, 1);                      // (the cap that keeps ranges >= kMinRows rows)
    s->dtrain_blocks = std::min(s->dtrain_blocks, c->n_cu * per_cu);
    if (const int tb = tune_int("ABD_TRAIN_BLOCKS_PER_CU", 0)) s->dtrain_blocks = std::max(1, std::min({c->n_cu * tb, c->blocks_max, dense_blocks(c, s->unit, 0, 1)}));
    s->dtrain_lookahead = std::max(2, std::min(ABD_TRAIN_RING / 2, tune_int("ABD_TRAIN_LOOKAHEAD", 3)));
    if (int rc = dtrain_alloc(s)) return rc;
  }
  s->lookahead = std::max(0, std::min(abd_sampler::kTrainRing - 2, tune_int("ABD_TRAIN_LOOKAHEAD", 8)));
  if (s->trains)
    if (int rc = train_alloc(s)) return rc;
  // (every evaluation of a sampler with trains is assembled on the device: see abd_sampler::trains)
  const double ones[ABD_N_THETA] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
  if (int rc = s->trains ? start_points(TrainEval{s, ones}, theta0) : start_points(RowEval(s, false), theta0)) return rc;
  for (int k = 0; k < n; ++k) {
    if (!std::isfinite(s->lp[(size_t)k])) return fail(ABD_ERR_ARG, "logp at the starting point of chain %d is not finite", chains[k]);
    s->ch[(size_t)k].init(theta0 + (size_t)k * ABD_N_THETA, s->lp[(size_t)k], s->gr.data() + (size_t)k * ABD_N_THETA,
                          opts->seed, (uint64_t)((int64_t)chains[k] + opts->chain_offset), opts->tune, opts->max_treedepth, opts->target_accept,
                          opts->dense_metric != 0);
  }
  if (opts->accumulate) HIP_TRY(s->d_sums.alloc_zero((size_t)n * 3 * c->G * c->N, c->stream));
  *out = sp.release();
  return ABD_OK;
}

void abd_sampler_destroy(abd_sampler* s) { delete s; }

int abd_sampler_run(abd_sampler* s, int64_t n_iter, double* theta, double* stats) {
  return abd_sampler_run_record(s, n_iter, theta, stats, nullptr);
}

}  // extern "C"

namespace {

// copy staged draws [0, filled) of chain k to the caller's arrays, starting at draw `first` (stream st, waited for)
int record_flush_chain(abd_sampler* s, const abd_record* rec, int k, int64_t first, int64_t filled, hipStream_t st) {
  if (filled == 0) return ABD_OK;
  abd_ctx* c = s->c;
  const size_t cells = (size_t)c->G * c->N, N = (size_t)c->N;
  const size_t per_var = (size_t)s->n * s->rec_chunk * cells;
  const size_t dev = (size_t)k * s->rec_chunk, host = (size_t)k * rec->capacity + first;
  if (rec->ab_n_mu) HIP_TRY(hipMemcpyAsync(rec->ab_n_mu + host * cells, s->d_rec_mu + dev * cells, filled * cells * sizeof(double), hipMemcpyDeviceToHost, st));
  if (rec->ab_s_mu) HIP_TRY(hipMemcpyAsync(rec->ab_s_mu + host * cells, s->d_rec_mu + per_var + dev * cells, filled * cells * sizeof(double), hipMemcpyDeviceToHost, st));
  if (rec->i_raw) HIP_TRY(hipMemcpyAsync(rec->i_raw + host * cells, s->d_rec_i8 + dev * cells, filled * cells, hipMemcpyDeviceToHost, st));
  if (rec->i) HIP_TRY(hipMemcpyAsync(rec->i + host * cells, s->d_rec_i8 + per_var + dev * cells, filled * cells, hipMemcpyDeviceToHost, st));
  if (rec->ab_s_waner) HIP_TRY(hipMemcpyAsync(rec->ab_s_waner + host * N, s->d_rec_i8 + 2 * per_var + dev * N, filled * N, hipMemcpyDeviceToHost, st));
  // per-reading rows (pointwise log-likelihood, posterior predictive replicates): staged in the device's sorted order,
  // scattered back to the caller's order of the readings
  const size_t Ks = (size_t)c->s.K, Kn = (size_t)c->n.K, Kt = Ks + Kn;
  struct Rows {
    const double* dev;
    double* out_s;
    double* out_n;
    std::vector<double> h;
  } rows[2] = {{s->d_rec_ll, rec->ll_s, rec->ll_n, {}}, {s->d_rec_yrep, rec->yrep_s, rec->yrep_n, {}}};
  for (Rows& r : rows)
    if ((r.out_s || r.out_n) && Kt) {
      r.h.resize((size_t)filled * Kt);
      HIP_TRY(hipMemcpyAsync(r.h.data(), r.dev + dev * Kt, r.h.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    }
  HIP_TRY(hipStreamSynchronize(st));
  for (const Rows& rw : rows)
    for (size_t d = 0; d < rw.h.size() / std::max<size_t>(Kt, 1); ++d) {
      const ReadingOut o[1] = {{rw.out_s ? rw.out_s + (host + d) * Ks : nullptr, rw.out_n ? rw.out_n + (host + d) * Kn : nullptr}};
      const double* r = rw.h.data() + d * Kt;
      scatter_readings(c, o, [r](int, size_t k) { return r[k]; });
    }
  return ABD_OK;
}

// One abd_sampler_run_record call as both run loops see it: the caller's arrays, and per chain the draws of its record that
// are staged on the device ([flushed_to, flushed_to + staged) of the caller's record).  The chains of a unit move through
// their iterations together; a chain belongs to one host thread.
struct RunFrame {
  abd_sampler* s;
  int64_t n_iter;
  double* theta;
  double* stats;
  const abd_record* rec;  // nullptr: nothing is recorded
  int64_t thin;           // iterations 0, thin, 2 thin, ... of the call are recorded
  std::chrono::steady_clock::time_point t_begin;
  bool profile;           // ABD_SAMPLER_PROFILE (arm_profile)
  struct Staging {
    int64_t staged = 0, flushed_to = 0;
  };
  std::vector<Staging> staging;
};

// the caller's theta and stats rows of chain j at iteration k of the call (its point is final); counts: accepted / proposed
// of the chain's sweep (nullptr: no sweep)
void write_draw(const RunFrame& f, int j, int64_t k, const unsigned long long* counts) {
  const abdnuts::Nuts& nu = f.s->ch[(size_t)j].nuts;
  const size_t row = (size_t)j * f.n_iter + k;
  if (f.theta) std::memcpy(f.theta + row * ABD_N_THETA, nu.q, sizeof(double) * ABD_N_THETA);
  if (!f.stats) return;
  double* o = f.stats + row * ABD_N_STATS;
  o[ABD_STAT_LP] = nu.lp;
  o[ABD_STAT_TREE_DEPTH] = nu.stats.tree_depth;
  o[ABD_STAT_N_STEPS] = nu.stats.n_steps;
  o[ABD_STAT_MEAN_TREE_ACCEPT] = nu.stats.mean_tree_accept;
  o[ABD_STAT_STEP_SIZE] = nu.stats.step_size;
  o[ABD_STAT_DIVERGING] = nu.stats.diverging ? 1.0 : 0.0;
  o[ABD_STAT_ENERGY] = nu.stats.energy;
  o[ABD_STAT_MAX_ENERGY_ERROR] = nu.stats.max_energy_error;
  o[ABD_STAT_GIBBS_ACCEPTED] = counts ? (double)counts[0] : 0.0;
  o[ABD_STAT_GIBBS_PROPOSED] = counts ? (double)counts[1] : 0.0;
  o[ABD_STAT_T_DONE] = std::chrono::duration<double>(std::chrono::steady_clock::now() - f.t_begin).count();
}

// The sweep of iteration k of the call on the sampler's chains lo .. lo + m - 1 (slot ids `ids`, points `theta`), queued on
// stream st: the sweep's random stream (its seed is derived from the sampler's, the chains' counter words are offset by
// chain_offset, the sweep number is the iteration) and the chains' own counts and work-queue heads.  The counts of chain j
// land in c->d_counts_chain + 2 j.
int queue_sweep(abd_sampler* s, int lo, int m, const int32_t* ids, const double* theta, int64_t k, hipStream_t st) {
  abd_ctx* c = s->c;
  return enqueue_gibbs(c, m, ids, theta, (s->o.seed << 20) ^ 0x5EEDull, (uint32_t)(s->it + k), (uint32_t)s->o.chain_offset, st,
                       c->d_counts_chain + 2 * (size_t)lo, c->d_work + c->n_slots + lo, nullptr);
}

// the device work of chain j's draw at iteration k of the call (point and discrete state are final), all on stream st, behind
// the chain's sweep and in front of its next one: the Deterministics into the draw's record and / or the running sums (one
// launch), the rest of the record, the pointwise log-likelihood, the posterior predictive.  These kernels read the discrete state and the point (by
// value), nothing else.  Then the chain's staging: a full chunk, and what is left at the call's last iteration, is copied
// out and waited for.  Nothing else is launched here.
int queue_draw(RunFrame& f, int j, int64_t k, hipStream_t st) {
  abd_sampler* s = f.s;
  abd_ctx* c = s->c;
  const abd_record* rec = (f.rec && k % f.thin == 0) ? f.rec : nullptr;  // (nullptr: this draw is not recorded)
  const int64_t iter = s->it + k;
  const bool draw = iter >= s->o.tune;
  RunFrame::Staging& sg = f.staging[(size_t)j];
  const int chain = s->chains[(size_t)j];
  const double* q = s->ch[(size_t)j].nuts.q;
  const size_t cells = (size_t)c->G * c->N, N = (size_t)c->N, Kt = (size_t)(c->s.K + c->n.K);
  const size_t per_var = (size_t)s->n * s->rec_chunk * cells, at = (size_t)j * s->rec_chunk + (size_t)sg.staged;
  double* sums = (draw && s->d_sums) ? s->d_sums + (size_t)j * 3 * cells : nullptr;
  int8_t* i = (rec && rec->i) ? s->d_rec_i8 + per_var + at * cells : nullptr;
  double* n_mu = (rec && rec->ab_n_mu) ? s->d_rec_mu + at * cells : nullptr;
  double* s_mu = (rec && rec->ab_s_mu) ? s->d_rec_mu + per_var + at * cells : nullptr;
  if (i || n_mu || s_mu || sums)
    if (int rc = launch_deterministics(c, chain, q, st, i, n_mu, s_mu, sums)) return rc;
  if (rec && rec->i_raw)
    if (int rc = launch_unpack(c, chain, s->d_rec_i8 + at * cells, st)) return rc;
  if (rec && rec->ab_s_waner)
    HIP_TRY(hipMemcpyAsync(s->d_rec_i8 + 2 * per_var + at * N, c->slots[(size_t)chain].waner, N, hipMemcpyDeviceToDevice, st));
  // pointwise log-likelihood: the record's row and / or -- a draw, accumulation on -- the running statistics
  double* ll = (rec && (rec->ll_s || rec->ll_n)) ? s->d_rec_ll + at * Kt : nullptr;
  double* acc = (draw && s->d_pw_acc) ? s->d_pw_acc + (size_t)j * 4 * Kt : nullptr;
  if (ll || acc)
    if (int rc = launch_pointwise(c, chain, q, st, ll, acc, iter - s->o.tune + 1)) return rc;
  // ... and per individual, a draw: one launch for the running statistics of T_j (accumulation on) and the rows of the LOO
  // matrix (abd_loo.hpp), whose staging goes into the matrix when it is full and at the call's last iteration
  if (draw && (s->d_ind_acc || s->loo.on()))
    if (int rc = s->loo.launch(c, j, chain, q, iter - s->o.tune, k + 1 == f.n_iter, s->d_ind_acc ? s->d_ind_acc + (size_t)j * 4 * N : nullptr, st))
      return rc;
  // posterior predictive: the record's replicate row (keyed by seed, the chain's global id and the iteration, so that
  // abd_posterior_predictive reproduces it) and / or -- a draw, accumulation on -- the check statistics
  double* yrep = (rec && (rec->yrep_s || rec->yrep_n)) ? s->d_rec_yrep + at * Kt : nullptr;
  double* pacc = (draw && s->d_pp_acc) ? s->d_pp_acc + (size_t)j * 3 * Kt : nullptr;
  if (yrep || pacc)
    if (int rc = launch_predictive(c, chain, q, st, s->o.seed, (uint32_t)((int64_t)chain + s->o.chain_offset), (uint64_t)iter, yrep,
                                   nullptr, pacc, iter - s->o.tune + 1))
      return rc;
  // the summaries: every draw, whatever is recorded (abd_sampler_run_record has checked the planned draws)
  if (draw) {
    const int64_t d = iter - s->o.tune;
    auto launch = [&](const auto& x) { return x.on() ? x.launch(c, j, chain, q, d, st) : ABD_OK; };
    if (int rc = launch(s->curves)) return rc;
    if (int rc = launch(s->diag)) return rc;
    if (int rc = launch(s->timelines)) return rc;
    if (int rc = launch(s->risk)) return rc;
  }
  if (rec) sg.staged += 1;
  if (f.rec && (sg.staged == s->rec_chunk || k + 1 == f.n_iter)) {
    if (int rc = record_flush_chain(s, f.rec, j, sg.flushed_to, sg.staged, st)) return rc;
    sg.flushed_to += sg.staged;
    sg.staged = 0;
  }
  return ABD_OK;
}

// host threads that drive the units of sampler_run_units: a power of two <= 8, so that units that share a HIP stream (u and
// u + 8) share their thread (one thread while abd_kernel_timing is on: the event bookkeeping of enqueue_group belongs to the
// context, not to a unit)
int unit_threads(const abd_sampler* s) {
  int T = 1;
  while (s->c->timing == 0 && 2 * T <= std::min({s->threads, n_units(s), (int)kMaxPipes})) T *= 2;
  return T;
}

// ABD_SAMPLER_PROFILE=1 (read once): both run loops report to stderr where the host's time went.  A run call clears the
// account of the time inside the launch calls (abd_host.hpp: LaunchProfile) and -- `launches`: its loop runs on one thread,
// which the account needs -- arms it; the call disarms it when its loop has ended.
bool arm_profile(bool launches) {
  static const bool profile = env_int("ABD_SAMPLER_PROFILE", 0) != 0;
  g_launch_profile = LaunchProfile();
  g_launch_profile.on = profile && launches;
  return profile;
}

// The profile of one host thread of sampler_run_units: how much of the wall time it spends handling results and queueing
// launches, and on what.  With the profile off every member is a test of `on` and nothing else.
struct Laps {
  using clk = std::chrono::steady_clock;
  const bool on;
  clk::time_point t_begin, t_busy, t_lap;
  bool busy = false;  // a result has been handled in this pass over the units: the thread is busy until the pass ends
  double busy_s = 0.0, fetch = 0.0, feed = 0.0, launch = 0.0, wait = 0.0;
  long handled = 0;
  explicit Laps(bool on) : on(on) {
    if (on) t_begin = clk::now();
  }
  static double seconds(clk::duration d) { return std::chrono::duration<double>(d).count(); }
  void result(const Unit& un) {  // a result of the unit has been seen: the laps of its handling start
    if (!on) return;
    t_lap = clk::now();
    if (!busy) t_busy = t_lap;
    busy = true;
    wait += seconds(t_lap - un.t_queued);
    ++handled;
  }
  void operator()(double Laps::*account) {  // the time since the last lap goes to `account`
    if (!on) return;
    const clk::time_point t = clk::now();
    this->*account += seconds(t - t_lap);
    t_lap = t;
  }
  void pass_end() {
    if (on && busy) busy_s += seconds(clk::now() - t_busy);
    busy = false;
  }
  void report(int tid, int T, int n_units, int B) const {
    if (!on) return;
    const double wall = seconds(clk::now() - t_begin), per = handled ? 1e6 / handled : 0.0;
    std::fprintf(stderr, "abd sampler: thread %d of %d, %d units of %d chains in all, %ld results handled in %.3f s: host busy %.0f %% "
                 "(%.2f us per result: %.2f assemble, %.2f NUTS, %.2f queueing the next evaluation); evaluation queued -> result seen %.2f us\n",
                 tid, T, n_units, B, handled, wall, 100.0 * busy_s / wall, per * busy_s, per * fetch, per * feed, per * launch, per * wait);
    if (g_launch_profile.on)
      std::fprintf(stderr, "abd sampler: inside hipLaunchKernelGGL: %.2f us per evaluation launch (%ld), %.2f us per sum launch (%ld)\n",
                   g_launch_profile.evals ? 1e6 * g_launch_profile.eval_s / g_launch_profile.evals : 0.0, g_launch_profile.evals,
                   g_launch_profile.sums ? 1e6 * g_launch_profile.sum_s / g_launch_profile.sums : 0.0, g_launch_profile.sums);
  }
};

// The sampler's chains run as independent UNITS of `unit` consecutive chains (1 for large dense cohorts, 4 otherwise;
// abd_sampler_create), unit u on HIP stream u mod 8, its evaluations through the back-end `ev` (above):
//   tree:      one evaluation launch per leapfrog for the unit's chains whose tree is still growing
//   sweep:     when all its trees have stopped, the unit's Gibbs sweep and the evaluation at the new state are queued
//              back to back on its stream (stream order: no host wait in between), counts copied to pinned memory
//   recording: queued on the same stream behind them
// The host polls for the result of whatever is in flight and moves each unit's state machine on.  No unit waits
// for another one's trees -- in lock step an iteration lasts as long as the LONGEST tree of all chains -- and the
// units' launches overlap on the device.  Within a unit the chains share launches (small cohorts are launch-bound:
// ~6 us of host time per evaluation launch).  Same compound step per chain, same random streams, and the numbers a
// unit's launch produces depend only on the unit (fixed grid), never on the other units or on timing.
// The units are driven by T host threads, thread t the units u = t (mod T): what a thread touches is private to its
// units (stream, result rows or record ring, tag sequence, chains, the caller's arrays per chain) or read-only, so the
// threads share nothing but the HIP runtime.  T = 1 for dense cohorts (the device bounds them), up to 4 for observation
// lists, where the host's two launches per evaluation (~7 us) are what bounds a single thread.
template <typename Eval>
int run_units(RunFrame& f, Eval ev, const int T) {
  abd_sampler* s = f.s;
  abd_ctx* c = s->c;
  const int64_t n_iter = f.n_iter;
  const int U = n_units(s);
  enum { EVAL, POST, DONE };  // a unit waits for: a leapfrog of its trees; the evaluation behind its sweep; nothing
  std::vector<Unit> units;
  auto stream_of = [&](int u) -> hipStream_t { return c->pipe[unit_pipe(c, u)].st; };
  auto grow = [&](int u) -> int {
    if (f.profile) units[(size_t)u].t_queued = Laps::clk::now();
    return ev.grow(u, units[(size_t)u]);
  };
  // end of iteration un.k of the unit's chains (points and discrete states are final): outputs, running sums, recording;
  // then the next iteration's first leapfrogs, or DONE
  auto finish_iteration = [&](int u, bool with_counts) -> int {
    Unit& un = units[(size_t)u];
    for (int j = un.lo; j < un.hi; ++j) write_draw(f, j, un.k, with_counts ? c->h_counts_chain.host() + 2 * (size_t)j : nullptr);
    // the next iteration's first leapfrogs go out BEFORE this iteration's recording is queued: the recording kernels read the
    // point (by value) and the discrete state, which only the next sweep -- queued after them -- changes, and the host's time
    // for queueing them (several launches per draw) passes while the device is already at work for the chain
    const bool last = un.k + 1 == n_iter;
    if (!last) {
      for (int j = un.lo; j < un.hi; ++j) s->ch[(size_t)j].begin();
      un.state = EVAL;
      if (int rc = grow(u)) return rc;
    }
    for (int j = un.lo; j < un.hi; ++j)
      if (int rc = queue_draw(f, j, un.k, stream_of(u))) return rc;
    un.k += 1;
    if (last) un.state = DONE;
    return ABD_OK;
  };
  // binary Gibbs-Metropolis on [i_raw, ab_s_waner] of the unit's chains, then logp and gradient at the new states: queued
  // back to back on the unit's stream
  auto sweep_and_eval = [&](int u) -> int {
    Unit& un = units[(size_t)u];
    hipStream_t st = stream_of(u);
    un.stage(s, false);
    if (int rc = queue_sweep(s, un.lo, un.m, un.ids.data(), un.th.data(), un.k, st)) return rc;
    HIP_TRY(hipMemcpyAsync(c->h_counts_chain.host() + 2 * (size_t)un.lo, c->d_counts_chain + 2 * (size_t)un.lo,
                           (size_t)un.m * 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    un.state = POST;
    if (f.profile) un.t_queued = Laps::clk::now();
    return ev.eval(u, un.m, un.ids.data(), un.th.data());
  };
  for (int u = 0; u < U; ++u) units.emplace_back(u * s->unit, std::min(s->n, (u + 1) * s->unit));
  for (int u = 0; u < U; ++u) {
    Unit& un = units[(size_t)u];
    un.state = n_iter ? EVAL : DONE;
    if (n_iter == 0) continue;
    for (int j = un.lo; j < un.hi; ++j) s->ch[(size_t)j].begin();
    if (int rc = grow(u)) return rc;
  }
  std::atomic<int> first_error{ABD_OK};
  std::vector<std::string> errors((size_t)T);
  auto worker = [&](int tid) -> int {
    if (hipSetDevice(c->device) != hipSuccess) return fail(ABD_ERR_HIP, "hipSetDevice failed");
    Laps lap(f.profile);
    for (long spins = 0;;) {
      bool any = false, progressed = false;
      if (first_error.load(std::memory_order_relaxed) != ABD_OK) return ABD_OK;  // another thread failed: stop queueing
      for (int u = tid; u < U; u += T) {
        Unit& un = units[(size_t)u];
        if (un.state == DONE) continue;
        any = true;
        if (!ev.ready(u)) continue;
        progressed = true;
        lap.result(un);
        const double *next_q = nullptr, *next_p_half = nullptr;
        if (int rc = ev.take(u, un.lp.data(), un.gr.data(), next_q, next_p_half)) return rc;
        lap(&Laps::fetch);
        if (un.state == POST) {  // the sweep and the evaluation behind it are done (the counts landed before: same stream)
          for (int q = 0; q < un.m; ++q)
            s->ch[(size_t)un.who[(size_t)q]].nuts.set_point(un.lp[(size_t)q], un.gr.data() + (size_t)q * ABD_N_THETA);
          if (int rc = finish_iteration(u, true)) return rc;
          continue;
        }
        for (int q = 0; q < un.m; ++q)
          s->ch[(size_t)un.who[(size_t)q]].nuts.feed(un.lp[(size_t)q], un.gr.data() + (size_t)q * ABD_N_THETA, next_q, next_p_half);
        lap(&Laps::feed);
        const int rc = grow(u);
        lap(&Laps::launch);
        if (rc) return rc;
        if (un.m) continue;  // some tree of the unit is still growing
        for (int j = un.lo; j < un.hi; ++j) s->ch[(size_t)j].end_transition();
        if (int rc2 = s->o.gibbs ? sweep_and_eval(u) : finish_iteration(u, false)) return rc2;
      }
      lap.pass_end();
      if (!any) break;
      if (progressed) {
        spins = 0;
      } else if (++spins > 4000000) {
        __atomic_fetch_add(&c->wait_fallbacks, (int64_t)1, __ATOMIC_RELAXED);  // no tag for tens of ms: synchronise the streams in flight (see abd_wait_fallbacks)
        for (int u = tid; u < U; u += T)
          if (units[(size_t)u].state != DONE) HIP_TRY(hipStreamSynchronize(stream_of(u)));
        spins = 0;
      } else {
        __builtin_ia32_pause();
      }
    }
    lap.report(tid, T, U, s->unit);
    return ABD_OK;
  };
  auto run_worker = [&](int tid) {
    const int rc = worker(tid);
    if (rc != ABD_OK) {
      errors[(size_t)tid] = last_error();  // the message is thread-local: hand it to the calling thread
      int expected = ABD_OK;
      first_error.compare_exchange_strong(expected, rc);
    }
  };
  {
    std::vector<std::thread> pool;
    for (int t = 1; t < T; ++t) pool.emplace_back(run_worker, t);
    run_worker(0);
    for (auto& th : pool) th.join();
  }
  if (first_error.load() != ABD_OK) {
    for (int t = 0; t < T; ++t)
      if (!errors[(size_t)t].empty()) return fail(first_error.load(), "%s", errors[(size_t)t].c_str());
    return fail(first_error.load(), "sampler thread failed");
  }
  return ABD_OK;
}

// ... with the back-end the sampler was created for, and its tags: one completion-tag sequence per unit when several threads
// drive them, disjoint from the context's and from each other's (unit u: (u + 1) 2^40 + k).  It belongs to the CONTEXT, like
// the result rows kSyncSlot + u the tags are compared against: monotone for the life of those rows, whichever sampler drives them
int sampler_run_units(RunFrame& f) {
  abd_sampler* s = f.s;
  abd_ctx* c = s->c;
  const int T = unit_threads(s);
  while (c->unit_seq.size() < (size_t)n_units(s)) c->unit_seq.push_back((double)(c->unit_seq.size() + 1) * 1099511627776.0);
  s->unit_tags = T > 1;
  return s->trains ? run_units(f, TrainEval{s}, T) : run_units(f, RowEval(s, T > 1), T);
}

// ---- dense cohorts: the compound step over leapfrog-train units (abd_sampler::dtrains) ----
// One host thread.  Per unit (1, 2 or 4 consecutive chains, stream unit_pipe(u)): launches are queued `dtrain_lookahead`
// steps ahead; every launch takes each chain of the unit that is inside a tree one leapfrog further (TrainChainArgs STEP),
// hands a new transition to a chain that is waiting for one (BEGIN, read by the launch's last workgroup) and leaves the
// others alone.  Per chain: the records are taken in order and fed to the NUTS state machine, which runs BEHIND the device;
// when it finds the tree ended, the steps still queued for the chain are stale (their records are never looked at) and the
// chain's iteration goes on beside the unit's launches: sweep + counts on the chain's own stream, then -- the discrete
// state has changed -- a BEGIN whose first step evaluates the start point (EVAL0) before the tree starts from it.
// Nothing a chain computes depends on the other chains or on timing: launch shape and step order are fixed per chain.
int sampler_run_trains(RunFrame& f) {
  abd_sampler* s = f.s;
  abd_ctx* c = s->c;
  const int64_t n_iter = f.n_iter;
  const int n = s->n, B = s->unit;
  const int n_units = abdi::n_units(s);
  enum { NEED_BEGIN, TREE, SWEEP, DONE };
  struct Step {
    int64_t idx;     // record index
    uint32_t epoch;  // the transition it belongs to
    bool eval0;
  };
  struct Run {
    int state = DONE;
    int64_t k = 0;           // iterations completed in this call
    uint32_t epoch = 0;      // counts the chain's transitions: steps of an earlier one are stale
    int parity = 0;          // use_slot of the chain's next step
    int steps_queued = 0, max_steps = 0;
    bool eval_first = false, eval_only = false;
    int begin_block = 0;
    int pend_slot = -1;      // the last step left its record beside pt[pend_slot] ...
    int64_t pend_idx = 0;    // ... for the next launch's service workgroup to pass on
    std::deque<Step> fifo;
  };
  std::vector<Run> runs((size_t)n);
  long n_launches = 0, n_records = 0, n_stale = 0;

  auto stage_begin = [&](int j, bool eval_first, bool eval_only) {
    // hand chain j's next transition to the device: begin_draw() has been called (momentum and directions drawn)
    Run& r = runs[(size_t)j];
    abd_sampler::DChain& d = s->dc[(size_t)j];
    const abdnuts::Nuts& nu = s->ch[(size_t)j].nuts;
    r.begin_block = (int)(d.n_begin++ % abd_sampler::kBeginBlocks);
    TrainBegin& b = d.begin.host()[r.begin_block];
    std::memcpy(b.q0, nu.q, sizeof b.q0);
    std::memcpy(b.p0, nu.p0_pending, sizeof b.p0);
    std::memcpy(b.g0, nu.g, sizeof b.g0);
    std::memcpy(b.inv_mass, nu.inv_mass, sizeof b.inv_mass);
    b.eps = nu.eps;
    b.dirs = nu.dir_bits;
    b.max_depth = eval_only ? 0 : nu.max_depth;
    b.eval_first = eval_first ? 1 : 0;
    __atomic_thread_fence(__ATOMIC_RELEASE);
    r.eval_first = eval_first;
    r.eval_only = eval_only;
    r.state = NEED_BEGIN;
  };
  // outputs of iteration r.k of chain j (point and discrete state are final) and its draw's device work, on the chain's own
  // stream; then the next transition
  auto iteration_done = [&](int j, bool with_counts) -> int {
    Run& r = runs[(size_t)j];
    abd_sampler::DChain& d = s->dc[(size_t)j];
    write_draw(f, j, r.k, with_counts ? d.done.host() : nullptr);
    if (int rc = queue_draw(f, j, r.k, d.side)) return rc;
    if (++r.k == n_iter) r.state = DONE;
    return ABD_OK;
  };
  // chain j's tree has ended (the NUTS state machine holds the new point): adaptation, then the sweep or the next transition
  auto transition_end = [&](int j) -> int {
    Run& r = runs[(size_t)j];
    abd_sampler::DChain& d = s->dc[(size_t)j];
    // steps still queued for the chain belong to a tree that is over: they run and may overlap its sweep, which is harmless
    // only because their records are never read
    r.epoch += 1;
    s->ch[(size_t)j].end_transition();
    if (s->o.gibbs) {
      const int32_t id = s->chains[(size_t)j];
      if (int rc = queue_sweep(s, j, 1, &id, s->ch[(size_t)j].nuts.q, r.k, d.side)) return rc;
      d.sweep_tag += 1.0;
      hipLaunchKernelGGL(abd_sweep_done_kernel, dim3(1), dim3(64), 0, d.side, c->d_counts_chain + 2 * (size_t)j, d.done.dev(),
                         reinterpret_cast<double*>(d.done.dev() + 2), d.sweep_tag);
      HIP_TRY(hipGetLastError());
      r.state = SWEEP;
      return ABD_OK;
    }
    if (int rc = iteration_done(j, false)) return rc;
    if (r.state != DONE) {
      s->ch[(size_t)j].begin();  // (logp and gradient at the new point are the proposal's)
      stage_begin(j, false, false);
    }
    return ABD_OK;
  };

  for (int j = 0; j < n && n_iter > 0; ++j) {
    s->ch[(size_t)j].begin();
    stage_begin(j, false, false);  // logp and gradient at the chain's point are known (abd_sampler_create, or the run before)
  }

  int rc_loop = ABD_OK;
  for (long spins = 0; rc_loop == ABD_OK;) {
    bool any = false, progressed = false;
    for (int u = 0; u < n_units && rc_loop == ABD_OK; ++u) {
      const int lo = u * B, hi = std::min(n, lo + B);
      // ---- take the records that have landed ----
      for (int j = lo; j < hi && rc_loop == ABD_OK; ++j) {
        Run& r = runs[(size_t)j];
        abd_sampler::DChain& d = s->dc[(size_t)j];
        abdnuts::Nuts& nu = s->ch[(size_t)j].nuts;
        while (!r.fifo.empty() && rc_loop == ABD_OK) {
          const Step e = r.fifo.front();
          if (e.epoch != r.epoch) {  // a step the device took beyond the end of its tree
            r.fifo.pop_front();
            ++n_stale;
            continue;
          }
          const TrainRecord& tr = d.ring.host()[e.idx % ABD_TRAIN_RING];
          if (*(volatile const double*)&tr.tag != (double)(e.idx + 1)) break;
          __atomic_thread_fence(__ATOMIC_ACQUIRE);
          r.fifo.pop_front();
          progressed = true;
          ++n_records;
          if (e.eval0) {
            // logp and gradient at the start point under the new discrete state: the iteration the sweep closed is complete
            nu.set_point(tr.lp, tr.g);
            if ((rc_loop = iteration_done(j, true)) != ABD_OK) break;
            if (r.state == DONE) break;  // (the evaluation was all this BEGIN asked for)
            nu.begin_finish();
            nu.adopt_request(tr.next_theta, tr.next_p_half);
          } else {
            nu.feed(tr.lp, tr.g, tr.next_theta, tr.next_p_half, true);
            if (!nu.active) rc_loop = transition_end(j);
          }
        }
      }
      if (rc_loop != ABD_OK) break;
      // ---- sweeps that have finished: the next transition starts with an evaluation at the new state ----
      for (int j = lo; j < hi; ++j) {
        Run& r = runs[(size_t)j];
        if (r.state != SWEEP) continue;
        const abd_sampler::DChain& dj = s->dc[(size_t)j];
        if (*reinterpret_cast<volatile const double*>(dj.done.host() + 2) != dj.sweep_tag) continue;
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        progressed = true;
        const bool last = r.k + 1 == n_iter;
        if (!last) s->ch[(size_t)j].begin_draw();
        stage_begin(j, true, last);
      }
      if (rc_loop != ABD_OK) break;
      // ---- keep the unit's launches queued ahead ----
      for (;;) {
        size_t out = 0;
        bool any_begin = false, any_step = false;
        for (int j = lo; j < hi; ++j) {
          const Run& r = runs[(size_t)j];
          out = std::max(out, r.fifo.size());
          any_begin |= r.state == NEED_BEGIN;
          any_step |= r.state == TREE && r.steps_queued < r.max_steps;
        }
        if (!any_begin && !(any_step && out < (size_t)s->dtrain_lookahead)) break;
        const bool step_now = out < (size_t)s->dtrain_lookahead;
        DenseTrainArgs a;
        std::memset(&a, 0, sizeof a);
        for (int k = 0; k < ABD_TRAIN_CB; ++k) a.tc[k].fwd_slot = -1;  // (a unit may have fewer chains than its shape: those slots stay SKIP)
        for (int j = lo; j < hi; ++j) {
          Run& r = runs[(size_t)j];
          abd_sampler::DChain& d = s->dc[(size_t)j];
          const ChainSlot& slot = c->slots[(size_t)s->chains[(size_t)j]];
          TrainChainArgs& tc = a.tc[j - lo];
          tc.st = d.st;
          tc.ring = d.ring.dev();
          tc.begin = d.begin.dev();
          tc.iw = slot.iw;
          tc.pl = slot.pl;
          tc.cnt = slot.cnt;
          tc.waner = slot.waner;
          tc.action = ABD_TR_SKIP;
          tc.fwd_slot = -1;
          if (r.state == NEED_BEGIN) {
            tc.action = ABD_TR_BEGIN;
            tc.begin = d.begin.dev() + r.begin_block;
            r.state = TREE;
            r.parity = 0;
            r.steps_queued = 0;
            r.max_steps = (r.eval_first ? 1 : 0) + (r.eval_only ? 0 : s->ch[(size_t)j].nuts.max_leaves());
            r.pend_slot = -1;  // (a record left there belongs to steps beyond the end of the last tree)
          } else if (r.state == TREE && r.steps_queued < r.max_steps && step_now) {
            tc.action = ABD_TR_STEP;
            tc.use_slot = r.parity;
            tc.rec_idx = d.n_rec++;
            tc.own = r.steps_queued + 1 == r.max_steps ? 1 : 0;  // nothing can follow the tree's last possible leaf
            if (r.pend_slot >= 0) {
              tc.fwd_slot = r.pend_slot;
              tc.fwd_idx = r.pend_idx;
            }
            r.pend_slot = tc.own ? -1 : (r.parity ^ 1);
            r.pend_idx = tc.rec_idx;
            r.fifo.push_back(Step{tc.rec_idx, r.epoch, r.eval_first && r.steps_queued == 0});
            r.parity ^= 1;
            r.steps_queued += 1;
          } else if (r.pend_slot >= 0) {
            tc.fwd_slot = r.pend_slot;  // the chain sits this launch out; its last record still goes to the host
            tc.fwd_idx = r.pend_idx;
            r.pend_slot = -1;
          }
        }
        if ((rc_loop = enqueue_dense_train(c, unit_pipe(c, u), B, s->dtrain_blocks, &a)) != ABD_OK) break;
        ++n_launches;
        progressed = true;
      }
      for (int j = lo; j < hi; ++j) any |= runs[(size_t)j].state != DONE;
    }
    if (rc_loop != ABD_OK || !any) break;
    if (progressed) {
      spins = 0;
    } else if (++spins > 40000000) {
      // nothing has moved for seconds: a record that never got its tag
      __atomic_fetch_add(&c->wait_fallbacks, (int64_t)1, __ATOMIC_RELAXED);
      (void)hipDeviceSynchronize();
      rc_loop = fail(ABD_ERR_STATE, "the native sampler's leapfrog trains stalled: a record never received its tag");
    } else {
      __builtin_ia32_pause();
    }
  }
  // what the device still has queued beyond the ends of the last trees must be through before anybody reuses the chains' state
  for (int u = 0; u < n_units; ++u) (void)hipStreamSynchronize(c->pipe[unit_pipe(c, u)].st);
  for (int j = 0; j < n; ++j) (void)hipStreamSynchronize(s->dc[(size_t)j].side);
  if (rc_loop != ABD_OK) return rc_loop;
  if (f.profile) {
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - f.t_begin).count();
    std::fprintf(stderr, "abd sampler (trains): %d units of %d chains, %ld launches, %ld records (%ld stale steps) in %.3f s; %.2f us inside the "
                 "launch call per launch\n", n_units, B, n_launches, n_records, n_stale, wall,
                 g_launch_profile.evals ? 1e6 * g_launch_profile.eval_s / g_launch_profile.evals : 0.0);
  }
  return ABD_OK;
}

}  // namespace

extern "C" {

int abd_sampler_run_record(abd_sampler* s, int64_t n_iter, double* theta, double* stats, const abd_record* rec) {
  if (!s) return fail(ABD_ERR_ARG, "sampler is NULL");
  if (n_iter < 0) return fail(ABD_ERR_ARG, "n_iter=%lld is negative", (long long)n_iter);
  abd_ctx* c = s->c;
  const int n = s->n;
  // (before anything is launched or marked as run)
  const int64_t upto = s->it + n_iter - s->o.tune;
  const struct { const char* what; bool on; int64_t planned; } summaries[5] = {
      {"loo: draws up to %lld pass the planned %lld", s->loo.on(), s->loo.planned()},
      {"curves: draws up to %lld do not fit capacity %lld", s->curves.on(), s->curves.planned()},
      {"diagnostics: draws up to %lld pass the planned %lld", s->diag.on(), s->diag.planned()},
      {"risk: draws up to %lld do not fit capacity %lld", s->risk.on(), s->risk.planned()},
      {"timelines: draws up to %lld pass the planned %lld", s->timelines.on(), s->timelines.planned()}};
  for (const auto& x : summaries)
    if (x.on && upto > x.planned) return fail(ABD_ERR_STATE, x.what, (long long)upto, (long long)x.planned);
  const bool with_ll = rec && (rec->ll_s || rec->ll_n);
  const bool with_yrep = rec && (rec->yrep_s || rec->yrep_n);
  const bool recording = rec && (rec->i_raw || rec->ab_s_waner || rec->i || rec->ab_n_mu || rec->ab_s_mu || with_ll || with_yrep);
  s->ran = true;
  if (recording) {
    if (rec->thin < 0) return fail(ABD_ERR_ARG, "record: thin=%lld is negative", (long long)rec->thin);
    const int64_t thin = std::max<int64_t>(1, rec->thin), n_rec = (n_iter + thin - 1) / thin;  // iterations 0, thin, 2 thin, ... of the call
    if (rec->first < 0 || rec->first + n_rec > rec->capacity)
      return fail(ABD_ERR_ARG, "record: draws [%lld, %lld) do not fit capacity %lld", (long long)rec->first,
                  (long long)(rec->first + n_rec), (long long)rec->capacity);
    if (int rc = alloc_record_staging(s, with_ll, with_yrep)) return rc;
  }
  RunFrame f{s, n_iter, theta, stats, recording ? rec : nullptr, recording ? std::max<int64_t>(1, rec->thin) : 1, {}, false, {}};
  f.staging.resize((size_t)n);
  for (auto& sg : f.staging) sg.flushed_to = recording ? rec->first : 0;
  HIP_TRY(hipSetDevice(c->device));
  if (int rc = flush_ring(c)) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));  // whatever the caller queued on the context's stream comes first
  f.profile = arm_profile(s->dtrains || unit_threads(s) == 1);
  f.t_begin = std::chrono::steady_clock::now();
  const int rc = s->dtrains ? sampler_run_trains(f) : sampler_run_units(f);
  g_launch_profile.on = false;
  if (rc) return rc;
  // the context's stream continues behind everything the run queued
  for (int pi = 1; pi < c->n_streams; ++pi) c->pipe[pi].busy = true;
  if (int rc = join_pipes(c)) return rc;
  const int64_t first_draw = std::max<int64_t>(s->it, s->o.tune);
  if (s->d_sums && s->it + n_iter > first_draw) s->n_accumulated += s->it + n_iter - first_draw;
  s->it += n_iter;
  return ABD_OK;
}

int abd_sampler_launch_shape(abd_sampler* s, int32_t out[4]) {
  if (!s || !out) return fail(ABD_ERR_ARG, "NULL argument");
  const abd_ctx* c = s->c;
  out[0] = s->unit;
  out[1] = s->dtrains ? ABD_TRAINS_DENSE : (s->trains ? ABD_TRAINS_LISTS : ABD_TRAINS_NONE);
  out[2] = s->dtrains ? dense_train_ranges(c, s->dtrain_blocks) : eval_grid(c, s->trains ? Caller::Train : Caller::Unit, s->unit);
  out[3] = s->dtrains ? 1 : unit_threads(s);
  return ABD_OK;
}

}  // extern "C"
