// Test harness (CPU only): drives the NUTS state machine of abdpymc_amd/csrc/abd_nuts.hpp against an
// independent-normal target whose moments are known in closed form.  Built by tests/test_nuts_native.py with g++.
#include "abd_nuts.hpp"

namespace {
// the leapfrog log of a harness run (abd_nuts.hpp: LeapfrogLog): chain c's rows go to rows[c][capacity][LOG_COLS], the rows it
// produced -- kept or not -- to n_total[c]; capacity < 0: no log is attached
struct LogOut {
  long long capacity = -1;
  double* rows = nullptr;
  long long* n_total = nullptr;
  void take(int c, const abdnuts::LeapfrogLog& log) const {
    if (capacity < 0) return;
    if (log.stored()) std::memcpy(rows + (size_t)c * capacity * abdnuts::LOG_COLS, log.rows.data(), (size_t)log.stored() * abdnuts::LOG_COLS * sizeof(double));
    n_total[c] = log.n_total;
  }
};

// target: independent normals (prec == NULL: mean, sd) or a correlated normal with precision matrix prec (17 x 17)
// eval_first: every transition starts with an evaluation of its start point (set_point), as a host-driven unit does after a sweep
int run_classic(const double* mean, const double* sd, const double* prec, long long tune, long long draws, unsigned long long seed,
                int n_chains, int dense, int eval_first, const LogOut& lo, double* out_q, double* out_stats) {
  using namespace abdnuts;
  auto eval = [&](const double* q, double* g) {
    double lp = 0;
    if (prec) {
      for (int r = 0; r < D; ++r) {
        double s = 0;
        for (int c = 0; c < D; ++c) s += prec[r * D + c] * (q[c] - mean[c]);
        g[r] = -s;
        lp -= 0.5 * s * (q[r] - mean[r]);
      }
      return lp;
    }
    for (int d = 0; d < D; ++d) {
      const double z = (q[d] - mean[d]) / sd[d];
      lp -= 0.5 * z * z;
      g[d] = -z / sd[d];
    }
    return lp;
  };
  // chains advance in lock step, one pending evaluation each, the way the device driver batches them
  AdaptiveNuts* ch = new AdaptiveNuts[n_chains];
  std::vector<LeapfrogLog> logs((size_t)n_chains, LeapfrogLog(lo.capacity < 0 ? 0 : lo.capacity));
  for (int c = 0; c < n_chains; ++c) {
    double q0[D], g0[D];
    for (int d = 0; d < D; ++d) q0[d] = mean[d] + sd[d] * (c % 2 ? 1.5 : -1.5);
    const double lp0 = eval(q0, g0);
    ch[c].init(q0, lp0, g0, seed, (unsigned long long)c, tune, 10, 0.8, dense != 0);
    if (lo.capacity >= 0) ch[c].nuts.attach_log(&logs[(size_t)c]);
  }
  for (long long it = 0; it < tune + draws; ++it) {
    for (int c = 0; c < n_chains; ++c) {
      if (eval_first) {
        double g[D];
        const double lp = eval(ch[c].nuts.q, g);
        ch[c].nuts.set_point(lp, g);
      }
      ch[c].begin();
    }
    bool any = true;
    while (any) {
      any = false;
      for (int c = 0; c < n_chains; ++c) {
        if (!ch[c].nuts.active) continue;
        any = true;
        double g[D];
        const double lp = eval(ch[c].nuts.request(), g);
        ch[c].nuts.feed(lp, g);
      }
    }
    for (int c = 0; c < n_chains; ++c) {
      ch[c].end_transition();
      if (it >= tune) {
        const long long k = it - tune;
        double* q = out_q + ((size_t)c * draws + k) * D;
        for (int d = 0; d < D; ++d) q[d] = ch[c].nuts.q[d];
        double* s = out_stats + ((size_t)c * draws + k) * 6;
        s[0] = ch[c].nuts.stats.lp;
        s[1] = ch[c].nuts.stats.tree_depth;
        s[2] = ch[c].nuts.stats.n_steps;
        s[3] = ch[c].nuts.stats.mean_tree_accept;
        s[4] = ch[c].nuts.stats.step_size;
        s[5] = ch[c].nuts.stats.diverging ? 1.0 : 0.0;
      }
    }
  }
  for (int c = 0; c < n_chains; ++c) lo.take(c, logs[(size_t)c]);
  delete[] ch;
  return 0;
}
}  // namespace

extern "C" int nuts_harness_run(const double* mean, const double* sd, const double* prec, long long tune, long long draws,
                                unsigned long long seed, int n_chains, int dense, double* out_q, double* out_stats) {
  return run_classic(mean, sd, prec, tune, draws, seed, n_chains, dense, 0, LogOut(), out_q, out_stats);
}

// ---- the leapfrog-train protocol (abd_train.hpp <-> abd_sampler.hip: sampler_run_trains), with the DEVICE's part restated on
// the CPU: a per-chain state machine that holds both ends of the tree and the pre-drawn doubling directions, takes one leapfrog
// per step -- across the halves of a doubling and across doublings -- and leaves a record (logp, gradient, next point) for the
// host, whose tree logic follows behind on the records (Nuts::feed(..., across_halves = true)).  Same draws, bit for bit, as
// the classic request / feed loop above: the arithmetic is stage_leapfrog's, operation by operation.
namespace {
struct DeviceChain {  // abd_types.hpp: TrainChain (+ the pending point of its slot)
  double end_q[2][abdnuts::D], end_p[2][abdnuts::D], end_g[2][abdnuts::D], inv_mass[abdnuts::D], eps = 0;
  unsigned dirs = 0;
  int max_depth = 0, phase = 0 /* 0 idle, 1 eval0, 2 leaf */, depth = 0, n_leaf = 0, n_target = 1, dir = 1;
  double pt_q[abdnuts::D], pt_ph[abdnuts::D];
};
struct DeviceRecord {
  double lp, g[abdnuts::D], next_q[abdnuts::D], next_ph[abdnuts::D];
};
void dev_stage(const double* q, const double* p, const double* g, double ve, const double* im, double* t2, double* ph) {
  for (int d = 0; d < abdnuts::D; ++d) {
    ph[d] = p[d] + (0.5 * ve) * g[d];    // train_stage: p_half = cur.p + 0.5 ve cur.g
    t2[d] = q[d] + ve * (im[d] * ph[d]);  //              req_q  = cur.q + ve (M^-1 p_half)
  }
}
// abd_train.hpp: train_step, action BEGIN
void dev_begin(DeviceChain& st, const double* q0, const double* p0, const double* g0, const double* inv_mass, double eps, unsigned dirs,
               int max_depth, bool eval_first) {
  using abdnuts::D;
  std::memcpy(st.inv_mass, inv_mass, sizeof(st.inv_mass));
  st.eps = eps;
  st.dirs = dirs;
  st.max_depth = max_depth;
  st.depth = 0;
  st.n_leaf = 0;
  st.n_target = 1;
  st.dir = 1;
  st.phase = 0;
  if (eval_first) {
    std::memcpy(st.pt_q, q0, sizeof(st.pt_q));
    std::memcpy(st.pt_ph, p0, sizeof(st.pt_ph));
    st.phase = 1;
    return;
  }
  for (int e = 0; e < 2; ++e) {
    std::memcpy(st.end_q[e], q0, sizeof(double) * D);
    std::memcpy(st.end_p[e], p0, sizeof(double) * D);
    std::memcpy(st.end_g[e], g0, sizeof(double) * D);
  }
  if (max_depth > 0) {
    st.dir = dirs & 1u ? 1 : -1;
    dev_stage(q0, p0, g0, (double)st.dir * eps, st.inv_mass, st.pt_q, st.pt_ph);
    st.phase = 2;
  }
}
// abd_train.hpp: train_step, a step (lp, g: the target at the pending point); false when the chain was idle
bool dev_step(DeviceChain& st, double lp, const double* g, DeviceRecord& rec) {
  using abdnuts::D;
  if (st.phase == 0) return false;
  const bool finite = std::isfinite(lp);
  double gd[D], tk[D], t2[D], ph[D];
  for (int d = 0; d < D; ++d) {
    gd[d] = finite ? g[d] : 0.0;
    tk[d] = st.pt_q[d];
    t2[d] = ph[d] = 0.0;
  }
  bool have_next = false;
  if (st.phase == 1) {
    for (int e = 0; e < 2; ++e) {
      std::memcpy(st.end_q[e], tk, sizeof tk);
      std::memcpy(st.end_p[e], st.pt_ph, sizeof tk);
      std::memcpy(st.end_g[e], gd, sizeof tk);
    }
    st.phase = 0;
    if (st.max_depth > 0) {
      st.dir = st.dirs & 1u ? 1 : -1;
      dev_stage(tk, st.pt_ph, gd, (double)st.dir * st.eps, st.inv_mass, t2, ph);
      have_next = true;
      st.phase = 2;
      st.depth = 0;
      st.n_leaf = 0;
      st.n_target = 1;
    }
  } else {
    const double ve = (double)st.dir * st.eps;
    double p[D], kick[D];
    for (int d = 0; d < D; ++d) {
      kick[d] = (0.5 * ve) * gd[d];
      p[d] = st.pt_ph[d] + kick[d];  // feed: cur.p = p_half + 0.5 ve g
    }
    if (st.n_leaf + 1 == st.n_target) {
      const int e = st.dir > 0 ? 1 : 0;
      std::memcpy(st.end_q[e], tk, sizeof tk);
      std::memcpy(st.end_p[e], p, sizeof tk);
      std::memcpy(st.end_g[e], gd, sizeof tk);
      st.depth += 1;
      st.phase = 0;
      if (st.depth < st.max_depth) {
        st.dir = (st.dirs >> st.depth) & 1u ? 1 : -1;
        const int o = st.dir > 0 ? 1 : 0;
        dev_stage(st.end_q[o], st.end_p[o], st.end_g[o], (double)st.dir * st.eps, st.inv_mass, t2, ph);
        have_next = true;
        st.phase = 2;
        st.n_leaf = 0;
        st.n_target = 1 << st.depth;
      }
    } else {
      for (int d = 0; d < D; ++d) {
        ph[d] = p[d] + kick[d];
        t2[d] = tk[d] + ve * (st.inv_mass[d] * ph[d]);
      }
      have_next = true;
      st.n_leaf += 1;
    }
  }
  rec.lp = lp;
  std::memcpy(rec.g, g, sizeof rec.g);
  std::memcpy(rec.next_q, t2, sizeof t2);
  std::memcpy(rec.next_ph, ph, sizeof ph);
  if (have_next) {
    std::memcpy(st.pt_q, t2, sizeof t2);
    std::memcpy(st.pt_ph, ph, sizeof ph);
  }
  return true;
}
}  // namespace

// independent normals, diagonal metric; eval_first: every transition starts with an evaluation of its start point (what the
// compound step does after a sweep: begin_draw / set_point / begin_finish / adopt_request); run_on: steps the device takes
// beyond the end of a tree before the host stops it (the look-ahead: never looked at)
namespace {
int run_trains(const double* mean, const double* sd, long long tune, long long draws, unsigned long long seed, int n_chains, int eval_first,
               int run_on, const LogOut& lo, double* out_q, double* out_stats) {
  using namespace abdnuts;
  auto eval = [&](const double* q, double* g) {
    double lp = 0;
    for (int d = 0; d < D; ++d) {
      const double z = (q[d] - mean[d]) / sd[d];
      lp -= 0.5 * z * z;
      g[d] = -z / sd[d];
    }
    return lp;
  };
  for (int c = 0; c < n_chains; ++c) {
    AdaptiveNuts ch;
    DeviceChain dev;
    double q0[D], g0[D];
    for (int d = 0; d < D; ++d) q0[d] = mean[d] + sd[d] * (c % 2 ? 1.5 : -1.5);
    ch.init(q0, eval(q0, g0), g0, seed, (unsigned long long)c, tune, 10, 0.8, false);
    LeapfrogLog log(lo.capacity < 0 ? 0 : lo.capacity);
    if (lo.capacity >= 0) ch.nuts.attach_log(&log);
    for (long long it = 0; it < tune + draws; ++it) {
      Nuts& nu = ch.nuts;
      DeviceRecord rec;
      double g[D];
      if (eval_first) {
        ch.begin_draw();
        dev_begin(dev, nu.q, nu.p0_pending, nu.g, nu.inv_mass, nu.eps, nu.dir_bits, nu.max_depth, true);
        const double lp = eval(dev.pt_q, g);
        if (!dev_step(dev, lp, g, rec)) return 2;
        nu.set_point(rec.lp, rec.g);
        nu.begin_finish();
        nu.adopt_request(rec.next_q, rec.next_ph);
      } else {
        ch.begin();
        dev_begin(dev, nu.q, nu.p0_pending, nu.g, nu.inv_mass, nu.eps, nu.dir_bits, nu.max_depth, false);
      }
      int steps = 0;
      while (nu.active) {
        if (std::memcmp(dev.pt_q, nu.request(), sizeof(double) * D) != 0) return 3;  // the device evaluates what the host asks for
        const double lp = eval(dev.pt_q, g);
        if (!dev_step(dev, lp, g, rec)) return 4;  // the device must not run out of steps before the host's tree ends
        nu.feed(rec.lp, rec.g, rec.next_q, rec.next_ph, true);
        if (++steps > nu.max_leaves()) return 5;
      }
      for (int k = 0; k < run_on; ++k) {  // what is queued behind the end of the tree
        const double lp = eval(dev.pt_q, g);
        if (!dev_step(dev, lp, g, rec)) break;
      }
      ch.end_transition();
      if (it >= tune) {
        const long long k = it - tune;
        double* q = out_q + ((size_t)c * draws + k) * D;
        for (int d = 0; d < D; ++d) q[d] = nu.q[d];
        double* s = out_stats + ((size_t)c * draws + k) * 6;
        s[0] = nu.stats.lp;
        s[1] = nu.stats.tree_depth;
        s[2] = nu.stats.n_steps;
        s[3] = nu.stats.mean_tree_accept;
        s[4] = nu.stats.step_size;
        s[5] = nu.stats.diverging ? 1.0 : 0.0;
      }
    }
    lo.take(c, log);
  }
  return 0;
}
}  // namespace

extern "C" int nuts_harness_run_trains(const double* mean, const double* sd, long long tune, long long draws, unsigned long long seed,
                                       int n_chains, int eval_first, int run_on, double* out_q, double* out_stats) {
  return run_trains(mean, sd, tune, draws, seed, n_chains, eval_first, run_on, LogOut(), out_q, out_stats);
}

// Either driver with the leapfrog log on (trains = 0: the classic loop, run_on ignored; capacity < 0: no log is attached):
// rows [n_chains][capacity][abdnuts::LOG_COLS], n_total [n_chains].  Independent normals, diagonal metric.
extern "C" int nuts_harness_run_logged(const double* mean, const double* sd, long long tune, long long draws, unsigned long long seed,
                                       int n_chains, int trains, int eval_first, int run_on, long long capacity, double* rows,
                                       long long* n_total, double* out_q, double* out_stats) {
  LogOut lo;
  lo.capacity = capacity;
  lo.rows = rows;
  lo.n_total = n_total;
  return trains ? run_trains(mean, sd, tune, draws, seed, n_chains, eval_first, run_on, lo, out_q, out_stats)
                : run_classic(mean, sd, nullptr, tune, draws, seed, n_chains, 0, eval_first, lo, out_q, out_stats);
}

// ---- the classic loop with everything a replay of its transitions needs (tests/test_nuts_replay_cpu.py): either target, either
// metric, eval_first, a tree depth of the caller's choice, and installations as abd_sampler_set_adaptation makes them
// (AdaptiveNuts::install, between two transitions).  inst: n_inst rows of INST_COLS doubles -- the iteration before whose
// transition the values are installed, the chain, whether a metric is given, the step size (<= 0: kept), the 17 entries of the
// metric; an installation on a chain that runs a dense metric is refused as the library refuses it (counted in the result, which
// is otherwise 0).  For ALL tune + draws iterations: out_q [C][T][17]; out_stats [C][T][8] -- lp, tree_depth, n_steps,
// mean_tree_accept, step_size, diverging, energy, max_energy_error; and what the chain holds once the iteration has ended (what
// abd_sampler_adaptation reads then): out_eps [C][T], out_inv_mass [C][T][17], out_metric [C][T][17][17] (the diagonal matrix
// while the metric is diagonal).  The leapfrog log as in nuts_harness_run_logged.
enum { INST_COLS = 4 + abdnuts::D };
extern "C" int nuts_harness_run_adapt(const double* mean, const double* sd, const double* prec, long long tune, long long draws,
                                      unsigned long long seed, int n_chains, int dense, int eval_first, int max_depth, int n_inst,
                                      const double* inst, long long capacity, double* rows, long long* n_total, double* out_q,
                                      double* out_stats, double* out_eps, double* out_inv_mass, double* out_metric) {
  using namespace abdnuts;
  LogOut lo;
  lo.capacity = capacity;
  lo.rows = rows;
  lo.n_total = n_total;
  auto eval = [&](const double* q, double* g) {
    double lp = 0;
    if (prec) {
      for (int r = 0; r < D; ++r) {
        double s = 0;
        for (int c = 0; c < D; ++c) s += prec[r * D + c] * (q[c] - mean[c]);
        g[r] = -s;
        lp -= 0.5 * s * (q[r] - mean[r]);
      }
      return lp;
    }
    for (int d = 0; d < D; ++d) {
      const double z = (q[d] - mean[d]) / sd[d];
      lp -= 0.5 * z * z;
      g[d] = -z / sd[d];
    }
    return lp;
  };
  const long long T = tune + draws;
  int refused = 0;
  std::vector<AdaptiveNuts> ch((size_t)n_chains);
  std::vector<LeapfrogLog> logs((size_t)n_chains, LeapfrogLog(capacity < 0 ? 0 : capacity));
  for (int c = 0; c < n_chains; ++c) {
    double q0[D], g0[D];
    for (int d = 0; d < D; ++d) q0[d] = mean[d] + sd[d] * (c % 2 ? 1.5 : -1.5);
    const double lp0 = eval(q0, g0);
    ch[(size_t)c].init(q0, lp0, g0, seed, (unsigned long long)c, tune, max_depth, 0.8, dense != 0);
    if (capacity >= 0) ch[(size_t)c].nuts.attach_log(&logs[(size_t)c]);
  }
  for (long long it = 0; it < T; ++it) {
    for (int i = 0; i < n_inst; ++i) {
      const double* r = inst + (size_t)i * INST_COLS;
      if ((long long)r[0] != it) continue;
      AdaptiveNuts& a = ch[(size_t)r[1]];
      if (a.nuts.dense) {
        refused += 1;
        continue;
      }
      a.install(r[2] != 0.0 ? r + 4 : nullptr, r[3]);
    }
    for (int c = 0; c < n_chains; ++c) {
      AdaptiveNuts& a = ch[(size_t)c];
      if (eval_first) {
        double g[D];
        const double lp = eval(a.nuts.q, g);
        a.nuts.set_point(lp, g);
      }
      a.begin();
      while (a.nuts.active) {
        double g[D];
        const double lp = eval(a.nuts.request(), g);
        a.nuts.feed(lp, g);
      }
      a.end_transition();
      const size_t row = (size_t)c * T + it;
      const Nuts& nu = a.nuts;
      for (int d = 0; d < D; ++d) out_q[row * D + d] = nu.q[d];
      double* s = out_stats + row * 8;
      s[0] = nu.stats.lp;
      s[1] = nu.stats.tree_depth;
      s[2] = nu.stats.n_steps;
      s[3] = nu.stats.mean_tree_accept;
      s[4] = nu.stats.step_size;
      s[5] = nu.stats.diverging ? 1.0 : 0.0;
      s[6] = nu.stats.energy;
      s[7] = nu.stats.max_energy_error;
      out_eps[row] = nu.eps;
      for (int d = 0; d < D; ++d) out_inv_mass[row * D + d] = nu.inv_mass[d];
      for (int r = 0; r < D; ++r)
        for (int k = 0; k < D; ++k) out_metric[(row * D + r) * D + k] = nu.dense ? nu.cov[r][k] : (r == k ? nu.inv_mass[r] : 0.0);
    }
  }
  for (int c = 0; c < n_chains; ++c) lo.take(c, logs[(size_t)c]);
  return refused;
}
