// abd_sampler.hpp -- the native sampler as its two translation units see it: abd_sampler.hip (creation and the two run loops) and
// abd_sampler_summaries.hip (what a caller switches on before the first run and reads after one).  Not part of the C ABI.
#pragma once

#include "abd_host.hpp"
#include "abd_nuts.hpp"

// The per-draw summaries of a sampler (abd_sampler_enable_*): each is its device buffers, what it was enabled with and the
// layout of the buffers -- stated once, as the offset of chain j's part (j = n: the buffer's length), for the enable function,
// the launch and the read-out alike.  planned(): the draws it was sized for; launch(): draw d = iteration - tune of sampler
// chain j (slot `chain`, point q) on stream st.
struct CurvesSummary {  // abd_curves.hpp: every draw's row, and every chain's own slab rows (the chains' launches run side by side)
  DevBuf<unsigned long long> rows, scratch;
  int64_t capacity = 0;
  double thr_s = 0.0, thr_n = 0.0;
  bool on() const { return rows != nullptr; }
  int64_t planned() const { return capacity; }
  size_t row_at(const abd_ctx* c, int j, int64_t d) const { return ((size_t)j * capacity + (size_t)d) * abdi::curves_row_cols(c); }
  size_t scratch_at(const abd_ctx* c, int j) const { return (size_t)j * abdi::curves_scratch_cols(c); }
  int launch(abd_ctx* c, int j, int chain, const double* q, int64_t d, hipStream_t st) const {
    return abdi::launch_curves(c, chain, q, thr_s, thr_n, st, scratch + scratch_at(c, j), rows + row_at(c, j, d));
  }
};

struct RiskSummary {  // abd_risk.hpp: every draw's table of 32 G 32-bit counts, and every chain's own packed slab rows
  DevBuf<uint32_t> tables;
  DevBuf<unsigned long long> scratch;
  int64_t capacity = 0;
  abd_risk_spec spec = {};
  bool on() const { return tables != nullptr; }
  int64_t planned() const { return capacity; }
  size_t table_at(const abd_ctx* c, int j, int64_t d) const { return ((size_t)j * capacity + (size_t)d) * abdi::risk_table_cols(c); }
  size_t scratch_at(const abd_ctx* c, int j) const { return (size_t)j * abdi::risk_scratch_cols(c); }
  int launch(abd_ctx* c, int j, int chain, const double* q, int64_t d, hipStream_t st) const {
    return abdi::launch_risk(c, chain, q, spec, st, scratch + scratch_at(c, j), tables + table_at(c, j, d));
  }
};

// abd_diag.hpp: convergence accumulators over all draws, individual-major planes per chain -- [n][2][7][G*N] of the two titers
// (ab_n_mu, then ab_s_mu), [n][G*N][4] and [n][G*N] of i -- and one plane [G*N] of staging for the read-out
struct DiagSummary {
  DevBuf<double> tit;
  DevBuf<uint32_t> inf;
  DevBuf<unsigned long long> cb2, stage;
  int64_t draws = 0, H = 0, L = 0;  // planned draws D, H = D / 2, batch length
  bool on() const { return tit != nullptr; }
  int64_t planned() const { return draws; }
  static size_t cells(const abd_ctx* c) { return (size_t)c->G * c->N; }
  size_t tit_at(const abd_ctx* c, int j, int titer = 0, int plane = 0) const { return (((size_t)j * 2 + titer) * 7 + plane) * cells(c); }
  size_t inf_at(const abd_ctx* c, int j) const { return (size_t)j * 4 * cells(c); }
  size_t cb2_at(const abd_ctx* c, int j) const { return (size_t)j * cells(c); }
  int launch(abd_ctx* c, int j, int chain, const double* q, int64_t d, hipStream_t st) const {
    if (d >= 2 * H) return ABD_OK;  // (an odd D: the last draw belongs to neither half)
    return abdi::launch_diag(c, chain, q, st, d, H, L, tit + tit_at(c, j), inf + inf_at(c, j), cb2 + cb2_at(c, j));
  }
};

// abd_timeline.hpp: per-individual timelines over all draws, individual-major planes per chain -- [n][2][G*N][32] words of the
// two titers' histograms (ab_n_mu, then ab_s_mu), [n][G*N][2] inf and cum, [n][N][8] ninf -- and the read-out's staging
struct TimelineSummary {
  DevBuf<uint32_t> hist, cell, ninf;
  DevBuf<unsigned long long> stage;
  size_t stage_bytes = 0;
  int64_t draws = 0;  // planned draws
  double range_n[2] = {0.0, 0.0}, range_s[2] = {0.0, 0.0};
  bool on() const { return hist != nullptr; }
  int64_t planned() const { return draws; }
  size_t hist_at(const abd_ctx* c, int j, int titer = 0) const { return ((size_t)j * 2 + titer) * c->G * c->N * (ABD_TIMELINE_BINS / 2); }
  size_t cell_at(const abd_ctx* c, int j) const { return (size_t)j * 2 * c->G * c->N; }
  size_t ninf_at(const abd_ctx* c, int j) const { return (size_t)j * ABD_TIMELINE_NINF * c->N; }
  int launch(abd_ctx* c, int j, int chain, const double* q, int64_t, hipStream_t st) const {
    return abdi::launch_timeline(c, chain, q, range_n, range_s, st, hist + hist_at(c, j, 0), hist + hist_at(c, j, 1), cell + cell_at(c, j),
                                 ninf + ninf_at(c, j));
  }
};

// abd_loo.hpp: PSIS-LOO by individual.  The kept draws' T_j = S_j + N_j in abd_psis.hpp's matrix, individual-major
// [ld][n C] -- ld = N padded to 64, C = ceil(draws / thin) kept draws per chain, chain j's kept draw c in column j C + c -- and per
// chain a staging block [2][kStage][ld] of the per-individual kernel's S_j rows, then its N_j rows, which abd_loo_store folds into
// the matrix kStage draws at a time.  stored / staged: per chain, the rows in the matrix and in the staging block (a chain belongs
// to one host thread).  launch: one per-individual launch per draw, shared with the WAIC accumulators `acc` (nullptr: off); then,
// with the block full or at the run call's last iteration, the store.
struct LooSummary {
  static constexpr int kStage = 16;
  DevBuf<double> mat, stage, out;  // out [3][ld]: elpd_loo, pareto k, lppd
  DevBuf<int32_t> cells, tail;     // [ld]: the individual's readings (0: padding, or none); n_tail
  int64_t draws = 0, thin = 1, C = 0;
  size_t ld = 0;
  std::vector<int64_t> stored, staged;
  bool on() const { return mat != nullptr; }
  int64_t planned() const { return draws; }
  int64_t capacity() const { return (int64_t)stored.size() * C; }
  double* stage_at(int j, int antigen, int64_t row) const { return stage + (((size_t)j * 2 + antigen) * kStage + (size_t)row) * ld; }
  int launch(abd_ctx* c, int j, int chain, const double* q, int64_t d, bool last, double* acc, hipStream_t st);
  int stats(abd_ctx* c);  // the launch of abd_psis_kernel over the whole matrix into out / tail, on the context's stream
};

struct abd_sampler {
  ~abd_sampler();  // quiesces; then the members go in reverse order (abd_host.hpp)
  abd_ctx* c = nullptr;
  int n = 0;
  abd_sampler_opts o{};
  std::vector<int32_t> chains;
  std::vector<abdnuts::AdaptiveNuts> ch;
  int64_t it = 0;
  int64_t n_accumulated = 0;  // draws in d_sums
  int64_t rec_chunk = 0;      // recording: device staging of up to rec_chunk draws per chain, [n][rec_chunk][...] per variable
  bool ran = false;  // abd_sampler_run* has been called (abd_sampler_enable_pointwise / _predictive are refused after that)
  std::vector<double> lp, gr;  // starting points' logp / gradient
  std::vector<abdnuts::LeapfrogLog> lf_log;  // abd_sampler_enable_leapfrog_log: chain k's log, ch[k].nuts points at it (empty: off)
  int unit = 1;                // chains per independent unit (sampler_run_units)
  int threads = 1;  // host threads that drive the units (sampler_run_units)
  // Leapfrog trains of observation lists (abd_types.hpp: TrainArgs): one chain per unit, diagonal metric.  Every evaluation of such a
  // sampler is a train launch -- it assembles logp and gradient on the device and leaves the next point of the half for
  // the launch queued behind it -- and the host keeps up to `lookahead` launches of a half queued ahead of the record it
  // is waiting for, so a chain's leapfrogs follow each other at the device's pace, not at the host's round trip.
  bool trains = false;
  bool unit_tags = false;  // the units' launches are tagged from the context's per-unit sequences (several host threads)
  int lookahead = 8;
  static constexpr int kTrainRing = 32;  // records per unit: > lookahead + 1
  struct TrainUnit {
    DevBuf<TrainPoint> slots;        // [2]
    MappedBuf<TrainRecord> rec;      // [kTrainRing]
    uint64_t prod = 0, cons = 0;     // launches queued / records taken (or given up: the rest of a half that ended early)
    double tags[kTrainRing] = {};
    int next_slot = 0;               // the slot the last queued launch leaves its successor's point in
    bool last_own_record = true;     // did the launch queued last write its own record (else its successor passes it on)
    int queued_in_half = 0;          // launches queued for the half that is being built
  };
  std::vector<TrainUnit> tu;
  // Leapfrog trains of dense cohorts (abd_types.hpp: TrainChain; abd_train.hpp): units of 1, 2 or 4 chains share their
  // launches, the device goes on from one half of a tree into the next by itself, the host's tree logic follows behind on
  // the records, and a chain's sweep runs on a stream of its own beside the unit's launches for the other chains.
  bool dtrains = false;
  int dtrain_blocks = 0;     // workgroups (with a range) of a unit's launch: the unit's fixed shape
  int dtrain_lookahead = 3;  // steps of a unit the host keeps queued ahead of the oldest record it has not seen
  struct DChain {
    Stream side;                     // the chain's sweep and its recording kernels
    DevBuf<TrainChain> st;
    MappedBuf<TrainRecord> ring;     // [ABD_TRAIN_RING]
    MappedBuf<TrainBegin> begin;     // [kBeginBlocks]
    // [0], [1] the sweep's accepted / proposed counts, [2] (as a double) the tag of the sweep they belong to
    MappedBuf<unsigned long long> done;
    double sweep_tag = 0.0;          // tag of the chain's last sweep (1, 2, 3, ...)
    int64_t n_rec = 0;               // records the steps queued so far produce (index of the next one)
    int64_t n_begin = 0;             // transitions handed over so far
  };
  static constexpr int kBeginBlocks = 4;
  std::vector<DChain> dc;
  // device buffers, declared behind the trains' streams: they go first
  DevBuf<double> d_sums;  // [n][3][G*N]
  DevBuf<double> d_rec_mu;   // [2][n][rec_chunk][G*N]  (ab_n_mu, ab_s_mu)
  DevBuf<int8_t> d_rec_i8;   // [2][n][rec_chunk][G*N]  (i_raw, i) then [n][rec_chunk][N] (waner)
  DevBuf<double> d_rec_ll;   // [n][rec_chunk][K_s + K_n]  pointwise log-likelihood, the device's sorted order (S, then N)
  // pointwise log-likelihood statistics of every draw (abd_readings.hpp: LogLik): [n][4][K_s + K_n] running max, scaled sum
  // of exp, mean, M2 per reading
  DevBuf<double> d_pw_acc;
  // the same statistics of every individual's joint log-likelihood T_j (abd_individual.hpp): [n][4][N]
  DevBuf<double> d_ind_acc;
  DevBuf<double> d_rec_yrep;  // [n][rec_chunk][K_s + K_n]  posterior predictive replicates, the device's sorted order
  // posterior predictive check statistics of every draw (abd_readings.hpp: Predictive): [n][3][K_s + K_n] mean, M2 of the
  // predictive mean, mean tail probability per reading
  DevBuf<double> d_pp_acc;
  // the per-draw summaries (above), in the order queue_draw launches them
  CurvesSummary curves;
  DiagSummary diag;
  TimelineSummary timelines;
  RiskSummary risk;
  LooSummary loo;  // (launched with the per-individual accumulators, not in that order: abd_loo.hpp)
};

namespace abdi {

inline int n_units(const abd_sampler* s) { return (s->n + s->unit - 1) / s->unit; }
// the draws a chain has made so far: what the read-outs report, and what a draw window is checked against
inline int64_t n_draws(const abd_sampler* s) { return std::max<int64_t>(0, s->it - s->o.tune); }

}  // namespace abdi
