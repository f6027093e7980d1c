// abd_host.hpp -- host-side internals shared by the translation units of libabd_hip.so:
//   abd_context.hip  context life cycle, discrete state, Deterministics, the closed-form host terms (priors, Jacobians)
//   abd_eval.hip     evaluation launches (dense panels / observation lists), pipes, completion tags, timing
//   abd_gibbs.hip    the device Gibbs sweep
//   abd_sampler.hip  the native compound sampler (NUTS state machine in abd_nuts.hpp + the sweep): creation and the run loops
//   abd_sampler_summaries.hip  what a caller of the sampler switches on before the first run and reads after one (abd_sampler.hpp)
//   abd_survival.hip the survival models of a finished run (a handle of its own, nothing of an abd_ctx)
// Nothing here is part of the C ABI (include/abd_hip.h).
//
// Device resources are members of owning handles (abd_owned.hpp); nothing is freed by hand.  Teardown: the destructors of
// abd_ctx and abd_sampler first quiesce -- set the device and synchronise every stream that may still use a member -- and
// then the members go in reverse declaration order: the pipes (a stream, then its partial buffers) and the events are
// declared before every other buffer, so they are the last to go.
#pragma once

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/abd_hip.h"
#include "abd_types.hpp"
#include "abd_owned.hpp"
#include "abd_terms.hpp"

static_assert(ABD_MAX_BATCH == ABD_MAX_BATCH_K, "header / kernel batch size mismatch");
static_assert(ABD_MAX_GAPS == 64 * ABD_MAXT_MAX, "header / kernel gap limit mismatch");
static_assert(ABD_N_THETA == ABD_NT, "header / kernel value-variable count mismatch");

namespace abdi {

int fail(int code, const char* fmt, ...);
const char* last_error();
void set_error(const std::string& msg);

#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess) return fail(ABD_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_));        \
  } while (0)

// The product library reads the few documented ABD_* environment variables of include/abd_hip.h (env_int) and nothing else.
// Development knobs (launch shapes, scheduler constants of the sweep) exist only in a tuning build, -DABD_TUNING
// (tools/README.md): in the product they are the compile-time defaults below.
inline int env_int(const char* name, int dflt) {
  const char* e = std::getenv(name);
  return e ? std::atoi(e) : dflt;
}
inline int tune_int(const char* name, int dflt) {
#ifdef ABD_TUNING
  return env_int(name, dflt);
#else
  (void)name;
  return dflt;
#endif
}

constexpr int kResultSlots = 1024;
constexpr int kSyncSlot = kResultSlots;  // private rows of the synchronous calls: they never touch a caller's slot
constexpr int kMaxPipes = 8;             // HIP streams of a context
constexpr int kMinRows = 4;
constexpr int64_t kSimStageBytes = (int64_t)1 << 30;  // abd_simulate: default device staging budget of one chunk of replicates

// ABD_SAMPLER_PROFILE: time the host spends inside hipLaunchKernelGGL for evaluation launches and their sums
struct LaunchProfile {
  bool on = false;
  double eval_s = 0.0, sum_s = 0.0;
  long evals = 0, sums = 0;
};
extern LaunchProfile g_launch_profile;

// Launch `kernel` with `lds` bytes of dynamic LDS (beyond 64 KiB the kernel has to be allowed them first); the launch's error.
template <typename K, typename... A>
hipError_t launch_kernel(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t st, const A&... args) {
  if (lds > 64 * 1024)
    if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds))
      return e;
  hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
  return hipGetLastError();
}

// run `launch` (a launch_kernel call); with ABD_SAMPLER_PROFILE on, its host time goes to the sums' or the evaluations' account
template <typename F>
hipError_t profiled_launch(bool sum, F&& launch) {
  if (!g_launch_profile.on) return launch();
  const auto t0 = std::chrono::steady_clock::now();
  const hipError_t e = launch();
  const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (sum) {
    g_launch_profile.sum_s += s;
    g_launch_profile.sums++;
  } else {
    g_launch_profile.eval_s += s;
    g_launch_profile.evals++;
  }
  return e;
}

// Who queues an evaluation launch (abd_eval.hip: plan_launch decides everything else from it and the number of chains)
struct Caller {
  enum Kind {
    Stream,  // stream-ordered (abd_logp_dlogp_batch_enqueue, abd_logp_dlogp_many): dense launches rotate over the pipes
    Sync,    // a synchronous call: pipe 0, behind everything queued before it
    Unit,    // a native-sampler unit: its own pipe, never joined with the others (units may be driven by several host threads)
    Train,   // one launch of an observation-list leapfrog train (TrainArgs), on its unit's pipe
  } kind;
  int pipe = 0;                // Unit, Train
  double* seq = nullptr;       // Unit, Train: the unit's own completion-tag sequence (nullptr: the context's)
  TrainArgs* train = nullptr;  // Train
};

struct AntigenDev {
  int64_t K = 0;
  DevBuf<unsigned char> y;  // sparse: R[K], sorted by (ind, gap)
  DevBuf<unsigned char> x;  // sparse: R[K]
  DevBuf<uint16_t> g;    // sparse: gap per obs
  DevBuf<int32_t> ptr;   // sparse: (N+1)
  DevBuf<int32_t> j;     // sparse: individual per obs
  DevBuf<unsigned char> yx;  // dense: [G][N] of {od, log_dilution}
  DevBuf<unsigned char> yxi;  // dense: the same pairs individual-major, [N][G] (the sweep kernels' reads)
  // dense, when the antigen has <= 256 distinct log dilutions: the split panels of one-chain launches (abd_dense.hpp: XC)
  DevBuf<unsigned char> od;  // [lane group][G][64] od in the storage type (lane-group-major)
  DevBuf<uint8_t> xc;    // [lane group][G][64] code of the cell's log dilution
  DevBuf<double> dict;   // [n_dict] the distinct log dilutions
  int n_dict = 0;
};

struct ChainSlot {
  DevBuf<uint64_t> rw;    // [nt][N] packed i_raw
  DevBuf<int8_t> waner;   // [N]
  // derived from (rw, waner) and kept current by every writer of the slot (abd_set_discrete, abd_flip_discrete, the sweep
  // kernels): the constrained infections the evaluation kernels read, and {sum(i_raw), sum(ab_s_waner)}
  DevBuf<uint64_t> iw;     // [nt][N] packed i = constrain(i_raw, pcrpos)   abd.py:640-667
  DevBuf<long long> cnt;   // [2]
  // dense cohorts: the exposure planes (abd_planes.hpp), transposed from iw by enqueue_planes behind every writer of iw
  DevBuf<uint64_t> pl;     // [n_lg][abd_plane_gaps(G)][2]
  bool set = false;
};

struct ResultSlot {
  int n = 0;
  bool grad = true;
  size_t row0 = 0;  // the slot's first row in abd_ctx::out (slot * n_slots, or inside the block of a launch of several steps: enqueue_fused)
  std::vector<int32_t> chains;
  std::vector<double> theta;  // n x 17
  std::vector<HostTerms> host;  // n: the host-side terms of every theta, computed when the evaluation is queued
  double tag_first = 0.0;       // completion tag of the slot's first group of <= ABD_MAX_BATCH rows (group g: tag_first + g)
};

}  // namespace abdi

using namespace abdi;

struct abd_ctx {
  int device = 0;
  int G = 0, N = 0, nt = 0, n_chunks = 1;
  int storage = ABD_STORE_F64;
  bool dense = false;
  bool xc_ok = false;  // dense and both antigens have split panels
  int xc_max_cb = 1;   // launches with at most this many chains per workgroup read them
  bool ignore_pcr = false;
  int n_slots = 0;
  int n_cu = 256;
  int n_lg = 0;           // 64-individual lane groups
  int blocks_x = 0;       // sparse kernel grid (wave per individual)
  int ob_n = 0, ob_s = 0, ob_c = 0;  // observation-lane kernel: workgroups per segment
  bool obs_lanes = true;  // sparse lists: lane per observation (abd_obs.hpp) or wave per individual
  int blocks_max = 0;     // rows per chain in `partials`
  int cpw_forced = 0;
  int dense_blocks = 0;   // dense kernel grid.x
  uint64_t chunk_mask[3][ABD_MAXT_MAX] = {};
  int splits[2] = {0, 0};  // the chunks' inner borders, n_chunks - 1 of them (abd_timeline.hpp: timeline_cum)
  ~abd_ctx();  // quiesces; then the members below go in reverse order, pipes and events last
  // A pipe = a HIP stream with its own pair of partial buffers and at most one Pending fixed-order sum (abd_eval.hip:
  // plan_launch names who sums a launch's partial rows: Pending, FinalizeNow or Own).  Pipe 0 is the context's stream
  // (everything synchronous runs there).  Stream-ordered dense launches rotate over n_pipes pipes: the next launch on
  // the same pipe sums a launch's partials in its first workgroups, so the streams never wait for each other and the
  // head of one launch overlaps the tail of the previous one.
  struct Pipe {
    Stream st;
    DevBuf<double> partials[2];  // [n_slots][blocks_max][ABD_NOUT], alternating per launch
    int pbuf = 0;
    bool on = false;  // pending: the fixed-order sum of the last launch's partials has not been queued yet
    int buf = 0, n = 0, blocks = 0;
    double* out = nullptr;
    double tag = 0.0;
    bool busy = false;  // pipe 1: work queued since the last join with pipe 0
  } pipe[kMaxPipes];
  hipStream_t stream = nullptr;  // = pipe[0].st, which owns it
  Event join_ev[kMaxPipes];
  std::vector<std::pair<Event, Event>> ev_pool;  // timing: start / end events (see `timing` below)
  std::vector<Event> win_end;  // timing 2: [window][kMaxPipes] end of each pipe's work in the window (the window ends with the latest)
  std::vector<uint32_t> win_mask;   // ... and which pipes had work in it
  AntigenDev s, n;
  std::vector<int64_t> order_s, order_n;  // reading k of the device's sorted order is the caller's reading order_*[k]
  std::vector<int32_t> seg_s, seg_n;  // [N + 1] offset of every individual's first reading in the sorted order
  DevBuf<uint64_t> vw;  // [nt][N]
  DevBuf<uint64_t> pw;  // [nt][N]
  DevBuf<double> exp2_tab;  // dense cohorts: 2^(j/1024) (abd_dense.hpp)
  DevBuf<int8_t> stage_gn;  // (G, N) upload staging for i_raw
  std::vector<ChainSlot> slots;
  int n_pipes = 4;        // streams that stream-ordered dense launches rotate over (1 = everything on the context's stream); at most one per hardware queue
  int n_streams = kMaxPipes;  // pipes that exist (the native sampler gives every chain a stream: chain k -> pipe k mod 8)
  int n_sync_slots = 4;   // private result rows of synchronous calls (slot kSyncSlot) and of the sampler's chains in flight
  int pipe_blocks = 0;    // dense grid of a launch that shares the chip with n_pipes - 1 others
  int group_blocks = 0;   // dense grid of a sampler unit's launch: one workgroup per CU, whatever the number of units
  int dbpc = 4;           // dense kernel: workgroups per CU of a launch that has the chip to itself
  int next_pipe = 0;
  double seq = 0.0;  // completion tags: 1, 2, 3, ... (exact in a double)
  // A sampler unit's dense launch sums its own partial rows (abd_dense.hpp; ABD_DENSE_OWN_SUM=0: second launch).  Same
  // bits; the result arrives 2-2.7 us later than from the pre-queued second launch, but the host spends 3.6 instead of
  // 7.2 us per result: config 3, evaluations/s seen by NUTS 33.6 k -> 36.9 k (1 chain), 53 k -> 59 k (8), 77 k -> 88 k (16),
  // unchanged with 4
  bool dense_own_sum = true;
  // ABD_DENSE_PLANES: the dense and train kernels take the exposure bookkeeping of the gap loop from the slots' planes
  // (abd_dense.hpp: dense_walk_planes) where the instantiation has a plane form; 0 = the legacy form everywhere.  Same bits.
  bool dense_planes = true;
  DevBuf<unsigned int> d_fin_count;  // [kMaxPipes][ABD_MAX_BATCH] zeroed counters of that sum
  DevBuf<unsigned int> d_train_count;  // [kMaxPipes][1 + ABD_TRAIN_SHARDS][ABD_TRAIN_CNT_STRIDE] zeroed counters of a dense train launch's count-in (abd_dense.hpp)
  uint32_t ind_offset = 0;  // global index of this context's first individual (Gibbs random streams)
  bool xcd_remap = true;
  int fin_rows = 2;
  int steps_behind = -1;  // abd_logp_dlogp_many: steps still to be queued behind the launch being queued (-1: unknown)
  double prior_const = 0.0;
  MappedBuf<double> out;  // result rows, [kResultSlots + n_sync_slots][n_slots][ABD_NOUT]
  std::vector<int> pending_slots;  // slots queued stream-ordered since the last abd_wait
  DevBuf<unsigned long long> d_counts;  // [n_slots][2] Gibbs accepted / proposed
  DevBuf<unsigned int> d_work;             // [2][n_slots] work queue heads of abd_gibbs_dense_kernel (second half: per-chain sweeps of the sampler)
  DevBuf<unsigned long long> d_counts_chain;  // [n_slots][2] counts of the sampler's per-chain sweeps ...
  MappedBuf<unsigned long long> h_counts_chain;  // ... and their pinned host copy (plain pinned: host() only)
  int g2_refill_min = ABD_G2_REFILL_MIN, g2_tail_lanes = ABD_G2_TAIL_LANES, g2_tail_age = ABD_G2_TAIL_AGE;  // scheduler knobs of abd_gibbs_dense_kernel (ABD_G2_*)
  DevBuf<double> d_stage;                  // staging of abd_pointwise_loglik / abd_posterior_predictive: stage_rows rows of K_s + K_n doubles
  int stage_rows = 0;
  DevBuf<double> d_ind_stage;              // staging of abd_individual_loglik: [2][N] (S_j, N_j), allocated on first use
  DevBuf<uint32_t> d_order;                // order_s then order_n as uint32 (the predictive stream's counter), uploaded on first use
  DevBuf<double> d_det;                    // staging of abd_deterministics: mu_n, mu_s (G*N doubles each), i (G*N bytes)
  DevBuf<int32_t> d_last;                  // [N] end of follow-up (abd_set_follow_up); empty: G - 1 for everyone
  DevBuf<unsigned long long> d_curves;     // abd_curves: the slab rows (curves_scratch_cols), then the call's row
  DevBuf<unsigned long long> d_risk;       // abd_risk: the packed slab rows (risk_scratch_cols), then the call's table (32-bit counts)
  std::vector<ResultSlot> results;
  // timing: 1 = HIP events around every evaluation-kernel launch, launches serialised on one stream with the full
  // grid (the isolated kernel); 2 = HIP events around every WINDOW of stream-ordered launches (first launch after an
  // abd_wait .. all pipes joined at the next abd_wait): the launch shape a stream-ordered caller really runs
  int timing = 0;
  bool win_open = false;
  int64_t win_launches = 0;  // steps (a launch may carry several: abd_fuse_plan.hpp) inside the windows collected so far
  size_t ev_used = 0;
  double ev_total_ms = 0.0;
  int64_t ev_count = 0;
  int queue_of_pipe[kMaxPipes] = {};  // probe_stream_queues: streams with the same number share a hardware queue
  int n_queues = 0;                   // 0 = not probed yet
  int pipe_order[kMaxPipes] = {0, 1, 2, 3, 4, 5, 6, 7};  // one stream of every hardware queue first (probe_stream_queues)
  std::vector<double> unit_seq;  // completion-tag sequences of the native sampler's units (abd_sampler.hip: sampler_run_units)
  int64_t wait_fallbacks = 0;  // synchronous calls whose completion tag never showed and that fell back to a stream synchronise
  char name[256] = {0};
};

namespace abdi {

// ---- abd_context.hip
ModelSizes model_sizes(const abd_ctx* c);
void assemble(const abd_ctx* c, const HostTerms& h, const double* t, const double* sums, double* logp, double* grad, bool with_priors = true);
ChainPar chain_par(const abd_ctx* c, int chain, const Transformed& tr);
ChainPar chain_par(const abd_ctx* c, int chain, const double* t);
void base_args(const abd_ctx* c, EvalArgs& a);
// Queue the transpose of iw into the exposure planes of m slots (<= ABD_MAX_BATCH_K) on stream st, behind whatever wrote iw
// there; n_lg lane groups from lg0 on (n_lg < 0: all).  Nothing to do for a cohort kept as observation lists.
int enqueue_planes(abd_ctx* c, int m, const int32_t* chains, hipStream_t st, int lg0 = 0, int n_lg = -1);
#ifdef ABD_STAMPS
unsigned long long* stamps_buffer();  // diagnostic build: in-kernel s_memrealtime stamps (tools/probe_stamps.py)
#endif
int probe_stream_queues(abd_ctx* c);
inline int unit_pipe(const abd_ctx* c, int u) { return c->pipe_order[u % c->n_streams]; }
int check_chains(abd_ctx* c, int n, const int32_t* chains);
// Deterministics of chain `chain` at theta on stream st: written (G, N) gap-major and / or added to running sums
int launch_deterministics(abd_ctx* c, int chain, const double* theta, hipStream_t st, int8_t* out_i, double* out_mun, double* out_mus, double* sums);
// Epidemic curves of chain `chain` at theta on stream st (abd_curves.hpp): slab rows into `scratch` (curves_scratch_cols(c)
// columns, the launch's own until it has run), the row of curves_row_cols(c) columns into `row`.  Touches no member of the
// context but d_last: the sampler's host threads call it side by side.
int launch_curves(abd_ctx* c, int chain, const double* theta, double thr_s, double thr_n, hipStream_t st, unsigned long long* scratch,
                  unsigned long long* row);
size_t curves_row_cols(const abd_ctx* c);
size_t curves_scratch_cols(const abd_ctx* c);
// a row as the C ABI hands it out: counts [4][G], n_infections [8], titer_sums [2][G]; nullptr skips
void split_curves_row(const abd_ctx* c, const unsigned long long* row, int64_t* counts, int64_t* n_infections, double* titer_sums);
// abd_risk_spec as the ABI defines a good one (window, edges, first_only): ABD_OK or fail(ABD_ERR_ARG, ...)
int check_risk_spec(const abd_ctx* c, const abd_risk_spec* spec);
// Risk table of chain `chain` at theta on stream st (abd_risk.hpp): packed slab rows into `scratch` (risk_scratch_cols(c)
// 64-bit words, the launch's own until it has run), the table of risk_table_cols(c) 32-bit counts into `table`.  The spec has
// passed check_risk_spec.  Touches no member of the context but d_last: the sampler's host threads call it side by side.
int launch_risk(abd_ctx* c, int chain, const double* theta, const abd_risk_spec& spec, hipStream_t st, unsigned long long* scratch,
                uint32_t* table);
size_t risk_table_cols(const abd_ctx* c);
size_t risk_scratch_cols(const abd_ctx* c);
// Draw d (= iteration - tune, in [0, 2 H)) of chain `chain` at theta into its convergence accumulators on stream st
// (abd_diag.hpp; H the half length, L the batch length): tit [2][7][G*N], inf [G*N][4] and cb2 [G*N] are the chain's own
// planes.  Touches no member of the context (its block carries d_last as every cell kernel's does; the kernel does not read it).
int launch_diag(abd_ctx* c, int chain, const double* theta, hipStream_t st, int64_t d, int64_t H, int64_t L, double* tit, uint32_t* inf,
                unsigned long long* cb2);
// One individual-major plane of the accumulators (first element src, elements `stride` bytes apart, `width` 4 or 8 bytes
// wide) into dst [G*N] in the caller's gap-major order, 8 bytes per cell, on stream st
int launch_diag_export(abd_ctx* c, const void* src, int stride, int width, unsigned long long* dst, hipStream_t st);
// One draw of chain `chain` at theta into its timeline counters on stream st (abd_timeline.hpp): hist_n and hist_s [G*N][32]
// words, cell [G*N][2] and ninf [N][8] are the chain's own planes; range_n / range_s the titer ranges (lo, hi).  Touches no member of
// the context but d_last: the sampler's host threads call it side by side.
int launch_timeline(abd_ctx* c, int chain, const double* theta, const double range_n[2], const double range_s[2], hipStream_t st,
                    uint32_t* hist_n, uint32_t* hist_s, uint32_t* cell, uint32_t* ninf);
// Gap rows [g0, g0 + n_g) of one individual-major histogram plane into dst [n_g][N][64] 16-bit counters on stream st
int launch_timeline_hist_export(abd_ctx* c, const uint32_t* src, int g0, int n_g, void* dst, hipStream_t st);
// Quantiles q[0 .. n_q) (device memory) of the histograms over range (lo, hi) pooled over n_chains planes `chain_stride` words
// apart into out [n_q][G][N] on stream st
int launch_timeline_quantiles(abd_ctx* c, const uint32_t* hist, int64_t chain_stride, int n_chains, const double range[2], int n_q,
                              const double* q, double* out, hipStream_t st);
// the chain's packed i_raw as (G, N) int8 on stream st
int launch_unpack(abd_ctx* c, int chain, int8_t* dst, hipStream_t st);

// ---- abd_eval.hip
// dynamic LDS of a dense launch with cpw chains per workgroup: power tables, block reduction, 2^(j/1024) table
size_t dense_lds_bytes(int G, int cpw);
int flush_pipe(abd_ctx* c, int pi);
int join_pipes(abd_ctx* c);
int flush_pending(abd_ctx* c);
int flush_ring(abd_ctx* c);
// Rows k, k - 1, ... first of result slot `slot` (mapped host memory), each written by its own workgroup as row, system-scope
// fence, tag: the last of them that does not carry `tag` yet, or first - 1 (and an acquire fence) when all have landed.  Never blocks.
inline int rows_missing(const abd_ctx* c, int slot, int first, int k, double tag) {
  volatile const double* rows = c->out.host() + (size_t)slot * c->n_slots * ABD_NOUT;
  while (k >= first && rows[(size_t)k * ABD_NOUT + ABD_NOUT - 1] == tag) --k;
  if (k < first) __atomic_thread_fence(__ATOMIC_ACQUIRE);
  return k;
}
// once the rows' stream has been synchronised: ABD_OK if rows [first, n) of the slot carry `tag`, else the first that never got it
int rows_never_tagged(abd_ctx* c, int slot, int first, int n, double tag);
int wait_rows(abd_ctx* c, int slot, int n, double tag, hipStream_t st = nullptr);
// queue the evaluation of n chains at theta into result slot `slot` (groups of <= ABD_MAX_BATCH chains, one launch each)
int enqueue_slot(abd_ctx* c, const Caller& who, int slot, int n, const int32_t* chains, const double* theta, bool grad);
// one launch of n chains at `steps` consecutive steps (n * steps <= ABD_MAX_BATCH; steps > 1: dense, stream-ordered) whose host
// terms are ready, host[s * n + j] those of step s, chain j; its sums go to rows[0 .. n * steps) in the same order
int enqueue_group(abd_ctx* c, const Caller& who, int n, const int32_t* chains, const HostTerms* host, bool grad, double* rows, int steps = 1);
int fetch_slot(abd_ctx* c, int slot, double* logp, double* grad, bool with_priors = true);
int enqueue_dense_train(abd_ctx* c, int pi, int cb, int blocks, DenseTrainArgs* a);
// workgroups with a range, as the kernel sees them: of a stepping train launch queued with `blocks` (enqueue_dense_train), and of a
// `kind` launch of n chains (enqueue_group)
int dense_train_ranges(const abd_ctx* c, int blocks);
int eval_grid(const abd_ctx* c, Caller::Kind kind, int n);
int dense_blocks(const abd_ctx* c, int cpw, int share = 0, int grid_rows = 1, int steps = 1);

// Pointwise log-likelihood of chain `chain` at theta on stream st (abd_readings.hpp: LogLik): the row ll (sorted order, S
// readings then N; nullptr skips) and / or the accumulators acc ([4][K_s + K_n]) updated by draw n_draw >= 1 (acc nullptr:
// not updated)
int launch_pointwise(abd_ctx* c, int chain, const double* theta, hipStream_t st, double* ll, double* acc, int64_t n_draw);
// Per-individual sums of the pointwise log-likelihood of chain `chain` at theta on stream st (abd_individual.hpp): the rows
// ll_s, ll_n ([N] each, S_j and N_j; nullptr skips) and / or the accumulators acc ([4][N]) updated with T_j = S_j + N_j by draw
// n_draw >= 1 (acc nullptr: not updated).  A context without readings gets its zeros.  Writes no member of the context:
// the sampler's host threads call it side by side.
int launch_individual_loglik(abd_ctx* c, int chain, const double* theta, hipStream_t st, double* ll_s, double* ll_n, double* acc,
                             int64_t n_draw);
// The caller's reading order on the device (c->d_order), uploaded once; ABD_ERR_ARG for 2^32 readings or more of an antigen.
// Not thread-safe: callers upload before any run loop starts.
int upload_order(abd_ctx* c);
// Posterior predictive of chain `chain` at theta on stream st (abd_readings.hpp: Predictive), the normals keyed by (seed,
// stream, draw): rows yrep / mean (sorted order, S readings then N; nullptr skips) and / or the accumulators acc
// ([3][K_s + K_n]) updated by draw n_draw >= 1 (acc nullptr: not updated).  upload_order must have succeeded.
int launch_predictive(abd_ctx* c, int chain, const double* theta, hipStream_t st, uint64_t seed, uint32_t stream, uint64_t draw,
                      double* yrep, double* mean, double* acc, int64_t n_draw);
// R rows of per-reading values in the device's sorted order (S readings, then N) back to the caller's order of each antigen
// (abd_create), in one pass over the readings: row v of sorted reading k is at(v, k) and goes to out[v].s (an S reading) or
// out[v].n (an N reading); nullptr skips
struct ReadingOut {
  double* s;
  double* n;
};
template <int R, typename At>
void scatter_readings(const abd_ctx* c, const ReadingOut (&out)[R], At at) {
  const size_t Ks = (size_t)c->s.K, Kn = (size_t)c->n.K;
  for (size_t k = 0; k < Ks; ++k) {
    const size_t o = (size_t)c->order_s[k];
    for (int v = 0; v < R; ++v)
      if (out[v].s) out[v].s[o] = at(v, k);
  }
  for (size_t k = 0; k < Kn; ++k) {
    const size_t o = (size_t)c->order_n[k];
    for (int v = 0; v < R; ++v)
      if (out[v].n) out[v].n[o] = at(v, Ks + k);
  }
}

// ---- abd_gibbs.hip
// the decision log of the launch's m chains in device memory, zeroed by the caller (abd_gibbs_sweep_log): rec [m][cap], n [m][N];
// with one, the sweep runs its logging instantiation
struct GibbsLogDev {
  GibbsRecord* rec = nullptr;
  int32_t* n = nullptr;
  int64_t cap = 0;
};
int enqueue_gibbs(abd_ctx* c, int m, const int32_t* chains, const double* theta, uint64_t seed, uint32_t sweep,
                  uint32_t stream_offset, hipStream_t st, unsigned long long* counts_dev, unsigned int* work_dev,
                  unsigned long long* stats_dev, const GibbsLogDev& log = GibbsLogDev());

}  // namespace abdi
