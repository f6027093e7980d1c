// abd_eval.hip -- evaluation launches of the C ABI (include/abd_hip.h): the dense-panel and observation-list kernels,
// the pipes (HIP streams) stream-ordered launches rotate over, completion tags in mapped host memory, device timing.
#include "abd_host.hpp"
#include "abd_fuse_plan.hpp"
#include "abd_eval_kernels.hpp"
#include "abd_train.hpp"
#include "abd_readings.hpp"
#include "abd_individual.hpp"
#include "abd_simulate.hpp"

namespace abdi {

LaunchProfile g_launch_profile;

size_t table_lds_bytes(int G, int cpw, int red_rows, bool exp2_tab = false);
size_t dense_lds_bytes(int G, int cpw) { return abd_dense_lds(G, cpw); }
size_t table_lds_bytes(int G, int cpw, int red_rows, bool exp2_tab) {
  return std::max<size_t>(ABD_FIN_PARTS * ABD_NOUT * sizeof(double),  // finalize scratch of the fused form
                          (size_t)(cpw * 2 + 1) * (G + 1) * sizeof(double2_t) + (size_t)red_rows * ABD_NOUT * sizeof(double) +
                              (exp2_tab ? (size_t)ABD_EXP2_TAB * sizeof(double) : 0));
}

// The evaluation kernels (abd_dense.hpp, abd_obs.hpp, abd_sparse.hpp) and their instantiations
enum class Family { Dense, Lanes, Sparse };  // dense panels; observation lists: lane per observation / wave per individual
using EvalKernel = void (*)(const EvalArgs);
// planes: the context wants the plane form of the gap loop (ABD_DENSE_PLANES) -- given where the instantiation has one
template <typename R, int CB, bool GRAD, bool XC>
EvalKernel dense_kernel(bool planes) {
  if constexpr (dense_plane_form<R, CB, GRAD, XC, false>::value)
    if (planes) return abd_dense_kernel<R, CB, GRAD, XC, true>;
  return abd_dense_kernel<R, CB, GRAD, XC, false>;
}
template <typename R, bool GRAD>
EvalKernel eval_kernel(Family f, int cpw, bool xc, bool wide, bool planes) {  // wide: more than 256 gaps, 8 words per individual
  switch (f) {
    case Family::Dense:  // xc: split panels, R + 1 instead of 2 R bytes per cell and antigen
      if (cpw == 4) return xc ? dense_kernel<R, 4, GRAD, true>(planes) : dense_kernel<R, 4, GRAD, false>(planes);
      if (cpw == 2) return xc ? dense_kernel<R, 2, GRAD, true>(planes) : dense_kernel<R, 2, GRAD, false>(planes);
      return xc ? dense_kernel<R, 1, GRAD, true>(planes) : dense_kernel<R, 1, GRAD, false>(planes);
    case Family::Sparse:  // no 4-chain form: it needs 169 VGPRs (2 waves per SIMD) and spills 245 SGPRs (plan_launch caps it at 2)
      if (cpw == 2) return wide ? abd_sparse_kernel<R, 2, GRAD, ABD_MAXT_MAX> : abd_sparse_kernel<R, 2, GRAD, ABD_MAXT>;
      return wide ? abd_sparse_kernel<R, 1, GRAD, ABD_MAXT_MAX> : abd_sparse_kernel<R, 1, GRAD, ABD_MAXT>;
    default:
      return wide ? abd_obs_kernel<R, GRAD, ABD_MAXT_MAX> : abd_obs_kernel<R, GRAD, ABD_MAXT>;
  }
}

// does a dense launch with cpw chains per workgroup read the split panels (od + one-byte dilution code) or the pair panels?
bool dense_xc(const abd_ctx* c, int cpw) { return c->xc_ok && cpw <= c->xc_max_cb; }

int pick_cpw(const abd_ctx* c, int n) {
  const int forced = c->cpw_forced;
  if (forced == 1 || forced == 2 || forced == 4) {
    if (n % forced == 0) return forced;
  }
  if (n % 4 == 0) return 4;
  if (n % 2 == 0) return 2;
  return 1;
}

// grid of the dense kernel: an exact multiple of the CU count (every wave slot gets the same number of
// gap rows), capped so a slot has at least kMinRows rows
// share: 0 = the launch has the chip to itself, 1 = it is one of n_pipes stream-ordered launches in flight,
// 2 = it is a native-sampler unit's, one of several in flight (c->group_blocks: one workgroup per CU)
// steps: consecutive steps the launch carries (abd_fuse_plan.hpp), grid_rows / steps rows each: a launch that shares the chip
// has 1 / steps of the ranges per row, so that a pipe's launch is as many workgroups as that of a single step
int dense_blocks(const abd_ctx* c, int cpw, int share, int grid_rows, int steps) {
  const int nsub = ABD_WAVES_PER_BLOCK / cpw;
  const int64_t rows = (int64_t)c->n_lg * c->G;
  const int64_t cap = std::max<int64_t>(1, rows / ((int64_t)kMinRows * nsub));
  // a launch with several grid rows (more than 4 chains) fills the chip with fewer, longer ranges per row
  const int64_t alone = std::max<int64_t>(c->n_cu, c->dense_blocks / std::max(1, grid_rows));
  const int64_t half = std::max<int64_t>(c->n_cu, c->group_blocks / std::max(1, grid_rows));
  const int64_t want = share == 1 ? std::max<int64_t>(1, c->pipe_blocks / std::max(1, steps)) : (share == 2 ? half : alone);
  return (int)std::max<int64_t>(1, std::min<int64_t>({want, cap, (int64_t)c->blocks_max}));
}

// do the partial rows of a launch of n_rows chains (rows of several steps: abd_fuse_plan.hpp) x `blocks` workgroups fit a pipe's buffer?
bool partial_rows_fit(const abd_ctx* c, int n_rows, int64_t blocks) { return (int64_t)n_rows * blocks <= (int64_t)c->n_slots * c->blocks_max; }

// The ranges of a dense launch of `blocks` workgroups x `nsub` ranges each: equal shares (+-1) of the n_lg x G rows; with
// one range per workgroup (nsub == 1) the first ABD_MAX_BATCH ranges -- the workgroups that may carry the fused
// fixed-order sum of an earlier launch -- are fin_rows shorter and the others share the difference.  The kernel works its
// range out from these five numbers (abd_types.hpp: EvalArgs::rg_*).
template <typename ARGS>
void range_split(const abd_ctx* c, int blocks, int nsub, ARGS& a, bool fused_sums = true) {
  const int64_t rows_total = (int64_t)c->n_lg * c->G, n_ranges = (int64_t)blocks * nsub;
  const int64_t n_short = (nsub == 1 && fused_sums) ? std::min<int64_t>(ABD_MAX_BATCH, n_ranges) : 0;
  const int64_t e_fin = (nsub == 1 && (rows_total + n_short * c->fin_rows) / n_ranges >= 2 * c->fin_rows) ? c->fin_rows : 0;
  const int64_t virt = rows_total + n_short * e_fin;
  a.rg_base = (int32_t)(virt / n_ranges);
  a.rg_extra = (int32_t)(virt % n_ranges);
  a.rg_e_fin = (int32_t)e_fin;
  a.rg_n_short = (int32_t)n_short;
  a.rg_g_magic = abd_div_magic((uint32_t)c->G);
}

// queue the Pending sum of pipe pi, if any, as its own launch
int flush_pipe(abd_ctx* c, int pi) {
  abd_ctx::Pipe& p = c->pipe[pi];
  if (p.on) {
    const hipError_t le = profiled_launch(true, [&] {
      return launch_kernel(abd_finalize_kernel, dim3(p.n), dim3(ABD_FIN_THREADS), 0, p.st, p.partials[p.buf], p.blocks, p.out, p.tag);
    });
    HIP_TRY(le);
    p.on = false;
  }
  return ABD_OK;
}

// pipe 0 continues only after everything queued on pipe 1 has finished
int join_pipes(abd_ctx* c) {
  for (int pi = 1; pi < c->n_streams; ++pi) {
    abd_ctx::Pipe& p = c->pipe[pi];
    if (!p.st) continue;
    if (int rc = flush_pipe(c, pi)) return rc;
    if (p.busy) {
      HIP_TRY(hipEventRecord(c->join_ev[pi], p.st));
      HIP_TRY(hipStreamWaitEvent(c->stream, c->join_ev[pi], 0));
      p.busy = false;
    }
  }
  c->next_pipe = 0;
  return ABD_OK;
}

int flush_pending(abd_ctx* c) {
  if (int rc = flush_pipe(c, 0)) return rc;
  return join_pipes(c);
}

// A launch goes on pipe pi: the pipe's Pending sum first (unless the launch has taken it over); join_pipes waits for a pipe
// other than 0 from now on
int use_pipe(abd_ctx* c, int pi) {
  if (int rc = flush_pipe(c, pi)) return rc;
  if (pi > 0) c->pipe[pi].busy = true;
  return ABD_OK;
}

// Who does the fixed-order sum of a launch's partial rows
enum class Sum {
  Pending,      // the next dense launch on the same pipe, in its first workgroups (EvalArgs::prev_*), or flush_pipe
  FinalizeNow,  // abd_finalize_kernel, queued right behind the launch
  Own,          // the launch's last workgroup (abd_dense.hpp, abd_obs.hpp: one counter per chain in d_fin_count)
};

// How an evaluation launch runs: everything enqueue_group needs beyond the chains themselves
struct LaunchPlan {
  Family family;
  int cpw;      // chains per workgroup
  dim3 grid;    // (workgroups, steps * n / cpw)
  size_t lds;
  int pipe;
  bool rotate;  // the pipe is the next one of the stream-ordered rotation
  bool join;    // pipe 0 behind everything queued on the other pipes
  Sum sum;
};

// n: chains of one step; steps: consecutive steps of those chains in the launch (1 unless abd_logp_dlogp_many fuses).  cpw,
// and with it the kernel's form, is that of a single step.
LaunchPlan plan_launch(const abd_ctx* c, const Caller& who, int n, int steps) {
  LaunchPlan p;
  p.family = c->dense ? Family::Dense : (c->obs_lanes ? Family::Lanes : Family::Sparse);
  p.cpw = p.family == Family::Lanes ? 1 : pick_cpw(c, n);
  if (p.family == Family::Sparse) p.cpw = std::min(p.cpw, 2);  // (no 4-chain form: eval_kernel)
  // stream-ordered dense launches rotate over the pipes (not under timing 1: one launch at a time); a unit's launches stay on
  // its own pipe; everything else runs on pipe 0 after a join
  const bool own_pipe = who.kind == Caller::Unit || who.kind == Caller::Train;
  p.rotate = who.kind == Caller::Stream && c->n_pipes > 1 && c->dense && c->timing != 1;
  p.join = !own_pipe && !p.rotate;
  p.pipe = own_pipe ? who.pipe : (p.rotate ? c->pipe_order[c->next_pipe] : 0);
  int blocks;
  if (p.family == Family::Dense) {
    // the last launch of a batch of stream-ordered steps ends alone on the chip: it gets the grid of a launch that has the
    // chip to itself (one wave per SIMD issues at half the rate; a K = 20 region 376 -> 373 us; a longer tail did not pay)
    const int share = who.kind == Caller::Unit ? 2 : (p.rotate && c->steps_behind != 0 ? 1 : 0);
    blocks = dense_blocks(c, p.cpw, share, steps * n / p.cpw, steps);
    p.lds = abd_dense_lds(c->G, p.cpw, dense_xc(c, p.cpw));
  } else if (p.family == Family::Lanes) {
    blocks = c->ob_n + c->ob_s + c->ob_c;
    p.lds = who.kind == Caller::Train ? abd_obs_lds_own_sum(c->G) : abd_obs_lds_head(c->G);
  } else {
    blocks = c->blocks_x;
    p.lds = table_lds_bytes(c->G, p.cpw, ABD_WAVES_PER_BLOCK * p.cpw);
  }
  p.grid = dim3(blocks, steps * n / p.cpw);
  // Who sums the partial rows:
  //   caller   dense cohort                                        observation lists
  //   Stream   Pending                                             FinalizeNow
  //   Sync     Pending                                             FinalizeNow
  //   Unit     Own (ABD_DENSE_OWN_SUM=1, <= ABD_TRAIN_ONE_LEVEL    FinalizeNow
  //            workgroups), else FinalizeNow
  //   Train    -- (an error: enqueue_group)                        Own (lane per observation)
  // Only the dense kernel can carry an earlier launch's sum; a unit's rows are awaited before anything else goes on its pipe.
  // A plain launch sums its own rows only with at most ABD_TRAIN_ONE_LEVEL workgroups -- a unit's grid is c->group_blocks,
  // one workgroup per CU -- on one counter per chain; beyond that abd_finalize_kernel adds the rows in the same order.  (An
  // observation-lane launch the host waits for is as fast with the second launch: profiles/README.md, history.)
  if (!c->dense)
    p.sum = who.kind == Caller::Train ? Sum::Own : Sum::FinalizeNow;
  else if (who.kind == Caller::Unit)
    p.sum = c->dense_own_sum && blocks <= ABD_TRAIN_ONE_LEVEL ? Sum::Own : Sum::FinalizeNow;
  else
    p.sum = Sum::Pending;
  return p;
}

int eval_grid(const abd_ctx* c, Caller::Kind kind, int n) { return (int)plan_launch(c, Caller{kind}, n, 1).grid.x; }

int enqueue_group(abd_ctx* c, const Caller& who, int n, const int32_t* chains, const HostTerms* host, bool grad, double* rows, int steps) {
  const LaunchPlan p = plan_launch(c, who, n, steps);
  const int n_rows = n * steps;  // chains of the launch as the kernel sees them: step s, chain j is row s * n + j
  if (steps < 1 || n_rows > ABD_MAX_BATCH || (steps > 1 && (p.family != Family::Dense || p.sum != Sum::Pending)))
    return fail(ABD_ERR_STATE, "internal: a launch of %d steps x %d chains", steps, n);
  if (steps > 1 && !partial_rows_fit(c, n_rows, p.grid.x))
    return fail(ABD_ERR_STATE, "internal: a launch of %d rows x %d workgroups exceeds the partial rows", n_rows, (int)p.grid.x);
  if (who.kind == Caller::Train && (n != 1 || p.family != Family::Lanes))
    return fail(ABD_ERR_STATE, "internal: a leapfrog-train launch needs one chain and the observation-lane kernel");
  if ((int)p.grid.x > c->blocks_max) return fail(ABD_ERR_STATE, "internal: grid %d exceeds partial rows %d", (int)p.grid.x, c->blocks_max);
  // completion tags: the context's sequence, or the caller's own (a sampler unit handled by its own host thread: its
  // result rows are private, so its tags only have to be unique among themselves)
  double& seq = who.seq ? *who.seq : c->seq;
  EvalArgs a;
  base_args(c, a);
  a.n_chains = n_rows;
  for (int k = 0; k < n_rows; ++k) a.ch[k] = chain_par(c, chains[k % n], host[k].tr);
  if (p.family == Family::Dense) range_split(c, (int)p.grid.x, ABD_WAVES_PER_BLOCK / p.cpw, a);
  a.fin_rows = c->fin_rows;
  a.xcd_remap = c->xcd_remap ? 1 : 0;
  if (p.rotate) {
    c->next_pipe = (c->next_pipe + 1) % c->n_pipes;  // (streams of different hardware queues first: probe_stream_queues)
  } else if (p.join) {
    if (int rc = join_pipes(c)) return rc;
  }
  abd_ctx::Pipe& pp = c->pipe[p.pipe];
  // the Pending sum on this pipe is done by this launch's first workgroups if it is a dense launch that does not sum its own
  // rows and has a workgroup for every chain of it
  if (p.family == Family::Dense && p.sum != Sum::Own && pp.on && pp.n <= (int)p.grid.x) {
    a.prev_partials = pp.partials[pp.buf];
    a.prev_out = pp.out;
    a.prev_n_chains = pp.n;
    a.prev_blocks = pp.blocks;
    a.prev_tag = pp.tag;
    pp.on = false;
  }
  if (int rc = use_pipe(c, p.pipe)) return rc;
  const int buf = pp.pbuf;
  pp.pbuf ^= 1;
  a.partials = pp.partials[buf];
  if (p.sum == Sum::Own) {
    a.fin_count = c->d_fin_count + (size_t)p.pipe * ABD_MAX_BATCH;
    a.fin_out = rows;
    a.fin_tag = seq + 1.0;
    if (who.train) {
      who.train->tag = seq + 1.0;
      a.train = *who.train;
    }
  }
  // timing 1: events around every launch; timing 2: the first stream-ordered launch after an abd_wait opens the window
  const bool stream_ordered = who.kind == Caller::Stream;
  hipEvent_t e1 = nullptr;
  if (c->timing == 1 || (c->timing == 2 && stream_ordered && !c->win_open)) {
    if (c->ev_used == c->ev_pool.size()) {
      Event a0, a1;
      HIP_TRY(a0.create());
      HIP_TRY(a1.create());
      c->ev_pool.emplace_back(std::move(a0), std::move(a1));
    }
    // window mode: every pipe is idle here (the previous abd_wait joined and synchronised them), so the stream of
    // the window's first launch carries its start; the end is recorded by flush_ring once all pipes have joined
    HIP_TRY(hipEventRecord(c->ev_pool[c->ev_used].first, pp.st));
    if (c->timing == 1) e1 = c->ev_pool[c->ev_used++].second;
    if (c->timing == 2) c->win_open = true;
  }
  if (c->timing == 2 && stream_ordered) c->win_launches += steps;  // (abd_kernel_time counts steps)
  const bool f32 = c->storage == ABD_STORE_F32, xc = p.family == Family::Dense && dense_xc(c, p.cpw), wide = c->nt > ABD_MAXT;
  const bool pf = c->dense_planes;
  const EvalKernel k = f32 ? (grad ? eval_kernel<float, true>(p.family, p.cpw, xc, wide, pf) : eval_kernel<float, false>(p.family, p.cpw, xc, wide, pf))
                           : (grad ? eval_kernel<double, true>(p.family, p.cpw, xc, wide, pf) : eval_kernel<double, false>(p.family, p.cpw, xc, wide, pf));
  const hipError_t le = profiled_launch(false, [&] { return launch_kernel(k, p.grid, dim3(ABD_BLOCK), p.lds, pp.st, a); });
  if (e1) HIP_TRY(hipEventRecord(e1, pp.st));
  HIP_TRY(le);
  seq += 1.0;
  if (p.sum == Sum::Own) return ABD_OK;
  pp.on = true;
  pp.buf = buf;
  pp.n = n_rows;
  pp.blocks = (int)p.grid.x;
  pp.out = rows;
  pp.tag = seq;
  return p.sum == Sum::FinalizeNow ? flush_pipe(c, p.pipe) : ABD_OK;
}

int flush_ring(abd_ctx* c) {
  if (c->win_open) {
    // timing 2: the window ends when the last pipe has finished its last launch and that launch's sum -- what a caller
    // that polls the completion tags waits for.  One end event per pipe, behind its pending sum and BEFORE the joins
    // (the joins' barrier packets on the context's stream come after the results and are not part of the work).
    const size_t w = c->ev_used;
    if (c->win_end.size() < (w + 1) * kMaxPipes) {
      const size_t old_n = c->win_end.size();
      c->win_end.resize((w + 1) * kMaxPipes);
      for (size_t k = old_n; k < c->win_end.size(); ++k) HIP_TRY(c->win_end[k].create());
    }
    if (c->win_mask.size() < w + 1) c->win_mask.resize(w + 1, 0u);
    c->win_mask[w] = 0u;
    for (int pi = 0; pi < c->n_streams; ++pi) {
      if (!c->pipe[pi].st || !(pi == 0 || c->pipe[pi].busy || c->pipe[pi].on)) continue;  // no work of this window on it
      if (int prc = flush_pipe(c, pi)) return prc;
      HIP_TRY(hipEventRecord(c->win_end[w * kMaxPipes + pi], c->pipe[pi].st));
      c->win_mask[w] |= 1u << pi;
    }
    c->ev_used++;
    c->win_open = false;
  }
  return flush_pending(c);
}

int rows_never_tagged(abd_ctx* c, int slot, int first, int n, double tag) {
  volatile const double* rows = c->out.host() + (size_t)slot * c->n_slots * ABD_NOUT;
  for (int q = first; q < n; ++q)
    if (rows[(size_t)q * ABD_NOUT + ABD_NOUT - 1] != tag) return fail(ABD_ERR_STATE, "result row %d of slot %d never received its completion tag", q, slot);
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  return ABD_OK;
}

// Wait for the rows of a synchronous call (written into mapped host memory) by polling their completion tag;
// falls back to a stream synchronise if it does not show up quickly.
int wait_rows(abd_ctx* c, int slot, int n, double tag, hipStream_t st) {
  // every row is written by its own workgroup, in no particular order: wait for each tag (rows_missing).  Rows of an earlier
  // group of the same call carry a smaller tag and count as landed once a later group's rows are there (groups complete in
  // stream order), so only the last group's tag value is awaited.
  const int first = ((n - 1) / ABD_MAX_BATCH) * ABD_MAX_BATCH;
  int k = n - 1;
  for (int spin = 0; spin < 2000000; ++spin) {
    if ((k = rows_missing(c, slot, first, k, tag)) < first) return ABD_OK;
    __builtin_ia32_pause();
  }
  // the tag did not show within ~2 M polls (tens of ms): the stream synchronise below is always correct, but it should
  // never be needed, so it is counted (abd_wait_fallbacks) instead of passing as a slow call -- and a row that still
  // lacks its tag afterwards is an error, not a result
  __atomic_fetch_add(&c->wait_fallbacks, (int64_t)1, __ATOMIC_RELAXED);
  HIP_TRY(hipStreamSynchronize(st ? st : c->stream));
  return rows_never_tagged(c, slot, first, n, tag);
}

// Wait until every row of a stream-ordered slot carries its completion tag (the rows are in mapped host memory).
// Polls; after a second hands over to a synchronise of the context's stream (which every pipe has joined by then).
int wait_slot(abd_ctx* c, int slot) {
  const ResultSlot& r = c->results[slot];
  volatile const double* rows = c->out.host() + r.row0 * ABD_NOUT;
  const auto t_poll = std::chrono::steady_clock::now();
  int k = r.n - 1;
  for (long spin = 0;; ++spin) {
    while (k >= 0 && rows[(size_t)k * ABD_NOUT + ABD_NOUT - 1] == r.tag_first + (double)(k / ABD_MAX_BATCH)) --k;
    if (k < 0) {
      __atomic_thread_fence(__ATOMIC_ACQUIRE);
      return ABD_OK;
    }
    __builtin_ia32_pause();
    if ((spin & 4095) == 4095 && std::chrono::steady_clock::now() - t_poll > std::chrono::seconds(1)) break;
  }
  __atomic_fetch_add(&c->wait_fallbacks, (int64_t)1, __ATOMIC_RELAXED);  // counted, then verified: see wait_rows
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (int q = 0; q < r.n; ++q)
    if (rows[(size_t)q * ABD_NOUT + ABD_NOUT - 1] != r.tag_first + (double)(q / ABD_MAX_BATCH))
      return fail(ABD_ERR_STATE, "result row %d of stream-ordered slot %d never received its completion tag", q, slot);
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  return ABD_OK;
}

int enqueue_slot(abd_ctx* c, const Caller& who, int slot, int n, const int32_t* chains, const double* theta, bool grad) {
  if (slot < 0 || slot >= kSyncSlot + c->n_sync_slots) return fail(ABD_ERR_ARG, "result slot %d outside [0, %d)", slot, kResultSlots);
  int rc = check_chains(c, n, chains);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  ResultSlot& r = c->results[slot];
  r.n = n;
  r.grad = grad;
  r.row0 = (size_t)slot * c->n_slots;
  r.chains.assign(chains, chains + n);
  r.theta.assign(theta, theta + (size_t)n * ABD_N_THETA);
  r.host.resize((size_t)n);
  for (int k = 0; k < n; ++k) r.host[(size_t)k] = prepare(theta + (size_t)k * ABD_N_THETA);
  // every result row lives in mapped host memory (one PCIe write of 16 doubles + tag per chain, ~3 us inside the kernel)
  double* rows = c->out.dev() + r.row0 * ABD_NOUT;
  r.tag_first = (who.seq ? *who.seq : c->seq) + 1.0;
  if (who.kind == Caller::Stream) c->pending_slots.push_back(slot);
  for (int k0 = 0; k0 < n; k0 += ABD_MAX_BATCH)
    if ((rc = enqueue_group(c, who, std::min(ABD_MAX_BATCH, n - k0), chains + k0, r.host.data() + k0, grad, rows + (size_t)k0 * ABD_NOUT)))
      return rc;
  return ABD_OK;
}

// Queue `steps` consecutive steps of the same n chains (theta: steps x n x 17) as ONE dense stream-ordered launch into result
// slots slot0 .. slot0 + steps - 1.  The launch's rows are one block, step s at rows [s n, (s + 1) n) of it, and the block
// starts where slot0's rows do: n <= n_chain_slots, so it ends inside the rows of the slots it fills.  All rows carry the
// launch's completion tag.
int enqueue_fused(abd_ctx* c, int slot0, int steps, int n, const int32_t* chains, const double* theta, bool grad) {
  if (slot0 < 0 || steps < 1 || slot0 + steps > kResultSlots || n > c->n_slots || n * steps > ABD_MAX_BATCH)
    return fail(ABD_ERR_STATE, "internal: %d fused steps of %d chains at result slot %d", steps, n, slot0);
  if (int rc = check_chains(c, n, chains)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const size_t row0 = (size_t)slot0 * c->n_slots;
  HostTerms host[ABD_MAX_BATCH];
  for (int s = 0; s < steps; ++s) {
    ResultSlot& r = c->results[slot0 + s];
    const double* th = theta + (size_t)s * n * ABD_N_THETA;
    r.n = n;
    r.grad = grad;
    r.row0 = row0 + (size_t)s * n;
    r.chains.assign(chains, chains + n);
    r.theta.assign(th, th + (size_t)n * ABD_N_THETA);
    r.host.resize((size_t)n);
    for (int k = 0; k < n; ++k) host[s * n + k] = r.host[(size_t)k] = prepare(th + (size_t)k * ABD_N_THETA);
    r.tag_first = c->seq + 1.0;
    c->pending_slots.push_back(slot0 + s);
  }
  return enqueue_group(c, Caller{Caller::Stream}, n, chains, host, grad, c->out.dev() + row0 * ABD_NOUT, steps);
}

// ---- leapfrog-train launches of dense cohorts (abd_train.hpp; abd_sampler.hip) ----
using TrainKernel = void (*)(const DenseTrainArgs);
template <typename R, int CB, bool XC>
TrainKernel train_kernel_form(bool planes) {
  if constexpr (dense_plane_form<R, CB, true, XC, true>::value)
    if (planes) return abd_train_kernel<R, CB, XC, true>;
  return abd_train_kernel<R, CB, XC, false>;
}
template <typename R>
TrainKernel train_kernel(int cb, bool xc, bool planes) {
  if (cb == 4) return xc ? train_kernel_form<R, 4, true>(planes) : train_kernel_form<R, 4, false>(planes);
  if (cb == 2) return xc ? train_kernel_form<R, 2, true>(planes) : train_kernel_form<R, 2, false>(planes);
  return xc ? train_kernel_form<R, 1, true>(planes) : train_kernel_form<R, 1, false>(planes);
}

// The service workgroup takes a workgroup slot: a grid that fills the chip exactly leaves it one (the ranges are equal shares of
// the plane whatever their number), or the last range would only start when the first workgroup has left.
int dense_train_ranges(const abd_ctx* c, int blocks) { return (blocks > 1 && blocks % c->n_cu == 0) ? blocks - 1 : blocks; }

// Queue one launch of a train unit of cb (1, 2 or 4) chains on pipe pi: a->tc[0 .. cb) filled by the caller, everything
// else here.  `blocks`: workgroups with a range (the unit's fixed shape: its chains' numbers depend on nothing else).
int enqueue_dense_train(abd_ctx* c, int pi, int cb, int blocks, DenseTrainArgs* a) {
  if (!c->dense) return fail(ABD_ERR_STATE, "internal: dense train launch on a cohort kept as observation lists");
  if (cb != 1 && cb != 2 && cb != 4) return fail(ABD_ERR_STATE, "internal: train unit of %d chains", cb);
  bool any_step = false, any_fwd = false;
  for (int k = 0; k < cb; ++k) {
    TrainChainArgs& tc = a->tc[k];
    if (tc.action != ABD_TR_SKIP || tc.fwd_slot >= 0) {
      if (!tc.st || !tc.ring || !tc.iw || !tc.pl || !tc.cnt || !tc.waner || (tc.action == ABD_TR_BEGIN && !tc.begin))
        return fail(ABD_ERR_STATE, "internal: train launch with a NULL pointer for chain %d of the unit", k);
      if ((tc.action == ABD_TR_STEP && (tc.use_slot | 1) != 1) || tc.fwd_slot > 1)
        return fail(ABD_ERR_STATE, "internal: train launch with slot %d / %d for chain %d of the unit", tc.use_slot, tc.fwd_slot, k);
    }
    any_step |= tc.action == ABD_TR_STEP;
    any_fwd |= tc.fwd_slot >= 0;
  }
  for (int k = cb; k < ABD_TRAIN_CB; ++k) {
    std::memset(&a->tc[k], 0, sizeof a->tc[k]);
    a->tc[k].fwd_slot = -1;
  }
  if (!any_step) blocks = 1;  // nothing to walk: one workgroup runs the state machines (new transitions)
  if (blocks < 1 || blocks > c->blocks_max) return fail(ABD_ERR_STATE, "internal: train grid %d outside [1, %d]", blocks, c->blocks_max);
  const bool xc = c->xc_ok;
  a->yx_n = c->n.yx;
  a->yx_s = c->s.yx;
  a->od_n = c->n.od;
  a->od_s = c->s.od;
  a->xc_n = c->n.xc;
  a->xc_s = c->s.xc;
  a->dict_n = c->n.dict;
  a->dict_s = c->s.dict;
  a->n_dict_n = c->n.n_dict;
  a->n_dict_s = c->s.n_dict;
  a->vw = c->vw;
  a->exp2_tab = c->exp2_tab;
  if (int rc = use_pipe(c, pi)) return rc;
  a->partials = c->pipe[pi].partials[0];
  a->fin_count = c->d_train_count + (size_t)pi * (1 + ABD_TRAIN_SHARDS) * ABD_TRAIN_CNT_STRIDE;
  if ((int64_t)cb * (blocks + ABD_TRAIN_SHARDS) > (int64_t)c->n_slots * c->blocks_max)
    return fail(ABD_ERR_STATE, "internal: train launch of %d x %d workgroups exceeds the partial rows", cb, blocks);
  a->prior_const = c->prior_const;
  a->xcd_remap = c->xcd_remap ? 1 : 0;
  a->service = any_fwd ? 1 : 0;
  // dense_train_ranges ALWAYS, whether this launch carries a service workgroup or not: the split of the plane decides the order
  // of the sums, and a chain's numbers must not depend on what its unit's other chains happen to have pending
  if (any_step) blocks = dense_train_ranges(c, blocks);
  a->G = c->G;
  a->N = c->N;
  a->n_lg = c->n_lg;
  a->K_n = (int32_t)c->n.K;
  a->K_s = (int32_t)c->s.K;
#ifdef ABD_STAMPS
  a->stamps = stamps_buffer();
#endif
  range_split(c, blocks, ABD_WAVES_PER_BLOCK / cb, *a, false);
  const size_t lds = abd_dense_lds(c->G, cb, xc, true);
  dim3 grid(blocks + a->service, 1);
  const TrainKernel k = c->storage == ABD_STORE_F32 ? train_kernel<float>(cb, xc, c->dense_planes) : train_kernel<double>(cb, xc, c->dense_planes);
  const hipError_t le = profiled_launch(false, [&] { return launch_kernel(k, grid, dim3(ABD_BLOCK), lds, c->pipe[pi].st, *a); });
  HIP_TRY(le);
  return ABD_OK;
}

int fetch_slot(abd_ctx* c, int slot, double* logp, double* grad, bool with_priors) {
  if (slot < 0 || slot >= kSyncSlot + c->n_sync_slots) return fail(ABD_ERR_ARG, "result slot %d outside [0, %d)", slot, kResultSlots);
  const ResultSlot& r = c->results[slot];
  if (r.n == 0) return fail(ABD_ERR_STATE, "result slot %d is empty", slot);
  const double* rows = c->out.host() + r.row0 * ABD_NOUT;
  for (int k = 0; k < r.n; ++k)
    assemble(c, r.host[(size_t)k], r.theta.data() + (size_t)k * ABD_N_THETA, rows + (size_t)k * ABD_NOUT, logp + k,
             (grad && r.grad) ? grad + (size_t)k * ABD_N_THETA : nullptr, with_priors);
  return ABD_OK;
}

// ---- per-reading launches (abd_readings.hpp) ----

// The readings, chain slot `chain`'s words and the curve at tr, as both walkers read them
Readings readings_of(const abd_ctx* c, int chain, const Transformed& tr) {
  Readings w;
  std::memset(&w, 0, sizeof w);
  if (c->dense) {
    w.y_n = c->n.yxi;
    w.y_s = c->s.yxi;
  } else {
    w.y_n = c->n.y;
    w.x_n = c->n.x;
    w.y_s = c->s.y;
    w.x_s = c->s.x;
    w.g_n = c->n.g;
    w.g_s = c->s.g;
    w.j_n = c->n.j;
    w.j_s = c->s.j;
    const int64_t cap = (int64_t)c->n_cu * 8;
    w.bn = (int32_t)std::min<int64_t>((c->n.K + ABD_BLOCK - 1) / ABD_BLOCK, cap);
    w.bs = (int32_t)std::min<int64_t>((c->s.K + ABD_BLOCK - 1) / ABD_BLOCK, cap);
  }
  const ChainSlot& sl = c->slots[(size_t)chain];
  w.vw = c->vw;
  w.iw = sl.iw;
  w.waner = sl.waner;
  constexpr double kLog2E = 1.4426950408889634074;
  w.rho[kAgN] = tr.rho_n;
  w.rho[kAgS] = tr.rho_s;
  w.init[kAgN] = tr.init_n;
  w.init[kAgS] = tr.init_s;
  w.perm[kAgN] = tr.perm_n;
  w.perm[kAgS] = tr.perm_s;
  w.b2[kAgN] = tr.b_n * kLog2E;
  w.b2[kAgS] = tr.b_s * kLog2E;
  w.d[kAgN] = tr.d_n;
  w.d[kAgS] = tr.d_s;
  w.temp_n = tr.temp_n;
  w.K_s = c->s.K;
  w.K_n = c->n.K;
  w.G = c->G;
  w.N = c->N;
  w.nt = c->nt;
  return w;
}

// One launch of op over every reading of chain slot `chain` at tr on stream st.  Dense: a wave per individual, three power
// tables, at most 8 workgroups per CU; lists: a lane per reading, two tables, bn + bs workgroups.
template <typename Op>
int launch_readings(abd_ctx* c, int chain, const Transformed& tr, const Op& op, hipStream_t st) {
  const ReadingArgs<Op> a{readings_of(c, chain, tr), op};
  const bool f32 = c->storage == ABD_STORE_F32, wide = c->nt > ABD_MAXT;
  using Kernel = void (*)(const ReadingArgs<Op>);
  Kernel k;
  int blocks;
  size_t lds;
  if (c->dense) {
    k = f32 ? (wide ? abd_readings_dense_kernel<Op, float, ABD_MAXT_MAX> : abd_readings_dense_kernel<Op, float, ABD_MAXT>)
            : (wide ? abd_readings_dense_kernel<Op, double, ABD_MAXT_MAX> : abd_readings_dense_kernel<Op, double, ABD_MAXT>);
    lds = cell_tables_bytes(c->G);
    blocks = std::max(1, std::min((c->N + ABD_WAVES_PER_BLOCK - 1) / ABD_WAVES_PER_BLOCK, c->n_cu * 8));
  } else {
    k = f32 ? (wide ? abd_readings_lists_kernel<Op, float, ABD_MAXT_MAX> : abd_readings_lists_kernel<Op, float, ABD_MAXT>)
            : (wide ? abd_readings_lists_kernel<Op, double, ABD_MAXT_MAX> : abd_readings_lists_kernel<Op, double, ABD_MAXT>);
    lds = (size_t)2 * (c->G + 1) * sizeof(double2_t);
    blocks = a.rd.bn + a.rd.bs;
  }
  HIP_TRY(launch_kernel(k, dim3(blocks), dim3(ABD_BLOCK), lds, st, a));
  return ABD_OK;
}

int launch_pointwise(abd_ctx* c, int chain, const double* theta, hipStream_t st, double* ll, double* acc, int64_t n_draw) {
  if (c->s.K + c->n.K == 0 || (!ll && !acc)) return ABD_OK;
  const Transformed tr = transform(theta);
  LogLik op;
  std::memset(&op, 0, sizeof op);
  op.ll = ll;
  op.acc = acc;
  op.n_draw = acc ? n_draw : 0;
  op.inv_n = acc ? 1.0 / (double)n_draw : 0.0;
  op.inv_sig[kAgN] = 1.0 / tr.sig_n;
  op.inv_sig[kAgS] = 1.0 / tr.sig_s;
  op.lnorm[kAgN] = -(theta[13] + 0.5 * kLog2Pi);  // log sigma is the value variable itself, as in the assembled loglik
  op.lnorm[kAgS] = -(theta[16] + 0.5 * kLog2Pi);
  return launch_readings(c, chain, tr, op, st);
}

int launch_individual_loglik(abd_ctx* c, int chain, const double* theta, hipStream_t st, double* ll_s, double* ll_n, double* acc,
                             int64_t n_draw) {
  if (!ll_s && !ll_n && !acc) return ABD_OK;
  const Transformed tr = transform(theta);
  IndLogLik op;
  std::memset(&op, 0, sizeof op);
  op.ll_s = ll_s;
  op.ll_n = ll_n;
  op.acc = acc;
  op.seg_s = c->s.ptr;  // (observation lists: uploaded with them, empty segments and all; dense panels have none)
  op.seg_n = c->n.ptr;
  op.n_draw = acc ? n_draw : 0;
  op.inv_n = acc ? 1.0 / (double)n_draw : 0.0;
  op.inv_sig[kAgN] = 1.0 / tr.sig_n;
  op.inv_sig[kAgS] = 1.0 / tr.sig_s;
  op.lnorm[kAgN] = -(theta[13] + 0.5 * kLog2Pi);  // as launch_pointwise
  op.lnorm[kAgS] = -(theta[16] + 0.5 * kLog2Pi);
  // one wave per individual in both layouts, three power tables, at most 8 workgroups per CU; a cohort without readings is
  // a lists cohort of empty segments: the launch writes its zeros
  const ReadingArgs<IndLogLik> a{readings_of(c, chain, tr), op};
  const bool f32 = c->storage == ABD_STORE_F32, wide = c->nt > ABD_MAXT;
  using Kernel = void (*)(const ReadingArgs<IndLogLik>);
  const Kernel k = c->dense ? (f32 ? (wide ? abd_individual_dense_kernel<float, ABD_MAXT_MAX> : abd_individual_dense_kernel<float, ABD_MAXT>)
                                   : (wide ? abd_individual_dense_kernel<double, ABD_MAXT_MAX> : abd_individual_dense_kernel<double, ABD_MAXT>))
                            : (f32 ? (wide ? abd_individual_lists_kernel<float, ABD_MAXT_MAX> : abd_individual_lists_kernel<float, ABD_MAXT>)
                                   : (wide ? abd_individual_lists_kernel<double, ABD_MAXT_MAX> : abd_individual_lists_kernel<double, ABD_MAXT>));
  const int blocks = std::max(1, std::min((c->N + ABD_WAVES_PER_BLOCK - 1) / ABD_WAVES_PER_BLOCK, c->n_cu * 8));
  HIP_TRY(launch_kernel(k, dim3(blocks), dim3(ABD_BLOCK), cell_tables_bytes(c->G), st, a));
  return ABD_OK;
}

int upload_order(abd_ctx* c) {
  if (c->d_order) return ABD_OK;
  const int64_t Ks = c->s.K, Kn = c->n.K;
  if (Ks >= ((int64_t)1 << 32) || Kn >= ((int64_t)1 << 32))
    return fail(ABD_ERR_ARG, "%lld / %lld readings: at most 2^32 - 1 per antigen can be keyed by their index", (long long)Ks, (long long)Kn);
  std::vector<uint32_t> h((size_t)std::max<int64_t>(1, Ks + Kn));
  for (int64_t k = 0; k < Ks; ++k) h[(size_t)k] = (uint32_t)c->order_s[(size_t)k];
  for (int64_t k = 0; k < Kn; ++k) h[(size_t)(Ks + k)] = (uint32_t)c->order_n[(size_t)k];
  DevBuf<uint32_t> d;  // (c->d_order is set only once the order is there: it is the "uploaded" flag)
  HIP_TRY(d.upload(h.data(), h.size()));
  c->d_order = std::move(d);
  return ABD_OK;
}

int launch_predictive(abd_ctx* c, int chain, const double* theta, hipStream_t st, uint64_t seed, uint32_t stream, uint64_t draw,
                      double* yrep, double* mean, double* acc, int64_t n_draw) {
  if (c->s.K + c->n.K == 0 || (!yrep && !mean && !acc)) return ABD_OK;
  if (!c->d_order) return fail(ABD_ERR_STATE, "internal: the reading order is not on the device (upload_order)");
  const Transformed tr = transform(theta);
  Predictive op;
  std::memset(&op, 0, sizeof op);
  op.ord = c->d_order;
  op.yrep = yrep;
  op.mean = mean;
  op.acc = acc;
  op.n_draw = acc ? n_draw : 0;
  op.inv_n = acc ? 1.0 / (double)n_draw : 0.0;
  op.sig[kAgN] = tr.sig_n;
  op.sig[kAgS] = tr.sig_s;
  op.inv_sig[kAgN] = 1.0 / tr.sig_n;
  op.inv_sig[kAgS] = 1.0 / tr.sig_s;
  // the stream (abd_readings.hpp): key (seed_lo, seed_hi), counter (r, stream, draw_lo, c3 of the antigen)
  op.seed_lo = (uint32_t)seed;
  op.seed_hi = (uint32_t)(seed >> 32);
  op.stream = stream;
  op.draw_lo = (uint32_t)draw;
  const uint32_t draw_hi = (uint32_t)(draw >> 32) & 0x3FFFFFFFu;
  op.c3[kAgS] = 0x80000000u | (0u << 30) | draw_hi;
  op.c3[kAgN] = 0x80000000u | (1u << 30) | draw_hi;
  return launch_readings(c, chain, tr, op, st);
}

// A synchronous per-reading call of chain slot `chain`: whatever was queued before it is summed and joined, then `launch` writes
// `rows` S-then-N rows into the context's staging on its stream, and they come back into h (left empty without readings or rows)
template <typename F>
int readings_sync(abd_ctx* c, int32_t chain, int rows, std::vector<double>& h, F&& launch) {
  if (int rc = check_chains(c, 1, &chain)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if (int rc = flush_ring(c)) return rc;
  const size_t Kt = (size_t)(c->s.K + c->n.K);
  if (Kt == 0 || rows == 0) return ABD_OK;
  if (!c->d_stage || c->stage_rows < rows) {  // the staging grows to the most rows a call has needed and is kept for the next call
    HIP_TRY(c->d_stage.alloc((size_t)rows * Kt));
    c->stage_rows = rows;
  }
  if (int rc = launch(c->d_stage)) return rc;
  h.resize((size_t)rows * Kt);
  HIP_TRY(hipMemcpyAsync(h.data(), c->d_stage, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return ABD_OK;
}

// A synchronous call: whatever was queued stream-ordered before it is summed and joined first (flush_ring), then the
// evaluation of n chains (logp and, with grad non-null, the gradient) on pipe 0, its rows awaited and assembled
int eval_sync(abd_ctx* c, int n, const int32_t* chains, const double* theta, double* logp, double* grad, bool with_priors = true) {
  if (int rc = flush_ring(c)) return rc;
  if (int rc = enqueue_slot(c, Caller{Caller::Sync}, kSyncSlot, n, chains, theta, grad != nullptr)) return rc;
  if (int rc = flush_pending(c)) return rc;  // (the sum of the last group follows right away)
  if (int rc = wait_rows(c, kSyncSlot, n, c->seq)) return rc;
  return fetch_slot(c, kSyncSlot, logp, grad, with_priors);
}


// ---- the cohort simulator (abd_simulate.hpp) ----

namespace {

int check_sim_antibody(const char* ag, const abd_sim_antibody& p) {
  const struct {
    const char* name;
    double v;
  } f[] = {{"protect_a", p.protect_a}, {"protect_b", p.protect_b}, {"elisa_b", p.elisa_b}, {"elisa_d", p.elisa_d},
           {"elisa_sd", p.elisa_sd}, {"init", p.init}, {"perm_rise", p.perm_rise}, {"temp_rise_i", p.temp_rise_i},
           {"temp_rise_v", p.temp_rise_v}, {"temp_wane", p.temp_wane}};
  for (const auto& e : f)
    if (!std::isfinite(e.v)) return fail(ABD_ERR_ARG, "%s.%s must be finite, got %g", ag, e.name, e.v);
  if (!(p.protect_b > 0.0)) return fail(ABD_ERR_ARG, "%s.protect_b must be > 0, got %g", ag, p.protect_b);
  if (!(p.elisa_b < 0.0)) return fail(ABD_ERR_ARG, "%s.elisa_b must be < 0, got %g", ag, p.elisa_b);
  if (!(p.elisa_d > 0.0)) return fail(ABD_ERR_ARG, "%s.elisa_d must be > 0, got %g", ag, p.elisa_d);
  if (!(p.elisa_sd > 0.0)) return fail(ABD_ERR_ARG, "%s.elisa_sd must be > 0, got %g", ag, p.elisa_sd);
  if (!(p.perm_rise >= 0.0)) return fail(ABD_ERR_ARG, "%s.perm_rise must be >= 0, got %g", ag, p.perm_rise);
  if (!(p.temp_rise_i >= 0.0)) return fail(ABD_ERR_ARG, "%s.temp_rise_i must be >= 0, got %g", ag, p.temp_rise_i);
  if (!(p.temp_rise_v >= 0.0)) return fail(ABD_ERR_ARG, "%s.temp_rise_v must be >= 0, got %g", ag, p.temp_rise_v);
  if (!(p.temp_wane > 0.0 && p.temp_wane <= 1.0)) return fail(ABD_ERR_ARG, "%s.temp_wane must be in (0, 1], got %g", ag, p.temp_wane);
  return ABD_OK;
}

SimWalkAb sim_walk_ab(const abd_sim_antibody& p) {
  return {p.protect_a, p.protect_b, p.init, p.perm_rise, p.temp_rise_i, p.temp_rise_v, p.temp_wane};
}

// the OD readings of one antigen (kAgS / kAgN) for the chunk's replicates, from the walk's staged titers
int launch_sim_readings(abd_ctx* c, int ag, const abd_sim_antibody& p, uint64_t seed, uint32_t rho0, int rc_n, const double* titer,
                        double* od) {
  const AntigenDev& d = ag == kAgS ? c->s : c->n;
  if (d.K == 0) return ABD_OK;
  SimReadArgs a;
  std::memset(&a, 0, sizeof a);
  a.yx = d.yxi;
  a.x = d.x;
  a.g = d.g;
  a.j = d.j;
  a.ord = c->d_order + (ag == kAgS ? 0 : c->s.K);
  a.titer = titer;
  a.od = od;
  a.b = p.elisa_b;
  a.d = p.elisa_d;
  a.sd = p.elisa_sd;
  a.K = d.K;
  a.G = c->G;
  a.N = c->N;
  a.seed_lo = (uint32_t)seed;
  a.seed_hi = (uint32_t)(seed >> 32);
  a.rho0 = rho0;
  a.c3 = kSimNoise | (uint32_t)ag;
  const bool f32 = c->storage == ABD_STORE_F32;
  const auto k = c->dense ? (f32 ? abd_sim_read_kernel<float, true> : abd_sim_read_kernel<double, true>)
                          : (f32 ? abd_sim_read_kernel<float, false> : abd_sim_read_kernel<double, false>);
  HIP_TRY(launch_kernel(k, dim3((unsigned)((d.K + 255) / 256), (unsigned)rc_n), dim3(256), 0, c->stream, a));
  return ABD_OK;
}

}  // namespace

}  // namespace abdi

extern "C" {

int abd_pointwise_loglik(abd_ctx* c, int32_t chain, const double* theta, double* ll_s, double* ll_n) {
  if (!c || !theta) return fail(ABD_ERR_ARG, "NULL argument");
  std::vector<double> h;
  if (int rc = readings_sync(c, chain, (ll_s || ll_n) ? 1 : 0, h,
                             [&](double* d) { return launch_pointwise(c, chain, theta, c->stream, d, nullptr, 0); }))
    return rc;
  const ReadingOut out[1] = {{ll_s, ll_n}};
  if (!h.empty()) scatter_readings(c, out, [&](int, size_t k) { return h[k]; });
  return ABD_OK;
}

int abd_individual_loglik(abd_ctx* c, int32_t chain, const double* theta, double* ll_s, double* ll_n) {
  if (!c || !theta || (!ll_s && !ll_n)) return fail(ABD_ERR_ARG, "NULL argument");
  if (int rc = check_chains(c, 1, &chain)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if (int rc = flush_ring(c)) return rc;
  const size_t N = (size_t)c->N;
  if (!c->d_ind_stage) HIP_TRY(c->d_ind_stage.alloc(2 * N));
  double* const d = c->d_ind_stage;
  if (int rc = launch_individual_loglik(c, chain, theta, c->stream, ll_s ? d : nullptr, ll_n ? d + N : nullptr, nullptr, 0)) return rc;
  if (ll_s) HIP_TRY(hipMemcpyAsync(ll_s, d, N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (ll_n) HIP_TRY(hipMemcpyAsync(ll_n, d + N, N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return ABD_OK;
}

int abd_posterior_predictive(abd_ctx* c, int32_t chain, const double* theta, uint64_t seed, uint32_t stream, uint64_t draw,
                             double* yrep_s, double* yrep_n, double* mean_s, double* mean_n) {
  if (!c || !theta) return fail(ABD_ERR_ARG, "NULL argument");
  const bool rep = yrep_s || yrep_n, mean = mean_s || mean_n;
  const size_t Kt = (size_t)(c->s.K + c->n.K);
  std::vector<double> h;
  if (int rc = readings_sync(c, chain, (rep || mean) ? 2 : 0, h, [&](double* d) {
        if (int urc = upload_order(c)) return urc;
        return launch_predictive(c, chain, theta, c->stream, seed, stream, draw, rep ? d : nullptr, mean ? d + Kt : nullptr, nullptr, 0);
      }))
    return rc;
  if (h.empty()) return ABD_OK;
  const ReadingOut out[2] = {{yrep_s, yrep_n}, {mean_s, mean_n}};
  scatter_readings(c, out, [&](int v, size_t k) { return h[v * Kt + k]; });
  return ABD_OK;
}

int abd_n_result_slots(abd_ctx*) { return kResultSlots; }

int abd_logp_dlogp_batch_enqueue(abd_ctx* c, int32_t slot, int32_t n, const int32_t* chains, const double* theta) {
  if (!c || !chains || !theta) return fail(ABD_ERR_ARG, "NULL argument");
  if (slot < 0 || slot >= kResultSlots) return fail(ABD_ERR_ARG, "result slot %d outside [0, %d)", slot, kResultSlots);
  return enqueue_slot(c, Caller{Caller::Stream}, slot, n, chains, theta, true);
}

int abd_wait(abd_ctx* c) {
  if (!c) return fail(ABD_ERR_ARG, "ctx is NULL");
  HIP_TRY(hipSetDevice(c->device));
  int rc = flush_ring(c);
  if (rc) return rc;
  // every stream-ordered slot's rows carry a tag: the newest slots land last, so poll backwards and stop early
  for (size_t q = c->pending_slots.size(); q-- > 0;)
    if (int wrc = wait_slot(c, c->pending_slots[q])) return wrc;
  c->pending_slots.clear();
  return ABD_OK;
}

int abd_fetch(abd_ctx* c, int32_t slot, double* logp, double* grad) {
  if (!c || !logp) return fail(ABD_ERR_ARG, "NULL argument");
  if (slot < 0 || slot >= kResultSlots) return fail(ABD_ERR_ARG, "result slot %d outside [0, %d)", slot, kResultSlots);
  return fetch_slot(c, slot, logp, grad);
}

int abd_fetch_many(abd_ctx* c, int32_t n_slots, const int32_t* slots, double* logp, double* grad) {
  if (!c || !slots || !logp) return fail(ABD_ERR_ARG, "NULL argument");
  size_t off = 0;
  for (int s = 0; s < n_slots; ++s) {
    if (slots[s] < 0 || slots[s] >= kResultSlots) return fail(ABD_ERR_ARG, "result slot %d outside [0, %d)", slots[s], kResultSlots);
    const int n = c->results[slots[s]].n;
    int rc = fetch_slot(c, slots[s], logp + off, grad ? grad + off * ABD_N_THETA : nullptr);
    if (rc) return rc;
    off += (size_t)n;
  }
  return ABD_OK;
}

int abd_logp_dlogp_many(abd_ctx* c, int32_t n_steps, int32_t n, const int32_t* chains, const double* theta, double* logp,
                        double* grad) {
  if (!c || !chains || !theta || !logp) return fail(ABD_ERR_ARG, "NULL argument");
  if (n_steps < 0) return fail(ABD_ERR_ARG, "n_steps=%d is negative", n_steps);
  const size_t per_step = (size_t)n * ABD_N_THETA;
  // Dense cohorts: consecutive steps share launches (abd_fuse_plan.hpp) where the launch's rows fit the partial and the result
  // rows; not under timing 1 (the isolated kernel, one single-step launch at a time)
  int max_steps = 1;
  if (c->dense && c->timing != 1 && n >= 1 && n <= c->n_slots && n <= ABD_MAX_BATCH) {
    const int cpw = pick_cpw(c, n);
    for (max_steps = std::min(kFuseMaxSteps, ABD_MAX_BATCH / n); max_steps > 1; --max_steps) {
      const int rows = max_steps * n / cpw;
      const int64_t widest = std::max(dense_blocks(c, cpw, 0, rows, max_steps), dense_blocks(c, cpw, 1, rows, max_steps));
      if (partial_rows_fit(c, max_steps * n, widest)) break;
    }
  }
  const int pipes = c->n_pipes > 1 && c->timing != 1 ? c->n_pipes : 1;
  const std::vector<FusedLaunch> plan = fuse_plan(n_steps, n, pipes, kResultSlots, tune_int("ABD_FUSE_STEPS", 0), max_steps, ABD_MAX_BATCH);
  size_t next = 0;  // the plan's launches never cross a window
  for (int s0 = 0; s0 < n_steps; s0 += kResultSlots) {  // windows of the result ring
    const int s1 = std::min(n_steps, s0 + kResultSlots);
    for (; next < plan.size() && plan[next].first < s1; ++next) {
      const FusedLaunch& l = plan[next];
      const int k = l.first;
      c->steps_behind = l.alone ? 0 : n_steps - k - l.steps;  // 0: the call's last launch, shaped for an empty chip
      const int rc = l.steps == 1 ? enqueue_slot(c, Caller{Caller::Stream}, k - s0, n, chains, theta + (size_t)k * per_step, grad != nullptr)
                                  : enqueue_fused(c, k - s0, l.steps, n, chains, theta + (size_t)k * per_step, grad != nullptr);
      c->steps_behind = -1;
      if (rc) return rc;
    }
    // the results land in mapped host memory slot by slot: queue the pending sums and the joins, then take every step's
    // result as soon as its tag shows -- the host-side assembly of the early steps overlaps the late steps' kernels
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = flush_ring(c)) return rc;
    for (int k = s0; k < s1; ++k) {
      if (int rc = wait_slot(c, k - s0)) return rc;
      if (int rc = fetch_slot(c, k - s0, logp + (size_t)k * n, grad ? grad + (size_t)k * per_step : nullptr)) return rc;
      // a step that shared a launch has its rows inside the first step's block, where a later enqueue into that slot writes:
      // it is taken here and leaves nothing behind for abd_fetch
      ResultSlot& r = c->results[k - s0];
      if (r.row0 != (size_t)(k - s0) * c->n_slots) r.n = 0;
    }
    c->pending_slots.clear();
  }
  return ABD_OK;
}

int abd_logp_dlogp_batch(abd_ctx* c, int32_t n, const int32_t* chains, const double* theta, double* logp, double* grad) {
  if (!c || !chains || !theta || !logp || !grad) return fail(ABD_ERR_ARG, "NULL argument");
  return eval_sync(c, n, chains, theta, logp, grad);
}

int abd_logp_dlogp(abd_ctx* c, int32_t chain, const double* theta, double* logp, double* grad) {
  return abd_logp_dlogp_batch(c, 1, &chain, theta, logp, grad);
}

int abd_loglik_dlogp(abd_ctx* c, int32_t chain, const double* theta, double* loglik, double* grad) {
  if (!c || !theta || !loglik || !grad) return fail(ABD_ERR_ARG, "NULL argument");
  return eval_sync(c, 1, &chain, theta, loglik, grad, false);
}

int abd_logp(abd_ctx* c, int32_t chain, const double* theta, double* logp) {
  if (!c || !theta || !logp) return fail(ABD_ERR_ARG, "NULL argument");
  return eval_sync(c, 1, &chain, theta, logp, nullptr);
}

int abd_kernel_timing(abd_ctx* c, int32_t mode) {
  if (!c) return fail(ABD_ERR_ARG, "ctx is NULL");
  if (mode < 0 || mode > 2) return fail(ABD_ERR_ARG, "timing mode %d outside {0, 1, 2}", mode);
  if (mode != c->timing) {
    HIP_TRY(hipSetDevice(c->device));
    if (int frc = flush_ring(c)) return frc;  // closes an open window, joins the pipes
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  c->timing = mode;
  return ABD_OK;
}

int abd_kernel_time(abd_ctx* c, double* total_ms, int64_t* launches, int32_t reset) {
  if (!c) return fail(ABD_ERR_ARG, "ctx is NULL");
  HIP_TRY(hipSetDevice(c->device));
  if (int frc = flush_ring(c)) return frc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (size_t k = 0; k < c->ev_used; ++k) {
    float ms = 0.f;
    if (c->timing == 2) {  // window: first launch's start .. the latest pipe's end
      for (int pi = 0; pi < c->n_streams; ++pi) {
        if (!c->pipe[pi].st || (k + 1) * kMaxPipes > c->win_end.size() || k >= c->win_mask.size() || !(c->win_mask[k] >> pi & 1u)) continue;
        float m = 0.f;
        if (hipEventElapsedTime(&m, c->ev_pool[k].first, c->win_end[k * kMaxPipes + pi]) == hipSuccess) ms = std::max(ms, m);
      }
    } else {
      HIP_TRY(hipEventElapsedTime(&ms, c->ev_pool[k].first, c->ev_pool[k].second));
    }
    c->ev_total_ms += ms;
    if (c->timing != 2) c->ev_count++;
  }
  if (c->timing == 2) {
    c->ev_count += c->win_launches;
    c->win_launches = 0;
  }
  c->ev_used = 0;
  if (total_ms) *total_ms = c->ev_total_ms;
  if (launches) *launches = c->ev_count;
  if (reset) {
    c->ev_total_ms = 0.0;
    c->ev_count = 0;
  }
  return ABD_OK;
}

int64_t abd_wait_fallbacks(abd_ctx* c) { return c ? c->wait_fallbacks : -1; }

int abd_simulate(abd_ctx* c, const abd_sim_params* par, const double* lam0, uint64_t seed, uint32_t first_replicate,
                 int32_t n_replicates, int8_t* infections, double* s_titer, double* n_titer, double* od_s, double* od_n,
                 int64_t* n_infected) {
  return abd_simulate_staged(c, par, lam0, seed, first_replicate, n_replicates, 0, infections, s_titer, n_titer, od_s, od_n, n_infected);
}

int abd_simulate_staged(abd_ctx* c, const abd_sim_params* par, const double* lam0, uint64_t seed, uint32_t first_replicate,
                        int32_t n_replicates, int64_t staging_bytes, int8_t* infections, double* s_titer, double* n_titer,
                        double* od_s, double* od_n, int64_t* n_infected) {
  if (!c) return fail(ABD_ERR_ARG, "ctx is NULL");
  if (staging_bytes < 0) return fail(ABD_ERR_ARG, "staging_bytes=%lld is negative", (long long)staging_bytes);
  if (staging_bytes == 0) staging_bytes = kSimStageBytes;
  if (!par) return fail(ABD_ERR_ARG, "params is NULL");
  if (!lam0) return fail(ABD_ERR_ARG, "lam0 is NULL");
  if (int rc = check_sim_antibody("s", par->s)) return rc;
  if (int rc = check_sim_antibody("n", par->n)) return rc;
  const int G = c->G, N = c->N;
  for (int g = 0; g < G; ++g)
    if (!std::isfinite(lam0[g])) return fail(ABD_ERR_ARG, "lam0[%d] must be finite, got %g", g, lam0[g]);
  if (n_replicates < 1) return fail(ABD_ERR_ARG, "n_replicates must be >= 1, got %d", n_replicates);
  if ((uint64_t)first_replicate + (uint64_t)n_replicates > ((uint64_t)1 << 32))
    return fail(ABD_ERR_ARG, "first_replicate + n_replicates = %llu exceeds 2^32", (unsigned long long)first_replicate + (unsigned long long)n_replicates);
  if (c->s.K == 0) od_s = nullptr;
  if (c->n.K == 0) od_n = nullptr;
  if (!infections && !s_titer && !n_titer && !od_s && !od_n && !n_infected) return ABD_OK;
  HIP_TRY(hipSetDevice(c->device));
  if (int rc = flush_ring(c)) return rc;
  if (od_s || od_n)
    if (int rc = upload_order(c)) return rc;

  // Staging of one chunk of replicates within the budget (at least one replicate): the outputs asked for, and the titers
  // the readings gather.  Every part starts on a 256-byte boundary.
  const size_t cells = (size_t)G * N, Ks = (size_t)c->s.K, Kn = (size_t)c->n.K;
  const bool want_s = s_titer || od_s, want_n = n_titer || od_n;
  auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t per_rep = (infections ? cells : 0) + ((want_s ? 1 : 0) + (want_n ? 1 : 0)) * cells * sizeof(double) +
                         (od_s ? Ks * sizeof(double) : 0) + (od_n ? Kn * sizeof(double) : 0) + (n_infected ? (size_t)G * 8 : 0);
  const int rc_max = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)n_replicates, (int64_t)((size_t)staging_bytes / per_rep), 65535}));
  DevBuf<unsigned char> stage;  // released on every return below; nothing is queued on it when an error returns (see sync)
  DevBuf<double> d_lam;
  HIP_TRY(d_lam.upload(lam0, (size_t)G));
  const size_t o_inf = 0;
  const size_t o_s = o_inf + pad(infections ? cells * rc_max : 0);
  const size_t o_n = o_s + pad(want_s ? cells * rc_max * sizeof(double) : 0);
  const size_t o_ods = o_n + pad(want_n ? cells * rc_max * sizeof(double) : 0);
  const size_t o_odn = o_ods + pad(od_s ? Ks * rc_max * sizeof(double) : 0);
  const size_t o_cnt = o_odn + pad(od_n ? Kn * rc_max * sizeof(double) : 0);
  const size_t total = o_cnt + pad(n_infected ? (size_t)G * rc_max * 8 : 0);
  HIP_TRY(stage.alloc(total));
  unsigned char* const sb = stage;
  int8_t* const d_inf = infections ? reinterpret_cast<int8_t*>(sb + o_inf) : nullptr;
  double* const d_s = want_s ? reinterpret_cast<double*>(sb + o_s) : nullptr;
  double* const d_n = want_n ? reinterpret_cast<double*>(sb + o_n) : nullptr;
  double* const d_ods = od_s ? reinterpret_cast<double*>(sb + o_ods) : nullptr;
  double* const d_odn = od_n ? reinterpret_cast<double*>(sb + o_odn) : nullptr;
  unsigned long long* const d_cnt = n_infected ? reinterpret_cast<unsigned long long*>(sb + o_cnt) : nullptr;

  // one chunk: the walk, the readings, the copies back; the stream is drained before the staging is reused or released
  auto chunk = [&](int r0, int rn) -> int {
    SimWalkArgs w;
    std::memset(&w, 0, sizeof w);
    w.par.s = sim_walk_ab(par->s);
    w.par.n = sim_walk_ab(par->n);
    w.lam0 = d_lam;
    w.vw = c->vw;
    w.pw = c->ignore_pcr ? nullptr : (const uint64_t*)c->pw;
    w.inf = d_inf;
    w.st = d_s;
    w.nt = d_n;
    w.cnt = d_cnt;
    w.seed_lo = (uint32_t)seed;
    w.seed_hi = (uint32_t)(seed >> 32);
    w.ind_offset = c->ind_offset;
    w.rho0 = first_replicate + (uint32_t)r0;
    w.G = G;
    w.N = N;
    if (d_cnt) HIP_TRY(hipMemsetAsync(d_cnt, 0, (size_t)G * rn * 8, c->stream));
    HIP_TRY(launch_kernel(abd_sim_walk_kernel, dim3((unsigned)c->n_lg, (unsigned)rn), dim3(64), 0, c->stream, w));
    if (d_ods)
      if (int rc = launch_sim_readings(c, kAgS, par->s, seed, w.rho0, rn, d_s, d_ods)) return rc;
    if (d_odn)
      if (int rc = launch_sim_readings(c, kAgN, par->n, seed, w.rho0, rn, d_n, d_odn)) return rc;
    const size_t r = (size_t)r0, n = (size_t)rn;
    if (infections) HIP_TRY(hipMemcpyAsync(infections + r * cells, d_inf, n * cells, hipMemcpyDeviceToHost, c->stream));
    if (s_titer) HIP_TRY(hipMemcpyAsync(s_titer + r * cells, d_s, n * cells * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (n_titer) HIP_TRY(hipMemcpyAsync(n_titer + r * cells, d_n, n * cells * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (od_s) HIP_TRY(hipMemcpyAsync(od_s + r * Ks, d_ods, n * Ks * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (od_n) HIP_TRY(hipMemcpyAsync(od_n + r * Kn, d_odn, n * Kn * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (n_infected) HIP_TRY(hipMemcpyAsync(n_infected + r * (size_t)G, d_cnt, n * (size_t)G * 8, hipMemcpyDeviceToHost, c->stream));
    return ABD_OK;
  };
  for (int r0 = 0; r0 < n_replicates; r0 += rc_max) {
    const int rc = chunk(r0, std::min(rc_max, n_replicates - r0));
    const hipError_t se = hipStreamSynchronize(c->stream);  // also after a failed chunk: nothing may still use the staging
    if (rc) return rc;
    HIP_TRY(se);
  }
  return ABD_OK;
}

}  // extern "C"
