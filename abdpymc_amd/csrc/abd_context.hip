// abd_context.hip -- context life cycle, discrete state and host-side closed forms of the C ABI (include/abd_hip.h).
//
// Replaces, for the joint-logp path only, what PyMC/PyTensor compile out of abdpymc.model()
// (reference abdpymc/abd.py:396-469): the closed-form prior terms + transform Jacobians are evaluated
// here on the host (17 scalars), the O(G*N) data term on the device (abd_dense.hpp, abd_obs.hpp, abd_sparse.hpp).
#include "abd_host.hpp"

#include <memory>
#include <unordered_map>
#include "abd_small.hpp"
#include "abd_curves.hpp"
#include "abd_risk.hpp"
#include "abd_diag.hpp"
#include "abd_timeline.hpp"

static_assert(ABD_TL_BINS == ABD_TIMELINE_BINS && ABD_TL_MAX_DRAWS == ABD_TIMELINE_MAX_DRAWS && ABD_TL_MAX_Q == ABD_TIMELINE_MAX_Q &&
                  ABD_TL_NINF == ABD_TIMELINE_NINF,
              "abd_timeline.hpp and include/abd_hip.h describe the same counters");

namespace abdi {

namespace {
thread_local std::string g_err = "";
}
int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
const char* last_error() { return g_err.c_str(); }
void set_error(const std::string& msg) { g_err = msg; }

// theta-independent part of the priors: -lnB(1, G-1) - 2 lnB(10, 1) + sum over the Gammas of
// alpha log beta - lgamma(alpha) + the Normals' -log sd - 1/2 log 2 pi (14 lgamma calls otherwise made per
// evaluation)
double prior_constant(int G) {
  double v = -(std::lgamma(1.0) + std::lgamma((double)(G - 1)) - std::lgamma((double)G));
  v += -2.0 * (std::lgamma(10.0) + std::lgamma(1.0) - std::lgamma(11.0));
  const double gmu[5] = {2.0, 1.0, 2.0, 1.0, 1.0};
  for (int q = 0; q < 5; ++q) {
    const double al = gmu[q] * gmu[q] / 0.25, be = gmu[q] / 0.25;
    v += al * std::log(be) - std::lgamma(al);
  }
  const double nsd[6] = {1.0, 1.0, 0.5, 0.5, 0.5, 0.5};
  for (int q = 0; q < 6; ++q) v += -std::log(nsd[q]) - 0.5 * kLog2Pi;
  return v;
}

ModelSizes model_sizes(const abd_ctx* c) {
  ModelSizes m;
  m.G = c->G;
  m.dense = c->dense ? 1 : 0;
  m.N = (double)c->N;
  m.cells = (double)c->G * (double)c->N;
  m.Kn = (double)c->n.K;
  m.Ks = (double)c->s.K;
  m.prior_const = c->prior_const;
  return m;
}

// Combine the device sums of one chain with the closed-form terms (abd_terms.hpp)
void assemble(const abd_ctx* c, const HostTerms& h, const double* t, const double* sums, double* logp, double* grad,
              bool with_priors) {
  assemble_terms(model_sizes(c), h, t, sums, logp, grad, with_priors);
}

ChainPar chain_par(const abd_ctx* c, int chain, const Transformed& tr) {
  ChainPar p;
  chain_par_from_tr(p, &tr.p);
  p.rw = c->slots[chain].rw;
  p.waner = c->slots[chain].waner;
  p.iw = c->slots[chain].iw;
  p.cnt = c->slots[chain].cnt;
  p.pl = c->slots[chain].pl;
  return p;
}
ChainPar chain_par(const abd_ctx* c, int chain, const double* t) { return chain_par(c, chain, transform(t)); }

int enqueue_planes(abd_ctx* c, int m, const int32_t* chains, hipStream_t st, int lg0, int n_lg) {
  if (!c->dense) return ABD_OK;
  if (m < 1 || m > ABD_MAX_BATCH_K) return fail(ABD_ERR_STATE, "internal: planes of %d slots in one launch", m);
  if (n_lg < 0) n_lg = c->n_lg - lg0;
  if (lg0 < 0 || n_lg < 1 || lg0 + n_lg > c->n_lg) return fail(ABD_ERR_STATE, "internal: planes of lane groups [%d, %d) of %d", lg0, lg0 + n_lg, c->n_lg);
  PlaneArgs a;
  std::memset(&a, 0, sizeof a);
  for (int k = 0; k < m; ++k) {
    a.src[k] = c->slots[(size_t)chains[k]].iw;
    a.dst[k] = c->slots[(size_t)chains[k]].pl;
  }
  a.N = c->N;
  a.G = c->G;
  a.which = 0;
  a.lg0 = lg0;
  hipLaunchKernelGGL(abd_planes_kernel, dim3(n_lg, c->nt, m), dim3(64), 0, st, a);
  HIP_TRY(hipGetLastError());
  return ABD_OK;
}

ConstrainArgs constrain_args(const abd_ctx* c) {
  ConstrainArgs a;
  std::memset(&a, 0, sizeof a);
  a.pw = c->ignore_pcr ? nullptr : c->pw;
  a.N = c->N;
  a.nt = c->nt;
  a.n_chunks = c->n_chunks;
  std::memcpy(a.chunk_mask, c->chunk_mask, sizeof a.chunk_mask);
  return a;
}

#ifdef ABD_STAMPS
unsigned long long* stamps_buffer() {
  static MappedBuf<unsigned long long>& stamps = *new MappedBuf<unsigned long long>();  // lives as long as the process
  if (!stamps) {
    (void)stamps.alloc(4096 * 16);
    if (const char* e = std::getenv("ABD_STAMPS_PTR_OUT")) {  // the probe reads the buffer through its address
      FILE* f = std::fopen(e, "w");
      if (f) {
        std::fprintf(f, "%llu\n", (unsigned long long)(uintptr_t)stamps.host());
        std::fclose(f);
      }
    }
  }
  return stamps.dev();
}
#endif

void base_args(const abd_ctx* c, EvalArgs& a) {
  std::memset(&a, 0, sizeof a);
  a.y_n = c->n.y;
  a.x_n = c->n.x;
  a.y_s = c->s.y;
  a.x_s = c->s.x;
  a.g_n = c->n.g;
  a.g_s = c->s.g;
  a.ptr_n = c->n.ptr;
  a.ptr_s = c->s.ptr;
  a.j_n = c->n.j;
  a.j_s = c->s.j;
  a.K_n = (int32_t)c->n.K;
  a.K_s = (int32_t)c->s.K;
  a.ob_n = c->ob_n;
  a.ob_s = c->ob_s;
  a.ob_c = c->ob_c;
  a.yx_n = c->n.yx;
  a.yx_s = c->s.yx;
  a.yxi_n = c->n.yxi;
  a.yxi_s = c->s.yxi;
  a.od_n = c->n.od;
  a.od_s = c->s.od;
  a.xc_n = c->n.xc;
  a.xc_s = c->s.xc;
  a.dict_n = c->n.dict;
  a.dict_s = c->s.dict;
  a.n_dict_n = c->n.n_dict;
  a.n_dict_s = c->s.n_dict;
  a.vw = c->vw;
  a.pw = c->ignore_pcr ? nullptr : c->pw;
  a.exp2_tab = c->exp2_tab;
#ifdef ABD_STAMPS
  a.stamps = stamps_buffer();
#endif
  a.G = c->G;
  a.N = c->N;
  a.nt = c->nt;
  a.n_chunks = c->n_chunks;
  a.n_lg = c->n_lg;
  std::memcpy(a.chunk_mask, c->chunk_mask, sizeof a.chunk_mask);
}
int probe_stream_queues(abd_ctx* c) {
  if (c->n_queues > 0) return ABD_OK;
  HIP_TRY(hipSetDevice(c->device));
  // Candidates: the context's streams plus as many spare ones.  HIP hands its hardware queues to streams in creation order
  // across the whole process, so the context's 8 streams rarely sit on them evenly (3 + 2 + 2 + 1 on this stack): after the
  // probe, streams of over-subscribed queues are exchanged for spare streams of under-subscribed ones, so that eight units
  // are two per queue, not three on one (the queue with the most units sets the pace of a run).
  constexpr int kCand = 2 * kMaxPipes;
  const int ns = c->n_streams;
  Stream spare[kMaxPipes];  // candidate ns + k; whatever the exchange leaves here goes when the function returns
  hipStream_t cand[kCand] = {};
  int n_cand = ns;
  for (int pi = 0; pi < ns; ++pi) cand[pi] = c->pipe[pi].st;
  for (; n_cand < ns + kMaxPipes; ++n_cand) {
    if (spare[n_cand - ns].create() != hipSuccess) {
      (void)hipGetLastError();
      break;
    }
    cand[n_cand] = spare[n_cand - ns];
  }
  DevBuf<unsigned long long> d;
  hipError_t le = d.alloc((size_t)kCand * 2);
  // Stream k's wave stays for 150 + 20 k us, so the waves end at least 20 us apart and a wave that had to wait for a
  // queue starts within a few us of exactly one earlier wave's end: it is behind that one.  A wave that starts while all
  // earlier ones are still there has a queue to itself.  A host hiccup between two launches can make a stream look
  // queued, never the other way round: up to three attempts, the one that finds the most queues counts.
  int best_nq = 0, best[kCand] = {};
  for (int attempt = 0; attempt < 3 && best_nq < 4 && le == hipSuccess; ++attempt) {
    le = hipDeviceSynchronize();
    for (int k = 0; k < n_cand && le == hipSuccess; ++k) {
      hipLaunchKernelGGL(abd_spin_kernel, dim3(1), dim3(64), 0, cand[k], d + 2 * k, 15000ull + 2000ull * (unsigned long long)k);
      le = hipGetLastError();
    }
    if (le == hipSuccess) le = hipDeviceSynchronize();
    unsigned long long h[kCand * 2] = {};
    if (le == hipSuccess) le = hipMemcpy(h, d, sizeof(unsigned long long) * 2 * (size_t)n_cand, hipMemcpyDeviceToHost);
    if (le != hipSuccess) break;
    int nq = 0, q_of[kCand] = {};
    unsigned long long busy_until[kCand] = {};
    for (int j = 0; j < n_cand; ++j) {
      int q = -1;
      for (int k = 0; k < nq && q < 0; ++k)
        if (h[2 * j] + 300 >= busy_until[k] && h[2 * j] <= busy_until[k] + 800) q = k;  // started 0-8 us after queue k drained
      if (q < 0) q = nq++;
      q_of[j] = q;
      busy_until[q] = h[2 * j + 1];
    }
    if (nq > best_nq) {
      best_nq = nq;
      std::copy(q_of, q_of + kCand, best);
    }
  }
  const int nq = std::max(1, best_nq);
  // exchange: pipe 0 is the context's main stream and stays; a pipe whose queue holds more than its share gives its stream
  // up for a spare one on the queue that holds the fewest
  if (le == hipSuccess && best_nq > 1) {
    int load[kCand] = {};
    bool used[kCand] = {};
    for (int pi = 0; pi < ns; ++pi) load[best[pi]]++;
    for (int pi = ns - 1; pi >= 1; --pi) {
      const int q = best[pi];
      int q_min = 0;
      for (int k = 1; k < nq; ++k)
        if (load[k] < load[q_min]) q_min = k;
      if (load[q] - load[q_min] < 2) continue;
      int k_spare = -1;
      for (int k = ns; k < n_cand && k_spare < 0; ++k)
        if (!used[k] && best[k] == q_min) k_spare = k;
      if (k_spare < 0) continue;
      used[k_spare] = true;
      std::swap(c->pipe[pi].st, spare[k_spare - ns]);
      cand[pi] = c->pipe[pi].st;
      best[pi] = q_min;
      load[q]--;
      load[q_min]++;
    }
  }
  HIP_TRY(le);
  // queue numbers in order of first appearance among the context's streams
  int renum[kCand], n_seen = 0;
  std::fill(renum, renum + kCand, -1);
  for (int pi = 0; pi < ns; ++pi) {
    if (renum[best[pi]] < 0) renum[best[pi]] = n_seen++;
    c->queue_of_pipe[pi] = renum[best[pi]];
  }
  c->n_queues = std::max(1, n_seen);
  // the sampler's unit u runs on stream pipe_order[u]: streams of different queues first, so that as many units as
  // there are queues really run side by side
  int k = 0;
  bool taken[kMaxPipes] = {};
  for (int round = 0; k < c->n_streams; ++round) {
    bool seen[kMaxPipes] = {};
    for (int pi = 0; pi < c->n_streams; ++pi)
      if (!taken[pi] && !seen[c->queue_of_pipe[pi]]) {
        seen[c->queue_of_pipe[pi]] = true;
        taken[pi] = true;
        c->pipe_order[k++] = pi;
      }
  }
  return ABD_OK;
}

int check_chains(abd_ctx* c, int n, const int32_t* chains) {
  if (!c) return fail(ABD_ERR_ARG, "ctx is NULL");
  if (n < 1 || n > c->n_slots) return fail(ABD_ERR_ARG, "n=%d outside [1, n_chain_slots=%d]", n, c->n_slots);
  for (int k = 0; k < n; ++k) {
    if (chains[k] < 0 || chains[k] >= c->n_slots) return fail(ABD_ERR_ARG, "chain %d outside [0, %d)", chains[k], c->n_slots);
    if (!c->slots[chains[k]].set) return fail(ABD_ERR_STATE, "chain slot %d has no discrete state (call abd_set_discrete)", chains[k]);
  }
  return ABD_OK;
}

struct SortedObs {
  std::vector<int64_t> order;  // order[k] = original index
  std::vector<int32_t> ptr;    // (N+1)
  bool one_per_cell = false;
};

int sort_obs(const abd_antigen_obs& o, int G, int N, const char* tag, SortedObs& out) {
  if (o.n_obs < 0) return fail(ABD_ERR_ARG, "%s: negative n_obs", tag);
  if (o.n_obs > 0 && (!o.idx_gap || !o.idx_ind || !o.log_dilution || !o.od)) return fail(ABD_ERR_ARG, "%s: NULL observation array", tag);
  if (o.n_obs >= (int64_t)std::numeric_limits<int32_t>::max()) return fail(ABD_ERR_ARG, "%s: too many observations", tag);
  const int64_t cells = (int64_t)G * N;
  std::vector<int32_t> count((size_t)cells + 1, 0);
  for (int64_t k = 0; k < o.n_obs; ++k) {
    const int64_t g = o.idx_gap[k], j = o.idx_ind[k];
    if (g < 0 || g >= G || j < 0 || j >= N) return fail(ABD_ERR_ARG, "%s: observation %lld has (gap=%lld, ind=%lld) outside (%d, %d)", tag, (long long)k, (long long)g, (long long)j, G, N);
    count[(size_t)(j * G + g) + 1]++;
  }
  out.one_per_cell = o.n_obs == cells;
  for (int64_t cidx = 0; cidx < cells; ++cidx) {
    if (count[(size_t)cidx + 1] != 1) out.one_per_cell = false;
    count[(size_t)cidx + 1] += count[(size_t)cidx];
  }
  out.order.resize((size_t)o.n_obs);
  std::vector<int32_t> cursor(count.begin(), count.end() - 1);
  for (int64_t k = 0; k < o.n_obs; ++k) {
    const int64_t cell = (int64_t)o.idx_ind[k] * G + o.idx_gap[k];
    out.order[(size_t)cursor[(size_t)cell]++] = k;  // stable
  }
  out.ptr.resize((size_t)N + 1);
  for (int j = 0; j <= N; ++j) out.ptr[(size_t)j] = count[(size_t)j * G];
  return ABD_OK;
}

template <typename R>
int upload_antigen(abd_ctx* c, const abd_antigen_obs& o, const SortedObs& so, AntigenDev& d) {
  const size_t K = (size_t)o.n_obs;
  const int G = c->G, N = c->N;
  d.K = o.n_obs;
  if (c->dense) {
    // gap-major panel of {od, log_dilution} pairs: element (g, j) at [g * N + j]
    std::vector<YX<R>> yx((size_t)G * N);
    for (int j = 0; j < N; ++j)
      for (int g = 0; g < G; ++g) {
        const int64_t src = so.order[(size_t)j * G + g];
        yx[(size_t)g * N + j] = YX<R>{(R)o.od[src], (R)o.log_dilution[src]};
      }
    HIP_TRY(d.yx.upload(yx.data(), yx.size() * sizeof(YX<R>)));
    {  // the individual-major copy the sweep kernels read: element (g, j) at [j * G + g]
      std::vector<YX<R>> yxi((size_t)G * N);
      for (int j = 0; j < N; ++j)
        for (int g = 0; g < G; ++g) yxi[(size_t)j * G + g] = yx[(size_t)g * N + j];
      HIP_TRY(d.yxi.upload(yxi.data(), yxi.size() * sizeof(YX<R>)));
    }
    // the split panels of one-chain launches: od alone + one byte per cell coding its log dilution (assays use a handful of
    // dilutions; lossless: the dictionary holds the values of the pair panel, i.e. rounded to the storage type).  Lane-group-major: element (g, j) at
    // [((j / 64) * G + g) * 64 + j % 64], so the rows a wave walks -- 64 individuals, gap after gap -- are one contiguous
    // stream (a 64-byte code row is half a cache line: in gap-major order its other half belongs to the neighbouring lane
    // group and was fetched again by that group's wave, 1.29 x the algorithmic bytes at config 5)
    std::vector<double> dict;
    std::unordered_map<uint64_t, uint8_t> code_of;  // bit pattern of a log dilution -> its code
    const size_t n_lg = ((size_t)N + 63) / 64;
    auto cell_of = [&](size_t g, size_t j) { return ((j / 64) * (size_t)G + g) * 64 + j % 64; };
    std::vector<uint8_t> code(n_lg * (size_t)G * 64, 0);
    bool fits = true;
    for (size_t k = 0; k < K && fits; ++k) {
      const double x = (double)(R)o.log_dilution[k];  // what the pair panel holds: the value in the storage type
      uint64_t bits;
      std::memcpy(&bits, &x, sizeof bits);  // bit-wise: -0.0, NaN payloads stay what they are
      auto it = code_of.find(bits);
      if (it == code_of.end()) {
        if (dict.size() == ABD_XDICT) {
          fits = false;
          break;
        }
        it = code_of.emplace(bits, (uint8_t)dict.size()).first;
        dict.push_back(x);
      }
      code[cell_of((size_t)o.idx_gap[k], (size_t)o.idx_ind[k])] = it->second;
    }
    if (fits) {
      std::vector<R> od(code.size(), (R)0);
      for (size_t j = 0; j < (size_t)N; ++j)
        for (size_t g = 0; g < (size_t)G; ++g) od[cell_of(g, j)] = yx[g * N + j].y;
      d.n_dict = (int)dict.size();
      HIP_TRY(d.od.upload(od.data(), od.size() * sizeof(R)));
      HIP_TRY(d.xc.upload(code.data(), code.size()));
      dict.resize(ABD_XDICT, 0.0);
      HIP_TRY(d.dict.upload(dict.data(), ABD_XDICT));
    }
    return ABD_OK;
  }
  std::vector<R> y(std::max<size_t>(K, 1)), x(std::max<size_t>(K, 1));
  std::vector<uint16_t> g(std::max<size_t>(K, 1));
  std::vector<int32_t> jj(std::max<size_t>(K, 1));
  for (size_t k = 0; k < K; ++k) {
    const int64_t src = so.order[k];
    y[k] = (R)o.od[src];
    x[k] = (R)o.log_dilution[src];
    g[k] = (uint16_t)o.idx_gap[src];
    jj[k] = (int32_t)o.idx_ind[src];
  }
  HIP_TRY(d.j.upload(jj.data(), jj.size()));
  HIP_TRY(d.y.upload(y.data(), y.size() * sizeof(R)));
  HIP_TRY(d.x.upload(x.data(), x.size() * sizeof(R)));
  HIP_TRY(d.g.upload(g.data(), g.size()));
  HIP_TRY(d.ptr.upload(so.ptr.data(), so.ptr.size()));
  return ABD_OK;
}

// (N, G) row-major 0/1 bytes (TiterData.vacs / .pcrpos) -> packed words [nt][N]
std::vector<uint64_t> pack_ng(const int8_t* src, int G, int N, int nt) {
  std::vector<uint64_t> w((size_t)nt * N, 0);
  if (!src) return w;
  for (int j = 0; j < N; ++j)
    for (int g = 0; g < G; ++g)
      if (src[(size_t)j * G + g]) w[(size_t)(g >> 6) * N + j] |= 1ull << (g & 63);
  return w;
}

// ---- abd_create, step by step (each returns ABD_OK or the code of the error it has set)
namespace {

int validate_desc(const abd_desc* d) {
  const int G = d->n_gaps, N = d->n_inds;
  if (G < 2) return fail(ABD_ERR_ARG, "n_gaps must be >= 2 (Beta(1, n_gaps - 1) prior on p), got %d", G);
  if (G > ABD_MAX_GAPS) return fail(ABD_ERR_ARG, "n_gaps=%d exceeds ABD_MAX_GAPS=%d", G, ABD_MAX_GAPS);
  if (N < 1) return fail(ABD_ERR_ARG, "n_inds must be >= 1, got %d", N);
  if ((int64_t)G * N >= (int64_t)1 << 31) return fail(ABD_ERR_ARG, "n_gaps*n_inds too large");
  if (d->n_chain_slots < 1) return fail(ABD_ERR_ARG, "n_chain_slots must be >= 1");
  if (d->storage != ABD_STORE_F64 && d->storage != ABD_STORE_F32) return fail(ABD_ERR_ARG, "unknown storage %d", d->storage);
  if (!d->vacs) return fail(ABD_ERR_ARG, "vacs is NULL");
  // check_splits (abd.py:604-622) -- same conditions, same messages
  if (d->n_splits < 0 || d->n_splits > 2) return fail(ABD_ERR_ARG, "only implemented 1-3 time chunks (0-2 splits)");
  for (int k = 0; k < d->n_splits; ++k)
    if (d->splits[k] < 0) return fail(ABD_ERR_ARG, "split indexes must be positive");
  if (d->n_splits == 2 && d->splits[0] > d->splits[1]) return fail(ABD_ERR_ARG, "splits must be in ascending order");
  if (d->n_splits > 0 && d->splits[d->n_splits - 1] > G) return fail(ABD_ERR_ARG, "largest split must be less than n_gaps - 1, (%d)", d->splits[d->n_splits - 1]);
  if (d->n_splits == 2 && d->splits[0] == d->splits[1]) return fail(ABD_ERR_ARG, "splits not unique");
  for (int64_t k = 0; k < (int64_t)G * N; ++k) {
    if ((d->vacs[k] != 0 && d->vacs[k] != 1)) return fail(ABD_ERR_ARG, "vacs must be 0/1");
    if (d->pcrpos && d->pcrpos[k] != 0 && d->pcrpos[k] != 1) return fail(ABD_ERR_ARG, "pcrpos must be 0/1");
  }
  return ABD_OK;
}

// the cohort's sizes, the device and the context's stream, the kernels' grids (one_per_cell: both antigens fill the panel)
int derive_sizes(abd_ctx* c, const abd_desc* d, bool one_per_cell) {
  const int G = d->n_gaps, N = d->n_inds;
  c->G = G;
  c->N = N;
  c->nt = (G + 63) / 64;
  c->prior_const = prior_constant(G);
  c->n_lg = (N + 63) / 64;
  c->n_chunks = d->n_splits + 1;
  for (int k = 0; k < d->n_splits; ++k) c->splits[k] = d->splits[k];
  c->storage = d->storage;
  c->dense = one_per_cell;
  // the dense kernel addresses the gap rows of a piece (up to G of them) with a 32-bit scalar offset (abd_dense.hpp);
  // beyond 2^28 cells (fp64; 2^29 in fp32 storage) per GPU the cohort takes the observation-list kernels instead
  if ((int64_t)N * (d->storage == ABD_STORE_F32 ? 8 : 16) * (G + 2) >= ((int64_t)1 << 32)) c->dense = false;
  // ... and splits the (lane group, gap) plane by 32-bit arithmetic: row / G by a 32-bit reciprocal must be exact for every
  // row of the plane (abd_types.hpp: abd_div_magic_exact; 6.8 M individuals at 200 gaps -- beyond the limit above anyway)
  if (!abd_div_magic_exact((uint64_t)c->n_lg * (uint64_t)G, (uint32_t)G)) c->dense = false;
  if (env_int("ABD_FORCE_SPARSE", 0)) c->dense = false;
  c->ignore_pcr = d->pcrpos == nullptr;
  c->n_slots = d->n_chain_slots;
  {
    const int edges[4] = {0, d->n_splits > 0 ? d->splits[0] : G, d->n_splits > 1 ? d->splits[1] : G, G};
    for (int ch = 0; ch < c->n_chunks; ++ch) {
      const int lo = edges[ch], hi = (ch == c->n_chunks - 1) ? G : edges[ch + 1];
      for (int g = lo; g < hi; ++g) c->chunk_mask[ch][g >> 6] |= 1ull << (g & 63);
    }
  }

  int dev = d->device;
  if (dev < 0) HIP_TRY(hipGetDevice(&dev));
  c->device = dev;
  HIP_TRY(hipSetDevice(dev));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, dev));
  c->n_cu = prop.multiProcessorCount;
  snprintf(c->name, sizeof c->name, "%s %s %d CUs", prop.name, prop.gcnArchName, prop.multiProcessorCount);
  HIP_TRY(c->pipe[0].st.create());
  c->stream = c->pipe[0].st;

  // sparse kernel: persistent waves, one individual at a time
  const int bpc = std::max(1, tune_int("ABD_BLOCKS_PER_CU", 2));
  const int sparse_max = std::max(1, std::min((N + ABD_WAVES_PER_BLOCK - 1) / ABD_WAVES_PER_BLOCK, c->n_cu * 16));
  c->blocks_x = std::max(1, std::min(sparse_max, c->n_cu * bpc));
  // dense kernel: 4 workgroups per CU = 4 waves per SIMD (<= 128 VGPRs, ~29 KB LDS each): one round, equal ranges
  c->dbpc = std::max(1, tune_int("ABD_DENSE_BLOCKS_PER_CU", 4));
  {
    const int cap = c->n_cu * 8;
    c->ob_n = (int)std::min<int64_t>((d->n.n_obs + ABD_BLOCK - 1) / ABD_BLOCK, cap);
    c->ob_s = (int)std::min<int64_t>((d->s.n_obs + ABD_BLOCK - 1) / ABD_BLOCK, cap);
    c->ob_c = 1;  // one workgroup carries the slot's counters (sum(i_raw), sum(ab_s_waner)) into the sums
    // lane per observation unless the lists are so full that a wave per individual keeps its 64 lanes busy
    // for two rounds or more and amortises the constraint pass (measured crossover, tools/bench_sparse.py)
    c->obs_lanes = d->s.n_obs + d->n.n_obs < (int64_t)256 * N;
    c->obs_lanes = env_int("ABD_OBS_LANES", c->obs_lanes ? 1 : 0) != 0;
  }
  c->blocks_max = std::max({sparse_max, c->n_cu * 16, c->ob_n + c->ob_s + c->ob_c});
  c->dense_blocks = std::min(c->n_cu * c->dbpc, c->blocks_max);
  if (dense_lds_bytes(G, 4) > 160 * 1024) return fail(ABD_ERR_ARG, "LDS tables for n_gaps=%d do not fit", G);
  return ABD_OK;
}

// the read-only panels: both antigens' readings, vaccinations, PCR positives, the 2^(j/1024) table, the upload staging
int upload_panels(abd_ctx* c, const abd_desc* d, SortedObs& so_s, SortedObs& so_n) {
  const int G = c->G, N = c->N;
  const auto upload = c->storage == ABD_STORE_F32 ? upload_antigen<float> : upload_antigen<double>;
  if (int rc = upload(c, d->s, so_s, c->s)) return rc;
  if (int rc = upload(c, d->n, so_n, c->n)) return rc;
  c->order_s = std::move(so_s.order);  // sorted position -> caller's index (abd_eval.hip: scatter_readings)
  c->order_n = std::move(so_n.order);
  c->seg_s = std::move(so_s.ptr);  // (observation lists: the device's copies are s.ptr, n.ptr)
  c->seg_n = std::move(so_n.ptr);
  c->xc_ok = c->dense && c->s.od && c->n.od;
  c->xc_max_cb = tune_int("ABD_XC_MAX_CB", c->xc_max_cb);
  const size_t words = (size_t)c->nt * N;
  const std::vector<uint64_t> vw = pack_ng(d->vacs, G, N, c->nt);
  const std::vector<uint64_t> pw = pack_ng(d->pcrpos, G, N, c->nt);
  HIP_TRY(c->vw.upload(vw.data(), words));
  HIP_TRY(c->pw.upload(pw.data(), words));
  if (c->dense) {
    // 2^(j/1024) rounded once from the 64-bit-mantissa value, stored pre-biased (abd_types.hpp: abd_exp2_prebias)
    std::vector<double> tab(ABD_EXP2_TAB);
    for (int j = 0; j < ABD_EXP2_TAB; ++j) {
      const double t = (double)exp2l((long double)j / (long double)ABD_EXP2_TAB);
      uint64_t bits;
      std::memcpy(&bits, &t, sizeof bits);
      bits = abd_exp2_prebias(bits, j);
      std::memcpy(&tab[(size_t)j], &bits, sizeof bits);
    }
    HIP_TRY(c->exp2_tab.upload(tab.data(), tab.size()));
  }
  HIP_TRY(c->stage_gn.alloc((size_t)G * N));
  return ABD_OK;
}

int create_slots(abd_ctx* c) {
  const size_t words = (size_t)c->nt * c->N;
  c->slots.resize((size_t)c->n_slots);
  for (auto& s : c->slots) {
    HIP_TRY(s.rw.alloc(words));
    HIP_TRY(s.waner.alloc((size_t)c->N));
    HIP_TRY(s.iw.alloc(words));
    HIP_TRY(s.cnt.alloc(2));
    if (c->dense) {
      // the planes: zero (padding gaps, and no infections yet), then the static vaccination masks
      HIP_TRY(s.pl.alloc_zero(abd_plane_words(c->n_lg, c->G), c->stream));
      PlaneArgs a;
      std::memset(&a, 0, sizeof a);
      a.src[0] = c->vw;
      a.dst[0] = s.pl;
      a.N = c->N;
      a.G = c->G;
      a.which = 1;
      hipLaunchKernelGGL(abd_planes_kernel, dim3(c->n_lg, c->nt, 1), dim3(64), 0, c->stream, a);
      HIP_TRY(hipGetLastError());
    }
  }
  c->dense_planes = env_int("ABD_DENSE_PLANES", 1) != 0;
  return ABD_OK;
}

// the pipes with their partial rows, the result rows in mapped host memory, the counters, the streams' hardware queues
int create_pipes(abd_ctx* c) {
  c->n_pipes = std::max(1, std::min(6, env_int("ABD_PIPES", c->n_pipes)));
  if (!c->dense) c->n_pipes = 1;  // only the dense kernel has a grid for sharing the chip; the others just overlap
  c->n_streams = kMaxPipes;
  c->n_sync_slots = std::max(4, c->n_slots);
  for (int pi = 1; pi < c->n_streams; ++pi) {
    HIP_TRY(c->pipe[pi].st.create());
    HIP_TRY(c->join_ev[pi].create(hipEventDisableTiming));
  }
  // a launch that shares the chip with the other pipes' launches gets 1/n_pipes of the workgroup slots: fewer,
  // longer ranges, i.e. less per-range set-up for the same work
  c->pipe_blocks = std::min(c->dense_blocks, c->n_cu * std::max(1, c->dbpc / c->n_pipes));  // measured best: 3 pipes x 1 workgroup per CU
  if (const int pb = tune_int("ABD_PIPE_BLOCKS", 0)) c->pipe_blocks = std::max(1, std::min(pb, c->blocks_max));
  // a sampler unit's launch: one workgroup per CU, whatever the number of units in flight -- a unit's numbers must not depend
  // on it.  256 on gfx950 = ABD_TRAIN_ONE_LEVEL: few enough for the launch to sum its own rows (abd_eval.hip: plan_launch)
  c->group_blocks = c->n_cu;
  if (const int gb = tune_int("ABD_GROUP_BLOCKS_PER_CU", 0)) c->group_blocks = std::max(1, std::min(c->n_cu * gb, c->blocks_max));
  for (int pi = 0; pi < kMaxPipes; ++pi)
    if (c->pipe[pi].st)
      for (int b = 0; b < 2; ++b) HIP_TRY(c->pipe[pi].partials[b].alloc((size_t)c->n_slots * c->blocks_max * ABD_NOUT));
  c->xcd_remap = tune_int("ABD_XCD_REMAP", 1) != 0;
  c->fin_rows = std::max(0, tune_int("ABD_FIN_ROWS", 2));
  // COHERENT (fine-grained) on purpose: synchronous calls poll a completion tag in this memory while the stream
  // is still running.  With hipHostMallocMapped alone the allocation is non-coherent: the GPU caches it and the
  // two 64-byte halves of a result row could reach the host in either order (tag visible, data stale).
  HIP_TRY(c->out.alloc((size_t)(kResultSlots + c->n_sync_slots) * c->n_slots * ABD_NOUT));
  HIP_TRY(c->d_counts.alloc((size_t)c->n_slots * 2 + 8));  // + 8 development counters
  HIP_TRY(c->d_work.alloc((size_t)2 * c->n_slots));
  HIP_TRY(c->d_counts_chain.alloc((size_t)c->n_slots * 2));
  HIP_TRY(c->d_fin_count.alloc_zero((size_t)kMaxPipes * ABD_MAX_BATCH, c->stream));
  HIP_TRY(c->d_train_count.alloc_zero((size_t)kMaxPipes * (1 + ABD_TRAIN_SHARDS) * ABD_TRAIN_CNT_STRIDE, c->stream));
  c->dense_own_sum = env_int("ABD_DENSE_OWN_SUM", 1) != 0;
  HIP_TRY(c->h_counts_chain.alloc_pinned((size_t)c->n_slots * 2));
  c->g2_refill_min = std::max(1, std::min(64, tune_int("ABD_G2_REFILL_MIN", ABD_G2_REFILL_MIN)));
  c->g2_tail_lanes = std::max(0, std::min(64, tune_int("ABD_G2_TAIL_LANES", ABD_G2_TAIL_LANES)));
  c->g2_tail_age = std::max(0, tune_int("ABD_G2_TAIL_AGE", ABD_G2_TAIL_AGE));
  c->results.resize((size_t)kResultSlots + c->n_sync_slots);
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (c->dense && c->n_pipes > 1) {
    // the pipes must sit on different hardware queues (two launches in one queue run one after the other: 4 pipes on
    // streams 0..3, two of which share a queue here, gave 143 k evals/s at config 3 against 192 k on streams 0, 1, 2, 5)
    if (int rc = probe_stream_queues(c)) return rc;
    c->n_pipes = std::min(c->n_pipes, c->n_queues);
  }
  return ABD_OK;
}

}  // namespace

namespace {

// The walk's fields of chain slot `chain` at theta: the only place ChainPar is copied into them
CellWalk cell_walk(const abd_ctx* c, int chain, const double* theta) {
  const ChainPar p = chain_par(c, chain, theta);
  CellWalk w;
  w.vw = c->vw, w.iw = p.iw, w.waner = p.waner, w.last = c->d_last;
  w.rho_n = p.rho_n, w.rho_s = p.rho_s, w.init_n = p.init_n, w.perm_n = p.perm_n, w.temp_n = p.temp_n;
  w.init_s = p.init_s, w.perm_s = p.perm_s;
  w.G = c->G, w.N = c->N, w.nt = c->nt;
  return w;
}

// who takes a workgroup's share of a cell kernel (abd_cells.hpp): a wave an individual, or the workgroup a slab of them.
// Either way at most 8 workgroups per CU, and no result depends on the grid.
enum class CellGrid { Individuals, Slabs };

// One launch of a cell kernel on stream st: `narrow` for cohorts of up to ABD_MAXT words of gaps, `wide` beyond;
// own_lds bytes of dynamic LDS behind the power tables
template <typename K, typename... A>
int launch_cells(const abd_ctx* c, K narrow, K wide, CellGrid grid, size_t own_lds, hipStream_t st, const A&... args) {
  const int shares = grid == CellGrid::Slabs ? abd_curves_slabs(c->N) : (c->N + ABD_WAVES_PER_BLOCK - 1) / ABD_WAVES_PER_BLOCK;
  const int blocks = std::max(1, std::min(shares, c->n_cu * 8));
  HIP_TRY(launch_kernel(c->nt > ABD_MAXT ? wide : narrow, dim3(blocks), dim3(ABD_BLOCK), cell_tables_bytes(c->G) + own_lds, st, args...));
  return ABD_OK;
}

}  // namespace

int launch_deterministics(abd_ctx* c, int chain, const double* theta, hipStream_t st, int8_t* out_i, double* out_mun, double* out_mus,
                          double* sums) {
  return launch_cells(c, abd_deterministics_kernel<ABD_MAXT>, abd_deterministics_kernel<ABD_MAXT_MAX>, CellGrid::Individuals, 0, st,
                      cell_walk(c, chain, theta), out_i, out_mun, out_mus, sums);
}

size_t curves_row_cols(const abd_ctx* c) { return (size_t)abd_curves_row_cols(c->G); }
size_t curves_scratch_cols(const abd_ctx* c) { return (size_t)abd_curves_slabs(c->N) * curves_row_cols(c); }

int launch_curves(abd_ctx* c, int chain, const double* theta, double thr_s, double thr_n, hipStream_t st, unsigned long long* scratch,
                  unsigned long long* row) {
  CurvesArgs a;
  a.w = cell_walk(c, chain, theta);
  a.slab_rows = scratch;
  a.thr_s = thr_s, a.thr_n = thr_n;
  a.n_slabs = abd_curves_slabs(c->N);
  if (int rc = launch_cells(c, abd_curves_kernel<ABD_MAXT>, abd_curves_kernel<ABD_MAXT_MAX>, CellGrid::Slabs, abd_curves_lds_bytes(c->G), st, a))
    return rc;
  const int sum_blocks = (int)((curves_row_cols(c) + ABD_CURVES_SUM_COLS - 1) / ABD_CURVES_SUM_COLS);
  HIP_TRY(launch_kernel(abd_curves_sum_kernel, dim3(sum_blocks), dim3(ABD_CURVES_SUM_PARTS * ABD_CURVES_SUM_COLS), 0, st, scratch, a.n_slabs,
                        c->G, row));
  return ABD_OK;
}

void split_curves_row(const abd_ctx* c, const unsigned long long* row, int64_t* counts, int64_t* n_infections, double* titer_sums) {
  const size_t G = (size_t)c->G;
  if (counts) std::memcpy(counts, row, 4 * G * sizeof(int64_t));
  if (n_infections) std::memcpy(n_infections, row + 4 * G, ABD_CURVES_NBIN * sizeof(int64_t));
  if (titer_sums) std::memcpy(titer_sums, row + 4 * G + ABD_CURVES_NBIN, 2 * G * sizeof(double));
}

int launch_diag(abd_ctx* c, int chain, const double* theta, hipStream_t st, int64_t d, int64_t H, int64_t L, double* tit, uint32_t* inf,
                unsigned long long* cb2) {
  DiagArgs a;
  a.w = cell_walk(c, chain, theta);
  a.tit = tit, a.inf = reinterpret_cast<DiagInf*>(inf), a.cb2 = cb2;
  a.d = diag_draw(d, H, L);
  return launch_cells(c, abd_diag_kernel<ABD_MAXT>, abd_diag_kernel<ABD_MAXT_MAX>, CellGrid::Individuals, 0, st, a);
}

int launch_diag_export(abd_ctx* c, const void* src, int stride, int width, unsigned long long* dst, hipStream_t st) {
  const int64_t tiles = (int64_t)((c->G + ABD_DIAG_TILE - 1) / ABD_DIAG_TILE) * ((c->N + ABD_DIAG_TILE - 1) / ABD_DIAG_TILE);
  hipLaunchKernelGGL(abd_diag_export_kernel, dim3((unsigned)tiles), dim3(256), 0, st, static_cast<const unsigned char*>(src), stride, width,
                     c->G, c->N, dst);
  HIP_TRY(hipGetLastError());
  return ABD_OK;
}

int launch_timeline(abd_ctx* c, int chain, const double* theta, const double range_n[2], const double range_s[2], hipStream_t st,
                    uint32_t* hist_n, uint32_t* hist_s, uint32_t* cell, uint32_t* ninf) {
  TimelineArgs a;
  a.w = cell_walk(c, chain, theta);
  a.hist_n = hist_n, a.hist_s = hist_s, a.cell = reinterpret_cast<TimelineCell*>(cell), a.ninf = ninf;
  a.rn = timeline_range(range_n[0], range_n[1]), a.rs = timeline_range(range_s[0], range_s[1]);
  a.n_splits = c->n_chunks - 1, a.s0 = c->splits[0], a.s1 = c->splits[1];
  return launch_cells(c, abd_timeline_kernel<ABD_MAXT>, abd_timeline_kernel<ABD_MAXT_MAX>, CellGrid::Individuals, 0, st, a);
}

int launch_timeline_hist_export(abd_ctx* c, const uint32_t* src, int g0, int n_g, void* dst, hipStream_t st) {
  const int64_t cells = (int64_t)n_g * c->N;  // 32 per pass of a workgroup
  const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((cells + 31) / 32, (int64_t)c->n_cu * 16));
  hipLaunchKernelGGL(abd_timeline_hist_export_kernel, dim3(blocks), dim3(256), 0, st, reinterpret_cast<const uint4*>(src), c->G, c->N, g0,
                     n_g, static_cast<uint4*>(dst));
  HIP_TRY(hipGetLastError());
  return ABD_OK;
}

int launch_timeline_quantiles(abd_ctx* c, const uint32_t* hist, int64_t chain_stride, int n_chains, const double range[2], int n_q,
                              const double* q, double* out, hipStream_t st) {
  const int64_t tiles = (int64_t)((c->G + ABD_TL_QTILE - 1) / ABD_TL_QTILE) * ((c->N + ABD_TL_QTILE - 1) / ABD_TL_QTILE);
  hipLaunchKernelGGL(abd_timeline_quantile_kernel, dim3((unsigned)tiles), dim3(256), 0, st, hist, chain_stride, n_chains, c->G, c->N,
                     timeline_range(range[0], range[1]), n_q, q, out);
  HIP_TRY(hipGetLastError());
  return ABD_OK;
}

size_t risk_table_cols(const abd_ctx* c) { return (size_t)abd_risk_table_cols(c->G); }
size_t risk_scratch_cols(const abd_ctx* c) { return (size_t)abd_curves_slabs(c->N) * (size_t)abd_risk_packed_cols(c->G); }

int check_risk_spec(const abd_ctx* c, const abd_risk_spec* spec) {
  if (!spec) return fail(ABD_ERR_ARG, "risk: spec is NULL");
  if (spec->start < 0 || spec->end > c->G || (int64_t)spec->end - spec->start < 2)
    return fail(ABD_ERR_ARG, "risk: window (%d, %d) needs 0 <= start, end <= %d and end - start >= 2", spec->start, spec->end, c->G);
  if (spec->first_only != 0 && spec->first_only != 1) return fail(ABD_ERR_ARG, "risk: first_only=%d is not 0 or 1", spec->first_only);
  const struct { const char* name; int n; const double* e; } ag[2] = {{"edges_s", spec->n_edges_s, spec->edges_s},
                                                                     {"edges_n", spec->n_edges_n, spec->edges_n}};
  for (const auto& x : ag) {
    if (x.n < 0 || x.n > ABD_RISK_MAX_EDGES) return fail(ABD_ERR_ARG, "risk: n_%s=%d outside [0, %d]", x.name, x.n, ABD_RISK_MAX_EDGES);
    for (int k = 0; k < x.n; ++k) {
      if (!std::isfinite(x.e[k])) return fail(ABD_ERR_ARG, "risk: %s[%d] is not finite", x.name, k);
      if (k && !(x.e[k] > x.e[k - 1])) return fail(ABD_ERR_ARG, "risk: %s is not strictly ascending at [%d]", x.name, k);
    }
  }
  return ABD_OK;
}

int launch_risk(abd_ctx* c, int chain, const double* theta, const abd_risk_spec& spec, hipStream_t st, unsigned long long* scratch,
                uint32_t* table) {
  RiskArgs a;
  a.w = cell_walk(c, chain, theta);
  a.slab_rows = scratch;
  for (int k = 0; k < ABD_RISK_MAX_EDGES; ++k) {
    a.edges_s[k] = k < spec.n_edges_s ? spec.edges_s[k] : HUGE_VAL;
    a.edges_n[k] = k < spec.n_edges_n ? spec.edges_n[k] : HUGE_VAL;
  }
  a.n_slabs = abd_curves_slabs(c->N);
  a.start = spec.start, a.end = spec.end, a.first_only = spec.first_only;
  if (int rc = launch_cells(c, abd_risk_kernel<ABD_MAXT>, abd_risk_kernel<ABD_MAXT_MAX>, CellGrid::Slabs, abd_risk_lds_bytes(c->G), st, a))
    return rc;
  const int sum_blocks = (int)((abd_risk_packed_cols(c->G) + ABD_RISK_SUM_COLS - 1) / ABD_RISK_SUM_COLS);
  HIP_TRY(launch_kernel(abd_risk_sum_kernel, dim3(sum_blocks), dim3(ABD_RISK_SUM_PARTS * ABD_RISK_SUM_COLS), 0, st, scratch, a.n_slabs, c->G,
                        table));
  return ABD_OK;
}

int launch_unpack(abd_ctx* c, int chain, int8_t* dst, hipStream_t st) {
  dim3 grid((c->N + 255) / 256, c->G);
  hipLaunchKernelGGL(abd_unpack_bits_kernel, grid, dim3(256), 0, st, c->slots[(size_t)chain].rw, dst, c->G, c->N);
  HIP_TRY(hipGetLastError());
  return ABD_OK;
}

}  // namespace abdi

// Quiesce: nothing on the context's streams may still use a member when the members go (abd_host.hpp)
abd_ctx::~abd_ctx() {
  (void)hipSetDevice(device);
  for (Pipe& p : pipe)
    if (p.st) (void)hipStreamSynchronize(p.st);
}

extern "C" {

const char* abd_version(void) { return "abdpymc_amd hip gfx950 0.2"; }

const char* abd_last_error(void) { return last_error(); }

int abd_create(const abd_desc* d, abd_ctx** out) {
  if (!d || !out) return fail(ABD_ERR_ARG, "desc / out is NULL");
  *out = nullptr;
  if (int rc = validate_desc(d)) return rc;
  SortedObs so_s, so_n;
  if (int rc = sort_obs(d->s, d->n_gaps, d->n_inds, "s", so_s)) return rc;
  if (int rc = sort_obs(d->n, d->n_gaps, d->n_inds, "n", so_n)) return rc;
  std::unique_ptr<abd_ctx> c(new (std::nothrow) abd_ctx());  // every early return below releases the half-built context
  if (!c) return fail(ABD_ERR_NOMEM, "out of host memory");
  if (int rc = derive_sizes(c.get(), d, so_s.one_per_cell && so_n.one_per_cell)) return rc;
  if (int rc = upload_panels(c.get(), d, so_s, so_n)) return rc;
  if (int rc = create_slots(c.get())) return rc;
  if (int rc = create_pipes(c.get())) return rc;
  *out = c.release();
  return ABD_OK;
}

int abd_destroy(abd_ctx* c) {
  delete c;
  return ABD_OK;
}

int abd_device_name(abd_ctx* c, char* buf, int32_t buflen) {
  if (!c || !buf || buflen < 1) return fail(ABD_ERR_ARG, "bad argument");
  snprintf(buf, (size_t)buflen, "%s", c->name);
  return ABD_OK;
}

int abd_is_dense(abd_ctx* c) { return c && c->dense ? 1 : 0; }
int abd_n_pipes(abd_ctx* c) { return c ? c->n_pipes : -1; }

int abd_set_discrete(abd_ctx* c, int32_t chain, const int8_t* i_raw, const int8_t* waner) {
  if (!c || !i_raw || !waner) return fail(ABD_ERR_ARG, "NULL argument");
  if (chain < 0 || chain >= c->n_slots) return fail(ABD_ERR_ARG, "chain %d outside [0, %d)", chain, c->n_slots);
  const size_t cells = (size_t)c->G * c->N;
  for (size_t k = 0; k < cells; ++k)
    if (i_raw[k] != 0 && i_raw[k] != 1) return fail(ABD_ERR_ARG, "i_raw must be 0/1");
  for (int j = 0; j < c->N; ++j)
    if (waner[j] != 0 && waner[j] != 1) return fail(ABD_ERR_ARG, "ab_s_waner must be 0/1");
  HIP_TRY(hipSetDevice(c->device));
  ChainSlot& s = c->slots[(size_t)chain];
  long long* const cnt = s.cnt;
  // synchronous copies: the caller's buffers may be reused immediately
  if (int jrc = join_pipes(c)) return jrc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipMemcpy(c->stage_gn, i_raw, cells, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(s.waner, waner, (size_t)c->N, hipMemcpyHostToDevice));
  dim3 grid((c->N + 255) / 256, c->nt);
  hipLaunchKernelGGL(abd_pack_bits_kernel, grid, dim3(256), 0, c->stream, c->stage_gn, s.rw, c->G, c->N, c->nt);
  HIP_TRY(hipGetLastError());
  // what the slot keeps beside the raw state: constrained words, sum(i_raw), sum(ab_s_waner)
  HIP_TRY(hipMemsetAsync(s.cnt, 0, 2 * sizeof(long long), c->stream));
  if (c->nt > ABD_MAXT)
    hipLaunchKernelGGL(abd_constrain_kernel<ABD_MAXT_MAX>, dim3((c->N + 255) / 256), dim3(256), 0, c->stream, constrain_args(c), s.rw,
                       s.waner, s.iw, reinterpret_cast<unsigned long long*>(cnt));
  else
    hipLaunchKernelGGL(abd_constrain_kernel<ABD_MAXT>, dim3((c->N + 255) / 256), dim3(256), 0, c->stream, constrain_args(c), s.rw,
                       s.waner, s.iw, reinterpret_cast<unsigned long long*>(cnt));
  HIP_TRY(hipGetLastError());
  if (int prc = enqueue_planes(c, 1, &chain, c->stream)) return prc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  s.set = true;
  return ABD_OK;
}

int abd_flip_discrete(abd_ctx* c, int32_t chain, int64_t flat) {
  if (!c) return fail(ABD_ERR_ARG, "ctx is NULL");
  if (chain < 0 || chain >= c->n_slots) return fail(ABD_ERR_ARG, "chain %d outside [0, %d)", chain, c->n_slots);
  const int64_t total = (int64_t)c->G * c->N + c->N;
  if (flat < 0 || flat >= total) return fail(ABD_ERR_ARG, "flat index %lld outside [0, %lld)", (long long)flat, (long long)total);
  if (!c->slots[(size_t)chain].set) return fail(ABD_ERR_STATE, "chain slot %d has no discrete state", chain);
  HIP_TRY(hipSetDevice(c->device));
  if (int jrc = join_pipes(c)) return jrc;
  ChainSlot& s = c->slots[(size_t)chain];
  long long* const cnt = s.cnt;
  if (c->nt > ABD_MAXT)
    hipLaunchKernelGGL(abd_flip_kernel<ABD_MAXT_MAX>, dim3(1), dim3(1), 0, c->stream, constrain_args(c), s.rw, s.waner, s.iw,
                       reinterpret_cast<unsigned long long*>(cnt), c->G, flat);
  else
    hipLaunchKernelGGL(abd_flip_kernel<ABD_MAXT>, dim3(1), dim3(1), 0, c->stream, constrain_args(c), s.rw, s.waner, s.iw,
                       reinterpret_cast<unsigned long long*>(cnt), c->G, flat);
  HIP_TRY(hipGetLastError());
  // (a flip of i_raw may move any constrained bit of its individual: that individual's lane group, every word)
  if (flat < (int64_t)c->G * c->N)
    if (int prc = enqueue_planes(c, 1, &chain, c->stream, (int)((flat % c->N) / 64), 1)) return prc;
  return ABD_OK;
}
int abd_deterministics(abd_ctx* c, int32_t chain, const double* theta, int8_t* i, double* mu_n, double* mu_s) {
  if (!c || !theta) return fail(ABD_ERR_ARG, "NULL argument");
  int rc = check_chains(c, 1, &chain);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if (int jrc = join_pipes(c)) return jrc;
  const size_t cells = (size_t)c->G * c->N;
  if (!c->d_det) HIP_TRY(c->d_det.alloc(2 * cells + (cells + 7) / 8));  // staging, kept for the next draw
  double* d_n = c->d_det;
  double* d_s = c->d_det + cells;
  int8_t* d_i = reinterpret_cast<int8_t*>(c->d_det + 2 * cells);
  if (int lrc = launch_deterministics(c, chain, theta, c->stream, i ? d_i : (int8_t*)nullptr, mu_n ? d_n : (double*)nullptr,
                                      mu_s ? d_s : (double*)nullptr, nullptr))
    return lrc;
  if (mu_n) HIP_TRY(hipMemcpyAsync(mu_n, d_n, cells * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (mu_s) HIP_TRY(hipMemcpyAsync(mu_s, d_s, cells * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (i) HIP_TRY(hipMemcpyAsync(i, d_i, cells, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return ABD_OK;
}

int abd_set_follow_up(abd_ctx* c, const int32_t* last_gap) {
  if (!c) return fail(ABD_ERR_ARG, "ctx is NULL");
  if (last_gap)
    for (int j = 0; j < c->N; ++j)
      if (last_gap[j] < -1 || last_gap[j] >= c->G)
        return fail(ABD_ERR_ARG, "last_gap[%d]=%d outside [-1, %d)", j, last_gap[j], c->G);
  HIP_TRY(hipSetDevice(c->device));
  if (int jrc = join_pipes(c)) return jrc;
  HIP_TRY(hipStreamSynchronize(c->stream));  // (a queued abd_curves launch may still read the old array)
  if (!last_gap) {
    c->d_last.reset();
    return ABD_OK;
  }
  DevBuf<int32_t> fresh;  // (the old follow-up stays if this one cannot be stored)
  HIP_TRY(fresh.upload(last_gap, (size_t)c->N));
  c->d_last = std::move(fresh);
  return ABD_OK;
}

int abd_curves(abd_ctx* c, int32_t chain, const double* theta, double thr_s, double thr_n, int64_t* counts, int64_t* n_infections,
               double* titer_sums) {
  if (!c || !theta) return fail(ABD_ERR_ARG, "NULL argument");
  int rc = check_chains(c, 1, &chain);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if (int jrc = join_pipes(c)) return jrc;
  const size_t n_scratch = curves_scratch_cols(c), n_row = curves_row_cols(c);
  if (!c->d_curves) HIP_TRY(c->d_curves.alloc(n_scratch + n_row));  // kept for the next call
  if (int lrc = launch_curves(c, chain, theta, thr_s, thr_n, c->stream, c->d_curves, c->d_curves + n_scratch)) return lrc;
  std::vector<unsigned long long> h(n_row);
  HIP_TRY(hipMemcpyAsync(h.data(), c->d_curves + n_scratch, n_row * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  split_curves_row(c, h.data(), counts, n_infections, titer_sums);
  return ABD_OK;
}

int abd_risk(abd_ctx* c, int32_t chain, const double* theta, const abd_risk_spec* spec, int64_t* table) {
  if (!c || !theta || !table) return fail(ABD_ERR_ARG, "NULL argument");
  int rc = check_chains(c, 1, &chain);
  if (rc) return rc;
  if (int src = check_risk_spec(c, spec)) return src;
  HIP_TRY(hipSetDevice(c->device));
  if (int jrc = join_pipes(c)) return jrc;
  const size_t n_scratch = risk_scratch_cols(c), n_tab = risk_table_cols(c);
  if (!c->d_risk) HIP_TRY(c->d_risk.alloc(n_scratch + (n_tab + 1) / 2));  // kept for the next call
  uint32_t* d_tab = reinterpret_cast<uint32_t*>(c->d_risk + n_scratch);
  if (int lrc = launch_risk(c, chain, theta, *spec, c->stream, c->d_risk, d_tab)) return lrc;
  std::vector<uint32_t> h(n_tab);
  HIP_TRY(hipMemcpyAsync(h.data(), d_tab, n_tab * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (size_t e = 0; e < n_tab; ++e) table[e] = (int64_t)h[e];
  return ABD_OK;
}

int abd_get_discrete(abd_ctx* c, int32_t chain, int8_t* i_raw, int8_t* waner) {
  if (!c) return fail(ABD_ERR_ARG, "ctx is NULL");
  int rc = check_chains(c, 1, &chain);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if (int jrc = join_pipes(c)) return jrc;
  ChainSlot& s = c->slots[(size_t)chain];
  if (i_raw) {
    if (int urc = launch_unpack(c, chain, c->stage_gn, c->stream)) return urc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(i_raw, c->stage_gn, (size_t)c->G * c->N, hipMemcpyDeviceToHost));
  } else {
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  if (waner) HIP_TRY(hipMemcpy(waner, s.waner, (size_t)c->N, hipMemcpyDeviceToHost));
  return ABD_OK;
}

int abd_set_launch_config(abd_ctx* c, int32_t blocks, int32_t chains_per_wave) {
  if (!c) return fail(ABD_ERR_ARG, "ctx is NULL");
  if (!(chains_per_wave == 0 || chains_per_wave == 1 || chains_per_wave == 2 || chains_per_wave == 4))
    return fail(ABD_ERR_ARG, "chains_per_wave must be 0 (auto), 1, 2 or 4");
  c->cpw_forced = chains_per_wave;
  if (blocks > 0) {
    if (c->dense)
      c->dense_blocks = std::max(1, std::min(blocks, c->blocks_max));
    else
      c->blocks_x = std::max(1, std::min(blocks, c->blocks_max));
  }
  return ABD_OK;
}

int abd_theta_prior(abd_ctx* c, const double* theta, double* logp, double* grad) {
  if (!c || !theta || !logp) return fail(ABD_ERR_ARG, "NULL argument");
  *logp = priors(prepare(theta), theta, c->G, 0.0, 0.0, 0.0, 0.0, grad, c->prior_const);
  return ABD_OK;
}

int abd_set_individual_offset(abd_ctx* c, int64_t first_individual) {
  if (!c) return fail(ABD_ERR_ARG, "ctx is NULL");
  if (first_individual < 0 || first_individual > 0xFFFFFFFFll) return fail(ABD_ERR_ARG, "first_individual=%lld out of range", (long long)first_individual);
  c->ind_offset = (uint32_t)first_individual;
  return ABD_OK;
}
int abd_stream_queues(abd_ctx* c, int32_t* queue_of_stream, int32_t n) {
  if (!c || !queue_of_stream) return fail(ABD_ERR_ARG, "NULL argument");
  if (int rc = probe_stream_queues(c)) return rc;
  for (int i = 0; i < n; ++i) queue_of_stream[i] = i < c->n_streams ? c->queue_of_pipe[i] : -1;
  return ABD_OK;
}

int64_t abd_algorithmic_bytes(abd_ctx* c, int32_t n_chains) {
  if (!c) return 0;
  const int64_t R = c->storage == ABD_STORE_F32 ? 4 : 8;
  const int64_t cells = (int64_t)c->G * c->N;
  // indicator panels are bit-packed in 64-gap words: vacs + pcrpos + one i_raw per chain, plus the waner bytes
  const int64_t bits = (int64_t)c->nt * c->N * 8 * (2 + n_chains) + (int64_t)n_chains * c->N;
  // one chain per launch reads the split panels (od + a one-byte dilution code per cell and antigen) where they exist
  const int cpw = n_chains % 4 == 0 ? 4 : (n_chains % 2 == 0 ? 2 : 1);  // abd_eval.hip: pick_cpw
  if (c->dense && c->xc_ok && cpw <= c->xc_max_cb) return cells * 2 * (R + 1) + bits;
  if (c->dense) return cells * 4 * R + bits;
  return (c->s.K + c->n.K) * (2 * R + 2) + 2 * (int64_t)(c->N + 1) * 4 + bits;
}

}  // extern "C"
