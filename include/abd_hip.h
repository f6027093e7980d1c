/*
 * abd_hip.h -- C ABI of the MI355X-native abdpymc joint log-probability hot path.
 *
 * This is the drop-in boundary for ONE path of davipatti/abdpymc: the joint logp (+ gradient) of the
 * antibody-dynamics model built by abdpymc.model() (reference abdpymc/abd.py:396-442) and evaluated by
 * PyMC's two compiled callables inside pm.sample() (reference call site abd.py:922):
 *
 *   Model.compile_logp()            point -> scalar logp          -> abd_logp
 *   Model.logp_dlogp_function()     theta[17] -> (logp, grad[17]) -> abd_logp_dlogp / _batch
 *   pm.Deterministic "i", "ab_n_mu", "ab_s_mu" (abd.py:649/667, 341, 389-391) -> abd_deterministics
 *
 * Plain C: pointers and sizes only.  The caller owns every host buffer passed in or out; the library
 * copies inputs at abd_create / abd_set_discrete and owns all device memory until abd_destroy.
 * Every function returns 0 on success and a negative abd_status on error; the message is available from
 * abd_last_error().  Numerical out-of-range (e.g. exp overflow of a sigma) is NOT an error: logp comes
 * back -inf / nan with status 0, as PyMC signals it (NUTS marks a divergence).
 *
 * theta layout (17 doubles, PyMC value variables in creation order; abd.py:424, 329-340, 367-388, 464-467):
 *   0 p_logodds__          1 ab_n_perm_log__     2 ab_n_temp_log__     3 ab_n_rho_logodds__   4 ab_n_init
 *   5 ab_s_perm_log__      6 ab_s_rho_logodds__  7 ab_s_p_waner_logodds__
 *   8 ab_s_tempinf_log__   9 ab_s_tempvac_log__  10 ab_s_init
 *   11 it_n_b  12 it_n_d  13 it_n_sigma_log__    14 it_s_b  15 it_s_d  16 it_s_sigma_log__
 */
#ifndef ABD_HIP_H
#define ABD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ABD_N_THETA 17
/* Limit of this library that the reference does not have: abdpymc takes any n_gaps (abd.py:101, 224-239); here the
 * kernels that hold an individual's gap axis in registers (observation lists, the sweep, the Deterministics) are built
 * for 4 and for 8 packed 64-bit words, so n_gaps <= 512 (abd_create refuses more with ABD_ERR_ARG; the dense evaluation
 * kernel reads words on demand and has no such limit of its own).  The reference's cohorts have 26 / 31 monthly gaps,
 * BASELINE's synthetic ones 60 / 200. */
#define ABD_MAX_GAPS 512
#define ABD_MAX_BATCH 16  /* chains per kernel launch (larger batches are split) */

typedef enum {
  ABD_OK = 0,
  ABD_ERR_ARG = -1,     /* bad argument (maps to ValueError in the Python mirror)            */
  ABD_ERR_HIP = -2,     /* HIP runtime failure; message carries hipGetErrorString             */
  ABD_ERR_STATE = -3,   /* e.g. logp on a chain slot whose discrete state was never set       */
  ABD_ERR_NOMEM = -4
} abd_status;

typedef enum { ABD_STORE_F64 = 0, ABD_STORE_F32 = 1 } abd_storage;

/* One antigen's observation list = reference AntigenTiterData (abd.py:22-43): OD readings gathered out
 * of the (gap, ind) titer matrix by mu[idx_gap, idx_ind] (abd.py:343, 393).  Any order; the library
 * sorts by (ind, gap) and detects the dense-panel case (exactly one reading in every cell). */
typedef struct {
  int64_t n_obs;
  const int32_t* idx_gap;      /* df.elapsed_months   abd.py:35 */
  const int32_t* idx_ind;      /* df.individual_i     abd.py:36 */
  const double* log_dilution;  /* abd.py:462 */
  const double* od;            /* abd.py:468 */
} abd_antigen_obs;

/* Everything abd.model(data, splits, ignore_pcrpos) closes over (abd.py:396-442). */
typedef struct {
  int32_t n_gaps;              /* G  = TiterData.n_gaps (abd.py:101); Beta prior of p uses it (abd.py:424) */
  int32_t n_inds;              /* N  = TiterData.n_inds (abd.py:102) */
  int32_t n_splits;            /* 0, 1 or 2 (abd.py:865-882) */
  int32_t splits[2];           /* ascending gap indexes, check_splits rules (abd.py:604-622) */
  int32_t storage;             /* abd_storage: precision the OD / log_dilution panels are HELD in on the device */
  int32_t n_chain_slots;       /* independent (i_raw, waner) states resident at once */
  int32_t device;              /* HIP device ordinal; <0 = current device */
  abd_antigen_obs s;           /* measurement '10222020-S' (abd.py:85) */
  abd_antigen_obs n;           /* measurement '40588-V08B' (abd.py:94) */
  const int8_t* vacs;          /* (N, G) row-major 0/1 = TiterData.vacs   (abd.py:114) */
  const int8_t* pcrpos;        /* (N, G) row-major 0/1 = TiterData.pcrpos (abd.py:115); NULL = ignore_pcrpos (abd.py:416-418) */
} abd_desc;

typedef struct abd_ctx abd_ctx;

/* Library identity / build info (static string). */
const char* abd_version(void);

/* Last error message of the calling thread (never NULL). */
const char* abd_last_error(void);

/* Build a context: validates like the reference (same conditions as abd.py:196-197, 604-622),
 * sorts + uploads the observation panels, allocates chain slots.  Lazily initialises HIP on first call
 * in the process (fork-safe: nothing touches the device at load time). */
int abd_create(const abd_desc* desc, abd_ctx** out);
int abd_destroy(abd_ctx* ctx);

/* Device description, e.g. "AMD Instinct MI355X gfx950 256 CUs". */
int abd_device_name(abd_ctx* ctx, char* buf, int32_t buflen);

/* Replace chain slot `chain`'s discrete state: i_raw is (G, N) row-major exactly as PyMC holds the
 * value variable "i_raw" (dims gap, ind; abd.py:427); waner is (N,) = "ab_s_waner" (abd.py:373).
 * Values must be 0/1. */
int abd_set_discrete(abd_ctx* ctx, int32_t chain, const int8_t* i_raw, const int8_t* waner);

/* Flip one bit of the resident discrete state without re-uploading it (what BinaryGibbsMetropolis does
 * between two logp calls).  flat < G*N addresses i_raw.ravel(); flat >= G*N addresses waner[flat-G*N]. */
int abd_flip_discrete(abd_ctx* ctx, int32_t chain, int64_t flat);

/* Read the resident discrete state of `chain` back: i_raw (G, N) and waner (N,), either may be NULL. */
int abd_get_discrete(abd_ctx* ctx, int32_t chain, int8_t* i_raw, int8_t* waner);

/* One binary Gibbs-Metropolis sweep over [i_raw, ab_s_waner] of each listed chain, in place, at theta
 * (n x 17): what PyMC's BinaryGibbsMetropolis.astep does to these two variables inside pm.sample
 * (abd.py:922) -- every dim proposed with probability 0.8 in a uniformly random order, Metropolis
 * acceptance on the joint logp -- using the fact that a flip only changes its own individual's terms.
 * Randomness is Philox4x32-10 keyed by (seed, sweep) with the chain's slot id in the counter: a chain's sweep
 * does not depend on which other chains are listed.  accepted / proposed (n each) may be NULL. */
int abd_gibbs_sweep(abd_ctx* ctx, int32_t n, const int32_t* chains, const double* theta, uint64_t seed,
                    uint32_t sweep, int64_t* accepted, int64_t* proposed);

/* The same sweep with a decision log, for tests: one record per proposal, in the individual's order, holding what the kernel
 * decided with.  It leaves the slot in exactly the state abd_gibbs_sweep does (same decisions, bit for bit) but runs a
 * logging instantiation of the kernel, so it is not the call to time.
 *   value     what was compared with log u: the log-ratio delta -- except on ABD_GIBBS_PATH_EARLY, where the walk over the gaps
 *             stopped at `stop` because the BOUND  prior - (current terms of gaps >= gf) + (new terms of gaps [gf, stop))
 *             had fallen below log u: value is that bound, and delta <= value
 *   log_u     the log of the acceptance uniform as the kernel computed it
 *   dim       0 .. G-1: i_raw[dim, individual]; G: ab_s_waner[individual]
 *   gf        dense panels: the first gap whose constrained infection the flip changes (0 for the ab_s_waner flip); -1: none
 *   stop      dense panels: the evaluation covered gaps [gf, stop); -1 where there was none
 *   path      ABD_GIBBS_PATH_*
 *   accepted  0 / 1
 * records: n x capacity, capacity >= n_inds * (n_gaps + 1) records per chain; the records of individual j of chain k start at
 * records[k * capacity + j * (n_gaps + 1)] and n_records[k * n_inds + j] of them are written (the rest is zero). */
enum {
  ABD_GIBBS_PATH_PRIOR = 1,          /* dense: the constrained infections do not change, the prior alone decides      */
  ABD_GIBBS_PATH_EARLY = 2,          /* dense: a lane's walk, stopped before the last gap (value is the bound)       */
  ABD_GIBBS_PATH_WALK = 3,           /* dense: a lane's walk to the last gap                                          */
  ABD_GIBBS_PATH_TAIL = 4,           /* dense: a lane's walk finished by the whole wave                               */
  ABD_GIBBS_PATH_WAVE_WANER = 5,     /* dense: whole-wave evaluation, the ab_s_waner flip                             */
  ABD_GIBBS_PATH_WAVE_OVERFLOW = 6,  /* dense: whole-wave evaluation, more new infections than a lane holds           */
  ABD_GIBBS_PATH_LIST = 7,           /* observation lists: the constrained state changed                              */
  ABD_GIBBS_PATH_LIST_PRIOR = 8      /* observation lists: it did not, the prior alone decides                        */
};
typedef struct {
  double value;
  double log_u;
  int16_t dim;
  int16_t gf;
  int16_t stop;
  uint8_t path;
  uint8_t accepted;
} abd_gibbs_record;
int abd_gibbs_sweep_log(abd_ctx* ctx, int32_t n, const int32_t* chains, const double* theta, uint64_t seed,
                        uint32_t sweep, int64_t* accepted, int64_t* proposed, abd_gibbs_record* records, int64_t capacity,
                        int32_t* n_records);

/* Scalar joint logp at (theta, resident discrete state of `chain`).  Replaces Model.compile_logp()'s
 * point function (a17). */
int abd_logp(abd_ctx* ctx, int32_t chain, const double* theta, double* logp);

/* logp and d logp / d theta.  Replaces Model.logp_dlogp_function() (a18). */
int abd_logp_dlogp(abd_ctx* ctx, int32_t chain, const double* theta, double* logp, double* grad);

/* Only the part of the joint logp that reads the OD panels -- the two observed Normal terms "it_n_lik",
 * "it_s_lik" (abd.py:459-469) -- and its gradient w.r.t. theta (entries the data term does not depend on
 * are 0).  For callers that keep the priors in PyMC and attach this as a pm.Potential. */
int abd_loglik_dlogp(abd_ctx* ctx, int32_t chain, const double* theta, double* loglik, double* grad);

/* n evaluations in as few launches as possible: chains[k] in [0, n_chain_slots), theta is n x 17,
 * logp n, grad n x 17.  The shared OD panels are read once per launch for all chains in it. */
int abd_logp_dlogp_batch(abd_ctx* ctx, int32_t n, const int32_t* chains, const double* theta,
                         double* logp, double* grad);

/* Stream-ordered form: enqueue returns as soon as the launch is queued; results land in result slot
 * `slot` (0 <= slot < abd_n_result_slots) and are read back with abd_fetch after abd_wait.
 * A NUTS driver that runs several chain groups uses this to overlap host work with the device.
 * Dense cohorts: consecutive enqueued launches rotate over up to four HIP streams that sit on different hardware
 * queues (measured at abd_create; launch k+4 sums launch k's partials), each with a quarter of the workgroups of a
 * synchronous launch, so four share the chip instead of one draining it between launches; abd_wait joins them.
 * Synchronous calls may be interleaved: they use rows of their own and leave every result slot alone.
 * Each form is bit-reproducible; the two forms use different launch shapes and agree to rounding (~1e-15). */
int abd_n_result_slots(abd_ctx* ctx);
int abd_logp_dlogp_batch_enqueue(abd_ctx* ctx, int32_t slot, int32_t n, const int32_t* chains,
                                 const double* theta);
int abd_wait(abd_ctx* ctx);
int abd_fetch(abd_ctx* ctx, int32_t slot, double* logp, double* grad);
/* abd_fetch for several slots in one call; outputs are concatenated in the order of `slots`. */
int abd_fetch_many(abd_ctx* ctx, int32_t n_slots, const int32_t* slots, double* logp, double* grad);
/* n_steps independent evaluations of the same chains in one call: theta is n_steps x n x 17, logp n_steps x n, grad
 * n_steps x n x 17 (NULL: logp only).  The stream-ordered form end to end -- enqueue every step, wait once, fetch --
 * for callers that hold many points at once (tempering, particle methods, a benchmark); result slots 0 .. are used.
 * Dense cohorts: the call has every theta in hand, so a launch carries up to four consecutive steps (at most 16 rows of
 * chains; how many depends on n_steps, n and the number of streams only), each step on a quarter of the ranges: the
 * per-range work of the kernel is paid once for the four.  Repeatable bit for bit; against single enqueued steps the
 * ranges differ, so the sums agree to rounding (~1e-15).  The call hands every result over itself and leaves none behind
 * in the result slots: abd_fetch of a slot is for what abd_logp_dlogp_batch_enqueue put there. */
int abd_logp_dlogp_many(abd_ctx* ctx, int32_t n_steps, int32_t n, const int32_t* chains, const double* theta,
                        double* logp, double* grad);

/* The three recorded Deterministics for chain slot `chain` at theta, each (G, N) row-major as PyMC
 * stores them (dims gap, ind).  Any output pointer may be NULL. */
int abd_deterministics(abd_ctx* ctx, int32_t chain, const double* theta, int8_t* i, double* ab_n_mu,
                       double* ab_s_mu);

/* The epidemic curves of one draw: the Deterministics of chain slot `chain` at theta reduced over the individuals on the
 * device.  last_gap[j] in [-1, G-1] is the end of individual j's follow-up (its last serum sample; -1: never followed) and
 * cell (g, j) is FOLLOWED iff g <= last_gap[j].
 *   counts [4][G]       row 0 infected       #{j followed at g: i[g, j] = 1}
 *                       row 1 ever_infected  #{j followed at g: i[g', j] = 1 for some g' <= g}
 *                       row 2 seropos_s      #{j followed at g: ab_s_mu[g, j] >= thr_s}
 *                       row 3 seropos_n      #{j followed at g: ab_n_mu[g, j] >= thr_n}
 *   n_infections [8]    entry k: individuals with last_gap[j] >= 0 that have exactly k infections in gaps 0 .. last_gap[j];
 *                       entry 7: 7 or more
 *   titer_sums [2][G]   row 0 the sum over the followed j of ab_s_mu[g, j], row 1 of ab_n_mu[g, j] (the caller divides by the
 *                       number followed, which depends on last_gap alone)
 * i, ab_s_mu, ab_n_mu are exactly what abd_deterministics returns.  thr_s, thr_n are on the titer scale; +inf switches a
 * count off.  Any output may be NULL.  A result depends on (N, G, last_gap, the slot's state, theta, the thresholds) only and
 * is bit-reproducible: fixed-order sums, no floating-point atomics (abdpymc_amd/csrc/abd_curves.hpp).  Non-finite theta:
 * non-finite sums, comparisons false, status 0. */
int abd_curves(abd_ctx* ctx, int32_t chain, const double* theta, double thr_s, double thr_n, int64_t* counts, int64_t* n_infections,
               double* titer_sums);
/* The follow-up the curves use: last_gap is (N,) with -1 <= last_gap[j] < G (ABD_ERR_ARG outside); NULL: everyone to G-1,
 * the state after abd_create.  Affects the curves only. */
int abd_set_follow_up(abd_ctx* ctx, const int32_t* last_gap);

/* Infection risk by titer of one draw: the person-time table of "infection in gap g given the titer of gap g - 1" of the
 * Deterministics of chain slot `chain` at theta, reduced over the individuals on the device.  The window is (start, end) with
 * 0 <= start, end <= G, end - start >= 2; edges_s[0 .. n_edges_s) and edges_n[0 .. n_edges_n) are finite, strictly ascending
 * bin edges on the titer scale (0 <= n_edges <= 7; the entries beyond n_edges are not read); first_only is 0 or 1.
 * Anything else is ABD_ERR_ARG.  Cell (g, j) is AT RISK iff start < g < end, g <= last_gap[j] (abd_set_follow_up) and,
 * when first_only, i[g', j] = 0 for every start < g' < g: at most one infection per individual inside the window.  It is an
 * EVENT iff it is at risk and i[g, j] = 1.
 *   table [2][2][G][8]   antigen (0 S, 1 N) x (0 at risk, 1 events) x gap x bin
 * A cell is counted in the bin #{e in edges: x >= e} of the titer of the PREVIOUS gap, x = ab_s_mu[g-1, j] for S and
 * ab_n_mu[g-1, j] for N, exactly what abd_deterministics returns; bins above n_edges stay empty, gaps outside the window are
 * zero.  The table depends on (N, G, last_gap, the slot's state, theta, the spec) only: integer sums, no atomics
 * (abdpymc_amd/csrc/abd_risk.hpp).  Non-finite theta: every comparison fails, so every cell at risk lands in bin 0; the
 * totals over the bins do not change and the status is 0. */
typedef struct abd_risk_spec {
  int32_t start, end, first_only, n_edges_s, n_edges_n;
  double edges_s[7], edges_n[7];
} abd_risk_spec;
int abd_risk(abd_ctx* ctx, int32_t chain, const double* theta, const abd_risk_spec* spec, int64_t* table);

/* Pointwise log-likelihood of the two observed Normals "it_s_lik", "it_n_lik" (abd.py:459-469) at theta and chain slot
 * `chain`'s discrete state: ll_s receives s.n_obs doubles, ll_n n.n_obs, in the order the readings were given to abd_create
 * (what pm.compute_log_likelihood records for one draw).  Either pointer may be NULL.  sum(ll_s) + sum(ll_n) is
 * abd_loglik_dlogp's loglik to rounding. */
int abd_pointwise_loglik(abd_ctx* ctx, int32_t chain, const double* theta, double* ll_s, double* ll_n);

/* Per individual j of the context: the sum of the pointwise log-likelihood over j's S readings (ll_s[N]) and N readings
 * (ll_n[N]); either pointer may be NULL, not both.  0 where j has no reading of that antigen.  The joint log-likelihood of
 * individual j is ll_s[j] + ll_n[j].  Summed on the device in a fixed order (one wave per individual, its readings in
 * ascending gap, a fixed butterfly over the lanes): two calls at the same state return the same bits, and a row differs from
 * any other summation of abd_pointwise_loglik's values by rounding only. */
int abd_individual_loglik(abd_ctx* ctx, int32_t chain, const double* theta, double* ll_s, double* ll_n);

/* Posterior predictive of the two observed Normals at theta and chain slot `chain`'s discrete state (what
 * pm.sample_posterior_predictive draws for one draw): per OD reading the noise-free mean m = d / (1 + exp(-b (x - a))) into
 * mean_*, and the replicate y_rep = m + sigma z into yrep_*, s.n_obs / n.n_obs doubles each in the caller's reading order; any
 * pointer may be NULL.  z ~ N(0, 1) comes from Philox4x32-10 with key (seed lo, seed hi) and counter (r, stream, draw lo,
 * 0x80000000 | antigen << 30 | (draw >> 32) & 0x3FFFFFFF) -- r the reading's index in the caller's order within its antigen
 * (S 0, N 1) -- as u1 = ((w0 >> 5) 2^26 + (w1 >> 6) + 0.5) 2^-53, u2 likewise of w2, w3, z = sqrt(-2 ln u1) cospi(2 u2).  So
 * the noise depends on (seed, stream, draw, antigen, r) only.  The native sampler records with seed = opts.seed, stream =
 * chain_offset + chain slot, draw = the iteration number.  ABD_ERR_ARG for 2^32 or more readings of an antigen. */
int abd_posterior_predictive(abd_ctx* ctx, int32_t chain, const double* theta, uint64_t seed, uint32_t stream, uint64_t draw,
                             double* yrep_s, double* yrep_n, double* mean_s, double* mean_n);

/* ---------------------------------------------------------------------------------------------------
 * The forward simulator of a cohort (reference abdpymc/simulation.py:222-279 Individual.infection_responses, 328-353
 * Cohort.simulate_row): what would this cohort's data look like under these dynamics, ELISA curves, protection curves and
 * this force of infection.  The context supplies the vaccinations, the PCR positives (none are forced on a context created
 * without pcrpos) and the readings' (gap, ind, log_dilution) -- on an fp32-storage context log_dilution as stored.
 * For replicate rho, individual j and gaps t = 0 .. G-1 in sequence, with s_temp = n_temp = 0 before gap 0 and s_prev,
 * n_prev the titers of gap t - 1 (the bare init values at t = 0):
 *   exposed = u_e < lam0[t];  p_x = 1 / (1 + exp(-protect_b_x (x_prev - protect_a_x)));  protected = u_s < p_s or u_n < p_n
 *   infected = pcrpos[j, t] == 1 or (exposed and not protected)
 *   s_temp = s_temp temp_wane_s + infected temp_rise_i_s + vacs[j, t] temp_rise_v_s
 *   n_temp = n_temp temp_wane_n + infected temp_rise_i_n                         (N's temp_rise_v is unused)
 *   s[t] = init_s + s_temp + (perm_rise_s once an infection or a vaccination has occurred in gaps 0 .. t)
 *   n[t] = init_n + n_temp + (perm_rise_n once an infection has)
 * There is no three-gap mask (the reference's simulator has none).  A reading k of antigen x at (gap, ind, log_dilution):
 *   od = elisa_d_x / (1 + exp(-elisa_b_x (log_dilution - x[ind, gap]))) + elisa_sd_x z_k
 * Random numbers: Philox4x32-10 with key (seed lo, seed hi) and the counters
 *   exposure       (ind_offset + j, rho, t, 0x40000000)       u_e from words 0, 1
 *   protection     (ind_offset + j, rho, t, 0x40000001)       u_s from words 0, 1; u_n from words 2, 3
 *   reading noise  (r, rho, 0, 0x40000010 | antigen)          z the first Box-Muller value, as abd_posterior_predictive forms it
 * with r the reading's index in the caller's order within its antigen (S 0, N 1), ind_offset from abd_set_individual_offset
 * and uniforms ((a >> 5) 2^26 + (b >> 6) + 0.5) 2^-53.  The sweep's counters have a fourth word of 0 and the predictive
 * stream sets its top bit, so none of the three streams meet.  Consequences:
 *   - a replicate depends on (seed, rho) only: not on how many replicates a call asks for, on how the call is cut into
 *     staging chunks, on which outputs are asked for, or on dense panels versus observation lists;
 *   - an individual's infections and titers depend on its GLOBAL index, so they are identical on a cohort sharded by
 *     individual; the reading noise is keyed by the local reading index and is not. */
typedef struct {
  double protect_a, protect_b;                                  /* protection curve: 50 % titer, slope (> 0) */
  double elisa_b, elisa_d, elisa_sd;                            /* OD curve: slope (< 0), maximum (> 0), noise sd (> 0) */
  double init, perm_rise, temp_rise_i, temp_rise_v, temp_wane;  /* dynamics: rises >= 0, 0 < temp_wane <= 1 */
} abd_sim_antibody;
typedef struct {
  abd_sim_antibody s, n;
} abd_sim_params;
/* Replicates first_replicate .. first_replicate + n_replicates - 1 (R of them) of the simulation at lam0 (G per-gap
 * infection probabilities).  infections, s_titer, n_titer: [R][N][G], each replicate (n_inds, n_gaps) row-major as the
 * reference's Cohort holds them; od_s, od_n: [R][s.n_obs], [R][n.n_obs] in the caller's reading order; n_infected: [R][G]
 * infections per gap.  Any output may be NULL.  Everything runs on the context's stream; the replicates pass through device
 * staging in chunks (abd_simulate_staged).  ABD_ERR_ARG, the message naming the field, for a parameter that is not
 * finite or breaks the rules above, a non-finite lam0 entry, n_replicates < 1, first_replicate + n_replicates beyond 2^32. */
int abd_simulate(abd_ctx* ctx, const abd_sim_params* params, const double* lam0, uint64_t seed, uint32_t first_replicate,
                 int32_t n_replicates, int8_t* infections, double* s_titer, double* n_titer, double* od_s, double* od_n,
                 int64_t* n_infected);
/* abd_simulate with the device memory one chunk of its replicates may occupy given for this call (0: the default, 1 GiB).  A
 * chunk holds at least one replicate whatever the budget.  The result does not depend on it. */
int abd_simulate_staged(abd_ctx* ctx, const abd_sim_params* params, const double* lam0, uint64_t seed, uint32_t first_replicate,
                        int32_t n_replicates, int64_t staging_bytes, int8_t* infections, double* s_titer, double* n_titer,
                        double* od_s, double* od_n, int64_t* n_infected);

/* ---------------------------------------------------------------------------------------------------
 * The compound step pm.sample assigns to this model (reference call site abd.py:921-922), run natively
 * for several chains: NUTS on the 17 continuous variables, then one Gibbs sweep of [i_raw, ab_s_waner], then a
 * re-evaluation at the new discrete state.  This removes the host-language cost per leapfrog (PyMC: Python;
 * SURVEY 8f rank 4).  The chains run as independent units of 1-8 consecutive chains, each on its own HIP stream
 * with its own result rows: a unit's pending leapfrog points go out as ONE evaluation launch, its sweep and the
 * re-evaluation are queued behind each other on its stream, and the host polls completion tags -- no unit waits
 * for another one's trees (as PyMC's one process per chain does not), and their launches overlap on the device.
 * What a unit computes depends only on the unit (fixed launch shape), never on the other units or on timing.
 * Leapfrog trains (diagonal metric; ABD_SAMPLER_TRAINS): the launch that evaluates a point also assembles logp and gradient,
 * finishes the leapfrog and leaves the next point in device memory for the launch the host has already queued behind it,
 * so a chain's leapfrogs follow each other at the device's pace, not at the host's round trip.
 *   - Dense cohorts (abd_train.hpp): every chain has a small state machine in device memory -- the two ends of its tree, the
 *     doubling directions of the transition (drawn by the host before the tree starts), the leaves still to go.  A launch takes
 *     the 1, 2 or 4 chains of its unit one leapfrog further each, whatever stage each of them is in, and goes on ACROSS the
 *     halves of a doubling and across doublings; the host reads the launches' records from a ring in mapped memory, runs the
 *     tree logic (U-turn tests, multinomial choice) behind the device and hands the chain its next transition when one is over.
 *     Steps queued beyond the end of a tree still run for that chain and may overlap its sweep; their records are never read,
 *     which is the only reason the overlap is harmless.  The chain's sweep runs on a side stream of its own while the other
 *     chains of the unit go on.  Units: one chain up to 4 chains, two up to 7, four beyond.
 *   - Observation lists: units of one chain; a train ends with the half of the doubling it serves.
 * A train run is exactly repeatable, does not depend on the other chains or on timing, and equals the host-driven run
 * (ABD_SAMPLER_TRAINS=0) to rounding, not bit for bit: the closed forms of the transforms are the device's exp / log1p
 * there.
 * Cohorts kept as observation lists are bound by the host's two kernel launches per evaluation, so their units are
 * driven by T host threads inside abd_sampler_run (T a power of two <= 8, 4 by default; thread t the units u with
 * u mod T == t: what a thread touches is private to its units); dense cohorts are bound by the device and use the calling
 * thread only.  abd_kernel_timing and the threaded sampler are mutually exclusive: while a timing mode is on, the units
 * are driven by the calling thread alone.
 * Step size: dual averaging to `target_accept`; metric: diagonal, windowed running variance of the tuning draws
 * (abdpymc_amd/csrc/abd_nuts.hpp).
 * Every evaluation a chain consumes on any of these drivers can be logged for tests (abd_sampler_enable_leapfrog_log below):
 * one row of 58 doubles -- kind, iteration, depth, n_leaf, dir, eps, lp, q[17], p_half[17], g[17] -- per start point and
 * leaf, where `iteration` names the tree the row belongs to and so the discrete state it was evaluated under: the state at
 * the start of the run for the run's first iteration and with gibbs = 0, else the state the sweep of iteration - 1 left.
 * Iterations [0, tune) adapt; later ones are draws.  Randomness: one xoshiro256++ stream per chain keyed by
 * (seed, chain slot) for NUTS; Philox keyed by (seed, iteration) for the sweep. */
typedef struct abd_sampler abd_sampler;

typedef struct abd_sampler_opts {
  int64_t tune;           /* iterations that adapt step size and metric */
  uint64_t seed;
  double target_accept;   /* 0.8 as pm.sample */
  int32_t max_treedepth;  /* 10 as pm.sample; at most 16 */
  int32_t gibbs;          /* 1: sweep [i_raw, ab_s_waner] after every NUTS transition; 0: continuous part only */
  int32_t accumulate;     /* 1: add i, ab_n_mu, ab_s_mu of every draw (iteration >= tune) into device sums */
  int32_t chain_offset;   /* chain slot k draws from random stream k + chain_offset: the global chain id when chains
                             are sharded over processes (one per GPU), so draws do not depend on the world size */
  int32_t dense_metric;   /* 0: diagonal M^-1, pm.sample's default; 1: full covariance of the tuning draws (PyMC:
                             init="adapt_full") -- this posterior is strongly correlated and trees get ~8x shorter */
  int32_t reserved;
} abd_sampler_opts;

#define ABD_N_STATS 11
/* columns of the per-iteration statistics row */
#define ABD_STAT_LP 0                /* joint logp after the whole compound step */
#define ABD_STAT_TREE_DEPTH 1
#define ABD_STAT_N_STEPS 2           /* leapfrogs = logp_dlogp evaluations of the transition */
#define ABD_STAT_MEAN_TREE_ACCEPT 3
#define ABD_STAT_STEP_SIZE 4
#define ABD_STAT_DIVERGING 5
#define ABD_STAT_ENERGY 6
#define ABD_STAT_MAX_ENERGY_ERROR 7
#define ABD_STAT_GIBBS_ACCEPTED 8
#define ABD_STAT_GIBBS_PROPOSED 9
#define ABD_STAT_T_DONE 10           /* seconds from the start of this abd_sampler_run call to the end of the chain's iteration
                                        (host clock): chains are independent, so they finish their iterations at different times */

/* chains[k] must hold a discrete state (abd_set_discrete); theta0 is n x 17, the starting points.
 * A sampler points into its context: destroy it before abd_destroy(ctx). */
int abd_sampler_create(abd_ctx* ctx, int32_t n, const int32_t* chains, const double* theta0,
                       const abd_sampler_opts* opts, abd_sampler** out);
void abd_sampler_destroy(abd_sampler* s);
/* Advance every chain by n_iter iterations.  theta: n x n_iter x 17, stats: n x n_iter x ABD_N_STATS
 * (either may be NULL).  The discrete state after the call is read with abd_get_discrete. */
int abd_sampler_run(abd_sampler* s, int64_t n_iter, double* theta, double* stats);

/* abd_sampler_run that also records, for every iteration of the call, the discrete state and the three
 * Deterministics of every chain -- what the reference keeps per draw in its InferenceData (abd.py:427, 373,
 * 649/667, 341, 389-391).  Each array is [n][capacity][...] (chain-major; (G, N) or (N,) per draw, as PyMC stores
 * them) and this call fills draws first .. first + n_iter - 1 of every chain; NULL arrays are skipped.  The
 * draws are staged on the device and copied out in large blocks (at config 3 a draw is 36 MB per chain). */
typedef struct abd_record {
  int64_t capacity;
  int64_t first;
  int64_t thin;        /* 0 or 1: every iteration of the call is recorded; K > 1: iterations 0, K, 2K, ... of the call, at
                          draws first, first + 1, ... (the reference thins afterwards, subsample_idata.py; at config 3 a
                          draw is 36 MB per chain, so here it is done while sampling) */
  int8_t* i_raw;
  int8_t* ab_s_waner;
  int8_t* i;
  double* ab_n_mu;
  double* ab_s_mu;
  double* ll_s;        /* [n][capacity][s.n_obs], [n][capacity][n.n_obs]: the pointwise log-likelihood of every recorded draw */
  double* ll_n;        /* (abd_pointwise_loglik), readings in the caller's order */
  double* yrep_s;      /* [n][capacity][s.n_obs], [n][capacity][n.n_obs]: the posterior predictive replicate of every recorded */
  double* yrep_n;      /* draw, bit-identical to abd_posterior_predictive at that draw's point (keys: abd_posterior_predictive) */
} abd_record;
int abd_sampler_run_record(abd_sampler* s, int64_t n_iter, double* theta, double* stats, const abd_record* rec);
/* Posterior means of the Deterministics of chain k (0 <= k < n) over the draws accumulated so far, each
 * (G, N); any pointer may be NULL.  *n_draws receives the number of accumulated draws. */
int abd_sampler_means(abd_sampler* s, int32_t k, double* i_mean, double* ab_n_mu_mean, double* ab_s_mu_mean,
                      int64_t* n_draws);
/* Pointwise log-likelihood statistics of every draw (iteration >= tune), accumulated on the device per chain and reading.
 * Allowed before the first abd_sampler_run* call (ABD_ERR_STATE after it); accumulate = 1 allocates 4 x (K_s + K_n)
 * doubles per chain (K_*: the antigens' n_obs), 0 releases them. */
int abd_sampler_enable_pointwise(abd_sampler* s, int32_t accumulate);
/* The statistics of chain k (0 <= k < n) over its draws so far: out is [3][K_s + K_n] (S readings first, then N, each in the
 * caller's order): row 0 log sum over draws of exp(ll) (not divided by the count), row 1 the mean of ll, row 2 the sum of
 * squared deviations from it (M2).  They merge exactly over chains and processes: log-add-exp for row 0, Chan et al.'s
 * pairwise formulas for rows 1 and 2 (abdpymc_amd/compare.py).  *n_draws (may be NULL) receives the number of draws. */
int abd_sampler_pointwise_stats(abd_sampler* s, int32_t k, double* out, int64_t* n_draws);
/* As abd_sampler_enable_pointwise, for T_j = S_j + N_j; refused after the first abd_sampler_run*.  The joint log-likelihood
 * of every individual's readings (abd_individual_loglik: ll_s[j] + ll_n[j]) at every draw (iteration >= tune, whatever is
 * recorded or thinned); accumulate = 1 allocates 4 x N doubles per chain, 0 releases them.  Independent of
 * abd_sampler_enable_pointwise: either, both or neither may be on.  The chains' trajectories do not change. */
int abd_sampler_enable_individual_loglik(abd_sampler* s, int32_t accumulate);
/* out[3][N]: lse, mean, m2 of T_j over the draws so far (as abd_sampler_pointwise_stats); n_readings[N] (may be NULL):
 * j's readings of both antigens.  An individual without readings has T_j = 0 at every draw: lse = log(n_draws), mean = m2 = 0.
 * *n_draws (may be NULL) receives the number of draws. */
int abd_sampler_individual_loglik_stats(abd_sampler* s, int32_t k, double* out, int64_t* n_draws, int64_t* n_readings);
/* Posterior predictive check statistics of every draw (iteration >= tune), accumulated on the device per chain and reading.
 * Allowed before the first abd_sampler_run* call (ABD_ERR_STATE after it); accumulate = 1 allocates 3 x (K_s + K_n) doubles
 * per chain, 0 releases them.  No random numbers are drawn: the chains' trajectories do not change. */
int abd_sampler_enable_predictive(abd_sampler* s, int32_t accumulate);
/* The statistics of chain k (0 <= k < n) over its draws so far: out is [3][K_s + K_n] (S readings first, then N, each in the
 * caller's order): row 0 the mean of the predictive mean m, row 1 the sum of its squared deviations (M2), row 2 the mean of
 * Phi((y - m) / sigma), the tail probability P(y_rep <= y).  They merge exactly over chains and processes: Chan et al. for
 * rows 0 and 1, a count-weighted mean for row 2 (abdpymc_amd/predictive.py).  *n_draws (may be NULL): the number of draws. */
int abd_sampler_predictive_stats(abd_sampler* s, int32_t k, double* out, int64_t* n_draws);
/* The epidemic curves (abd_curves) of every draw (iteration >= tune) of every chain, kept on the device: a row of 6 G + 8
 * numbers per draw, whatever abd_record and its thin ask for.  Allowed before the first abd_sampler_run* call (ABD_ERR_STATE
 * after it); capacity > 0 allocates rows for that many draws per chain, 0 releases them.  While they are enabled an
 * abd_sampler_run* call whose draws would pass capacity fails with ABD_ERR_STATE before anything is launched.  The follow-up
 * is the context's (abd_set_follow_up) at the time of each draw.  No random numbers are drawn: the chains' trajectories do
 * not change. */
int abd_sampler_enable_curves(abd_sampler* s, int64_t capacity, double thr_s, double thr_n);
/* Draws first .. first + count - 1 of chain k (0 <= k < n; draw 0 is iteration `tune`): counts [count][4][G], n_infections
 * [count][8], titer_sums [count][2][G] as abd_curves lays them out; any may be NULL.  *n_draws (may be NULL) receives the
 * number of draws the chain has.  ABD_ERR_ARG for a range beyond it.  May be called between run calls. */
int abd_sampler_curves(abd_sampler* s, int32_t k, int64_t first, int64_t count, int64_t* counts, int64_t* n_infections,
                       double* titer_sums, int64_t* n_draws);
/* The risk table (abd_risk) of every draw (iteration >= tune) of every chain, kept on the device: 64 G counts of 32 bits
 * per draw (a count is at most N < 2^31), whatever abd_record and its thin ask for.  Allowed before the first abd_sampler_run*
 * call (ABD_ERR_STATE after it); capacity > 0 allocates rows for that many draws per chain (ABD_ERR_NOMEM, the message naming
 * the bytes, if they do not fit), 0 releases them; ABD_ERR_ARG for a spec abd_risk refuses.  While it is enabled an
 * abd_sampler_run* call whose draws would pass capacity fails with ABD_ERR_STATE before anything is launched.  The follow-up
 * is the context's (abd_set_follow_up) at the time of each draw.  No random numbers are drawn: the chains' trajectories do
 * not change. */
int abd_sampler_enable_risk(abd_sampler* s, int64_t capacity, const abd_risk_spec* spec);
/* Draws first .. first + count - 1 of chain k (0 <= k < n; draw 0 is iteration `tune`): table [count][2][2][G][8] as abd_risk
 * lays it out; may be NULL.  *n_draws (may be NULL) receives the number of draws the chain has.  ABD_ERR_ARG for a range
 * beyond it, ABD_ERR_STATE when the table is not enabled.  May be called between run calls. */
int abd_sampler_risk(abd_sampler* s, int32_t k, int64_t first, int64_t count, int64_t* table, int64_t* n_draws);

/* PSIS-LOO by individual for the titer model: T_j = S_j + N_j (abd_individual_loglik: ll_s[j] + ll_n[j]) of every
 * kept draw of every chain stays on the device, a matrix of 8 bytes per kept draw and slot of 64-padded individuals, and
 * every individual's column over all chains is Pareto-smoothed there by the estimator of abd_survival_loo_stats.
 * _enable: before the first abd_sampler_run* call (ABD_ERR_STATE after it).  Draw d = iteration - tune is kept when
 *   d % thin == 0: C = ceil(draws_per_chain / thin) rows per chain; 0 draws releases.  ABD_ERR_ARG, before the device is touched,
 *   for a negative size, thin < 1 or n_chains * C above ABD_SAMPLER_LOO_MAX_DRAWS (the message names the product and the cap);
 *   ABD_ERR_NOMEM, the message naming the bytes.  While it is enabled an abd_sampler_run* call whose draws would pass
 *   draws_per_chain fails with ABD_ERR_STATE before anything is launched.  The per-individual launch of a draw is shared with
 *   abd_sampler_enable_individual_loglik, whose accumulators keep their bits; the chains' trajectories do not change.
 * _rows: chain k's kept rows first .. first + count - 1 as ll[count][N] in the caller's order of individuals (NULL: none
 *   copied); *n_rows (may be NULL) receives the rows the chain holds.  ABD_ERR_ARG for a window beyond them.  May be called
 *   between run calls.
 * _stats: over the S = n_chains * C draws of a finished run, chain-major: elpd_loo[N], pareto_k[N] (+inf where the tail has at
 *   most 4 draws), lppd[N] = log mean exp(T_j), n_tail[N], *n_draws = S and n_readings[N] (the last two may be NULL); an
 *   individual without readings gets elpd_loo = lppd = 0, pareto_k = NaN, n_tail = 0.  ABD_ERR_STATE, naming the chain, unless
 *   every chain holds exactly C rows.  Consumes nothing: a second call returns the same bits. */
#define ABD_SAMPLER_LOO_MAX_DRAWS 16384
int abd_sampler_enable_loo(abd_sampler* s, int64_t draws_per_chain, int32_t thin);
int abd_sampler_loo_rows(abd_sampler* s, int32_t k, int64_t first, int64_t count, double* ll, int64_t* n_rows);
int abd_sampler_loo_stats(abd_sampler* s, double* elpd_loo, double* pareto_k, double* lppd, int32_t* n_tail, int64_t* n_draws,
                          int64_t* n_readings);

/* Per-cell convergence accumulators over ALL draws: what split R-hat and a batch-means effective sample size of the
 * Deterministics "i", "ab_n_mu", "ab_s_mu" need, kept on the device because a run at full size never keeps its draws
 * (abdpymc_amd/csrc/abd_diag.hpp; abdpymc_amd/diagnostics.py: from_draws is the same definition as NumPy, rhat / ess read it).
 *
 * planned_draws = D >= 2 and batch_len = L >= 1.  Draw d = 0, 1, ... is iteration tune + d.
 *   H = D / 2 (integer division) is the half length: half 0 is draws 0 .. H-1, half 1 draws H .. 2H-1.  A draw >= 2H (the last
 *   one when D is odd) is not accumulated.  A run call whose draws would pass D fails with ABD_ERR_STATE before anything is
 *   launched.
 *   Each half is cut into B = H / L whole batches of L draws from its start; the trailing H % L draws of a half enter the
 *   half's moments but no batch.  No batch straddles the halves.
 * Per chain and cell (g, j), for x = ab_n_mu and for x = ab_s_mu (the Deterministics' titers), seven doubles, all 0 at first:
 *   mean_h, M2_h for h = 0, 1 -- Welford, n the draw's 1-based place in its half, inv_n = 1.0 / n computed by the host:
 *       d = x - mean;  mean += d * inv_n;  M2 += d * (x - mean)
 *   cur -- the running sum of the open batch: cur = x on the first draw of a batch, else cur += x
 *   bm_mean, bm_M2 -- Welford over the closed batches' means, updated by the draw that closes a batch, inv_L = 1.0 / L and
 *   inv_b = 1.0 / (batches closed so far in this chain, this one included, both halves pooled):
 *       bm = cur * inv_L;  e = bm - bm_mean;  bm_mean += e * inv_b;  bm_M2 += e * (bm - bm_mean)
 * and for i, whose value is 0 or 1 so that every moment is a function of counts, integers only:
 *   uint32 c_h0, c_h1 (ones in either half), uint32 cur (ones in the open batch), uint32 sum_cb (the sum of the closed
 *   batches' counts), uint64 sum_cb2 (the sum of their squares).
 * That is 136 bytes per cell and chain.  A cell belongs to one lane, a chain has its own planes, the update is a fixed-order
 * read-modify-write: there are no atomics of any kind and the result is bit-reproducible -- it depends on the draws alone,
 * not on the launch shape, on how the run is cut into calls, on abd_record or on thin.  No random numbers are drawn: the
 * trajectories do not change.
 *
 * Allowed before the first abd_sampler_run* call (ABD_ERR_STATE after it).  planned_draws = 0 releases the buffers;
 * planned_draws of 1 or negative, or planned_draws > 0 with batch_len < 1: ABD_ERR_ARG.  ABD_ERR_NOMEM, the message naming
 * the bytes, when the device cannot hold them. */
int abd_sampler_enable_diagnostics(abd_sampler* s, int64_t planned_draws, int64_t batch_len);
/* The accumulators of chain k, (G, N) gap-major per plane like the Deterministics: i_counts [4][G*N] = c_h0, c_h1, sum_cb,
 * sum_cb2 (widened to int64); ab_n_mu and ab_s_mu [6][G*N] = mean_h0, M2_h0, mean_h1, M2_h1, bm_mean, bm_M2; info[4] = draws
 * in half 0, draws in half 1, batches closed, L.  Any pointer may be NULL.  May be called between run calls.  ABD_ERR_STATE
 * ("not enabled") without abd_sampler_enable_diagnostics. */
int abd_sampler_diagnostics(abd_sampler* s, int32_t k, int64_t* i_counts, double* ab_n_mu, double* ab_s_mu, int64_t info[4]);

/* Per-individual timelines over ALL draws: what the reference's per-individual figure (timelines.py: plot_individual) reads
 * from the (draw, gap, ind) arrays of the whole posterior -- the spread of the two titers of a cell, its infection probability
 * and the probability of at least one infection so far inside the cell's time chunk -- kept on the device because a run at full
 * size never keeps its draws (abdpymc_amd/csrc/abd_timeline.hpp; abdpymc_amd/timelines.py: from_draws is the same definition
 * as NumPy).  Accumulated per chain for every draw (iteration >= tune), whatever abd_record and its thin ask for.
 *
 * Titer histograms.  Per cell (g, j), for x = ab_n_mu over [lo_n, hi_n) and for x = ab_s_mu over [lo_s, hi_s) (the
 * Deterministics' titers), ABD_TIMELINE_BINS = 64 counters of 16 bits, all 0 at first.  With inv_w = 62 / (hi - lo) computed
 * once by the host, a draw adds 1 to bin
 *       0 if x < lo;   63 if x >= hi or x is NaN;   else 1 + min(61, (int)floor((x - lo) * inv_w))
 * so that bins 1 .. 62 are 62 interior bins of width w = (hi - lo) / 62.  16-bit counters: planned_draws <= 65535.
 * Infection timing, integers only.  Per cell two uint32: inf, the draws with i[g, j] = 1, and cum, the draws with i[g', j] = 1
 * for some g' <= g in the same chunk as g (chunk borders 0, splits..., n_gaps of abd_desc; no splits: one chunk).  Per
 * individual ninf[8], uint32: the draws by the number of infections at gaps <= last[j], [7] pooling 7 and more; last is the
 * context's follow-up (abd_set_follow_up) at the time of each draw, n_gaps - 1 without one, and the row of a never-followed
 * individual (last = -1) stays 0.  The cell planes ignore the follow-up.
 * That is 264 bytes per cell and chain.  A cell belongs to one lane, a chain has its own planes, the update is a plain
 * read-modify-write: there are no atomics of any kind and the result is bit-reproducible -- it depends on the draws alone, not
 * on the launch shape, on how the run is cut into calls, on abd_record or on thin.  No random numbers are drawn: the
 * trajectories do not change.
 *
 * Allowed before the first abd_sampler_run* call (ABD_ERR_STATE after it).  planned_draws = 0 releases the buffers;
 * planned_draws negative or above ABD_TIMELINE_MAX_DRAWS, or planned_draws > 0 with a range that is not finite and ascending
 * (lo < hi, hi - lo finite): ABD_ERR_ARG.  ABD_ERR_NOMEM, the message naming the bytes, when the device cannot hold them (about
 * 0.5 GB per chain at 10 000 x 200).  A run call whose draws would pass planned_draws fails with ABD_ERR_STATE before anything is
 * launched. */
#define ABD_TIMELINE_BINS 64
#define ABD_TIMELINE_MAX_DRAWS 65535
#define ABD_TIMELINE_MAX_Q 8
#define ABD_TIMELINE_NINF 8
int abd_sampler_enable_timelines(abd_sampler* s, int64_t planned_draws, double lo_n, double hi_n, double lo_s, double hi_s);
/* The counters of chain k (0 <= k < n) over its draws so far, gap-major like the Deterministics: hist_n and hist_s
 * [G][N][64] uint16, inf and cum [G][N] (widened to int64), ninf [N][8] (widened to int64); *n_draws the number of draws.  Any
 * pointer may be NULL.  May be called between run calls.  ABD_ERR_STATE ("not enabled") without abd_sampler_enable_timelines. */
int abd_sampler_timelines(abd_sampler* s, int32_t k, uint16_t* hist_n, uint16_t* hist_s, int64_t* inf, int64_t* cum, int64_t* ninf,
                          int64_t* n_draws);
/* Quantiles of the titers per cell from the histograms POOLED over the sampler's chains (32-bit sums), computed on the device:
 * 8 bytes per quantile and cell reach the host instead of 128 per chain and cell.  1 <= n_q <= ABD_TIMELINE_MAX_Q, each q in
 * [0, 1] (else ABD_ERR_ARG); out_n and out_s are [n_q][G][N], either may be NULL.  With c[0..63] a cell's pooled counts, C
 * their inclusive cumulative sums and n their total:  n = 0 gives NaN;  else t = q n and b the smallest bin with c[b] > 0
 * and C[b] >= t:  b = 0 gives lo,  b = 63 gives hi,  else  lo + w ((b - 1) + (t - C[b-1]) / c[b])
 * (abdpymc_amd/timelines.py: quantiles is the same definition as NumPy). */
int abd_sampler_timeline_quantiles(abd_sampler* s, int32_t n_q, const double* q, double* out_n, double* out_s);
/* Current diagonal of M^-1 (17) and step size of chain k; `metric` (17 x 17, may be NULL) receives the full
 * M^-1 (the diagonal matrix when the metric is diagonal). */
int abd_sampler_adaptation(abd_sampler* s, int32_t k, double* inv_mass, double* step_size, double* metric);
/* Install a diagonal M^-1 (17 entries, all > 0; NULL keeps the chain's) and / or a step size (<= 0 keeps the chain's) for chain
 * k between two abd_sampler_run calls, e.g. one adaptation pooled over the chains (PyMC: pm.sample(step=pm.NUTS(scaling=...,
 * step_scale=...))).  The next transition runs with exactly these values.  After tuning they stay.  During iterations < tune
 * the chain goes on adapting from there, which re-seeds the adaptation that a value replaces: a step size starts the dual
 * average over (no history, mu = log(10 step_size)); a metric makes the variance estimate's foreground window the prior "10
 * draws at the chain's current point with variance inv_mass", empties its background window and starts the count of its
 * 101-draw windows over.  A value that is kept leaves its adaptation untouched.  Nothing is installed when a value is refused
 * (ABD_ERR_ARG), or when the chain already runs a dense metric (ABD_ERR_STATE). */
int abd_sampler_set_adaptation(abd_sampler* s, int32_t k, const double* inv_mass, double step_size);

/* The leapfrog log: a test and debug facility (no per-draw summary; off by default, one branch per evaluation when off).  Every
 * evaluation a chain's NUTS state CONSUMES is appended to the chain's own host buffer as one row of ABD_LEAPFROG_COLS doubles,
 * on all three drivers (dense trains, observation-list trains, host-driven units) at the one place they share
 * (abdpymc_amd/csrc/abd_nuts.hpp: attach_log / set_point / feed).  Steps the device took beyond the end of a tree are never fed
 * and so never logged.  Columns:
 *   0 kind        ABD_LEAPFROG_INIT: the chain's start point (row 0, written when the log is enabled);  ABD_LEAPFROG_START: the
 *                 start point of a transition, evaluated again after a sweep;  ABD_LEAPFROG_LEAF: a leapfrog of a tree
 *   1 iteration   the sampler's iteration counter of the tree the row belongs to (a START row: the tree that starts from it; the
 *                 one behind the last iteration of a run call: the next call's first)
 *   2 depth, 3 n_leaf, 4 dir   the doubling the leaf belongs to, its index in that half, the half's direction +-1 (0 unless LEAF)
 *   5 eps         the chain's step size
 *   6 lp          logp as the evaluation gave it
 *   7 .. 23   q       the unconstrained point that was evaluated
 *   24 .. 40  p_half  the half-kicked momentum the leaf was reached with (0 unless LEAF)
 *   41 .. 57  g       the gradient as the evaluation gave it
 * The iteration rule: a row was evaluated under the discrete state at the start of the run if its iteration is the run's
 * first or opts.gibbs is 0, else under the state the sweep of iteration - 1 left (abd_record: i_raw, ab_s_waner of that draw).
 * Consecutive LEAF rows a, b of one half (same iteration and depth, n_leaf_b = n_leaf_a + 1) are one leapfrog apart: with
 * ve = dir eps,  q_b = q_a + ve M^-1 (p_half_a + ve g_a)  and  p_half_b = p_half_a + ve g_a.
 * capacity_rows_per_chain = 0 turns the log off.  Allowed before the first abd_sampler_run* call (ABD_ERR_STATE after it). */
#define ABD_LEAPFROG_COLS 58
#define ABD_LEAPFROG_INIT 0
#define ABD_LEAPFROG_START 1
#define ABD_LEAPFROG_LEAF 2
int abd_sampler_enable_leapfrog_log(abd_sampler* s, int64_t capacity_rows_per_chain);
/* Rows first .. first + count - 1 of chain k's log into rows ([count][ABD_LEAPFROG_COLS]); *n_total (may be NULL): the rows the
 * chain has produced so far -- those beyond the capacity are counted and dropped, and asking for one is ABD_ERR_ARG.  May be
 * called between run calls. */
int abd_sampler_leapfrog_log(abd_sampler* s, int32_t k, int64_t first, int64_t count, double* rows, int64_t* n_total);
/* The launch shape the sampler settled on: out[0] chains per unit; out[1] how its leapfrogs run (ABD_TRAINS_*); out[2] the
 * workgroups with a range that a leapfrog launch of a full unit has as the kernel sees it (dense trains: more than 256 sum
 * their partial rows in two levels; host-driven units: the grid of an evaluation launch of all the unit's chains); out[3] the
 * host threads that drive the units.  What ABD_SAMPLER_UNIT, ABD_SAMPLER_TRAINS, ABD_TRAIN_BLOCKS_PER_CU and
 * ABD_GROUP_BLOCKS_PER_CU came to. */
#define ABD_TRAINS_NONE 0
#define ABD_TRAINS_LISTS 1
#define ABD_TRAINS_DENSE 2
int abd_sampler_launch_shape(abd_sampler* s, int32_t out[4]);

/* ---------------------------------------------------------------------------------------------------
 * One chain over several GPUs (cohorts too large or too slow for one): the joint logp is a sum over
 * individuals plus terms of theta alone, so each process holds a context over ITS slice of the individuals and
 *   logp(theta) = sum over processes of abd_logp_dlogp(...)  -  (processes - 1) x abd_theta_prior(theta)
 * (likewise the gradient): one all-reduce of 18 doubles per evaluation.  The Gibbs sweep needs no exchange at all;
 * abd_set_individual_offset makes it draw the random numbers of the individual's GLOBAL index, so the sharded
 * sweep is bit-identical to the unsharded one.  Python: abdpymc_amd.distributed.IndividualShards. */
/* The part of the joint logp that depends on theta only (continuous priors + log-Jacobians; no Bernoulli
 * term, no data term) and its gradient (may be NULL). */
int abd_theta_prior(abd_ctx* ctx, const double* theta, double* logp, double* grad);
int abd_set_individual_offset(abd_ctx* ctx, int64_t first_individual);

/* Measurement hooks used by bench.py.  mode 1: every evaluation kernel launch is bracketed by HIP events on
 * the stream it is launched on, and stream-ordered launches all go to ONE stream with the full grid (normally
 * they rotate over four, so that launches share the chip: a launch's own duration is only meaningful when
 * nothing else is in flight) -- the isolated kernel.  mode 2: the launch shape is left alone and HIP events
 * bracket every WINDOW of stream-ordered launches (first abd_logp_dlogp_batch_enqueue after an abd_wait ..
 * every stream joined at the next abd_wait) -- device time per launch as a stream-ordered caller runs them.
 * mode 0: off.  abd_kernel_time returns the accumulated device time and launch count since the last reset
 * (synchronises).  In mode 2 the count is in STEPS: a launch of abd_logp_dlogp_many that carries several steps counts
 * as that many, so device time / count stays the device time per step of n chains whatever the launches are. */
int abd_kernel_timing(abd_ctx* ctx, int32_t mode);
/* Every waiting call (synchronous evaluations, abd_wait, abd_logp_dlogp_many, the native sampler) waits for its result
 * rows by polling a completion tag in mapped host memory; if a tag does not show in time (~2 M polls / 1 s) the call
 * falls back to a stream synchronise, checks the tags again and fails with ABD_ERR_STATE if a row still lacks its tag.
 * Number of such fall-backs since abd_create: anything but 0 means the tag path has regressed. */
int64_t abd_wait_fallbacks(abd_ctx* ctx);
/* HIP multiplexes its streams over a few hardware queues, and kernels of streams that share a queue run one after the
 * other.  Measures (once per context, ~0.5 ms) which of the context's n <= 8 streams share one: streams with the same
 * number in queue_of_stream[] do.  The native sampler gives its units streams of different queues first. */
int abd_stream_queues(abd_ctx* ctx, int32_t* queue_of_stream, int32_t n);
int abd_kernel_time(abd_ctx* ctx, double* total_ms, int64_t* launches, int32_t reset);

/* Tuning hook (benchmarks / experiments): number of 256-thread workgroups of the evaluation grid
 * (<= 0 keeps the current value) and chains evaluated per wavefront (0 = automatic, else 1, 2 or 4). */
int abd_set_launch_config(abd_ctx* ctx, int32_t blocks, int32_t chains_per_wave);


/* Compulsory bytes one launch of `n_chains` evaluations has to read in THIS library's device layout:
 * dense: G*N*4R (the two [od, log_dilution] panels) + bit-packed indicator words
 * (vacs, pcrpos, one i_raw per chain: 8 bytes per individual per 64 gaps each) + n_chains*N waner bytes.
 * (SURVEY 8d's byte-per-cell figure, G*N*(4R + 2 + n_chains) + n_chains*N, is larger.) */
int64_t abd_algorithmic_bytes(abd_ctx* ctx, int32_t n_chains);

/* 1 if the observation panels were recognised as dense (one S and one N reading in every cell). */
int abd_is_dense(abd_ctx* ctx);
/* HIP streams that stream-ordered dense launches rotate over (1 for cohorts kept as observation lists). */
int abd_n_pipes(abd_ctx* ctx);

/* ---------------------------------------------------------------------------------------------------
 * The survival models of a finished run (reference survival.py:116-153: model_alone, model_combined): Poisson hazard
 *   infected[j, t] ~ Poisson(exposure[j, t] * lam0[t] * invlogit(sum_k b_k (titer_k[j, t] - a_k)))
 * over N individuals and T intervals, with K = 1 titer (alone) or K = 2 (combined: S, N).  A handle keeps the arrays on the
 * device; an evaluation returns logp and its gradient at unconstrained points
 *   theta[D] = a[K], b[K], _lam0_raw_mu, _lam0_raw_sd_log__, __lam0_raw_z[T]        D = 2 K + 2 + T
 * (PyMC's creation order; lam0 = invlogit(_lam0_raw_mu + exp(_lam0_raw_sd_log__) * __lam0_raw_z)).  It is independent of
 * abd_ctx.  Python: abdpymc_amd.survival. */
typedef struct {
  int32_t n_inds;              /* N >= 1 */
  int32_t n_intervals;         /* T = end - start - 1, 1 <= T <= ABD_MAX_GAPS - 1 */
  int32_t n_titers;            /* K: 1 or 2 */
  int32_t device;              /* HIP device ordinal; <0 = current device */
  const double* infected;      /* (N, T) row-major; >= 0, may be fractional; NaN = no follow-up in that cell */
  const double* exposure;      /* (N, T) row-major; >= 0; NaN likewise; a cell with infected > 0 and exposure 0 is refused */
  const double* titer[2];      /* (N, T) row-major each, finite wherever the cell is followed; titer[1] is read for K = 2 only */
  double ab_sd;                /* a_k, b_k ~ Normal(0, ab_sd): 1 alone, 0.5 combined (survival.py:121-122, 140-143) */
  double lam0_mu_mean;         /* _lam0_raw_mu ~ Normal(lam0_mu_mean, lam0_mu_sd): -3, 0.5 */
  double lam0_mu_sd;
  double lam0_sd_rate;         /* _lam0_raw_sd ~ Exponential(lam0_sd_rate): 2 */
  double lam0_z_sd;            /* __lam0_raw_z ~ Normal(0, lam0_z_sd): 1 */
} abd_survival_desc;

typedef struct abd_survival abd_survival;

/* Checks the descriptor and every cell (ABD_ERR_ARG; before the device is touched), copies the arrays to the device. */
int abd_survival_create(const abd_survival_desc* desc, abd_survival** out);
int abd_survival_destroy(abd_survival* s);
/* D = 2 K + 2 + T (T + Gr + 5 for a handle of abd_survival_create_groups, T + P + 5 for one of abd_survival_create_periods), or
 * -1 for NULL. */
int32_t abd_survival_dim(abd_survival* s);
/* logp[n] and grad[n][D] at theta[n][D]; up to ABD_MAX_BATCH points share a launch (more are split).  A point's result is
 * the same bits alone and in any batch. */
int abd_survival_logp_dlogp(abd_survival* s, int32_t n, const double* theta, double* logp, double* grad);
/* The raw device sums at one point, for parity tests: sums[T + 2 + K] = S_t[T], L, W_0, W_k[K] with
 * sigma = invlogit(eta), S_t = sum_j exposure sigma, L = sum_{infected > 0} infected log sigma,
 * w = (infected - exposure lam0_t sigma)(1 - sigma), W_0 = sum w, W_k = sum w titer_k. */
int abd_survival_loglik_sums(abd_survival* s, const double* theta, double* sums);

/* The survival model by group (reference survival.py:155-174: model_alone_groups): one titer, one shared slope b, and a
 * midpoint a_g per group of individuals under a hierarchical prior,
 *   infected[j, t] ~ Poisson(exposure[j, t] * lam0[t] * invlogit(b (titer[j, t] - a[group[j]])))
 *   theta[D] = _lam0_raw_mu, _lam0_raw_sd_log__, __lam0_raw_z[T], a_mu, a_sd_log__, _a_z[Gr], b        D = T + Gr + 5
 * (PyMC's creation order for this model; a_g = a_mu + exp(a_sd_log__) * _a_z_g).  The handle is an abd_survival: abd_survival_dim,
 * _logp_dlogp, _loglik_sums and _destroy work on it.  Its loglik_sums are sums[T + 2 + Gr] = S_t[T], L, W_x, W0_g[Gr] with S_t, L
 * and w as above, W_x = sum w titer, W0_g = sum of w over the individuals of group g. */
#define ABD_SURVIVAL_MAX_GROUPS 256

typedef struct {
  int32_t n_inds;              /* N >= 1 */
  int32_t n_intervals;         /* T, 1 <= T <= ABD_MAX_GAPS - 1 */
  int32_t n_groups;            /* Gr, 1 <= Gr <= ABD_SURVIVAL_MAX_GROUPS; a group may be empty */
  int32_t device;              /* HIP device ordinal; <0 = current device */
  const double* infected;      /* (N, T) row-major, as in abd_survival_desc */
  const double* exposure;      /* (N, T) row-major */
  const double* titer;         /* (N, T) row-major, finite wherever the cell is followed */
  const int32_t* group;        /* (N), each in [0, Gr) */
  double lam0_mu_mean;         /* _lam0_raw_mu ~ Normal(lam0_mu_mean, lam0_mu_sd): 0, 0.5 (this model passes no hyper_mu) */
  double lam0_mu_sd;
  double lam0_sd_rate;         /* _lam0_raw_sd ~ Exponential(lam0_sd_rate): 2 */
  double lam0_z_sd;            /* __lam0_raw_z ~ Normal(0, lam0_z_sd): 1 */
  double a_mu_sd;              /* a_mu ~ Normal(0, a_mu_sd): 0.5 */
  double a_sd_rate;            /* a_sd ~ Exponential(a_sd_rate): 2 */
  double a_z_sd;               /* _a_z ~ Normal(0, a_z_sd): 1 */
  double b_sd;                 /* b ~ Normal(0, b_sd): 0.5 */
} abd_survival_groups_desc;

/* Checks the descriptor, every label and every cell (ABD_ERR_ARG; before the device is touched), copies the arrays to the device
 * sorted by group. */
int abd_survival_create_groups(const abd_survival_groups_desc* desc, abd_survival** out);

/* The survival model by period (put together from the reference's helpers as model_alone_groups is, for the fits that
 * plotting.plot_protection(interval=) and plot_protection_timevariable read): one titer, one shared slope b, and a midpoint a_p
 * per period of time under a hierarchical prior, every interval t belonging to one period p(t),
 *   infected[j, t] ~ Poisson(exposure[j, t] * lam0[t] * invlogit(b (titer[j, t] - a[period[t]])))
 *   theta[D] = _lam0_raw_mu, _lam0_raw_sd_log__, __lam0_raw_z[T], a_mu, a_sd_log__, _a_z[P], b        D = T + P + 5
 * (the grouped layout with Gr -> P; a_p = a_mu + exp(a_sd_log__) * _a_z_p).  P = T with period[t] = t is the time-variable model,
 * P = 2 or 3 one midpoint per variant era; the labels need not be monotone.  The handle is an abd_survival: abd_survival_dim,
 * _logp_dlogp, _loglik_sums, _individual_loglik, the three _waic_* and _destroy work on it.  Its loglik_sums are
 * sums[2 T + 2] = S_t[T], L, W_x, W0_t[T] with S_t, L and w as above, W_x = sum w titer, W0_t = sum of w over the individuals in
 * interval t; the library folds W0_t into W0_p = sum_{t in p} W0_t on the host (d/da_p = -b W0_p). */
typedef struct {
  int32_t n_inds;              /* N >= 1 */
  int32_t n_intervals;         /* T, 1 <= T <= ABD_MAX_GAPS - 1 */
  int32_t n_periods;           /* P, 1 <= P <= T; a period may be without intervals (its _a_z sees its prior alone) */
  int32_t device;              /* HIP device ordinal; <0 = current device */
  const double* infected;      /* (N, T) row-major, as in abd_survival_desc */
  const double* exposure;      /* (N, T) row-major */
  const double* titer;         /* (N, T) row-major, finite wherever the cell is followed */
  const int32_t* period;       /* (T), each in [0, P) */
  double lam0_mu_mean;         /* _lam0_raw_mu ~ Normal(lam0_mu_mean, lam0_mu_sd): -3, 0.5 (hyper_mu = -3, as model_alone) */
  double lam0_mu_sd;
  double lam0_sd_rate;         /* _lam0_raw_sd ~ Exponential(lam0_sd_rate): 2 */
  double lam0_z_sd;            /* __lam0_raw_z ~ Normal(0, lam0_z_sd): 1 */
  double a_mu_sd;              /* a_mu ~ Normal(0, a_mu_sd): 0.5 */
  double a_sd_rate;            /* a_sd ~ Exponential(a_sd_rate): 2 */
  double a_z_sd;               /* _a_z ~ Normal(0, a_z_sd): 1 */
  double b_sd;                 /* b ~ Normal(0, b_sd): 0.5 */
} abd_survival_periods_desc;

/* Checks the descriptor, every label and every cell (ABD_ERR_ARG; before the device is touched), copies the arrays to the device
 * in the caller's order of individuals. */
int abd_survival_create_periods(const abd_survival_periods_desc* desc, abd_survival** out);

/* The per-individual log-likelihood of a handle of any kind, for comparing fitted models of one cohort (WAIC by individual):
 *   ll[p][j] = sum_t log Poisson(infected[j, t] | exposure[j, t] * lam0[t] * invlogit(eta[j, t]))
 * at theta[n][D] in the handle's layout, with PyMC's convention for fractional infected
 * (y log mu - mu - lgamma(y + 1), a cell with y = 0 has no log term).  ll is (n, N) row-major in the caller's order of
 * individuals, also for a grouped handle; an individual without a followed cell gets exactly 0.  Any n: up to ABD_MAX_BATCH
 * points share a launch.  A point's row is the same bits alone and in any batch; sum_j ll[p][j] is the data part of logp. */
int abd_survival_individual_loglik(abd_survival* s, int32_t n, const double* theta, double* ll);
/* Running statistics of ll[.][j] over draws, kept on the device.  _accumulate folds the n draws of theta[n][D] in order (any n;
 * the result does not depend on how the draws are split over calls); _reset forgets all draws; _stats reads, in the caller's
 * order of individuals, lse[N] = log sum_draws exp(ll), mean[N], m2[N] = sum_draws (ll - mean)^2, the number of draws folded and
 * n_cells[N], every individual's number of followed cells (exposure > 0).  _stats before any _accumulate is ABD_ERR_ARG. */
int abd_survival_waic_reset(abd_survival* s);
int abd_survival_waic_accumulate(abd_survival* s, int32_t n, const double* theta);
int abd_survival_waic_stats(abd_survival* s, double* lse, double* mean, double* m2, int64_t* n_draws, int32_t* n_cells);

/* PSIS-LOO by individual of a handle of any kind: the whole draws x individuals matrix of ll[.][j] is kept on the
 * device and every individual's column is Pareto-smoothed there (Vehtari et al. 2024 with r_eff = 1; the tail of
 * M = min(S / 5, ceil(3 sqrt(S))) draws, Zhang & Stephens' fit with the loo package's priors).
 * _reserve: room for `capacity` draws, 8 bytes per draw and slot of 64-padded individuals; forgets the draws held; 0 releases.
 *   ABD_ERR_ARG for a capacity that is negative or above ABD_SURVIVAL_LOO_MAX_DRAWS, ABD_ERR_NOMEM, the message naming the bytes,
 *   when the device cannot hold them.
 * _reset: forgets the draws held, keeps the room.
 * _accumulate: evaluates theta[n][D] (any n) and stores the rows as the next n draws; _append_rows stores the host rows ll[n][N]
 *   (the caller's order of individuals) in their place.  ABD_ERR_STATE, with nothing stored, when nothing is reserved or the draws
 *   would pass the capacity.  A stored row is the bits abd_survival_individual_loglik returns.
 * _rows: the draws first .. first + count - 1 back as ll[count][N]; ABD_ERR_ARG beyond the draws held.
 * _stats: over the S draws held, in the caller's order of individuals: elpd_loo[N], pareto_k[N] (+inf where the tail has at most 4
 *   draws), lppd[N] = log mean exp(ll), n_tail[N], the number of draws and n_cells[N]; an individual without a followed cell gets
 *   elpd_loo = lppd = 0, pareto_k = NaN, n_tail = 0.  The same bits however the draws were split over calls.  Consumes nothing: it
 *   may be called again after more draws.  ABD_ERR_ARG before any draw. */
#define ABD_SURVIVAL_LOO_MAX_DRAWS 16384
int abd_survival_loo_reserve(abd_survival* s, int64_t capacity);
int abd_survival_loo_reset(abd_survival* s);
int abd_survival_loo_accumulate(abd_survival* s, int32_t n, const double* theta);
int abd_survival_loo_append_rows(abd_survival* s, int32_t n, const double* ll);
int abd_survival_loo_rows(abd_survival* s, int64_t first, int64_t count, double* ll);
int abd_survival_loo_stats(abd_survival* s, double* elpd_loo, double* pareto_k, double* lppd, int32_t* n_tail, int64_t* n_draws,
                           int32_t* n_cells);

/* Posterior predictive checks of a handle of any kind.  For draw d and cell (j, t):
 *   mu = exposure[j, t] * lam0[t] * invlogit(eta[j, t]),   r ~ Poisson(mu)
 * where r is a function of (seed, d, the caller's index j, t) alone: Philox4x32-10 with key (seed lo, seed hi) and counter
 * (j, t, low word of d, 0x40000020), inverted sequentially.  Both are summed over the cells of titer bins and over individuals.
 *
 * _configure: n_var in {1, 2} binning variables, chosen freely (they need not be the model's own titer).  titers[v] is (N, T) in
 * the caller's order, edges[v] holds n_edges[v] <= 7 finite, strictly ascending edges; the bin of a cell is the number of edges
 * <= its titer, at most 8 bins.  Cells without follow-up belong to no bin.  Computes the constants of the data, uploads the bin
 * planes and sets the draw counter to 0.  ABD_ERR_ARG: n_var outside {1, 2}, more than 7 edges, edges not finite or not strictly
 * ascending, a non-finite titer in a followed cell, an exposure above 4; the handle keeps its earlier configuration then.  A
 * second call reconfigures. */
int abd_survival_predictive_configure(abd_survival* s, int32_t n_var, const double* const* titers, const int32_t* n_edges,
                                      const double* const* edges, uint64_t seed);
/* The draw counter back to 0: the next draw folded is draw 0 and the per-individual accumulators start again. */
int abd_survival_predictive_reset(abd_survival* s);
/* Folds the n draws theta[n][D] (any n; up to ABD_MAX_BATCH share a launch) as draws n0 .. n0 + n - 1, n0 the number folded since
 * the last reset or configuration.  expected[n][n_var][8] = sum of mu and replicate[n][n_var][8] = sum of r over the cells of
 * each bin (0 for a bin without followed cells).  Every output and every accumulator is the same bits however the draws are
 * split over calls.  ABD_ERR_ARG before _configure. */
int abd_survival_predictive_accumulate(abd_survival* s, int32_t n, const double* theta, double* expected, int64_t* replicate);
/* Per individual, in the caller's order, over the draws folded: sum_e[N] = sum_d sum_t mu, sum_r[N] = sum_d sum_t r, n_pos[N] =
 * the draws with sum_t r >= 1; n_draws.  ABD_ERR_ARG before _configure and before any draw. */
int abd_survival_predictive_stats(abd_survival* s, double* sum_e, int64_t* sum_r, int64_t* n_pos, int64_t* n_draws);
/* The constants of the configuration: observed[n_var][8] = sum of infected, person_time[n_var][8] = sum of exposure and
 * n_cells[n_var][8] = the followed cells of each bin (compensated sums on the host), observed_ind[N] = sum_t infected[j, t]. */
int abd_survival_predictive_observed(abd_survival* s, double* observed, double* person_time, int64_t* n_cells, double* observed_ind);
/* The per-cell replicates rep[n][N][T] (caller's order) of theta[n][D] as draws draw0 .. draw0 + n - 1: exactly the replicates
 * _accumulate draws for those indices.  Folds nothing and leaves the draw counter alone.  ABD_ERR_ARG before _configure. */
int abd_survival_replicate(abd_survival* s, int32_t n, const double* theta, int64_t draw0, int32_t* rep);

/* Per-draw fits: the model of abd_survival_desc over an ensemble of M datasets, one per recorded draw of the run, all
 * resident at once; every point of an evaluation names the dataset it is evaluated on, so that chains on different datasets
 * share a launch.  A dataset made from a draw's binary infections has event-time form: individual j is at risk (exposure 1) in
 * the intervals t < n_risk[j] and is infected in interval event[j], which is n_risk[j] - 1 or -1 (never infected while followed).
 * The handle is a type of its own: the per-individual, WAIC and predictive calls of abd_survival do not take it.  theta, D and
 * the priors are those of abd_survival_desc; the constant C of the data is 0 and Y_t counts the events of interval t. */
typedef struct {
  int32_t n_datasets;          /* M >= 1 */
  int32_t n_inds;              /* N >= 1 */
  int32_t n_intervals;         /* T, 1 <= T <= ABD_MAX_GAPS - 1 */
  int32_t n_titers;            /* K: 1 or 2 */
  int32_t device;              /* HIP device ordinal; <0 = current device */
  const int32_t* n_risk;       /* (M, N) row-major, each in [0, T] */
  const int32_t* event;        /* (M, N) row-major, each -1 or n_risk - 1 */
  const double* titer[2];      /* (M, T, N) row-major each: interval-major planes; finite wherever t < n_risk, anything elsewhere
                                  (it is not read into a sum); titer[1] is read for K = 2 only */
  double ab_sd;                /* the five priors of abd_survival_desc */
  double lam0_mu_mean;
  double lam0_mu_sd;
  double lam0_sd_rate;
  double lam0_z_sd;
} abd_survival_draws_desc;

typedef struct abd_survival_draws abd_survival_draws;

/* Checks the descriptor and every dataset (ABD_ERR_ARG, naming the dataset, the individual and the interval of the first
 * offender; before the device is touched), copies the titer planes and the two integers per individual to the device. */
int abd_survival_draws_create(const abd_survival_draws_desc* desc, abd_survival_draws** out);
int abd_survival_draws_destroy(abd_survival_draws* s);
/* D = 2 K + 2 + T (T + Gr + 5 for a handle of abd_survival_draws_create_groups, T + P + 5 for one of
 * abd_survival_draws_create_periods), or -1 for NULL. */
int32_t abd_survival_draws_dim(abd_survival_draws* s);
/* logp[n] and grad[n][D] at theta[n][D], point q on dataset[q] in [0, M) (ABD_ERR_ARG otherwise; nothing is launched then).  Any
 * n: up to ABD_MAX_BATCH points share a launch.  A point's result is the same bits alone, in any batch and in any row of it, and
 * the same bits an abd_survival handle made of that dataset's (infected, exposure, titer) arrays returns. */
int abd_survival_draws_logp_dlogp(abd_survival_draws* s, int32_t n, const int32_t* dataset, const double* theta, double* logp, double* grad);
/* The raw device sums of one point on one dataset, as abd_survival_loglik_sums: sums[T + 2 + K] (T + 2 + Gr for a handle of
 * abd_survival_draws_create_groups, 2 T + 2 for one of abd_survival_draws_create_periods). */
int abd_survival_draws_loglik_sums(abd_survival_draws* s, int32_t dataset, const double* theta, double* sums);

/* Per-draw fits of the models by group and by period: the model of abd_survival_groups_desc / abd_survival_periods_desc
 * over an ensemble of M datasets in event-time form.  The labels belong to the individuals (group) or to the intervals (period)
 * and are shared by all datasets.  The handle is an abd_survival_draws that knows its form, as an abd_survival does:
 * abd_survival_draws_dim (D = T + Gr + 5, or T + P + 5), _logp_dlogp, _loglik_sums and _destroy work on it.  theta and the
 * loglik_sums are those of the plug-in handle of the form; the constant C of the data is 0 and Y_t counts the events of interval t.
 * A point on dataset m returns, bit for bit, what a handle of abd_survival_create_groups / abd_survival_create_periods made of that
 * dataset's (infected, exposure, titer) and the same labels returns. */
typedef struct {
  int32_t n_datasets;          /* M >= 1 */
  int32_t n_inds;              /* N >= 1 */
  int32_t n_intervals;         /* T, 1 <= T <= ABD_MAX_GAPS - 1 */
  int32_t n_groups;            /* Gr, 1 <= Gr <= ABD_SURVIVAL_MAX_GROUPS; a group may be empty */
  int32_t device;              /* HIP device ordinal; <0 = current device */
  const int32_t* n_risk;       /* (M, N) row-major, each in [0, T] */
  const int32_t* event;        /* (M, N) row-major, each -1 or n_risk - 1 */
  const double* titer;         /* (M, T, N) row-major: interval-major planes; finite wherever t < n_risk, anything elsewhere */
  const int32_t* group;        /* (N), each in [0, Gr) */
  double lam0_mu_mean;         /* the eight priors of abd_survival_groups_desc, with its defaults: 0, 0.5 */
  double lam0_mu_sd;
  double lam0_sd_rate;         /* 2 */
  double lam0_z_sd;            /* 1 */
  double a_mu_sd;              /* 0.5 */
  double a_sd_rate;            /* 2 */
  double a_z_sd;               /* 1 */
  double b_sd;                 /* 0.5 */
} abd_survival_draws_groups_desc;

typedef struct {
  int32_t n_datasets;          /* M >= 1 */
  int32_t n_inds;              /* N >= 1 */
  int32_t n_intervals;         /* T, 1 <= T <= ABD_MAX_GAPS - 1 */
  int32_t n_periods;           /* P, 1 <= P <= T; a period may be without intervals */
  int32_t device;              /* HIP device ordinal; <0 = current device */
  const int32_t* n_risk;       /* (M, N) row-major, each in [0, T] */
  const int32_t* event;        /* (M, N) row-major, each -1 or n_risk - 1 */
  const double* titer;         /* (M, T, N) row-major: interval-major planes; finite wherever t < n_risk, anything elsewhere */
  const int32_t* period;       /* (T), each in [0, P) */
  double lam0_mu_mean;         /* the eight priors of abd_survival_periods_desc, with its defaults: -3, 0.5 */
  double lam0_mu_sd;
  double lam0_sd_rate;         /* 2 */
  double lam0_z_sd;            /* 1 */
  double a_mu_sd;              /* 0.5 */
  double a_sd_rate;            /* 2 */
  double a_z_sd;               /* 1 */
  double b_sd;                 /* 0.5 */
} abd_survival_draws_periods_desc;

/* Check the descriptor, every label and every dataset (ABD_ERR_ARG, before the device is touched: what abd_survival_draws_create
 * refuses, naming the dataset, the individual and the interval of the first offender, datasets in order; a label outside [0, Gr)
 * or [0, P); Gr outside [1, ABD_SURVIVAL_MAX_GROUPS]; P outside [1, T]; what the form's prior check refuses), then copy the titer
 * planes and the two integers per individual to the device -- by group in the plug-in handle's order, sorted by group and every
 * group padded to whole tiles of 64. */
int abd_survival_draws_create_groups(const abd_survival_draws_groups_desc* desc, abd_survival_draws** out);
int abd_survival_draws_create_periods(const abd_survival_draws_periods_desc* desc, abd_survival_draws** out);

/* Model comparison of per-draw fits: the per-individual log-likelihood, its WAIC statistics and PSIS-LOO of an
 * abd_survival_draws handle of any of the three creators, per dataset.  Every point names its dataset, point q is on dataset[q]
 * in [0, M) (ABD_ERR_ARG otherwise, "point q: dataset m outside [0, M)"; nothing is launched then); any n, up to ABD_MAX_BATCH
 * points of any datasets share a launch.  Per-individual outputs are in the caller's order of individuals, by group too.
 * _individual_loglik: ll[n][N]; a row on dataset m is, bit for bit, what abd_survival_individual_loglik returns on a handle of
 *   abd_survival_create / _create_groups / _create_periods made of that dataset's (infected, exposure, titer) and the same labels.
 * _waic_accumulate folds the rows of theta[n][D], each into the statistics of its own dataset, in order.  The statistics of dataset
 *   m depend on that dataset's rows and their order alone: not on how the rows were split over calls or launches, and not on which
 *   other datasets' rows stood between them; they are the bits of abd_survival_waic_* on the plug-in handle of that dataset.
 *   _waic_reset forgets all draws of all datasets.  _waic_stats: lse, mean, m2 [M][N], n_draws[M], n_cells[M][N] (= n_risk); a
 *   dataset without a draw holds NaN and n_draws = 0; ABD_ERR_ARG before any draw of any dataset.
 * _loo_reserve: room for `capacity` draws PER DATASET, 8 bytes per draw, dataset and slot of 64-padded individuals; forgets the
 *   draws held; 0 releases.  ABD_ERR_ARG for a capacity that is negative or above ABD_SURVIVAL_LOO_MAX_DRAWS, ABD_ERR_NOMEM, the
 *   message naming the bytes, when the device cannot hold them.  _loo_reset forgets the draws held, keeps the room.
 * _loo_accumulate evaluates theta[n][D] and stores every row as the next draw of its dataset.  ABD_ERR_STATE, before anything is
 *   launched and with nothing stored, when nothing is reserved or the rows of the call would take a dataset past the capacity.
 * _loo_stats: per dataset over the S_m draws it holds, the estimator of abd_survival_loo_stats with n_cells = n_risk: elpd_loo,
 *   pareto_k, lppd, n_tail [M][N] and n_draws[M]; the bits of abd_survival_loo_stats on the plug-in handle of that dataset with
 *   the same draws.  A dataset without a draw holds NaN, n_tail = 0 and n_draws = 0.  ABD_ERR_STATE when nothing is reserved,
 *   ABD_ERR_ARG before any draw of any dataset. */
int abd_survival_draws_individual_loglik(abd_survival_draws* s, int32_t n, const int32_t* dataset, const double* theta, double* ll);
int abd_survival_draws_waic_reset(abd_survival_draws* s);
int abd_survival_draws_waic_accumulate(abd_survival_draws* s, int32_t n, const int32_t* dataset, const double* theta);
int abd_survival_draws_waic_stats(abd_survival_draws* s, double* lse, double* mean, double* m2, int64_t* n_draws, int32_t* n_cells);
int abd_survival_draws_loo_reserve(abd_survival_draws* s, int64_t capacity_per_dataset);
int abd_survival_draws_loo_reset(abd_survival_draws* s);
int abd_survival_draws_loo_accumulate(abd_survival_draws* s, int32_t n, const int32_t* dataset, const double* theta);
int abd_survival_draws_loo_stats(abd_survival_draws* s, double* elpd_loo, double* pareto_k, double* lppd, int32_t* n_tail, int64_t* n_draws);

/* ---------------------------------------------------------------------------------------------------
 * Environment variables the library reads (all optional; read at abd_create / abd_sampler_create / first use).
 * This table is complete: the product library calls getenv for nothing else (development knobs of launch shapes
 * exist only in a tuning build compiled with -DABD_TUNING, tools/README.md).
 *
 *   variable             default             meaning
 *   ABD_PIPES            4                   HIP streams (one per hardware queue) that stream-ordered dense launches
 *                                            rotate over; 1 = every launch alone on the context's stream (profiling)
 *   ABD_OBS_LANES        by list density     observation lists: 1 = lane-per-observation kernel, 0 = wave-per-individual
 *   ABD_FORCE_SPARSE     0                   1 = keep a dense panel as observation lists (exercises the list kernels)
 *   ABD_DENSE_OWN_SUM    1                   0 = a sampler unit's launch is summed by a second launch (same bits; no leapfrog trains then)
 *   ABD_DENSE_PLANES     1                   0 = the dense and train kernels keep the exposure bookkeeping of the gap loop in the
 *                                            vector unit (legacy form) instead of reading the slots' exposure planes (same bits)
 *   ABD_SAMPLER_THREADS  1 dense / 4 lists   host threads that drive the native sampler's units (<= 8 are used)
 *   ABD_SAMPLER_UNIT     by cohort           chains per independent unit of the native sampler (dense: 1 up to 4 chains, 2 up to 7,
 *                                            4 beyond; 1, 2 or 4)
 *   ABD_SAMPLER_TRAINS   1                   0 = no leapfrog trains: the host sees every leapfrog before the next is queued
 *   ABD_SAMPLER_PROFILE  0                   1 = abd_sampler_run reports on stderr where the host thread's time went
 *   ABD_GIBBS_STATS      0                   1 = abd_gibbs_sweep reports the dense sweep's scheduler counters on stderr
 * (The Python layer adds ABD_HIP_LIB, the path of this library, and ABD_RECORD_BUDGET_GB, the host memory a process may spend
 * on per-draw (G, N) records; bench.py adds ABD_DIST_BACKEND.  The HIP runtime's HIP_FORCE_DEV_KERNARG must stay at its
 * default of 1: kernel arguments in host memory cost 3-5 us per launch.) */

#ifdef __cplusplus
}
#endif
#endif /* ABD_HIP_H */
