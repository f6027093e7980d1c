"""
A self-contained compound sampler for the model's two callables, used by ``abdpymc-infer`` when PyMC is not
installed: NUTS on the 17 continuous variables (calls ``logp_dlogp``) + binary Gibbs-Metropolis on
``[i_raw, ab_s_waner]`` (calls ``logp`` once per proposed flip) -- the step assignment ``pm.sample`` makes for
this model (reference call site abd.py:922).

The samplers only see callables, so they are tested on CPU against closed-form targets; on the GPU they are
driven by :class:`abdpymc_amd.model.AbdModel`.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, Optional, Tuple

import numpy as np

# ---------------------------------------------------------------------------------------------------
# NUTS (Hoffman & Gelman 2014, Algorithm 6: slice variant with dual-averaging step size), diagonal metric
# ---------------------------------------------------------------------------------------------------


class DualAveraging:
    def __init__(self, eps0: float, target: float = 0.8, gamma: float = 0.05, t0: float = 10.0, kappa: float = 0.75):
        self.mu = math.log(10.0 * eps0)
        self.target, self.gamma, self.t0, self.kappa = target, gamma, t0, kappa
        self.h_bar, self.log_eps_bar, self.m = 0.0, 0.0, 0
        self.eps = eps0

    def update(self, accept_stat: float) -> float:
        self.m += 1
        m = self.m
        self.h_bar = (1 - 1 / (m + self.t0)) * self.h_bar + (self.target - accept_stat) / (m + self.t0)
        log_eps = self.mu - math.sqrt(m) / self.gamma * self.h_bar
        eta = m ** (-self.kappa)
        self.log_eps_bar = eta * log_eps + (1 - eta) * self.log_eps_bar
        self.eps = math.exp(log_eps)
        return self.eps

    def final(self) -> float:
        return math.exp(self.log_eps_bar)


class Nuts:
    """One NUTS transition kernel over q in R^d for ``fn(q) -> (logp, grad)``."""

    def __init__(self, fn: Callable[[np.ndarray], Tuple[float, np.ndarray]], dim: int, rng: np.random.Generator,
                 max_treedepth: int = 10, target_accept: float = 0.8):
        self.fn, self.dim, self.rng = fn, dim, rng
        self.max_treedepth = max_treedepth
        self.inv_mass = np.ones(dim)  # diagonal M^-1 (posterior variances)
        self.da: Optional[DualAveraging] = None
        self.eps = 0.1
        self.target_accept = target_accept
        self.n_grad = 0

    def _grad(self, q):
        self.n_grad += 1
        lp, g = self.fn(q)
        if not np.isfinite(lp):
            return -np.inf, np.zeros_like(q)
        return float(lp), np.asarray(g, dtype=float)

    def _leapfrog(self, q, p, g, eps):
        p = p + 0.5 * eps * g
        q = q + eps * self.inv_mass * p
        lp, g = self._grad(q)
        p = p + 0.5 * eps * g
        return q, p, lp, g

    def _energy(self, lp, p):
        return lp - 0.5 * float(np.sum(self.inv_mass * p * p))

    def find_reasonable_eps(self, q, lp, g) -> float:
        eps = 0.1
        p = self.rng.standard_normal(self.dim) / np.sqrt(self.inv_mass)
        h0 = self._energy(lp, p)
        _, p1, lp1, _ = self._leapfrog(q, p, g, eps)
        dh = self._energy(lp1, p1) - h0
        a = 1.0 if (np.isfinite(dh) and dh > math.log(0.5)) else -1.0
        for _ in range(50):
            if not np.isfinite(dh):
                dh = -np.inf
            if a * dh <= -a * math.log(2.0):
                break
            eps *= 2.0**a
            _, p1, lp1, _ = self._leapfrog(q, p, g, eps)
            dh = self._energy(lp1, p1) - h0
        return eps

    def _build(self, q, p, g, log_u, v, j, eps, h0):
        if j == 0:
            q1, p1, lp1, g1 = self._leapfrog(q, p, g, v * eps)
            h1 = self._energy(lp1, p1)
            if not np.isfinite(h1):
                h1 = -np.inf
            n1 = int(log_u <= h1)
            s1 = log_u < h1 + 1000.0
            alpha = min(1.0, math.exp(min(0.0, h1 - h0))) if np.isfinite(h1) else 0.0
            return q1, p1, g1, q1, p1, g1, q1, lp1, g1, n1, s1, alpha, 1
        qm, pm, gm, qp, pp, gp, q1, lp1, g1, n1, s1, a1, na1 = self._build(q, p, g, log_u, v, j - 1, eps, h0)
        if s1:
            if v == -1:
                qm, pm, gm, _, _, _, q2, lp2, g2, n2, s2, a2, na2 = self._build(qm, pm, gm, log_u, v, j - 1, eps, h0)
            else:
                _, _, _, qp, pp, gp, q2, lp2, g2, n2, s2, a2, na2 = self._build(qp, pp, gp, log_u, v, j - 1, eps, h0)
            if n2 > 0 and self.rng.random() < n2 / max(n1 + n2, 1):
                q1, lp1, g1 = q2, lp2, g2
            a1, na1 = a1 + a2, na1 + na2
            dq = qp - qm
            s1 = s2 and float(np.dot(dq, self.inv_mass * pm)) >= 0 and float(np.dot(dq, self.inv_mass * pp)) >= 0
            n1 += n2
        return qm, pm, gm, qp, pp, gp, q1, lp1, g1, n1, s1, a1, na1

    def step(self, q, lp, g, adapt: bool):
        """One transition.  Returns (q, logp, grad, stats)."""
        eps = self.eps
        p0 = self.rng.standard_normal(self.dim) / np.sqrt(self.inv_mass)
        h0 = self._energy(lp, p0)
        log_u = h0 + math.log(self.rng.random() + 1e-300)
        qm = qp = q
        pm = pp = p0
        gm = gp = g
        j, n, s = 0, 1, True
        q_new, lp_new, g_new = q, lp, g
        alpha, n_alpha = 0.0, 1
        while s and j < self.max_treedepth:
            v = -1 if self.rng.random() < 0.5 else 1
            if v == -1:
                qm, pm, gm, _, _, _, q1, lp1, g1, n1, s1, alpha, n_alpha = self._build(qm, pm, gm, log_u, v, j, eps, h0)
            else:
                _, _, _, qp, pp, gp, q1, lp1, g1, n1, s1, alpha, n_alpha = self._build(qp, pp, gp, log_u, v, j, eps, h0)
            if s1 and self.rng.random() < min(1.0, n1 / n):
                q_new, lp_new, g_new = q1, lp1, g1
            n += n1
            dq = qp - qm
            s = s1 and float(np.dot(dq, self.inv_mass * pm)) >= 0 and float(np.dot(dq, self.inv_mass * pp)) >= 0
            j += 1
        acc = alpha / max(n_alpha, 1)
        if adapt and self.da is not None:
            self.eps = self.da.update(acc)
        return q_new, lp_new, g_new, dict(tree_depth=j, mean_tree_accept=acc, step_size=eps, n_steps=n_alpha,
                                          diverging=not s and j < self.max_treedepth and acc == 0.0)


# ---------------------------------------------------------------------------------------------------
# Binary Gibbs-Metropolis (PyMC's BinaryGibbsMetropolis.astep semantics: transit_p = 0.8, shuffled order)
# ---------------------------------------------------------------------------------------------------


def binary_gibbs_sweep(n_bits: int, flip_logp: Callable[[int], float], unflip: Callable[[int], None], logp_curr: float,
                       rng: np.random.Generator, transit_p: float = 0.8):
    """
    One sweep over all binary dims in random order.  ``flip_logp(idx)`` flips bit idx of the resident state
    and returns the joint logp there; ``unflip(idx)`` reverts a rejected flip.  Returns (logp, n_accepted,
    n_proposed).
    """
    order = rng.permutation(n_bits)
    propose = rng.random(n_bits) < transit_p
    n_acc = n_prop = 0
    for idx, do in zip(order, propose):
        if not do:
            continue  # same value proposed: nothing to evaluate
        n_prop += 1
        lp_prop = flip_logp(int(idx))
        d = lp_prop - logp_curr
        if np.isfinite(lp_prop) and (d >= 0 or math.log(rng.random() + 1e-300) < d):
            logp_curr = lp_prop
            n_acc += 1
        else:
            unflip(int(idx))
    return logp_curr, n_acc, n_prop


# ---------------------------------------------------------------------------------------------------
# Compound driver for one chain of the abd model
# ---------------------------------------------------------------------------------------------------


def sample_chain(model, chain: int, tune: int, draws: int, seed: int, record_deterministics: bool = True,
                 progress: Optional[Callable[[int, int], None]] = None, device_gibbs: bool = True) -> Dict[str, np.ndarray]:
    """Run tune + draws iterations of [NUTS; binary Gibbs] on chain slot ``chain`` of an AbdModel."""
    from .model import THETA_NAMES, constrain

    rng = np.random.default_rng([seed, chain])
    ctx = model.ctx
    G, N = model.n_gaps, model.n_inds
    pt = model.initial_point()
    i_raw = pt["i_raw"].astype(np.int8)
    waner = pt["ab_s_waner"].astype(np.int8)
    ctx.set_discrete(chain, i_raw, waner)
    q = model.ravel(pt) + rng.uniform(-1, 1, size=len(THETA_NAMES))  # start jitter U(-1, 1) on the value variables: pm.sample's default init 'jitter+adapt_diag'

    def fn(x):
        return ctx.logp_dlogp(chain, x)

    nuts = Nuts(fn, len(THETA_NAMES), rng)
    lp, g = fn(q)
    nuts.eps = nuts.find_reasonable_eps(q, lp, g)
    nuts.da = DualAveraging(nuts.eps)

    n_bits = G * N + N
    use_device_sweep = hasattr(ctx, "gibbs_sweep") and device_gibbs

    # host-driven fallback (one joint-logp evaluation per proposed flip, the reference's cost model)
    def flip_logp(idx):
        ctx.flip_discrete(chain, idx)
        if idx < G * N:
            i_raw.ravel()[idx] ^= 1
        else:
            waner[idx - G * N] ^= 1
        return ctx.logp(chain, q)

    def unflip(idx):
        ctx.flip_discrete(chain, idx)
        if idx < G * N:
            i_raw.ravel()[idx] ^= 1
        else:
            waner[idx - G * N] ^= 1

    out_q = np.empty((draws, len(THETA_NAMES)))
    out_i_raw = np.empty((draws, G, N), dtype=np.int8)
    out_w = np.empty((draws, N), dtype=np.int8)
    stats = {k: np.empty(draws) for k in ("lp", "tree_depth", "mean_tree_accept", "step_size", "n_steps", "gibbs_accept")}
    det = None
    if record_deterministics:
        det = dict(i=np.empty((draws, G, N), dtype=np.int8), ab_n_mu=np.empty((draws, G, N)), ab_s_mu=np.empty((draws, G, N)))

    # mass-matrix adaptation: variances of the tuning draws in expanding windows
    window_start, window_len = max(10, tune // 10), max(20, tune // 8)
    window = []
    for it in range(tune + draws):
        tuning = it < tune
        q, lp, g, st = nuts.step(q, lp, g, adapt=tuning)
        if use_device_sweep:
            # the whole sweep in one launch: each individual's G + 1 proposals on its own wave (abd_gibbs.hpp)
            acc, prop = ctx.gibbs_sweep([chain], q[None, :], seed=(seed << 20) ^ 0x5EED, sweep=it)
            n_acc, n_prop = int(acc[0]), int(prop[0])
            if not tuning:
                i_raw, waner = ctx.get_discrete(chain)
        else:
            lp, n_acc, n_prop = binary_gibbs_sweep(n_bits, flip_logp, unflip, lp, rng)
        lp, g = fn(q)  # logp and gradient at the new discrete state
        if tuning:
            if it >= window_start:
                window.append(q.copy())
            if len(window) >= window_len and it < tune - 20:
                var = np.var(np.asarray(window), axis=0)
                nuts.inv_mass = (len(window) / (len(window) + 5.0)) * var + 1e-3 * (5.0 / (len(window) + 5.0))
                window, window_len = [], int(window_len * 1.5)
                nuts.eps = nuts.find_reasonable_eps(q, lp, g)
                nuts.da = DualAveraging(nuts.eps)
            if it == tune - 1:
                nuts.eps = nuts.da.final()
        else:
            k = it - tune
            out_q[k] = q
            out_i_raw[k] = i_raw
            out_w[k] = waner
            stats["lp"][k] = lp
            for name in ("tree_depth", "mean_tree_accept", "step_size", "n_steps"):
                stats[name][k] = st[name]
            stats["gibbs_accept"][k] = n_acc / max(n_prop, 1)
            if det is not None:
                d_i, d_n, d_s = ctx.deterministics(chain, q)
                det["i"][k], det["ab_n_mu"][k], det["ab_s_mu"][k] = d_i, d_n, d_s
        if progress is not None:
            progress(it + 1, tune + draws)

    res = {name: out_q[:, k].copy() for k, name in enumerate(THETA_NAMES)}
    res.update(constrain(out_q))
    res["i_raw"] = out_i_raw
    res["ab_s_waner"] = out_w
    if det is not None:
        res.update(det)
    res.update({f"stat_{k}": v for k, v in stats.items()})
    res["n_grad_evals"] = np.asarray(nuts.n_grad)
    return res


def record_bytes(chains: int, n_rec: int, G: int, N: int, record_deterministics: bool, record_discrete: bool,
                 n_readings: int = 0, n_replicates: int = 0) -> int:
    """Host bytes of the per-draw arrays of a run that records ``n_rec`` draws per chain: i (int8) + ab_n_mu + ab_s_mu
    (float64) per cell for the Deterministics, i_raw (int8) per cell + ab_s_waner (int8) per individual for the discrete state,
    a float64 per OD reading for the pointwise log-likelihood (``n_readings``: readings of both antigens; 0 = not recorded)
    and a float64 per OD reading for the posterior predictive replicates (``n_replicates``; 0 = not recorded)."""
    per_draw = ((G * N * 17 if record_deterministics else 0) + (G * N + N if record_discrete else 0) + 8 * int(n_readings)
                + 8 * int(n_replicates))
    return chains * n_rec * per_draw


def record_budget_bytes() -> int:
    """What the per-draw arrays of one process may take on the host (``ABD_RECORD_BUDGET_GB``, default 8 GiB)."""
    import os

    return int(float(os.environ.get("ABD_RECORD_BUDGET_GB", "8")) * 2 ** 30)


def sample_native(model, tune: int, draws: int, chains: int = 1, seed: int = 0, record_deterministics: bool = True,
                  record_discrete: bool = True, progress: Optional[Callable[[int, int, int], None]] = None,
                  target_accept: float = 0.8, max_treedepth: int = 10, chunk: int = 50,
                  chain_offset: int = 0, dense_metric: bool = False, thin: int = 1,
                  budget_bytes: Optional[int] = None, log_likelihood: bool = False,
                  waic: bool = False, posterior_predictive: bool = False, ppc: bool = False, curves: bool = False,
                  sero_thresholds=None, diagnostics: bool = False, diag_batch: Optional[int] = None,
                  risk=None, timelines: bool = False, timeline_ranges=((-4, 8), (-4, 8)), timeline_q=(0.025, 0.5, 0.975),
                  timelines_hist: bool = False) -> Dict[str, np.ndarray]:
    """
    The compound step inside the library (``abd_sampler_*``): the chains advance as independent units, each at its own
    pace (NUTS transitions as leapfrog trains on the device, the Gibbs sweep, the re-evaluation at the new state); nothing
    a chain draws depends on the others.  Posterior means of the three Deterministics over ALL draws are accumulated on
    the device and returned as ``mean_i``, ``mean_ab_n_mu``, ``mean_ab_s_mu`` (what the reference's downstream analysis
    reads: survival.py:64-69, 105-114); per-draw copies of the (gap, ind) arrays only when asked for, and only of every
    ``thin``-th draw (draws 0, thin, 2 thin, ...: ``draw_index``) -- the reference keeps every draw and thins afterwards
    (subsample_idata.py); at BASELINE config 3 a draw is 36 MB per chain, so here it is done while sampling.  The 17
    value variables and the sampler statistics are kept for every draw.  A run whose per-draw arrays would exceed
    ``budget_bytes`` on the host (default ``record_budget_bytes()``) is refused with the ``thin`` that would fit.
    ``chain_offset`` is the global id of this process's first chain when chains are sharded over GPUs: local
    chain c uses the random streams of global chain ``chain_offset + c``.

    ``log_likelihood``: also record the pointwise log-likelihood of every OD reading at the recorded draws (thinned like the
    (gap, ind) arrays) as ``log_likelihood_it_s_lik`` / ``log_likelihood_it_n_lik`` (chains, n_rec, K), what
    ``pm.compute_log_likelihood`` adds to an InferenceData.  ``waic``: accumulate its per-reading statistics over ALL
    draws on the device (any cohort size) and return them as ``waic_lse`` / ``waic_mean`` / ``waic_m2`` (chains, K_s + K_n;
    S readings first), ``waic_n_draws`` (chains,) and ``waic_n_obs`` (chains, 2) = (K_s, K_n): ``compare.waic`` reads them.

    ``posterior_predictive``: also record a posterior predictive replicate of every OD reading at the recorded draws (thinned
    likewise) as ``posterior_predictive_it_s_lik`` / ``posterior_predictive_it_n_lik`` (chains, n_rec, K), what
    ``pm.sample_posterior_predictive`` returns; chain c's replicate of iteration t (tune included) is
    ``Context.posterior_predictive(.., seed, chain_offset + c, t)`` (``predictive.sample_posterior_predictive``).  ``ppc``:
    accumulate per-reading check statistics over ALL draws on the device -- ``ppc_mean`` / ``ppc_m2`` (mean and sum of squared
    deviations of the predictive mean) and ``ppc_pit`` (mean of P(y_rep <= y | draw)), each (chains, K_s + K_n), S readings
    first, ``ppc_n_draws`` (chains,) and ``ppc_n_obs`` (chains, 2): ``predictive.summary`` reads them.  Neither option draws
    from any random stream the chains use: their trajectories do not change.

    ``curves``: keep the epidemic curves of EVERY draw, reduced over the individuals on the device (``curves.py``; ``thin`` does
    not apply): ``curves_infected`` / ``curves_ever_infected`` / ``curves_seropos_s`` / ``curves_seropos_n`` (counts) and
    ``curves_titer_s`` / ``curves_titer_n`` (titer sums), each (chains, draws, G), ``curves_n_infections`` (chains, draws, 8) and
    ``curves_n_followed`` (chains, G); ``curves.summary`` reads them.  An individual counts up to its last serum sample
    (``model.data.last_gap`` where the model's data has one, else every gap); ``sero_thresholds`` = (thr_s, thr_n) on the titer
    scale switch the seropositive counts on.  The trajectories do not change either.

    ``diagnostics``: accumulate per cell, over ALL draws on the device, what split R-hat and a batch-means effective sample size
    of ``i``, ``ab_n_mu``, ``ab_s_mu`` need (``diagnostics.py``; ``thin`` does not apply): ``diag_i_counts`` (chains, 4, G, N) int64,
    ``diag_ab_n_mu`` / ``diag_ab_s_mu`` (chains, 6, G, N) and ``diag_info`` (chains, 4); ``diagnostics.rhat`` / ``ess`` / ``summary``
    read them.  ``diag_batch`` is the batch length (default ``max(1, floor(sqrt(draws // 2)))``).  Needs ``draws >= 2``; the
    arrays' host bytes count against ``budget_bytes``.  The trajectories do not change either.

    ``risk`` = a ``risk.spec``: keep the infection-risk-by-titer table of EVERY draw, reduced over the individuals on the device
    (``risk.py``; ``thin`` does not apply): ``risk_table`` (chains, draws, 2, 2, G, 8) int64 -- antigen (S, N) x (at risk, events)
    x gap x bin of the previous gap's titer -- and the spec, one row per chain: ``risk_edges_s`` / ``risk_edges_n`` (chains, 7),
    NaN beyond the edges given, and ``risk_window`` (chains, 3) = (start, end, first_only); ``risk.summary`` reads them.  The
    follow-up is the curves'.  The table's host bytes count against ``budget_bytes``.  The trajectories do not change either.

    ``timelines``: accumulate per cell, over ALL draws on the device, what a per-individual timeline needs (``timelines.py``;
    ``thin`` does not apply): histograms of the two titers over ``timeline_ranges`` = ((lo_n, hi_n), (lo_s, hi_s)) (default: the
    reference's plot range) and the infection timing counters.  Per chain ``tl_inf`` / ``tl_cum`` (chains, G, N) int64 -- draws
    with an infection in the cell; with one so far in the cell's time chunk --, ``tl_ninf`` (chains, N, 8) int64 -- draws by the
    number of infections within follow-up (the curves') --, ``tl_info`` (chains, 1) the draws, ``tl_range`` (chains, 2, 2) and
    ``tl_q`` (chains, Q); pooled over the chains by a device kernel ``tl_q_n`` / ``tl_q_s`` (Q, G, N), the quantiles ``timeline_q``
    (1 to 8 levels; ``timelines.summary`` reads the smallest, the one nearest 0.5 and the largest as lower, median and upper;
    ``None``: no pooled quantiles, none of the three keys -- for a caller that pools the histograms of several processes itself)
    of ``ab_n_mu`` / ``ab_s_mu``; with ``timelines_hist`` also the histograms ``tl_hist_n`` / ``tl_hist_s`` (chains,
    G, N, 64) uint16.  ``timelines.summary`` / ``individual`` read them.  At most 65535 draws per chain; the arrays' host bytes
    count against ``budget_bytes``.  The trajectories do not change either.
    """
    from . import curves as curves_mod
    from . import timelines as tl_mod
    from . import diagnostics as diag_mod
    from . import risk as risk_mod
    from .model import THETA_NAMES, constrain

    ctx = model.ctx
    G, N = model.n_gaps, model.n_inds
    if thin < 1:
        raise ValueError(f"thin must be >= 1, got {thin}")
    n_rec = (draws + thin - 1) // thin
    K_s, K_n = (ctx.n_obs_s, ctx.n_obs_n) if (log_likelihood or waic or posterior_predictive or ppc) else (0, 0)  # readings of it_s_lik / it_n_lik
    per_reading = log_likelihood or posterior_predictive  # per-draw rows of the readings
    if diagnostics:
        if draws < 2:
            raise ValueError(f"diagnostics need draws >= 2 (two half-chains), got {draws}")
        diag_batch = diag_mod.default_batch(draws) if diag_batch is None else int(diag_batch)
        if diag_batch < 1:
            raise ValueError(f"diag_batch must be >= 1, got {diag_batch}")
    if record_deterministics or record_discrete or per_reading:
        budget = record_budget_bytes() if budget_bytes is None else int(budget_bytes)
        need = record_bytes(chains, n_rec, G, N, record_deterministics, record_discrete,
                            n_readings=(K_s + K_n) if log_likelihood else 0,
                            n_replicates=(K_s + K_n) if posterior_predictive else 0)
        if need > budget:
            per_draw = need // max(n_rec, 1)
            fit = max(1, budget // max(per_draw, 1))          # draws per chain set that fit
            thin_fit = -(-draws // fit)
            raise ValueError(
                f"recording {n_rec} draws of {chains} chains x ({G}, {N}) needs {need / 2 ** 30:.1f} GiB of host arrays, over the "
                f"budget of {budget / 2 ** 30:.1f} GiB: thin >= {thin_fit} fits (or record less: no_deterministics / "
                f"record_discrete=False; the posterior means are returned either way; ABD_RECORD_BUDGET_GB raises the budget)")
    if diagnostics:
        budget = record_budget_bytes() if budget_bytes is None else int(budget_bytes)
        own = diag_mod.result_bytes(chains, G, N)
        need = own + record_bytes(chains, n_rec, G, N, record_deterministics, record_discrete,
                                  n_readings=(K_s + K_n) if log_likelihood else 0,
                                  n_replicates=(K_s + K_n) if posterior_predictive else 0)
        if need > budget:
            raise ValueError(
                f"the diagnostics of {chains} chains x ({G}, {N}) take {own / 2 ** 30:.2f} GiB of host arrays (16 planes of 8 bytes "
                f"per cell and chain) and the recorded draws {(need - own) / 2 ** 30:.2f} GiB, over the budget of "
                f"{budget / 2 ** 30:.2f} GiB: record fewer draws (thin, no_deterministics / record_discrete=False) or raise "
                f"ABD_RECORD_BUDGET_GB")
    if risk is not None:
        risk = risk_mod.spec(risk["start"], risk["end"], risk["edges_s"], risk["edges_n"], risk["first_only"], n_gaps=G)
        budget = record_budget_bytes() if budget_bytes is None else int(budget_bytes)
        own = chains * draws * 4 * G * risk_mod.N_BINS * 8
        need = own + (diag_mod.result_bytes(chains, G, N) if diagnostics else 0) + record_bytes(
            chains, n_rec, G, N, record_deterministics, record_discrete, n_readings=(K_s + K_n) if log_likelihood else 0,
            n_replicates=(K_s + K_n) if posterior_predictive else 0)
        if need > budget:
            raise ValueError(
                f"the risk tables of {chains} chains x {draws} draws x {G} gaps take {own / 2 ** 30:.2f} GiB of host arrays (32 counts "
                f"of 8 bytes per gap and draw) and the other recorded arrays {(need - own) / 2 ** 30:.2f} GiB, over the budget of "
                f"{budget / 2 ** 30:.2f} GiB: fewer draws, record less (thin, no_deterministics / record_discrete=False) or raise "
                f"ABD_RECORD_BUDGET_GB")
    if timelines:
        timeline_ranges = tuple(tl_mod.check_range(*r) for r in timeline_ranges)
        if len(timeline_ranges) != 2:
            raise ValueError("timeline_ranges must be ((lo_n, hi_n), (lo_s, hi_s))")
        pooled = timeline_q is not None  # (None: the device's pooled quantiles are not read out)
        timeline_q = np.atleast_1d(np.asarray(timeline_q if pooled else [0.5], dtype=np.float64))
        if timeline_q.ndim != 1 or not 1 <= timeline_q.size <= tl_mod.MAX_Q or not ((timeline_q >= 0) & (timeline_q <= 1)).all():
            raise ValueError(f"timeline_q must be 1 to {tl_mod.MAX_Q} numbers in [0, 1]")
        if not 1 <= draws <= tl_mod.MAX_DRAWS:
            raise ValueError(f"timelines count in 16 bits: 1 to {tl_mod.MAX_DRAWS} draws per chain, got {draws}")
        budget = record_budget_bytes() if budget_bytes is None else int(budget_bytes)
        own = tl_mod.result_bytes(chains, G, N, timeline_q.size if pooled else 0, timelines_hist)
        need = own + (diag_mod.result_bytes(chains, G, N) if diagnostics else 0) + (
            chains * draws * 4 * G * risk_mod.N_BINS * 8 if risk is not None else 0) + record_bytes(
            chains, n_rec, G, N, record_deterministics, record_discrete, n_readings=(K_s + K_n) if log_likelihood else 0,
            n_replicates=(K_s + K_n) if posterior_predictive else 0)
        if need > budget:
            raise ValueError(
                f"the timelines of {chains} chains x ({G}, {N}) take {own / 2 ** 30:.2f} GiB ({own} bytes) of host arrays"
                f"{' (the histograms: 256 bytes per cell and chain)' if timelines_hist else ''} and the other recorded arrays "
                f"{(need - own) / 2 ** 30:.2f} GiB, over the budget of {budget / 2 ** 30:.2f} GiB: record less (thin, "
                f"no_deterministics / record_discrete=False) or raise ABD_RECORD_BUDGET_GB")
    chunk = max(thin, chunk - chunk % thin) if thin > 1 else chunk  # calls record iterations 0, thin, ... of THEIR range
    pt = model.initial_point()
    q0 = np.empty((chains, len(THETA_NAMES)))
    for c in range(chains):
        rng = np.random.default_rng([seed, chain_offset + c])
        ctx.set_discrete(c, pt["i_raw"].astype(np.int8), pt["ab_s_waner"].astype(np.int8))
        q0[c] = model.ravel(pt) + rng.uniform(-1, 1, size=len(THETA_NAMES))  # start jitter U(-1, 1) on the value variables: pm.sample's default init 'jitter+adapt_diag'
    smp = ctx.sampler(np.arange(chains), q0, tune=tune, seed=seed, target_accept=target_accept,
                      max_treedepth=max_treedepth, gibbs=True, accumulate=True, chain_offset=chain_offset,
                      dense_metric=dense_metric, pointwise=waic, predictive=ppc, curves=draws if curves else 0,
                      sero_thresholds=sero_thresholds, diagnostics=(draws, diag_batch) if diagnostics else None,
                      risk=draws if risk is not None else 0, risk_spec=risk,
                      timelines=(draws, *timeline_ranges) if timelines else None)
    if curves or risk is not None or timelines:
        last_gap = getattr(getattr(model, "data", None), "last_gap", None)
        ctx.set_follow_up(last_gap)
    n_grad = chains  # the evaluation at the starting points
    done = 0

    def advance(n):
        nonlocal done, n_grad
        th, st = smp.run(n)
        n_grad += int(st["n_steps"].sum()) + n * chains  # leapfrogs + the re-evaluation after each sweep
        done += n
        if progress is not None:
            for c in range(chains):
                progress(c, done, tune + draws)
        return th, st

    left = tune
    while left > 0:
        advance(min(chunk, left))
        left -= min(chunk, left)
    thetas, stats = [], []
    out_i_raw = np.empty((chains, n_rec, G, N), dtype=np.int8) if record_discrete else None
    out_w = np.empty((chains, n_rec, N), dtype=np.int8) if record_discrete else None
    det = None
    if record_deterministics:
        det = dict(i=np.empty((chains, n_rec, G, N), dtype=np.int8), ab_n_mu=np.empty((chains, n_rec, G, N)),
                   ab_s_mu=np.empty((chains, n_rec, G, N)))
    ll = dict(ll_s=np.empty((chains, n_rec, K_s)), ll_n=np.empty((chains, n_rec, K_n))) if log_likelihood else {}
    if posterior_predictive:
        ll.update(yrep_s=np.empty((chains, n_rec, K_s)), yrep_n=np.empty((chains, n_rec, K_n)))
    k = 0
    while k < draws:
        n = min(chunk, draws - k)
        if record_deterministics or record_discrete or per_reading:
            # staged on the device, copied out in large blocks straight into the arrays above
            th, st = smp.run_record(n, k // thin, i_raw=out_i_raw, ab_s_waner=out_w, thin=thin, **(det or {}), **ll)
            n_grad += int(st["n_steps"].sum()) + n * chains
            done += n
            if progress is not None:
                for c in range(chains):
                    progress(c, done, tune + draws)
        else:
            th, st = advance(n)
        thetas.append(th)
        stats.append(st)
        k += n
    out_q = np.concatenate(thetas, axis=1) if thetas else np.empty((chains, 0, len(THETA_NAMES)))
    res = {name: out_q[:, :, j].copy() for j, name in enumerate(THETA_NAMES)}
    res.update(constrain(out_q))
    if record_discrete:
        res["i_raw"], res["ab_s_waner"] = out_i_raw, out_w
    if det is not None:
        res.update(det)
    if log_likelihood:
        res["log_likelihood_it_s_lik"], res["log_likelihood_it_n_lik"] = ll["ll_s"], ll["ll_n"]
    if posterior_predictive:
        res["posterior_predictive_it_s_lik"], res["posterior_predictive_it_n_lik"] = ll["yrep_s"], ll["yrep_n"]
    for on, stats_of, prefix, names in ((waic, smp.pointwise_stats, "waic", ("lse", "mean", "m2")),
                                        (ppc, smp.predictive_stats, "ppc", ("mean", "m2", "pit"))):
        if not on:
            continue
        per_chain = [stats_of(c) for c in range(chains)]
        for j, name in enumerate(names):
            res[f"{prefix}_{name}"] = np.stack([o[j] for o, _ in per_chain])
        res[f"{prefix}_n_draws"] = np.array([n for _, n in per_chain], dtype=np.int64)
        res[f"{prefix}_n_obs"] = np.tile(np.array([K_s, K_n], dtype=np.int64), (chains, 1))
    if curves:
        per_chain = [smp.curves(c) for c in range(chains)]
        res.update(curves_mod.as_result(*(np.stack([pc[k] for pc in per_chain]) for k in ("counts", "n_infections", "titer_sums")),
                                        curves_mod.n_followed(np.full(N, G - 1) if last_gap is None else last_gap, G)))
    if risk is not None:
        res.update(risk_mod.as_result(np.stack([smp.risk(c) for c in range(chains)]), risk))
    if diagnostics:
        per_chain = [smp.diagnostics(c) for c in range(chains)]
        for key, name in (("i_counts", "diag_i_counts"), ("ab_n_mu", "diag_ab_n_mu"), ("ab_s_mu", "diag_ab_s_mu"), ("info", "diag_info")):
            res[name] = np.stack([pc[key] for pc in per_chain])
    if timelines:
        per_chain = [smp.timelines(c, hist=timelines_hist) for c in range(chains)]
        for key in ("inf", "cum", "ninf") + (("hist_n", "hist_s") if timelines_hist else ()):
            res["tl_" + key] = np.stack([pc[key] for pc in per_chain])
        res["tl_info"] = np.array([[pc["n_draws"]] for pc in per_chain], dtype=np.int64)
        res["tl_range"] = np.tile(np.array(timeline_ranges, dtype=np.float64), (chains, 1, 1))
        if pooled:
            res["tl_q"] = np.tile(timeline_q, (chains, 1))
            res["tl_q_n"], res["tl_q_s"] = smp.timeline_quantiles(timeline_q)
    if record_discrete or det is not None or per_reading:
        res["draw_index"] = np.tile(np.arange(0, draws, thin, dtype=np.int64), (chains, 1))  # which draws the (gap, ind) arrays hold
    if draws:
        means = [smp.means(c) for c in range(chains)]
        for j, name in enumerate(("mean_i", "mean_ab_n_mu", "mean_ab_s_mu")):
            res[name] = np.stack([m[j] for m in means])
        cat = {name: np.concatenate([s[name] for s in stats], axis=1) for name in stats[0]}
        for name in ("lp", "tree_depth", "mean_tree_accept", "step_size", "n_steps", "diverging", "energy"):
            res[f"stat_{name}"] = cat[name]
        res["stat_gibbs_accept"] = cat["gibbs_accepted"] / np.maximum(cat["gibbs_proposed"], 1)
    res["n_grad_evals"] = np.full(chains, n_grad // chains)
    smp.close()
    return res


def sample(model, tune: int, draws: int, chains: int = 1, seed: int = 0, record_deterministics: bool = True,
           progress: Optional[Callable[[int, int, int], None]] = None, device_gibbs: bool = True,
           native: bool = True, record_discrete: bool = True, chain_offset: int = 0,
           dense_metric: bool = False, thin: int = 1, budget_bytes: Optional[int] = None, log_likelihood: bool = False,
           waic: bool = False, posterior_predictive: bool = False, ppc: bool = False, curves: bool = False,
           sero_thresholds=None, diagnostics: bool = False, diag_batch: Optional[int] = None, risk=None,
           timelines: bool = False, timeline_ranges=((-4, 8), (-4, 8)), timeline_q=(0.025, 0.5, 0.975),
           timelines_hist: bool = False) -> Dict[str, np.ndarray]:
    """``pm.sample(tune, draws)`` for the abd model: returns arrays with leading (chain, draw) axes (the per-draw
    (gap, ind) arrays hold every ``thin``-th draw: ``sample_native``)."""
    if chains > model.n_chains:
        raise ValueError(f"model was built with {model.n_chains} chain slots, {chains} requested")
    if native and device_gibbs and hasattr(model.ctx, "sampler"):
        return sample_native(model, tune, draws, chains, seed, record_deterministics, record_discrete, progress,
                             chain_offset=chain_offset, dense_metric=dense_metric, thin=thin, budget_bytes=budget_bytes,
                             log_likelihood=log_likelihood, waic=waic, posterior_predictive=posterior_predictive, ppc=ppc,
                             curves=curves, sero_thresholds=sero_thresholds, diagnostics=diagnostics, diag_batch=diag_batch,
                             risk=risk, timelines=timelines, timeline_ranges=timeline_ranges, timeline_q=timeline_q,
                             timelines_hist=timelines_hist)
    if timelines:
        raise ValueError("timelines need the native sampler (sample(native=True)): the counters of every draw are accumulated inside it")
    if risk is not None:
        raise ValueError("risk needs the native sampler (sample(native=True)): every draw is reduced on the device inside it")
    if diagnostics:
        raise ValueError("diagnostics need the native sampler (sample(native=True)): the moments of every draw are accumulated inside it")
    if curves:
        raise ValueError("curves need the native sampler (sample(native=True)): every draw is reduced on the device inside it")
    if posterior_predictive or ppc:
        raise ValueError("posterior_predictive / ppc need the native sampler (sample(native=True)): the replicates and the check "
                         "statistics are drawn and accumulated inside it")
    if log_likelihood or waic:
        raise ValueError("log_likelihood / waic need the native sampler (sample(native=True)): the pointwise log-likelihood "
                         "is recorded and accumulated inside it")
    if chain_offset or dense_metric or thin != 1:
        raise ValueError("chain_offset / dense_metric / thin need the native sampler")
    per_chain = []
    for c in range(chains):
        cb = (lambda a, b, c=c: progress(c, a, b)) if progress else None
        per_chain.append(sample_chain(model, c, tune, draws, seed, record_deterministics, cb, device_gibbs))
    return {k: np.stack([pc[k] for pc in per_chain]) for k in per_chain[0]}
