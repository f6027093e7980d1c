"""
Posterior predictive checks of the observed OD readings (``it_s_lik``, ``it_n_lik``; abd.py:459-469): replicates as
``pm.sample_posterior_predictive`` draws them, and per-reading check statistics as ``az.plot_ppc`` / ``az.plot_bpv`` look at
them, from what the native sampler accumulates on the device (``sample(..., ppc=True)``) or records
(``sample(..., posterior_predictive=True)``).

Per reading k and draw s, with the noise-free predictive mean m_sk = d_s / (1 + exp(-b_s (x_k - a_sk))):

    y_rep_sk = m_sk + sigma_s z_sk,  z_sk ~ N(0, 1)        (abd_hip.h: abd_posterior_predictive, the stream of the normals)
    pit_sk   = Phi((y_k - m_sk) / sigma_s) = P(y_rep_sk <= y_k | draw s)

Accumulated statistics per reading -- ``mean`` = the mean of m_sk over draws, ``m2`` = sum_s (m_sk - mean)^2, ``pit`` = the mean
of pit_sk, with the draw count ``n`` -- merge exactly over chains and processes: Chan et al.'s pairwise update for
``mean`` / ``m2``, a count-weighted mean for ``pit``.  Over the draws ``pit`` is the Rao-Blackwellised tail probability
p_k = P(y_rep_k <= y_k | y): readings with p_k near 0 or 1 are ones the model does not reproduce (saturated wells, a misfit
dilution).  The predictive sd of reading k is sqrt(Var_s(m_sk) + E_s[sigma_s^2]) (law of total variance).
"""
from __future__ import annotations

from typing import Dict, Iterable, Mapping, Tuple

import numpy as np

from .summaries import Summary, per_reading_result

Stats = Tuple[np.ndarray, np.ndarray, np.ndarray, int]  # (mean, m2, pit, n)

TAIL = 0.025  # p_k below TAIL or above 1 - TAIL counts as extreme
N_BINS = 20
PPC_KEYS = ("ppc_p_it_s_lik", "ppc_p_it_n_lik")  # what the CLI adds per reading


def stats_from_matrix(m, pit) -> Stats:
    """(draws, K) predictive means and tail probabilities -> the accumulated statistics of those draws."""
    m, pit = np.asarray(m, dtype=np.float64), np.asarray(pit, dtype=np.float64)
    if m.ndim != 2 or m.shape != pit.shape:
        raise ValueError(f"m and pit must be (draws, readings) of one shape, got {m.shape} and {pit.shape}")
    n = m.shape[0]
    if n == 0:
        K = m.shape[1]
        return np.zeros(K), np.zeros(K), np.zeros(K), 0
    mean = m.mean(axis=0)
    return mean, ((m - mean) ** 2).sum(axis=0), pit.mean(axis=0), n


def merge(*stats: Stats) -> Stats:
    """Combine the statistics of disjoint sets of draws (chains, ranks) into those of their union."""
    if not stats:
        raise ValueError("nothing to merge")
    mean, m2, pit, n = (np.asarray(stats[0][0], float), np.asarray(stats[0][1], float), np.asarray(stats[0][2], float),
                        int(stats[0][3]))
    for s in stats[1:]:
        mean_b, m2_b, pit_b, n_b = np.asarray(s[0], float), np.asarray(s[1], float), np.asarray(s[2], float), int(s[3])
        if n_b == 0:
            continue
        if n == 0:
            mean, m2, pit, n = mean_b, m2_b, pit_b, n_b
            continue
        tot = n + n_b
        d = mean_b - mean
        mean = mean + d * (n_b / tot)
        m2 = m2 + m2_b + d * d * (n * n_b / tot)
        pit = pit + (pit_b - pit) * (n_b / tot)
        n = tot
    return mean, m2, pit, n


def chain_stats(res: Mapping[str, np.ndarray]) -> Iterable[Stats]:
    """The per-chain statistics of a ``sample(..., ppc=True)`` result (leading chain axis, gathered over ranks or not)."""
    for c in range(np.asarray(res["ppc_n_draws"]).shape[0]):
        yield res["ppc_mean"][c], res["ppc_m2"][c], res["ppc_pit"][c], int(res["ppc_n_draws"][c])


def summary(res: Mapping[str, np.ndarray]) -> Dict[str, object]:
    """The check of a ``sample(..., ppc=True)`` result, per observed variable (``it_s_lik``, ``it_n_lik``): ``mean`` and ``sd``
    of the posterior predictive of every reading, its tail probability ``p``, the counts ``n_low`` (p < TAIL), ``n_high``
    (p > 1 - TAIL), ``n_extreme`` and ``share_extreme`` of the readings, and ``hist``: counts of p in N_BINS equal bins of
    [0, 1].  sigma^2 is averaged over every draw of ``it_*_sigma`` (the scalars are never thinned)."""
    mean, m2, pit, n = merge(*chain_stats(res))
    if n < 1:
        raise ValueError("no draws")
    k_s = int(np.asarray(res["ppc_n_obs"])[0][0])
    out: Dict[str, object] = {"n_draws": int(n)}
    for name, sl, sig in (("it_s_lik", slice(0, k_s), "it_s_sigma"), ("it_n_lik", slice(k_s, None), "it_n_sigma")):
        p = pit[sl]
        sig2 = float(np.mean(np.square(np.asarray(res[sig], dtype=np.float64))))
        n_low, n_high = int((p < TAIL).sum()), int((p > 1.0 - TAIL).sum())
        out[name] = dict(mean=mean[sl], sd=np.sqrt(m2[sl] / n + sig2), p=p, n_readings=int(p.size), n_low=n_low,
                         n_high=n_high, n_extreme=n_low + n_high, share_extreme=(n_low + n_high) / p.size if p.size else 0.0,
                         hist=np.histogram(p, bins=N_BINS, range=(0.0, 1.0))[0])
    return out


def sample_posterior_predictive(model, res: Mapping[str, np.ndarray], tune: int, seed: int, chain_offset: int = 0,
                                slot: int = 0) -> Dict[str, np.ndarray]:
    """``pm.sample_posterior_predictive(idata)`` for a trace that recorded ``i_raw`` / ``ab_s_waner``: a replicate of every
    reading at every recorded draw -> ``{"it_s_lik": (chains, n_rec, K_s), "it_n_lik": (chains, n_rec, K_n)}``.  The normals of
    chain c's draw d are keyed as the sampler keys them (seed, stream chain_offset + c, draw tune + d), so for the sampler's
    ``seed`` and ``tune`` this reproduces its ``posterior_predictive_*`` bit for bit.  Runs on chain slot ``slot``."""
    from .model import THETA_NAMES

    if "i_raw" not in res or "ab_s_waner" not in res:
        raise ValueError("the trace holds no discrete state (i_raw, ab_s_waner): sample with record_discrete=True")
    theta = np.stack([np.asarray(res[n]) for n in THETA_NAMES], axis=-1)  # (chains, draws, 17)
    chains = theta.shape[0]
    idx = np.asarray(res["draw_index"]) if "draw_index" in res else np.tile(np.arange(theta.shape[1]), (chains, 1))
    ctx = model.ctx
    out_s = np.empty((chains, idx.shape[1], ctx.n_obs_s))
    out_n = np.empty((chains, idx.shape[1], ctx.n_obs_n))
    for c in range(chains):
        for r, d in enumerate(idx[c]):
            ctx.set_discrete(slot, res["i_raw"][c, r], res["ab_s_waner"][c, r])
            out_s[c, r], out_n[c, r] = ctx.posterior_predictive(slot, theta[c, d], seed=seed, stream=chain_offset + c,
                                                                draw=int(tune) + int(d))
    return {"it_s_lik": out_s, "it_n_lik": out_n}


class _Ppc(Summary):
    """``ppc``: accumulate per-reading check statistics over ALL draws on the device -- ``ppc_mean`` / ``ppc_m2`` (mean and sum of
    squared deviations of the predictive mean) and ``ppc_pit`` (mean of P(y_rep <= y | draw)), each (chains, K_s + K_n), S readings
    first, ``ppc_n_draws`` (chains,) and ``ppc_n_obs`` (chains, 2): ``summary`` reads them.  It draws from no random stream the
    chains use: their trajectories do not change."""

    name = "ppc"
    options = {"ppc": False}
    prefix = "ppc_"
    dims = {"ppc_p_it_s_lik": ["it_s_lik_dim_0"], "ppc_p_it_n_lik": ["it_n_lik_dim_0"]}
    record_row = "posterior_predictive"
    native_only = ("posterior_predictive / ppc need the native sampler (sample(native=True)): the replicates and the check "
                   "statistics are drawn and accumulated inside it")

    def enable(self, smp, plan):
        smp.enable_predictive()

    def collect(self, smp, plan, last_gap):
        return per_reading_result("ppc_", ("mean", "m2", "pit"), [smp.predictive_stats(c) for c in range(plan["chains"])], smp.n_obs)

    def add_arguments(self, parser):
        parser.add_argument("--ppc", help="Accumulate a posterior predictive check of the OD readings on the device over all draws and "
                            "report per antigen the readings with an extreme tail probability p = P(y_rep <= y | y) (per reading "
                            "ppc_p_it_s_lik / ppc_p_it_n_lik in the output).", action="store_true")

    def report(self, res, data):
        """The tail probability of every reading goes into ``res`` (keys PPC_KEYS)."""
        sm = summary(res)
        res["ppc_p_it_s_lik"], res["ppc_p_it_n_lik"] = sm["it_s_lik"]["p"], sm["it_n_lik"]["p"]
        return [f"PPC {name}: {a['n_extreme']} of {a['n_readings']} readings ({100 * a['share_extreme']:.2f} %) with p < 0.025 "
                f"({a['n_low']}) or p > 0.975 ({a['n_high']}); {sm['n_draws']} draws" for name, a in ((n, sm[n]) for n in ("it_s_lik", "it_n_lik"))]

    def group(self, key):
        return "constant_data" if key in PPC_KEYS else None  # (the accumulators themselves are not written)


SUMMARY = _Ppc()
