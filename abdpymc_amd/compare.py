"""
Model comparison from the pointwise log-likelihood of the observed OD readings (``it_s_lik``, ``it_n_lik``; abd.py:459-469):
WAIC as ArviZ computes it, from the statistics the native sampler accumulates on the device (``sample(..., waic=True)``) or
from a recorded matrix (``sample(..., log_likelihood=True)``), and the paired comparison of variants of one cohort
(``--split_delta`` / ``--split_omicron`` / ``--ignore_pcrpos``).

Convention (``az.waic(..., scale="log")``): over the S draws of all chains pooled,

    lppd_i    = log( (1 / S) sum_s exp(ll_si) )
    p_waic_i  = Var_s(ll_si), ddof 0 (xarray's default, which ArviZ uses)
    elpd_i    = lppd_i - p_waic_i,     elpd_waic = sum_i elpd_i,     p_waic = sum_i p_waic_i
    se        = sqrt(n * Var_i(elpd_i)), ddof 0, n readings
    warning   when some p_waic_i > 0.4 (the count is returned)

Accumulated statistics per reading -- ``lse`` = log sum_s exp(ll_si) (not divided by the count), ``mean`` = the mean of ll_si,
``m2`` = sum_s (ll_si - mean)^2, with the draw count ``n`` -- merge exactly over chains and processes: log-add-exp for
``lse``, Chan et al.'s pairwise update for ``mean`` / ``m2``.
"""
from __future__ import annotations

from typing import Dict, Iterable, Mapping, Tuple

import numpy as np

from .summaries import Summary, per_reading_result

Stats = Tuple[np.ndarray, np.ndarray, np.ndarray, int]  # (lse, mean, m2, n)

WARN_P_WAIC = 0.4
WAIC_KEYS = ("elpd_waic_i_it_s_lik", "elpd_waic_i_it_n_lik", "p_waic_i_it_s_lik", "p_waic_i_it_n_lik")  # what the CLI adds per reading


def stats_from_matrix(ll) -> Stats:
    """(draws, K) pointwise log-likelihood -> the accumulated statistics of those draws."""
    ll = np.asarray(ll, dtype=np.float64)
    if ll.ndim != 2:
        raise ValueError(f"ll must be (draws, readings), got shape {ll.shape}")
    n = ll.shape[0]
    if n == 0:
        K = ll.shape[1]
        return np.full(K, -np.inf), np.zeros(K), np.zeros(K), 0
    m = ll.max(axis=0)
    lse = m + np.log(np.exp(ll - m).sum(axis=0))
    mean = ll.mean(axis=0)
    m2 = ((ll - mean) ** 2).sum(axis=0)
    return lse, mean, m2, n


def merge(*stats: Stats) -> Stats:
    """Combine the statistics of disjoint sets of draws (chains, ranks) into those of their union."""
    if not stats:
        raise ValueError("nothing to merge")
    lse, mean, m2, n = (np.asarray(stats[0][0], float), np.asarray(stats[0][1], float), np.asarray(stats[0][2], float),
                        int(stats[0][3]))
    for s in stats[1:]:
        lse_b, mean_b, m2_b, n_b = np.asarray(s[0], float), np.asarray(s[1], float), np.asarray(s[2], float), int(s[3])
        if n_b == 0:
            continue
        if n == 0:
            lse, mean, m2, n = lse_b, mean_b, m2_b, n_b
            continue
        tot = n + n_b
        d = mean_b - mean
        lse = np.logaddexp(lse, lse_b)
        mean = mean + d * (n_b / tot)
        m2 = m2 + m2_b + d * d * (n * n_b / tot)
        n = tot
    return lse, mean, m2, n


def chain_stats(res: Mapping[str, np.ndarray]) -> Iterable[Stats]:
    """The per-chain statistics of a ``sample(..., waic=True)`` result (leading chain axis, gathered over ranks or not)."""
    for c in range(np.asarray(res["waic_n_draws"]).shape[0]):
        yield res["waic_lse"][c], res["waic_mean"][c], res["waic_m2"][c], int(res["waic_n_draws"][c])


def waic_from_stats(stats: Stats, n_obs=None) -> Dict[str, object]:
    """WAIC (module docstring) from merged statistics.  ``n_obs`` = (K_s, K_n) adds the per-antigen split of ``elpd_i``."""
    lse, mean, m2, n = stats
    if n < 1:
        raise ValueError("no draws")
    lppd_i = np.asarray(lse, float) - np.log(n)
    p_waic_i = np.asarray(m2, float) / n
    elpd_i = lppd_i - p_waic_i
    K = elpd_i.size
    out = dict(elpd_waic=float(elpd_i.sum()), p_waic=float(p_waic_i.sum()),
               se=float(np.sqrt(K * np.var(elpd_i))) if K else 0.0, elpd_i=elpd_i, p_waic_i=p_waic_i,
               n_warn=int((p_waic_i > WARN_P_WAIC).sum()), n_draws=int(n), n_readings=int(K))
    if n_obs is not None:
        k_s = int(n_obs[0])
        out["elpd_waic_i_s"], out["elpd_waic_i_n"] = elpd_i[:k_s], elpd_i[k_s:]
        out["p_waic_i_s"], out["p_waic_i_n"] = p_waic_i[:k_s], p_waic_i[k_s:]
    return out


def waic(res: Mapping[str, np.ndarray]) -> Dict[str, object]:
    """WAIC of a ``sample(..., waic=True)`` result: the chains' accumulators merged, then ``waic_from_stats``.  A result
    that holds only the recorded matrices (``log_likelihood=True``) is handed to ``waic_from_matrix``."""
    if "waic_n_draws" in res:
        n_obs = np.asarray(res["waic_n_obs"])[0] if "waic_n_obs" in res else None
        return waic_from_stats(merge(*chain_stats(res)), n_obs)
    if "log_likelihood_it_s_lik" in res:
        s, n = np.asarray(res["log_likelihood_it_s_lik"]), np.asarray(res["log_likelihood_it_n_lik"])
        return waic_from_matrix(np.concatenate([s, n], axis=-1), n_obs=(s.shape[-1], n.shape[-1]))
    raise ValueError("the result has neither waic_* accumulators nor log_likelihood_* matrices")


def waic_from_matrix(ll, n_obs=None) -> Dict[str, object]:
    """WAIC of a pointwise log-likelihood matrix (chains, draws, K) or (draws, K): the draws of all chains are pooled."""
    ll = np.asarray(ll, dtype=np.float64)
    return waic_from_stats(stats_from_matrix(ll.reshape(-1, ll.shape[-1])), n_obs)


def compare(results: Mapping[str, Mapping[str, np.ndarray]]) -> Dict[str, Dict[str, float]]:
    """Rank fitted variants of ONE cohort (same readings in the same order) by elpd_waic.  Per variant: ``elpd_waic``,
    ``p_waic``, ``se``, ``elpd_diff`` (best minus this one, >= 0) and its paired standard error
    ``dse = sqrt(K * Var_i(elpd_i^best - elpd_i^this))`` (ddof 0; ``az.compare``'s), ``rank`` (0 = best)."""
    w = {name: (r if "elpd_i" in r else waic(r)) for name, r in results.items()}
    sizes = {name: v["elpd_i"].size for name, v in w.items()}
    if len(set(sizes.values())) > 1:
        raise ValueError(f"variants differ in their readings: {sizes}")
    order = sorted(w, key=lambda k: -w[k]["elpd_waic"])
    best = w[order[0]]
    out = {}
    for rank, name in enumerate(order):
        v = w[name]
        diff = best["elpd_i"] - v["elpd_i"]
        K = diff.size
        out[name] = dict(rank=rank, elpd_waic=v["elpd_waic"], p_waic=v["p_waic"], se=v["se"],
                         elpd_diff=float(best["elpd_waic"] - v["elpd_waic"]),
                         dse=float(np.sqrt(K * np.var(diff))) if K else 0.0, n_warn=v["n_warn"])
    return out


class _Waic(Summary):
    """``waic``: accumulate the per-reading statistics of the pointwise log-likelihood over ALL draws on the device (any cohort
    size) and return them as ``waic_lse`` / ``waic_mean`` / ``waic_m2`` (chains, K_s + K_n; S readings first), ``waic_n_draws``
    (chains,) and ``waic_n_obs`` (chains, 2) = (K_s, K_n): ``waic`` reads them.  The trajectories do not change."""

    name = "waic"
    options = {"waic": False}
    prefix = "waic_"
    derived_keys = WAIC_KEYS
    dims = {k: ["it_s_lik_dim_0" if "it_s_lik" in k else "it_n_lik_dim_0"] for k in WAIC_KEYS}
    record_row = "log_likelihood"
    native_only = ("log_likelihood / waic need the native sampler (sample(native=True)): the pointwise log-likelihood "
                   "is recorded and accumulated inside it")

    def enable(self, smp, plan):
        smp.enable_pointwise()

    def collect(self, smp, plan, last_gap):
        return per_reading_result("waic_", ("lse", "mean", "m2"), [smp.pointwise_stats(c) for c in range(plan["chains"])], smp.n_obs)

    def add_arguments(self, parser):
        parser.add_argument("--waic", help="Accumulate the pointwise log-likelihood of the OD readings on the device over all draws and "
                            "report WAIC (elpd_waic, p_waic, se; per reading elpd_waic_i / p_waic_i in the output).", action="store_true")

    def report(self, res, data):
        """The per-reading values go into ``res`` (keys WAIC_KEYS)."""
        w = waic(res)
        res["elpd_waic_i_it_s_lik"], res["elpd_waic_i_it_n_lik"] = w["elpd_waic_i_s"], w["elpd_waic_i_n"]
        res["p_waic_i_it_s_lik"], res["p_waic_i_it_n_lik"] = w["p_waic_i_s"], w["p_waic_i_n"]
        return [f"WAIC: elpd_waic {w['elpd_waic']:.3f}  p_waic {w['p_waic']:.3f}  se {w['se']:.3f}  ({w['n_readings']} readings, "
                f"{w['n_draws']} draws; {w['n_warn']} readings with p_waic_i > 0.4)"]

    def group(self, key):
        return "constant_data" if key in WAIC_KEYS else None  # (the accumulators themselves are not written)


SUMMARY = _Waic()
