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

The readings of one individual are not exchangeable draws: they all hang on that individual's infection column and waner
flag.  ``by="individual"`` (``sample(..., waic=True, waic_by="individual")``) runs the same formulas over the
joint log-likelihood of every individual's readings, T_sj = sum over j's readings of ll_sk: ``elpd_i`` / ``p_waic_i`` have one
entry per individual, ``se`` and ``compare``'s ``dse`` run over the individuals that have a reading (the others contribute an
exact 0 to the sums), and the p_waic > 0.4 count is of individuals.  WAIC is less reliable the larger the unit: expect more
individuals above 0.4 than readings.

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
IND_KEYS = ("elpd_waic_ind", "p_waic_ind")  # ... and per individual
WAIC_BY = ("reading", "individual", "both")


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


def chain_stats(res: Mapping[str, np.ndarray], by: str = "reading") -> Iterable[Stats]:
    """The per-chain statistics of a ``sample(..., waic=True)`` result (leading chain axis, gathered over ranks or not):
    per reading, or -- ``by="individual"`` -- per individual (``waic_by``)."""
    pre = {"reading": "waic_", "individual": "waic_ind_"}[by]
    for c in range(np.asarray(res["waic_n_draws"]).shape[0]):
        yield res[pre + "lse"][c], res[pre + "mean"][c], res[pre + "m2"][c], int(res["waic_n_draws"][c])


def individual_matrix(ll_s, ll_n, idx_ind_s, idx_ind_n, n_inds: int) -> np.ndarray:
    """Pointwise log-likelihood matrices (..., K_s) and (..., K_n) (``log_likelihood_it_s_lik`` / ``_it_n_lik``) with the
    individual of every reading -> (..., n_inds): every individual's joint log-likelihood, S readings added in the order
    given, then N; 0 for an individual without readings."""
    ll_s, ll_n = np.asarray(ll_s, dtype=np.float64), np.asarray(ll_n, dtype=np.float64)
    if ll_s.shape[:-1] != ll_n.shape[:-1]:
        raise ValueError(f"ll_s {ll_s.shape} and ll_n {ll_n.shape} differ in their leading axes")
    out = np.zeros(ll_s.shape[:-1] + (int(n_inds),))
    for ll, idx in ((ll_s, idx_ind_s), (ll_n, idx_ind_n)):
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        if idx.size != ll.shape[-1]:
            raise ValueError(f"{idx.size} individuals for {ll.shape[-1]} readings")
        if idx.size and (idx.min() < 0 or idx.max() >= n_inds):
            raise ValueError(f"individual outside [0, {n_inds})")
        np.add.at(out, (Ellipsis, idx), ll)
    return out


def waic_from_individual_stats(stats: Stats, n_readings) -> Dict[str, object]:
    """WAIC by individual (module docstring) from the merged statistics of T_j and ``n_readings`` (N,), every individual's
    number of readings.  The dictionary of ``waic_from_stats`` with one entry per individual in ``elpd_i`` / ``p_waic_i``
    (an exact 0 without readings), plus ``n_individuals`` (those with a reading: ``se`` runs over them) and ``n_readings_i``."""
    lse, mean, m2, n = stats
    if n < 1:
        raise ValueError("no draws")
    n_readings = np.asarray(n_readings, dtype=np.int64)
    has = n_readings > 0
    p_waic_i = np.where(has, np.asarray(m2, float) / n, 0.0)
    elpd_i = np.where(has, np.asarray(lse, float) - np.log(n) - p_waic_i, 0.0)
    m = int(has.sum())
    return dict(elpd_waic=float(elpd_i.sum()), p_waic=float(p_waic_i.sum()),
                se=float(np.sqrt(m * np.var(elpd_i[has]))) if m else 0.0, elpd_i=elpd_i, p_waic_i=p_waic_i,
                n_warn=int((p_waic_i > WARN_P_WAIC).sum()), n_draws=int(n), n_readings=int(n_readings.sum()),
                n_individuals=m, n_readings_i=n_readings)


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


def waic(res: Mapping[str, np.ndarray], by=None) -> Dict[str, object]:
    """WAIC of a ``sample(..., waic=True)`` result: the chains' accumulators merged, then ``waic_from_stats``.  A result
    that holds only the recorded matrices (``log_likelihood=True``) is handed to ``waic_from_matrix``.
    ``by``: "reading", "individual" (``waic_by``; ``waic_from_individual_stats``) or ``None``: per reading where the result
    has it, else per individual."""
    if by not in (None, "reading", "individual"):
        raise ValueError(f"by must be 'reading' or 'individual', got {by!r}")
    if by is None:
        by = "individual" if "waic_ind_lse" in res and "waic_lse" not in res else "reading"
    if by == "individual":
        if "waic_ind_lse" not in res:
            raise ValueError("the result has no waic_ind_* accumulators (sample(..., waic=True, waic_by='individual')); a recorded "
                             "matrix is regrouped with individual_matrix and handed to waic_from_matrix(..., groups=...)")
        return waic_from_individual_stats(merge(*chain_stats(res, by="individual")), np.asarray(res["waic_ind_n_readings"])[0])
    if "waic_lse" in res:
        n_obs = np.asarray(res["waic_n_obs"])[0] if "waic_n_obs" in res else None
        return waic_from_stats(merge(*chain_stats(res)), n_obs)
    if "log_likelihood_it_s_lik" in res:
        s, n = np.asarray(res["log_likelihood_it_s_lik"]), np.asarray(res["log_likelihood_it_n_lik"])
        return waic_from_matrix(np.concatenate([s, n], axis=-1), n_obs=(s.shape[-1], n.shape[-1]))
    raise ValueError("the result has neither waic_* accumulators nor log_likelihood_* matrices")


def waic_from_matrix(ll, n_obs=None, groups=None, n_groups=None) -> Dict[str, object]:
    """WAIC of a pointwise log-likelihood matrix (chains, draws, K) or (draws, K): the draws of all chains are pooled.
    ``groups`` (K,): the individual of every column -- the columns are summed by individual first (``n_groups`` of them,
    default ``max(groups) + 1``) and the result is WAIC by individual (``waic_from_individual_stats``)."""
    ll = np.asarray(ll, dtype=np.float64)
    if groups is None:
        return waic_from_stats(stats_from_matrix(ll.reshape(-1, ll.shape[-1])), n_obs)
    groups = np.asarray(groups, dtype=np.int64).reshape(-1)
    n_groups = int(n_groups) if n_groups is not None else (int(groups.max()) + 1 if groups.size else 0)
    T = individual_matrix(ll, ll[..., :0], groups, groups[:0], n_groups)
    return waic_from_individual_stats(stats_from_matrix(T.reshape(-1, n_groups)), np.bincount(groups, minlength=n_groups))


def compare(results: Mapping[str, Mapping[str, np.ndarray]], by=None, ic: str = "waic") -> Dict[str, Dict[str, float]]:
    """Rank fitted variants of ONE cohort (same readings in the same order) by elpd_waic.  Per variant: ``elpd_waic``,
    ``p_waic``, ``se``, ``elpd_diff`` (best minus this one, >= 0) and its paired standard error
    ``dse = sqrt(K * Var_i(elpd_i^best - elpd_i^this))`` (ddof 0; ``az.compare``'s), ``rank`` (0 = best).
    ``by`` as in ``waic``.  By individual, i runs over the n individuals with a reading: ``dse = sqrt(n * Var_j(elpd_j^best -
    elpd_j^this))``.  Variants that lack the statistics asked for, or that are not all of one kind, are a ``ValueError``
    that names them.
    ``ic="loo"``: by elpd_loo of PSIS-LOO by individual (``sample(..., loo=True)`` results, or dictionaries of
    ``loo_from_individual``): ``rank``, ``elpd_loo``, ``p_loo``, ``se``, ``elpd_diff``, ``dse`` over the individuals with readings as
    above, and ``n_bad``, the individuals with a Pareto k above 0.7.  Variants without ``loo_*`` keys, or whose individuals with
    readings differ, are a ``ValueError`` that names them."""
    if ic not in ("waic", "loo"):
        raise ValueError(f"ic must be 'waic' or 'loo', got {ic!r}")
    if ic == "loo":
        if by not in (None, "individual"):
            raise ValueError(f"LOO is by individual, got by={by!r}")
        return _compare_loo(results)
    w, lacking = {}, []
    for name, r in results.items():
        if "elpd_i" in r:  # a dictionary of waic / waic_from_*
            if by is not None and (by == "individual") != ("n_individuals" in r):
                lacking.append(name)
            w[name] = r
            continue
        try:
            w[name] = waic(r, by)
        except ValueError:
            if by is None:
                raise
            lacking.append(name)
    if lacking:
        raise ValueError(f"variants without WAIC by {by}: {sorted(lacking)}")
    kinds = {name: "individual" if "n_individuals" in v else "reading" for name, v in w.items()}
    if len(set(kinds.values())) > 1:
        raise ValueError(f"variants mix WAIC by reading and by individual: {kinds}")
    individual = "individual" in kinds.values()
    sizes = {name: v["elpd_i"].size for name, v in w.items()}
    if len(set(sizes.values())) > 1:
        raise ValueError(f"variants differ in their {'individuals' if individual else 'readings'}: {sizes}")
    if individual and any(not np.array_equal(v["n_readings_i"] > 0, next(iter(w.values()))["n_readings_i"] > 0) for v in w.values()):
        raise ValueError("variants differ in which individuals have readings")
    order = sorted(w, key=lambda k: -w[k]["elpd_waic"])
    best = w[order[0]]
    out = {}
    for rank, name in enumerate(order):
        v = w[name]
        diff = best["elpd_i"] - v["elpd_i"]
        if individual:
            diff = diff[v["n_readings_i"] > 0]
        K = diff.size
        out[name] = dict(rank=rank, elpd_waic=v["elpd_waic"], p_waic=v["p_waic"], se=v["se"],
                         elpd_diff=float(best["elpd_waic"] - v["elpd_waic"]),
                         dse=float(np.sqrt(K * np.var(diff))) if K else 0.0, n_warn=v["n_warn"])
    return out


# ---- PSIS-LOO over the columns of a resident matrix: the host path of ``survival.loo`` ----

WARN_PARETO_K = 0.7


def _logsumexp(v: np.ndarray) -> float:
    m = v.max()
    return float(m + np.log(np.exp(v - m).sum()))


def psis_tail_len(S: int) -> int:
    """M, the most draws the tail of S draws holds: min(S // 5, ceil(3 sqrt(S)))."""
    return min(int(S) // 5, int(np.ceil(3.0 * np.sqrt(float(S)))))


def pareto_k_threshold(S: int) -> float:
    """min(1 - 1 / log10(S), 0.7): the k above which S draws are too few for the estimate (Vehtari et al. 2024)."""
    return min(1.0 - 1.0 / np.log10(S), WARN_PARETO_K) if S > 1 else -np.inf


def _psis_column(ll: np.ndarray):
    """One column (S,) in draw order -> (elpd_loo, pareto_k, lppd, n_tail): DESIGN.md §27, step by step."""
    S = ll.size
    a = -ll
    x = a - a.max()
    M = psis_tail_len(S)
    cut = max(np.partition(x, S - M - 1)[S - M - 1], np.log(np.finfo(np.float64).tiny))  # the (M + 1)-th largest, clipped
    tail = np.flatnonzero(x > cut)
    n = tail.size
    k = np.inf
    if n > 4:
        order = tail[np.argsort(x[tail], kind="stable")]  # ascending, ties in draw order
        ecut = np.exp(cut)
        t = np.exp(x[order]) - ecut
        m = 30 + int(np.floor(np.sqrt(n)))
        j = np.arange(1, m + 1, dtype=np.float64)
        b = (1.0 - np.sqrt(m / (j - 0.5))) / (3.0 * t[int(n / 4 + 0.5) - 1]) + 1.0 / t[-1]
        kj = np.log1p(-b[:, None] * t[None, :]).mean(axis=1)
        L = n * (np.log(-b / kj) - kj - 1.0)
        w = 1.0 / np.exp(L[None, :] - L[:, None]).sum(axis=1)
        b_hat = float((b * w).sum())
        k_raw = float(np.log1p(-b_hat * t).mean())
        sigma = -k_raw / b_hat
        k = (n * k_raw + 5.0) / (n + 10.0)
        lp = np.log1p(-(np.arange(n) + 0.5) / n)
        q = -sigma * lp if k == 0.0 else sigma * np.expm1(-k * lp) / k
        x = x.copy()
        x[order] = np.minimum(np.log(q + ecut), 0.0)
    lw = x - _logsumexp(x)
    return _logsumexp(ll + lw), k, _logsumexp(ll) - np.log(S), n


def psis_loo_from_matrix(ll, n_cells=None):
    """(draws, N) per-unit log-likelihood, the draws of all chains pooled -> (elpd_i, pareto_k_i, lppd_i, n_tail_i), each (N,):
    Pareto-smoothed importance sampling leave-one-out of every column with r_eff = 1 (which defines every step;
    the device computes the same in ``abd_psis_kernel``).  ``pareto_k_i`` is +inf where the tail has at most 4 draws.
    ``n_cells`` (N,): a unit with 0 is left out -- elpd = lppd = 0, k = NaN, n_tail = 0; default: the units whose column is
    exactly 0 throughout, which is what a survival model gives an individual without a followed cell."""
    ll = np.asarray(ll, dtype=np.float64)
    if ll.ndim != 2 or ll.shape[0] < 1:
        raise ValueError(f"ll must be (draws, units) with at least one draw, got shape {ll.shape}")
    N = ll.shape[1]
    out = np.all(ll == 0.0, axis=0) if n_cells is None else np.asarray(n_cells).reshape(-1) == 0
    elpd, k, lppd, n_tail = np.zeros(N), np.full(N, np.nan), np.zeros(N), np.zeros(N, dtype=np.int64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for j in np.flatnonzero(~out):
            elpd[j], k[j], lppd[j], n_tail[j] = _psis_column(np.ascontiguousarray(ll[:, j]))
    return elpd, k, lppd, n_tail


def loo_from_individual(elpd_i, pareto_k_i, lppd_i, n_cells, n_draws: int) -> Dict[str, object]:
    """PSIS-LOO by individual from the per-individual values: ``elpd_loo``, ``p_loo`` = sum(lppd_i - elpd_i), ``se`` =
    sqrt(n Var_j(elpd_j)) (ddof 0) over the ``n_individuals`` with a followed cell, ``n_draws``; ``n_bad`` = the individuals with
    k > 0.7 and ``n_warn`` = those above ``k_threshold`` = min(1 - 1 / log10(S), 0.7); ``worst`` = the individual with the
    largest k (None without one); the arrays ``elpd_i``, ``p_loo_i``, ``pareto_k``, ``lppd_i`` and ``n_readings_i`` (the followed
    cells).  An individual without a followed cell enters no sum and no count, as in ``waic_from_individual_stats``."""
    elpd_i, lppd_i = np.asarray(elpd_i, dtype=np.float64), np.asarray(lppd_i, dtype=np.float64)
    k_i, n_cells = np.asarray(pareto_k_i, dtype=np.float64), np.asarray(n_cells, dtype=np.int64)
    if n_draws < 1:
        raise ValueError("no draws")
    has = n_cells > 0
    elpd_i, lppd_i = np.where(has, elpd_i, 0.0), np.where(has, lppd_i, 0.0)
    p_loo_i = lppd_i - elpd_i
    m = int(has.sum())
    thr = pareto_k_threshold(int(n_draws))
    kk = np.where(has, k_i, -np.inf)
    return dict(elpd_loo=float(elpd_i.sum()), p_loo=float(p_loo_i.sum()), se=float(np.sqrt(m * np.var(elpd_i[has]))) if m else 0.0,
                elpd_i=elpd_i, p_loo_i=p_loo_i, pareto_k=np.where(has, k_i, np.nan), lppd_i=lppd_i, n_bad=int((kk > WARN_PARETO_K).sum()),
                n_warn=int((kk > thr).sum()), k_threshold=float(thr), worst=int(np.argmax(kk)) if m else None, n_draws=int(n_draws),
                n_readings=int(n_cells.sum()), n_individuals=m, n_readings_i=n_cells)


LOO_KEYS = ("loo_elpd_i", "loo_pareto_k", "loo_lppd_i", "loo_n_readings", "loo_n_draws")  # what loo_from_result reads


def loo_from_result(res: Mapping[str, np.ndarray]) -> Dict[str, object]:
    """``loo_from_individual`` of the ``loo_*`` keys of a ``sample(..., loo=True)`` result (``loo.loo``)."""
    missing = [k for k in LOO_KEYS if k not in res]
    if missing:
        raise ValueError(f"the result lacks {missing} (sample(..., loo=True))")
    return loo_from_individual(res["loo_elpd_i"], res["loo_pareto_k"], res["loo_lppd_i"], res["loo_n_readings"],
                               int(np.asarray(res["loo_n_draws"]).reshape(-1)[0]))


def _compare_loo(results) -> Dict[str, Dict[str, float]]:
    """``compare(..., ic="loo")``"""
    w, lacking = {}, []
    for name, r in results.items():
        if "elpd_loo" in r and "elpd_i" in r:  # a dictionary of loo_from_individual
            w[name] = r
            continue
        try:
            w[name] = loo_from_result(r)
        except ValueError:
            lacking.append(name)
    if lacking:
        raise ValueError(f"variants without LOO by individual (loo_* keys): {sorted(lacking)}")
    has = {name: np.asarray(v["n_readings_i"]) > 0 for name, v in w.items()}
    kinds = [h.tobytes() + bytes(str(h.size), "ascii") for h in has.values()]
    usual = max(kinds, key=kinds.count)  # the first of the most frequent
    odd = sorted(name for name, k in zip(has, kinds) if k != usual)
    if odd:
        raise ValueError(f"variants differ from the others in their individuals with readings: {odd}")
    order = sorted(w, key=lambda k: -w[k]["elpd_loo"])
    best = w[order[0]]
    out = {}
    for rank, name in enumerate(order):
        v = w[name]
        diff = (best["elpd_i"] - v["elpd_i"])[has[name]]
        n = diff.size
        out[name] = dict(rank=rank, elpd_loo=v["elpd_loo"], p_loo=v["p_loo"], se=v["se"], elpd_diff=float(best["elpd_loo"] - v["elpd_loo"]),
                         dse=float(np.sqrt(n * np.var(diff))) if n else 0.0, n_bad=v["n_bad"])
    return out


class _Waic(Summary):
    """``waic``: accumulate the per-reading statistics of the pointwise log-likelihood over ALL draws on the device (any cohort
    size) and return them as ``waic_lse`` / ``waic_mean`` / ``waic_m2`` (chains, K_s + K_n; S readings first), ``waic_n_draws``
    (chains,) and ``waic_n_obs`` (chains, 2) = (K_s, K_n): ``waic`` reads them.  The trajectories do not change.

    ``waic_by``: the unit the statistics are kept for.  "reading" (the default): the above.  "individual": the same
    statistics of every individual's joint log-likelihood T_j (the sum over its readings of both antigens, summed on the
    device in a fixed order) as ``waic_ind_lse`` / ``waic_ind_mean`` / ``waic_ind_m2`` (chains, N), with
    ``waic_ind_n_readings`` (chains, N) and ``waic_n_draws``; nothing is kept per reading.  "both": both sets."""

    name = "waic"
    options = {"waic": False, "waic_by": "reading"}
    prefix = "waic_"
    derived_keys = WAIC_KEYS + IND_KEYS
    dims = dict({k: ["it_s_lik_dim_0" if "it_s_lik" in k else "it_n_lik_dim_0"] for k in WAIC_KEYS}, **{k: ["ind"] for k in IND_KEYS})
    record_row = "log_likelihood"
    native_only = ("log_likelihood / waic need the native sampler (sample(native=True)): the pointwise log-likelihood "
                   "is recorded and accumulated inside it")

    def plan(self, opts, draws, chains, G, N):
        if opts["waic_by"] not in WAIC_BY:
            raise ValueError(f"waic_by must be one of {WAIC_BY}, got {opts['waic_by']!r}")
        return super().plan(opts, draws, chains, G, N)

    def enable(self, smp, plan):
        if plan["waic_by"] != "individual":
            smp.enable_pointwise()
        if plan["waic_by"] != "reading":
            smp.enable_individual_loglik()

    def collect(self, smp, plan, last_gap):
        res = {}
        if plan["waic_by"] != "individual":
            res = per_reading_result("waic_", ("lse", "mean", "m2"), [smp.pointwise_stats(c) for c in range(plan["chains"])], smp.n_obs)
        if plan["waic_by"] != "reading":
            per_chain = [smp.individual_loglik_stats(c) for c in range(plan["chains"])]
            for j, name in enumerate(("lse", "mean", "m2")):
                res["waic_ind_" + name] = np.stack([o[j] for o, _, _ in per_chain])
            res["waic_ind_n_readings"] = np.stack([np.asarray(r, dtype=np.int64) for _, _, r in per_chain])
            res["waic_n_draws"] = np.array([n for _, n, _ in per_chain], dtype=np.int64)
        return res

    def add_arguments(self, parser):
        parser.add_argument("--waic", help="Accumulate the pointwise log-likelihood of the OD readings on the device over all draws and "
                            "report WAIC (elpd_waic, p_waic, se; per reading elpd_waic_i / p_waic_i in the output).", action="store_true")
        parser.add_argument("--waic_by", choices=WAIC_BY, default=None,
                            help="With --waic: the unit WAIC is computed over.  reading (default): every OD reading.  individual: the "
                            "joint log-likelihood of each individual's readings, the exchangeable unit of the cohort (se over "
                            "individuals; elpd_waic_ind / p_waic_ind in the output).  both: both.")

    def cli_options(self, args, data, chains, world):
        if args.waic_by is not None and not args.waic:
            raise SystemExit("--waic_by needs --waic")
        return {"waic": args.waic, "waic_by": args.waic_by or "reading"}

    def report(self, res, data):
        """The per-reading values go into ``res`` (keys WAIC_KEYS), the per-individual ones too (IND_KEYS)."""
        lines = []
        if "waic_lse" in res:
            w = waic(res, by="reading")
            res["elpd_waic_i_it_s_lik"], res["elpd_waic_i_it_n_lik"] = w["elpd_waic_i_s"], w["elpd_waic_i_n"]
            res["p_waic_i_it_s_lik"], res["p_waic_i_it_n_lik"] = w["p_waic_i_s"], w["p_waic_i_n"]
            lines.append(f"WAIC: elpd_waic {w['elpd_waic']:.3f}  p_waic {w['p_waic']:.3f}  se {w['se']:.3f}  ({w['n_readings']} readings, "
                         f"{w['n_draws']} draws; {w['n_warn']} readings with p_waic_i > 0.4)")
        if "waic_ind_lse" in res:
            w = waic(res, by="individual")
            res["elpd_waic_ind"], res["p_waic_ind"] = w["elpd_i"], w["p_waic_i"]
            line = (f"WAIC by individual: elpd_waic {w['elpd_waic']:.3f}  p_waic {w['p_waic']:.3f}  se {w['se']:.3f}  "
                    f"({w['n_individuals']} individuals, {w['n_draws']} draws; {w['n_warn']} with p_waic_j > 0.4")
            if w["n_individuals"]:  # the individual the model predicts worst, among those with readings
                j = int(np.argmin(np.where(w["n_readings_i"] > 0, w["elpd_i"], np.inf)))
                ids = getattr(data, "coords", {}).get("ind")
                line += f"; worst: individual {j if ids is None else ids[j]} elpd {w['elpd_i'][j]:.3f}"
            lines.append(line + ")")
        return lines

    def group(self, key):
        return "constant_data" if key in WAIC_KEYS + IND_KEYS else None  # (the accumulators themselves are not written)


SUMMARY = _Waic()
