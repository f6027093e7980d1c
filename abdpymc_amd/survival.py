"""
The survival models of a finished run (reference ``abdpymc/survival.py``): does the S or the N titer of month g - 1 lower the
infection hazard of month g?

    infected[j, t] ~ Poisson(exposure[j, t] * lam0[t] / (1 + exp(-sum_k b_k (titer_k[j, t] - a_k))))

``SurvivalAnalysis`` builds the reference's arrays from the posterior means of a run (``risk.survival_arrays``); ``model_alone`` /
``model_combined`` put them on the device, where one kernel gives the data sums of logp and its gradient (``abd_survival`` in
``include/abd_hip.h``); ``sample`` runs ``sampler.Nuts`` on that evaluator as PyMC's NUTS runs on the reference's
models; ``protection`` is what ``plotting.plot_protection`` draws.  ``model_alone_groups`` gives every group of individuals its
own midpoint ``a`` under a hierarchical prior, with one slope ``b`` (``abd_survival_create_groups``).  Per-draw
(non-plug-in) fits are not here.

    python -m abdpymc_amd.survival --posterior FILE --ititers_data DIR --start S --end E --model s|n|combined --out FILE
    python -m abdpymc_amd.survival ... --model s_groups|n_groups --groups FILE [--group_name NAME]
"""
from __future__ import annotations

import argparse
import math
import sys
from typing import Callable, Dict, Optional

import numpy as np

from . import risk
from .sampler import DualAveraging, Nuts
from .summaries import interval

# ab_sd, lam0_mu_mean, lam0_mu_sd, lam0_sd_rate, lam0_z_sd (survival.py:121-122, 140-143; make_hierarchical_lam0)
PRIORS = {1: (1.0, -3.0, 0.5, 2.0, 1.0), 2: (0.5, -3.0, 0.5, 2.0, 1.0)}

# lam0_mu_mean, lam0_mu_sd, lam0_sd_rate, lam0_z_sd, a_mu_sd, a_sd_rate, a_z_sd, b_sd (survival.py:167-169: make_hierarchical_lam0
# without hyper_mu, make_hierarchical_normal("a"), b ~ N(0, 0.5))
PRIORS_GROUPS = (0.0, 0.5, 2.0, 1.0, 0.5, 2.0, 1.0, 0.5)


def _month_add(t0: str, months: int) -> str:
    y, m = str(t0).strip()[:7].split("-")
    k = int(y) * 12 + int(m) - 1 + int(months)
    return f"{k // 12:04d}-{k % 12 + 1:02d}"


def _means(src) -> Dict[str, np.ndarray]:
    """``i``, ``ab_s_mu``, ``ab_n_mu`` (G, N) posterior means of a dict of means (the reference's MAP form), or of a result /
    posterior ``.npz`` of this package (``mean_*`` (chains, G, N), else draws (chains, draws, G, N))."""
    if isinstance(src, (str, bytes)) or hasattr(src, "__fspath__"):
        with np.load(src) as f:
            src = {k: f[k] for k in f.files if k in ("i", "ab_s_mu", "ab_n_mu", "mean_i", "mean_ab_s_mu", "mean_ab_n_mu")}
    out = {}
    for name in ("i", "ab_s_mu", "ab_n_mu"):
        if "mean_" + name in src:
            v = np.asarray(src["mean_" + name], dtype=np.float64)
            v = v.mean(axis=0) if v.ndim == 3 else v
        elif name in src:
            v = np.asarray(src[name], dtype=np.float64)
            if v.ndim == 4:
                v = v.mean(axis=(0, 1))
        else:
            raise ValueError(f"neither mean_{name} nor {name} in the posterior")
        if v.ndim != 2:
            raise ValueError(f"{name}: expected (G, N) means, (chains, G, N) means or (chains, draws, G, N) draws, got {v.shape}")
        out[name] = v
    return out


class SurvivalModel:
    """One Poisson hazard model: ``names`` of the unconstrained point's entries, ``dim``, ``logp_dlogp(q)`` on the device
    ((D,) -> (logp, grad); (n, D) -> arrays, up to 16 points per launch), ``constrain(q)`` and ``close()``."""

    def __init__(self, infected, exposure, titers, antigens, priors=None, device: int = -1):
        from ._native import Survival

        self.antigens = tuple(antigens)
        self.K = len(titers)
        self.priors = PRIORS[self.K] if priors is None else tuple(float(v) for v in priors)
        self._dev = Survival(infected, exposure, titers, self.priors, device=device)
        self.T = self._dev.n_intervals
        self.dim = self._dev.dim
        ab = [f"{v}_{ag}" for v in "ab" for ag in self.antigens] if self.K > 1 else ["a", "b"]
        self.names = tuple(ab + ["_lam0_raw_mu", "_lam0_raw_sd_log__"] + [f"__lam0_raw_z_{t}" for t in range(self.T)])

    def logp_dlogp(self, q):
        return self._dev.logp_dlogp(q)

    def loglik_sums(self, q):
        return self._dev.loglik_sums(q)

    def constrain(self, q) -> Dict[str, np.ndarray]:
        return constrain(q, self.K)

    def close(self):
        self._dev.close()


def constrain(q, K: int) -> Dict[str, np.ndarray]:
    """``a``, ``b`` (..., K; no titer axis for K = 1), ``lam0`` (..., T), ``_lam0_raw_mu``, ``_lam0_raw_sd`` of points (..., D)."""
    q = np.asarray(q, dtype=np.float64)
    a, b = q[..., :K], q[..., K:2 * K]
    mu, sd = q[..., 2 * K], np.exp(q[..., 2 * K + 1])
    r = mu[..., None] + sd[..., None] * q[..., 2 * K + 2:]
    with np.errstate(over="ignore"):
        lam0 = 1.0 / (1.0 + np.exp(-r))
    if K == 1:
        a, b = a[..., 0], b[..., 0]
    return {"a": a, "b": b, "lam0": lam0, "_lam0_raw_mu": mu, "_lam0_raw_sd": sd}


def group_indices(groups, n_inds: int):
    """(labels, indices): the sorted unique labels (the reference's coords, ``np.sort(np.unique(groups))``) and each individual's
    index into them."""
    groups = np.asarray(groups)
    if groups.shape != (n_inds,):
        raise ValueError(f"groups must hold one label per individual, shape ({n_inds},), got {groups.shape}")
    labels, idx = np.unique(groups, return_inverse=True)
    return labels, idx.reshape(-1).astype(np.int32)


def constrain_groups(q, T: int, Gr: int) -> Dict[str, np.ndarray]:
    """``a`` (..., Gr), ``a_mu``, ``a_sd``, ``b``, ``lam0`` (..., T), ``_lam0_raw_mu``, ``_lam0_raw_sd`` of points (..., T + Gr + 5)."""
    q = np.asarray(q, dtype=np.float64)
    mu, sd = q[..., 0], np.exp(q[..., 1])
    r = mu[..., None] + sd[..., None] * q[..., 2:2 + T]
    with np.errstate(over="ignore"):
        lam0 = 1.0 / (1.0 + np.exp(-r))
    a_mu, a_sd = q[..., T + 2], np.exp(q[..., T + 3])
    a = a_mu[..., None] + a_sd[..., None] * q[..., T + 4:T + 4 + Gr]
    return {"a": a, "a_mu": a_mu, "a_sd": a_sd, "b": q[..., T + 4 + Gr], "lam0": lam0, "_lam0_raw_mu": mu, "_lam0_raw_sd": sd}


def names_groups(T: int, Gr: int):
    """The unconstrained point's entries in PyMC's creation order for ``model_alone_groups`` (lam0 comes first)."""
    return tuple(["_lam0_raw_mu", "_lam0_raw_sd_log__"] + [f"__lam0_raw_z_{t}" for t in range(T)] + ["a_mu", "a_sd_log__"]
                 + [f"_a_z_{g}" for g in range(Gr)] + ["b"])


def initial_point_groups(T: int, Gr: int, priors=PRIORS_GROUPS) -> np.ndarray:
    """PyMC's initial point: the prior means, ``m = lam0_mu_mean``, ``s = a_sd_log__ = -log rate``, the rest 0."""
    q0 = np.zeros(T + Gr + 5)
    q0[0], q0[1], q0[T + 3] = priors[0], -math.log(priors[2]), -math.log(priors[5])
    return q0


class SurvivalGroupsModel:
    """The Poisson hazard model by group: ``names``, ``dim``, ``groups`` (the sorted unique labels), ``group_name``,
    ``logp_dlogp(q)`` and ``loglik_sums(q)`` on the device, ``constrain(q)``, ``initial_point()`` and ``close()``."""

    K = 1

    def __init__(self, infected, exposure, titer, antigen, groups, group_name="group", priors=None, device: int = -1):
        from ._native import SURVIVAL_MAX_GROUPS, SurvivalGroups

        self.antigens = (antigen,)
        self.group_name = str(group_name)
        self.groups, self.group_index = group_indices(groups, np.asarray(infected).shape[0])
        self.Gr = len(self.groups)
        if self.Gr > SURVIVAL_MAX_GROUPS:
            raise ValueError(f"{self.Gr} groups: at most {SURVIVAL_MAX_GROUPS}")
        self.priors = PRIORS_GROUPS if priors is None else tuple(float(v) for v in priors)
        self._dev = SurvivalGroups(infected, exposure, titer, self.group_index, self.Gr, self.priors, device=device)
        self.T = self._dev.n_intervals
        self.dim = self._dev.dim
        self.names = names_groups(self.T, self.Gr)

    def logp_dlogp(self, q):
        return self._dev.logp_dlogp(q)

    def loglik_sums(self, q):
        return self._dev.loglik_sums(q)

    def constrain(self, q) -> Dict[str, np.ndarray]:
        return constrain_groups(q, self.T, self.Gr)

    def initial_point(self) -> np.ndarray:
        return initial_point_groups(self.T, self.Gr, self.priors)

    def close(self):
        self._dev.close()


class SurvivalAnalysis:
    """The reference's ``SurvivalAnalysis(abd_inference, start, end, cohort_data)``: ``infected``, ``exposure``, ``s_titer``,
    ``n_titer`` (n_ind, n_int), ``n_int = end - start - 1``, ``intervals``, ``t0`` (the month of the arrays' first interval).
    ``means_or_idata``: a dict of (G, N) means ``i``, ``ab_s_mu``, ``ab_n_mu``, or a result / posterior ``.npz`` of this package."""

    def __init__(self, means_or_idata, start: int, end: int, cohort_data, device: int = -1):
        self.start, self.end, self.cohort_data, self.device = int(start), int(end), cohort_data, device
        mean = _means(means_or_idata)
        last_gap = getattr(cohort_data, "last_gap", None)
        arrays = risk.survival_arrays(mean["i"], mean["ab_s_mu"], mean["ab_n_mu"], last_gap, self.start, self.end)
        self.infected, self.exposure = arrays["infected"], arrays["exposure"]
        self.s_titer, self.n_titer = arrays["s_titer"], arrays["n_titer"]
        self.intervals = np.arange(self.end - self.start - 1)
        self.n_int = len(self.intervals)
        t0 = getattr(cohort_data, "t0", None)
        self.t0 = _month_add(t0, self.start + 1) if t0 else None

    def model_alone(self, antigen: str) -> SurvivalModel:
        if antigen not in ("S", "N"):
            raise ValueError(f"antigen must be 'S' or 'N', got {antigen!r}")
        titer = self.s_titer if antigen == "S" else self.n_titer
        return SurvivalModel(self.infected, self.exposure, [titer], (antigen,), device=self.device)

    def model_alone_groups(self, antigen: str, groups, group_name: str = "group") -> SurvivalGroupsModel:
        """The reference's ``model_alone_groups``: ``groups`` holds one label per individual (any sortable values); the model's
        ``groups`` are the sorted unique labels and ``a`` has one entry per label in that order."""
        if antigen not in ("S", "N"):
            raise ValueError(f"antigen must be 'S' or 'N', got {antigen!r}")
        titer = self.s_titer if antigen == "S" else self.n_titer
        return SurvivalGroupsModel(self.infected, self.exposure, titer, antigen, groups, group_name, device=self.device)

    def model_combined(self) -> SurvivalModel:
        return SurvivalModel(self.infected, self.exposure, [self.s_titer, self.n_titer], ("S", "N"), device=self.device)


def _chain(fn: Callable, dim: int, tune: int, draws: int, rng: np.random.Generator, target_accept: float = 0.8,
           q0: Optional[np.ndarray] = None, adapt: bool = True, step_size: Optional[float] = None):
    """One chain of ``sampler.Nuts`` on ``fn(q) -> (logp, grad)`` with ``sampler.sample_chain``'s adaptation: start jitter U(-1, 1),
    ``find_reasonable_eps``, dual averaging, variances of the tuning draws in expanding windows.  ``adapt=False`` keeps the unit
    metric and ``step_size`` (tests).  Returns (draws (draws, dim), stats)."""
    q = (np.zeros(dim) if q0 is None else np.asarray(q0, dtype=np.float64)) + rng.uniform(-1, 1, size=dim)
    nuts = Nuts(fn, dim, rng, target_accept=target_accept)
    lp, g = fn(q)
    if adapt:
        nuts.eps = nuts.find_reasonable_eps(q, lp, g)
        nuts.da = DualAveraging(nuts.eps, target=target_accept)
    else:
        nuts.eps = float(step_size)
    out = np.empty((draws, dim))
    stats = {k: np.empty(draws) for k in ("lp", "tree_depth", "mean_tree_accept", "step_size", "n_steps", "diverging")}
    window_start, window_len = max(10, tune // 10), max(20, tune // 8)
    window = []
    for it in range(tune + draws):
        tuning = it < tune
        q, lp, g, st = nuts.step(q, lp, g, adapt=tuning and adapt)
        if tuning and adapt:
            if it >= window_start:
                window.append(q.copy())
            if len(window) >= window_len and it < tune - 20:
                var = np.var(np.asarray(window), axis=0)
                nuts.inv_mass = (len(window) / (len(window) + 5.0)) * var + 1e-3 * (5.0 / (len(window) + 5.0))
                window, window_len = [], int(window_len * 1.5)
                nuts.eps = nuts.find_reasonable_eps(q, lp, g)
                nuts.da = DualAveraging(nuts.eps, target=target_accept)
            if it == tune - 1:
                nuts.eps = nuts.da.final()
        elif not tuning:
            k = it - tune
            out[k] = q
            stats["lp"][k] = lp
            for name in ("tree_depth", "mean_tree_accept", "step_size", "n_steps", "diverging"):
                stats[name][k] = st[name]
    return out, stats


def sample(model, tune: int = 1000, draws: int = 1000, chains: int = 4, seed: int = 0, target_accept: float = 0.8,
           evaluator: Optional[Callable] = None) -> Dict[str, np.ndarray]:
    """NUTS on ``model`` (a ``SurvivalModel``, or anything with ``dim``, ``names``, ``K``): (chains, draws) arrays of the
    unconstrained entries under ``model.names``, of ``a``, ``b``, ``lam0``, ``_lam0_raw_mu``, ``_lam0_raw_sd``, and ``stat_*``.
    A model that offers ``initial_point()`` and ``constrain(q)`` (``SurvivalGroupsModel``) is started and read through them; its
    fit also holds ``groups`` and ``group_name`` where the model has them.
    ``evaluator``: a callable ``q -> (logp, grad)`` in place of the device (tests)."""
    fn = evaluator if evaluator is not None else model.logp_dlogp
    dim, K = model.dim, model.K
    if hasattr(model, "initial_point"):
        q0 = np.asarray(model.initial_point(), dtype=np.float64)
    else:
        q0 = np.zeros(dim)
        pri = getattr(model, "priors", PRIORS[K])
        q0[2 * K], q0[2 * K + 1] = pri[1], -math.log(pri[3])  # PyMC's initial point: the prior means of _lam0_raw_mu and _lam0_raw_sd
    per_chain = [_chain(fn, dim, tune, draws, np.random.default_rng([seed, c]), target_accept, q0) for c in range(chains)]
    q = np.stack([p[0] for p in per_chain])
    res = {name: q[:, :, k].copy() for k, name in enumerate(model.names)}
    res.update(model.constrain(q) if hasattr(model, "constrain") else constrain(q, K))
    for name in per_chain[0][1]:
        res["stat_" + name] = np.stack([p[1][name] for p in per_chain])
    res["antigens"] = np.array(getattr(model, "antigens", ("S", "N")[:K]))
    if hasattr(model, "groups"):
        res["groups"] = np.asarray(model.groups)
        res["group_name"] = np.array(getattr(model, "group_name", "group"))
    return res


def protection(res, x, antigen: Optional[str] = None, prob: float = 0.95, group=None) -> Dict[str, np.ndarray]:
    """``1 - 1 / (1 + exp(-b (x - a)))`` at titers ``x`` per draw, over all draws of all chains: ``mean``, ``median``, ``lower``,
    ``upper`` (each of ``x``'s shape).  ``antigen``: which titer of a combined fit ('S' or 'N'; the other held at its midpoint).
    ``group``: which group's ``a`` of a grouped fit (one of ``res["groups"]``)."""
    a, b = np.asarray(res["a"], dtype=np.float64), np.asarray(res["b"], dtype=np.float64)
    if "groups" in res:
        labels = np.asarray(res["groups"])
        hit = np.flatnonzero(labels == group) if group is not None else []
        if len(hit) != 1:
            raise ValueError(f"a grouped fit: group must be one of {labels.tolist()}, got {group!r}")
        a = a[..., int(hit[0])]
    elif group is not None:
        raise ValueError("group= is for a grouped fit (model_alone_groups)")
    if a.ndim == 3:
        names = [str(v) for v in np.asarray(res.get("antigens", ("S", "N")))]
        if antigen not in names:
            raise ValueError(f"a combined fit: antigen must be one of {names}, got {antigen!r}")
        k = names.index(antigen)
        a, b = a[..., k], b[..., k]
    elif antigen is not None and "antigens" in res and str(np.asarray(res["antigens"])[0]) != antigen:
        raise ValueError(f"this fit is of antigen {np.asarray(res['antigens'])[0]}, not {antigen}")
    x = np.asarray(x, dtype=np.float64)
    a, b = a.reshape((-1,) + (1,) * x.ndim), b.reshape((-1,) + (1,) * x.ndim)
    with np.errstate(over="ignore"):
        p = 1.0 - 1.0 / (1.0 + np.exp(-b * (x[None] - a)))
    out = interval(p, prob)
    out["mean"] = p.mean(axis=0)
    return out


def summary(res) -> Dict[str, Dict[str, np.ndarray]]:
    """Split R-hat and batch-means ESS (``diagnostics.rhat`` / ``ess``) with mean and sd of ``a``, ``b``, ``lam0``."""
    from . import diagnostics

    out = {}
    for name in ("a", "b", "lam0"):
        x = np.asarray(res[name], dtype=np.float64)
        mo = diagnostics.from_draws(x, diagnostics.default_batch(x.shape[1]))
        out[name] = {"mean": x.mean(axis=(0, 1)), "sd": x.std(axis=(0, 1), ddof=1), "rhat": diagnostics.rhat(mo),
                     "ess": diagnostics.ess(mo)}
    return out


RHAT_WARN = 1.05


def report_line(res, prob: float = 0.95) -> str:
    """Medians of a and b with intervals, the protection at titers 0, 2 and 4, and the largest split R-hat of a and b -- with a
    warning above ``RHAT_WARN``: the model has a second, flat mode, and medians pooled over chains that sit in
    different modes describe neither."""
    pct = int(round(100 * prob))
    names = [str(v) for v in np.asarray(res["antigens"])]
    parts = []
    if "groups" in res:
        return _report_line_groups(res, prob, pct, names[0])
    for k, ag in enumerate(names):
        for v in "ab":
            d = np.asarray(res[v])
            d = (d[..., k] if d.ndim == 3 else d).reshape(-1)
            iv = interval(d, prob)
            parts.append(f"{v}[{ag}] {iv['median']:.3f} ({pct} % interval {iv['lower']:.3f} to {iv['upper']:.3f})")
        pr = protection(res, np.array([0.0, 2.0, 4.0]), antigen=ag if len(names) > 1 else None, prob=prob)
        parts.append(f"protection[{ag}] at titer 0 / 2 / 4: " + " / ".join(
            f"{100 * m:.1f} % ({100 * lo:.1f} to {100 * hi:.1f})" for m, lo, hi in zip(pr["median"], pr["lower"], pr["upper"])))
    sm = summary(res)
    rhat = float(np.nanmax([np.nanmax(sm["a"]["rhat"]), np.nanmax(sm["b"]["rhat"])]))
    parts.append(_rhat_part(rhat))
    return "survival: " + "; ".join(parts)


def _rhat_part(rhat: float) -> str:
    return f"max R-hat of a, b {rhat:.3f}" + (f" -- ABOVE {RHAT_WARN}: THE CHAINS DISAGREE (they may sit in different modes); "
                                             "do not read the pooled figures, look at a and b per chain" if not rhat <= RHAT_WARN else "")


def _report_line_groups(res, prob: float, pct: int, ag: str) -> str:
    """A grouped fit's line: per group ``a`` with its interval and the protection at titers 0 / 2 / 4, ``b`` once, the largest
    R-hat of the ``a_g`` and ``b``."""
    gname = str(np.asarray(res.get("group_name", "group")))
    parts = []
    for k, label in enumerate(np.asarray(res["groups"]).tolist()):
        iv = interval(np.asarray(res["a"])[..., k].reshape(-1), prob)
        pr = protection(res, np.array([0.0, 2.0, 4.0]), prob=prob, group=label)
        parts.append(f"a[{ag}, {gname} {label}] {iv['median']:.3f} ({pct} % interval {iv['lower']:.3f} to {iv['upper']:.3f}), "
                     "protection at titer 0 / 2 / 4: " + " / ".join(
                         f"{100 * m:.1f} % ({100 * lo:.1f} to {100 * hi:.1f})" for m, lo, hi in zip(pr["median"], pr["lower"], pr["upper"])))
    iv = interval(np.asarray(res["b"]).reshape(-1), prob)
    parts.append(f"b[{ag}] {iv['median']:.3f} ({pct} % interval {iv['lower']:.3f} to {iv['upper']:.3f})")
    sm = summary(res)
    parts.append(_rhat_part(float(np.nanmax([np.nanmax(sm["a"]["rhat"]), np.nanmax(sm["b"]["rhat"])]))))
    return "survival: " + "; ".join(parts)


def read_groups(path: str, n_inds: int) -> np.ndarray:
    """One label per individual in cohort order from ``.npy`` or a text file (one label per line; numbers where every line is one)."""
    path = str(path)
    if path.endswith(".npy"):
        labels = np.load(path, allow_pickle=False)
    else:
        with open(path) as f:
            rows = [line.strip() for line in f if line.strip()]
        try:
            labels = np.array([int(v) for v in rows])
        except ValueError:
            try:
                labels = np.array([float(v) for v in rows])
            except ValueError:
                labels = np.array(rows)
    labels = np.asarray(labels).reshape(-1)
    if labels.shape[0] != n_inds:
        raise ValueError(f"{path}: {labels.shape[0]} labels for {n_inds} individuals")
    return labels


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m abdpymc_amd.survival", description="Fit a survival model of a finished run.  Prints one line on stdout: medians and intervals of a and b, "
                                 "the protection at titers 0, 2 and 4, the largest R-hat of a and b.")
    ap.add_argument("--posterior", required=True, help="A posterior .npz of abdpymc-infer (mean_i, mean_ab_s_mu, mean_ab_n_mu, or draws).")
    ap.add_argument("--ititers_data", required=True, help="The cohort directory the run was made from.")
    ap.add_argument("--start", type=int, required=True, help="First gap of the analysis (titers from here).")
    ap.add_argument("--end", type=int, required=True, help="One past the last gap of the analysis.")
    ap.add_argument("--model", choices=("s", "n", "combined", "s_groups", "n_groups"), default="combined")
    ap.add_argument("--groups", help="With --model s_groups / n_groups: a .npy or text file, one label per individual in cohort order.")
    ap.add_argument("--group_name", default="group", help="What the labels of --groups are (the reference's coordinate name).")
    ap.add_argument("--out", required=True, help="Output file (.npz; NetCDF where ArviZ imports and the name does not end in .npz).")
    ap.add_argument("--tune", type=int, default=1000)
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--chains", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", type=int, default=-1)
    args = ap.parse_args(argv)
    from .data import TiterData

    data = TiterData.from_disk(args.ititers_data)
    try:
        sa = SurvivalAnalysis(args.posterior, args.start, args.end, data, device=args.device)
        if args.model.endswith("_groups"):
            if not args.groups:
                raise ValueError(f"--model {args.model} needs --groups FILE")
            model = sa.model_alone_groups(args.model[0].upper(), read_groups(args.groups, sa.infected.shape[0]), args.group_name)
        else:
            model = sa.model_combined() if args.model == "combined" else sa.model_alone(args.model.upper())
    except ValueError as e:
        raise SystemExit(f"survival: {e}")
    res = sample(model, tune=args.tune, draws=args.draws, chains=args.chains, seed=args.seed)
    model.close()
    print(report_line(res))  # the one line, on stdout; progress and the file's name go to stderr
    out = write(res, args.out, sa)
    print(f"wrote {out}", file=sys.stderr)
    return 0


def write(res, path: str, sa: "SurvivalAnalysis") -> str:
    """``.npz``; NetCDF through ``cli.write_posterior`` where ArviZ imports and the name does not end in ``.npz`` (no test covers
    that branch: ArviZ is optional and the suite does not require it)."""
    path = str(path)
    if not path.endswith(".npz"):
        try:
            import arviz  # noqa: F401

            from .cli import write_posterior

            data = {k: v for k, v in res.items() if k not in ("antigens", "groups", "group_name")}
            return write_posterior(data, path, dict(gap=sa.intervals, ind=np.arange(sa.infected.shape[0])))
        except ImportError:
            path += ".npz"
    np.savez_compressed(path, **res, intervals=sa.intervals, t0=np.array(sa.t0 or ""))
    return path


if __name__ == "__main__":
    raise SystemExit(main())
