"""
The survival models of a finished run (reference ``abdpymc/survival.py``): does the S or the N titer of month g - 1 lower the
infection hazard of month g?

    infected[j, t] ~ Poisson(exposure[j, t] * lam0[t] / (1 + exp(-sum_k b_k (titer_k[j, t] - a_k))))

``SurvivalAnalysis`` builds the reference's arrays from the posterior means of a run (``risk.survival_arrays``); ``model_alone`` /
``model_combined`` put them on the device, where one kernel gives the data sums of logp and its gradient (``abd_survival`` in
``include/abd_hip.h``); ``sample`` runs ``sampler.Nuts`` on that evaluator as PyMC's NUTS runs on the reference's
models; ``protection`` is what ``plotting.plot_protection`` draws.  ``model_alone_groups`` gives every group of individuals its
own midpoint ``a`` under a hierarchical prior, with one slope ``b`` (``abd_survival_create_groups``);
``model_alone_periods`` does the same along the time axis, one midpoint per month or per era of intervals
(``abd_survival_create_periods``): the fit ``plotting.plot_protection(interval=)`` reads.

Those are plug-in fits: the data are posterior means.  Per-draw fits carry the run's uncertainty about who was infected when, and
at which titer, into a, b and the protection (multiple imputation): ``SurvivalAnalysis.draws`` makes a dataset of every
chosen recorded draw (``event_time`` of ``risk.survival_arrays``), ``model_alone_draws`` / ``model_combined_draws`` keep all of them
on the device, where every point of a launch reads its own dataset (``abd_survival_draws``), ``sample_draws`` runs one ``_chain``
per dataset with up to 16 of them sharing every launch, and ``draws_summary`` pools them and says how much of the variance lies
between the datasets.  ``model_alone_groups_draws`` / ``model_alone_periods_draws`` are the per-draw fits of the models by group
and by period (``abd_survival_draws_create_groups`` / ``_periods``): ``draws_summary`` then gives every midpoint against
the first, ``a[S|label] - a[S|first label]``, with its share of variance between the datasets and the share of draws above 0.
``waic_draws`` / ``loo_draws`` score a per-draw fit by WAIC / PSIS-LOO over the individuals per dataset, every draw on the dataset of
its chain, and pool the datasets by Rubin's rule; ``compare_draws`` ranks such fits of one ``SurvivalDraws``.  Predictive
checks of a per-draw fit are not built, and the command line fits the grouped and period models plug-in only.

There is one chain, ``_chain_gen``: a generator over ``sampler.Nuts`` and ``sampler.WindowedAdaptation`` that yields the points it
needs evaluated.  ``_chain`` (and so ``sample``) drives it against a callable; ``sample_draws`` drives many against one batched
evaluator.  A per-draw fit of another model needs an evaluator of ``(datasets, points)`` and nothing here.

Which titer predicts protection?  ``waic(model, fit)`` scores a fitted model by WAIC over the individuals -- the device gives every
individual's log-likelihood at every draw and keeps the running statistics (``abd_survival_individual_loglik``,
``abd_survival_waic_*``) -- and ``compare({"S": fit_s, "N": fit_n, ...})`` ranks the fits of one cohort and window
with paired standard errors (``compare.compare``).  ``loo(model, fit)`` is the better score: PSIS-LOO over the individuals, the
whole draws x individuals matrix kept and every column Pareto-smoothed on the device (``abd_survival_loo_*``), with a
Pareto k per individual that says whom the estimate can be trusted for; ``compare(fits, ic="loo")`` ranks by it.

    python -m abdpymc_amd.survival --posterior FILE --ititers_data DIR --start S --end E --model s|n|combined --out FILE [--waic] [--loo]
    python -m abdpymc_amd.survival --compare fit_s.npz fit_n.npz fit_combined.npz --ic loo
    python -m abdpymc_amd.survival ... --model s_groups|n_groups --groups FILE [--group_name NAME]
    python -m abdpymc_amd.survival ... --model s_periods|n_periods [--periods monthly|splits|FILE] [--split_delta] [--split_omicron]
    python -m abdpymc_amd.survival --compare fit_s.npz fit_n.npz fit_combined.npz
    python -m abdpymc_amd.survival ... --ppc [--ppc_edges_s E1,E2,...] [--ppc_edges_n E1,...] [--ppc_seed SEED]
    python -m abdpymc_amd.survival ... --model s|n|combined --per_draw M [--per_draw_chains C]

Does the best of them fit?  ``predictive(model, fit, by)`` is the posterior predictive check: per draw the device forms every cell's
expected count, draws a Poisson replicate of it and sums both over titer bins of one or two freely chosen binning variables and
over individuals (``abd_survival_predictive_*``, ``abd_survival_replicate``); the observed infections of a bin are
set against the replicated ones.  ``sample_posterior_predictive`` gives the per-cell replicates of chosen draws.
"""
from __future__ import annotations

import argparse
import math
import sys
from typing import Callable, Dict, Optional

import numpy as np

from . import compare as _compare
from . import risk
from .sampler import Nuts, WindowedAdaptation, drive
from .summaries import interval

_interval_of_draws = interval  # ``protection`` has an argument called ``interval``

# ab_sd, lam0_mu_mean, lam0_mu_sd, lam0_sd_rate, lam0_z_sd (survival.py:121-122, 140-143; make_hierarchical_lam0)
PRIORS = {1: (1.0, -3.0, 0.5, 2.0, 1.0), 2: (0.5, -3.0, 0.5, 2.0, 1.0)}

# lam0_mu_mean, lam0_mu_sd, lam0_sd_rate, lam0_z_sd, a_mu_sd, a_sd_rate, a_z_sd, b_sd (survival.py:167-169: make_hierarchical_lam0
# without hyper_mu, make_hierarchical_normal("a"), b ~ N(0, 0.5))
PRIORS_GROUPS = (0.0, 0.5, 2.0, 1.0, 0.5, 2.0, 1.0, 0.5)

# the same eight for model_alone_periods: make_hierarchical_lam0(hyper_mu=-3.0) as model_alone, the rest as the grouped model
PRIORS_PERIODS = (-3.0, 0.5, 2.0, 1.0, 0.5, 2.0, 1.0, 0.5)


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


def posterior_draws(src) -> Dict[str, np.ndarray]:
    """``i``, ``ab_s_mu``, ``ab_n_mu`` as (chains, draws, G, N) arrays: the recorded draws of a result of ``sampler.sample`` or of a
    posterior ``.npz`` of this package.  ``ValueError`` where only the means are there."""
    if isinstance(src, (str, bytes)) or hasattr(src, "__fspath__"):
        with np.load(src) as f:
            src = {k: f[k] for k in f.files if k in ("i", "ab_s_mu", "ab_n_mu")}
    out = {}
    for name in ("i", "ab_s_mu", "ab_n_mu"):
        v = np.asarray(src[name]) if name in src else None
        if v is None or v.ndim != 4:
            raise ValueError(f"no draws of {name} in the posterior (only means, or a dict of means): per-draw fits need the recorded "
                             "(chains, draws, G, N) arrays -- record them with abdpymc-infer --thin K (and without --no_deterministics)")
        out[name] = v
    if not (out["i"].shape == out["ab_s_mu"].shape == out["ab_n_mu"].shape):
        raise ValueError("i, ab_s_mu, ab_n_mu must share a shape (chains, draws, G, N)")
    return out


def event_time(infected, exposure):
    """(n_risk, event), each (N,) int32, of arrays (N, T) in event-time form -- what ``risk.survival_arrays`` makes of a draw's
    binary infections: per individual ``exposure`` is 1 on a prefix of ``n_risk`` intervals and 0 or NaN behind it, and ``infected``
    is 1 in at most one cell, which is then cell ``event = n_risk - 1``, and 0 or NaN everywhere else (``event = -1`` without an
    infection).  ``ValueError`` for arrays of any other form (a fractional ``infected``: the plug-in arrays of posterior means)."""
    y, e = np.asarray(infected, dtype=np.float64), np.asarray(exposure, dtype=np.float64)
    if y.ndim != 2 or e.shape != y.shape:
        raise ValueError("infected and exposure must share a shape (N, T)")
    N, T = y.shape
    at = e == 1.0
    n_risk = at.sum(axis=1).astype(np.int32)
    t = np.arange(T)[None, :]
    prefix = t < n_risk[:, None]
    with np.errstate(invalid="ignore"):
        rest_e = np.isnan(e) | (e == 0.0)
        zero_y = np.isnan(y) | (y == 0.0)
    if not (at == prefix).all() or not rest_e[~prefix].all():
        j = int(np.flatnonzero(((at != prefix) | (~prefix & ~rest_e)).any(axis=1))[0])
        raise ValueError(f"individual {j}: exposure is not 1 on a prefix of the intervals and 0 or NaN behind it (not a per-draw dataset)")
    one = y == 1.0
    if not (one | zero_y).all():
        j = int(np.flatnonzero((~(one | zero_y)).any(axis=1))[0])
        raise ValueError(f"individual {j}: infected must be 0, 1 or NaN in every cell (a fractional value: these are plug-in arrays "
                         "of posterior means, not a per-draw dataset)")
    event = np.where(one.any(axis=1), one.argmax(axis=1), -1).astype(np.int32)
    bad = (one.sum(axis=1) > 1) | ((event >= 0) & (event != n_risk - 1))
    if bad.any():
        j = int(np.flatnonzero(bad)[0])
        raise ValueError(f"individual {j}: the one infection must lie in the last interval at risk, n_risk - 1 = {int(n_risk[j]) - 1}")
    return n_risk, event


def event_time_arrays(n_risk, event, T: int):
    """(infected, exposure), each (N, T): the arrays ``event_time`` reads, NaN behind the intervals at risk."""
    n_risk, event = np.asarray(n_risk), np.asarray(event)
    t = np.arange(int(T))[None, :]
    at = t < n_risk[:, None]
    return np.where(at, (t == event[:, None]).astype(np.float64), np.nan), np.where(at, 1.0, np.nan)


class SurvivalDraws:
    """M per-draw datasets of one cohort and window (``SurvivalAnalysis.draws``): ``n_risk``, ``event`` (M, N) int32, ``s_titer``,
    ``n_titer`` (M, T, N) -- interval-major, the rows ``start .. end - 2`` of the draw's (G, N) arrays as they are -- and ``source``
    (M, 2), the (chain, draw) every dataset was made from.  ``events()`` gives Y (M, T), the infections per interval."""

    def __init__(self, n_risk, event, s_titer, n_titer, source):
        self.n_risk, self.event = np.ascontiguousarray(n_risk, dtype=np.int32), np.ascontiguousarray(event, dtype=np.int32)
        self.s_titer, self.n_titer = np.ascontiguousarray(s_titer, dtype=np.float64), np.ascontiguousarray(n_titer, dtype=np.float64)
        self.source = np.asarray(source, dtype=np.int64).reshape(-1, 2)
        self.n_datasets, self.n_inds = self.n_risk.shape
        self.n_int = self.s_titer.shape[1]
        if self.event.shape != self.n_risk.shape or self.s_titer.shape != (self.n_datasets, self.n_int, self.n_inds) \
                or self.n_titer.shape != self.s_titer.shape or self.source.shape[0] != self.n_datasets:
            raise ValueError("n_risk, event (M, N), s_titer, n_titer (M, T, N) and source (M, 2) do not fit together")

    def events(self) -> np.ndarray:
        Y = np.zeros((self.n_datasets, self.n_int))
        m, j = np.nonzero(self.event >= 0)
        np.add.at(Y, (m, self.event[m, j]), 1.0)
        return Y

    def arrays(self, m: int):
        """Dataset m as ``SurvivalModel`` takes it: (infected, exposure, s_titer, n_titer), each (N, T)."""
        y, e = event_time_arrays(self.n_risk[m], self.event[m], self.n_int)
        return y, e, self.s_titer[m].T.copy(), self.n_titer[m].T.copy()


class _DrawsDeviceModel:
    """What the per-draw models pass on to their handle ``_dev`` (``_native.SurvivalDraws``, ``SurvivalDrawsGroups`` or
    ``SurvivalDrawsPeriods``), every point on its own dataset, and what they take of the ensemble.  WAIC and PSIS-LOO by individual
    are kept per dataset (the methods ``draws_*``, named as the C calls are; ``waic_draws``, ``loo_draws``); they have no predictive checks: those are the plug-in models'."""

    def _ensemble(self, draws: "SurvivalDraws"):
        self.n_datasets, self.T, self.dim = draws.n_datasets, draws.n_int, self._dev.dim
        self.source = draws.source
        self.n_risk = draws.n_risk  # (M, N): the followed cells of every individual in every dataset

    def logp_dlogp(self, dataset, q):
        return self._dev.logp_dlogp(dataset, q)

    def loglik_sums(self, dataset, q):
        return self._dev.loglik_sums(dataset, q)

    def draws_individual_loglik(self, dataset, q):
        """(n,) (or one index) and (n, D) -> (n, N): every individual's log-likelihood at every point on the point's dataset -- the
        bits of the plug-in model of ``SurvivalDraws.arrays(m)``."""
        return self._dev.draws_individual_loglik(dataset, q)

    def draws_waic_reset(self):
        self._dev.draws_waic_reset()

    def draws_waic_accumulate(self, dataset, q):
        """Folds the draws ``q`` (n, D), in order, each into the statistics of its own dataset ``dataset`` (n,)."""
        self._dev.draws_waic_accumulate(dataset, q)

    def draws_waic_stats(self):
        """(lse, mean, m2 (M, N), n_draws (M,), n_cells (M, N)): per dataset, the statistics of the draws folded since ``draws_waic_reset``."""
        return self._dev.draws_waic_stats()

    def draws_loo_reserve(self, capacity: int):
        """Room on the device for ``capacity`` draws of ``draws_individual_loglik`` per dataset (at most 16384); 0 releases it."""
        self._dev.draws_loo_reserve(capacity)

    def draws_loo_reset(self):
        self._dev.draws_loo_reset()

    def draws_loo_accumulate(self, dataset, q):
        """Evaluates the draws ``q`` (n, D) and stores every row as the next draw of its dataset."""
        self._dev.draws_loo_accumulate(dataset, q)

    def draws_loo_stats(self):
        """(elpd_loo, pareto_k, lppd, n_tail (M, N), n_draws (M,)): PSIS-LOO of every individual per dataset over the draws held."""
        return self._dev.draws_loo_stats()

    def close(self):
        self._dev.close()


class SurvivalDrawsModel(_DrawsDeviceModel):
    """One Poisson hazard model over an ensemble of per-draw datasets (``abd_survival_draws`` in ``include/abd_hip.h``):
    ``names``, ``dim``, ``K``, ``n_datasets``, ``logp_dlogp(dataset, q)`` on the device -- an index and (D,) -> (logp, grad); (n,) and
    (n, D) -> arrays, every point on its own dataset, up to 16 per launch -- ``loglik_sums(dataset, q)``, ``constrain(q)`` and
    ``close()``.  ``draws_individual_loglik``, ``draws_waic_*`` and ``draws_loo_*`` work per dataset (``waic_draws``, ``loo_draws``, ``compare_draws``;
    DESIGN 30); it has no predictive checks: those are the plug-in model's."""

    def __init__(self, draws: SurvivalDraws, titers, antigens, priors=None, device: int = -1):
        from ._native import SurvivalDraws as _Dev

        self.antigens = tuple(antigens)
        self.K = len(titers)
        self.priors = PRIORS[self.K] if priors is None else tuple(float(v) for v in priors)
        self._dev = _Dev(draws.n_risk, draws.event, titers, self.priors, device=device)
        self._ensemble(draws)
        ab = [f"{v}_{ag}" for v in "ab" for ag in self.antigens] if self.K > 1 else ["a", "b"]
        self.names = tuple(ab + ["_lam0_raw_mu", "_lam0_raw_sd_log__"] + [f"__lam0_raw_z_{t}" for t in range(self.T)])

    def constrain(self, q) -> Dict[str, np.ndarray]:
        return constrain(q, self.K)


class _DeviceModel:
    """What the models pass on to their handle ``_dev`` (``_native.Survival``, ``SurvivalGroups`` or ``SurvivalPeriods``)."""

    def logp_dlogp(self, q):
        return self._dev.logp_dlogp(q)

    def loglik_sums(self, q):
        return self._dev.loglik_sums(q)

    def individual_loglik(self, q):
        """(n, D) -> (n, N): every individual's log-likelihood over its intervals at every point (0 without a followed cell)."""
        return self._dev.individual_loglik(q)

    def waic_reset(self):
        self._dev.waic_reset()

    def waic_accumulate(self, q):
        """Folds the draws ``q`` (n, D), in order, into the statistics of ``individual_loglik`` that the device keeps."""
        self._dev.waic_accumulate(q)

    def waic_stats(self):
        """((lse, mean, m2, n_draws), n_cells): ``compare``'s statistics of the draws folded since ``waic_reset``."""
        return self._dev.waic_stats()

    def loo_reserve(self, capacity: int):
        """Room on the device for ``capacity`` draws of ``individual_loglik`` (at most 16384); 0 releases it."""
        self._dev.loo_reserve(capacity)

    def loo_reset(self):
        self._dev.loo_reset()

    def loo_accumulate(self, q):
        """Evaluates the draws ``q`` (n, D) and stores their rows, in order, in the matrix on the device."""
        self._dev.loo_accumulate(q)

    def loo_append_rows(self, ll):
        """Stores host rows (n, N) in the place of evaluated ones."""
        self._dev.loo_append_rows(ll)

    def loo_rows(self, first: int, count: int):
        """(count, N): the stored draws ``first .. first + count - 1``."""
        return self._dev.loo_rows(first, count)

    def loo_stats(self):
        """(elpd_loo, pareto_k, lppd, n_tail, n_draws, n_cells): PSIS-LOO of every individual over the draws held."""
        return self._dev.loo_stats()

    def predictive_configure(self, titers, edges, seed: int = 0):
        """The binning variables of ``predictive``: one or two titer arrays (N, T), each with up to 7 strictly ascending edges."""
        self._dev.predictive_configure(titers, edges, seed)

    def predictive_reset(self):
        self._dev.predictive_reset()

    def predictive_accumulate(self, q):
        """Folds the draws ``q`` (n, D), in order: (expected, replicate), each (n, n_var, 8), per draw and bin."""
        return self._dev.predictive_accumulate(q)

    def predictive_stats(self):
        """(sum_e, sum_r, n_pos, n_draws): per individual over the draws folded since ``predictive_reset``."""
        return self._dev.predictive_stats()

    def predictive_observed(self):
        """(observed, person_time, n_cells (n_var, 8), observed_ind (N,)): the constants of the configuration."""
        return self._dev.predictive_observed()

    def replicate(self, q, draw0: int = 0):
        """(n, D) -> (n, N, T) int32: the per-cell replicates of the draws ``draw0 .. draw0 + n - 1``."""
        return self._dev.replicate(q, draw0)

    def close(self):
        self._dev.close()


class SurvivalModel(_DeviceModel):
    """One Poisson hazard model: ``names`` of the unconstrained point's entries, ``dim``, ``logp_dlogp(q)`` on the device
    ((D,) -> (logp, grad); (n, D) -> arrays, up to 16 points per launch), ``constrain(q)`` and ``close()``."""

    def __init__(self, infected, exposure, titers, antigens, priors=None, device: int = -1):
        from ._native import Survival

        self.antigens = tuple(antigens)
        self.K = len(titers)
        self.priors = PRIORS[self.K] if priors is None else tuple(float(v) for v in priors)
        self._dev = Survival(infected, exposure, titers, self.priors, device=device)
        self.n_cells = followed_cells(infected, exposure)
        self.followed = followed_mask(infected, exposure)
        self.T = self._dev.n_intervals
        self.dim = self._dev.dim
        ab = [f"{v}_{ag}" for v in "ab" for ag in self.antigens] if self.K > 1 else ["a", "b"]
        self.names = tuple(ab + ["_lam0_raw_mu", "_lam0_raw_sd_log__"] + [f"__lam0_raw_z_{t}" for t in range(self.T)])

    def constrain(self, q) -> Dict[str, np.ndarray]:
        return constrain(q, self.K)


def followed_cells(infected, exposure) -> np.ndarray:
    """(N,) int64: every individual's number of followed cells, exposure > 0 (NaN in either array: no follow-up)."""
    y, e = np.asarray(infected, dtype=np.float64), np.asarray(exposure, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return ((e > 0) & ~np.isnan(y)).sum(axis=1).astype(np.int64)


def followed_mask(infected, exposure) -> np.ndarray:
    """(N, T) bool: the followed cells, exposure > 0 (NaN in either array: no follow-up)."""
    y, e = np.asarray(infected, dtype=np.float64), np.asarray(exposure, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (e > 0) & ~np.isnan(y)


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


class SurvivalGroupsModel(_DeviceModel):
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
        self.n_cells = followed_cells(infected, exposure)
        self.followed = followed_mask(infected, exposure)
        self.T = self._dev.n_intervals
        self.dim = self._dev.dim
        self.names = names_groups(self.T, self.Gr)

    def constrain(self, q) -> Dict[str, np.ndarray]:
        return constrain_groups(q, self.T, self.Gr)

    def initial_point(self) -> np.ndarray:
        return initial_point_groups(self.T, self.Gr, self.priors)


def period_indices(periods, n_intervals: int):
    """(labels, indices): the sorted unique labels and each interval's index into them."""
    periods = np.asarray(periods)
    if periods.shape != (n_intervals,):
        raise ValueError(f"periods must hold one label per interval, shape ({n_intervals},), got {periods.shape}")
    labels, idx = np.unique(periods, return_inverse=True)
    return labels, idx.reshape(-1).astype(np.int32)


class SurvivalPeriodsModel(_DeviceModel):
    """The Poisson hazard model by period: ``names``, ``dim``, ``periods`` (the sorted unique labels), ``period_index`` (T,),
    ``period_name``, ``logp_dlogp(q)`` and ``loglik_sums(q)`` on the device, ``constrain(q)``, ``initial_point()`` and ``close()``.
    The unconstrained point has the grouped model's layout with one ``_a_z`` per period."""

    K = 1

    def __init__(self, infected, exposure, titer, antigen, periods, period_name="period", priors=None, device: int = -1):
        from ._native import SurvivalPeriods

        self.antigens = (antigen,)
        self.period_name = str(period_name)
        self.periods, self.period_index = period_indices(periods, np.asarray(infected).shape[1])
        self.P = len(self.periods)
        self.priors = PRIORS_PERIODS if priors is None else tuple(float(v) for v in priors)
        self._dev = SurvivalPeriods(infected, exposure, titer, self.period_index, self.P, self.priors, device=device)
        self.n_cells = followed_cells(infected, exposure)
        self.followed = followed_mask(infected, exposure)
        self.T = self._dev.n_intervals
        self.dim = self._dev.dim
        self.names = names_groups(self.T, self.P)

    def constrain(self, q) -> Dict[str, np.ndarray]:
        return constrain_groups(q, self.T, self.P)

    def initial_point(self) -> np.ndarray:
        return initial_point_groups(self.T, self.P, self.priors)


class SurvivalDrawsGroupsModel(_DrawsDeviceModel):
    """The Poisson hazard model by group over an ensemble of per-draw datasets (``abd_survival_draws_create_groups``):
    ``names``, ``dim``, ``K`` = 1, ``n_datasets``, ``source``, ``groups`` (the sorted unique labels), ``group_name``, ``Gr``,
    ``initial_point()``, ``constrain(q)``, ``logp_dlogp(dataset, q)`` and ``loglik_sums(dataset, q)`` on the device, ``close()``."""

    K = 1

    def __init__(self, draws: SurvivalDraws, titer, antigen, groups, group_name="group", priors=None, device: int = -1):
        from ._native import SURVIVAL_MAX_GROUPS, SurvivalDrawsGroups

        self.antigens = (antigen,)
        self.group_name = str(group_name)
        self.groups, self.group_index = group_indices(groups, draws.n_inds)
        self.Gr = len(self.groups)
        if self.Gr > SURVIVAL_MAX_GROUPS:
            raise ValueError(f"{self.Gr} groups: at most {SURVIVAL_MAX_GROUPS}")
        self.priors = PRIORS_GROUPS if priors is None else tuple(float(v) for v in priors)
        self._dev = SurvivalDrawsGroups(draws.n_risk, draws.event, titer, self.group_index, self.Gr, self.priors, device=device)
        self._ensemble(draws)
        self.names = names_groups(self.T, self.Gr)

    def constrain(self, q) -> Dict[str, np.ndarray]:
        return constrain_groups(q, self.T, self.Gr)

    def initial_point(self) -> np.ndarray:
        return initial_point_groups(self.T, self.Gr, self.priors)


class SurvivalDrawsPeriodsModel(_DrawsDeviceModel):
    """The Poisson hazard model by period over an ensemble of per-draw datasets (``abd_survival_draws_create_periods``):
    ``names``, ``dim``, ``K`` = 1, ``n_datasets``, ``source``, ``periods`` (the sorted unique labels), ``period_index`` (T,),
    ``period_name``, ``P``, ``initial_point()``, ``constrain(q)``, ``logp_dlogp(dataset, q)`` and ``loglik_sums(dataset, q)`` on the
    device, ``close()``."""

    K = 1

    def __init__(self, draws: SurvivalDraws, titer, antigen, periods, period_name="period", priors=None, device: int = -1):
        from ._native import SurvivalDrawsPeriods

        self.antigens = (antigen,)
        self.period_name = str(period_name)
        self.periods, self.period_index = period_indices(periods, draws.n_int)
        self.P = len(self.periods)
        self.priors = PRIORS_PERIODS if priors is None else tuple(float(v) for v in priors)
        self._dev = SurvivalDrawsPeriods(draws.n_risk, draws.event, titer, self.period_index, self.P, self.priors, device=device)
        self._ensemble(draws)
        self.names = names_groups(self.T, self.P)

    def constrain(self, q) -> Dict[str, np.ndarray]:
        return constrain_groups(q, self.T, self.P)

    def initial_point(self) -> np.ndarray:
        return initial_point_groups(self.T, self.P, self.priors)


class SurvivalAnalysis:
    """The reference's ``SurvivalAnalysis(abd_inference, start, end, cohort_data)``: ``infected``, ``exposure``, ``s_titer``,
    ``n_titer`` (n_ind, n_int), ``n_int = end - start - 1``, ``intervals``, ``t0`` (the month of the arrays' first interval).
    ``means_or_idata``: a dict of (G, N) means ``i``, ``ab_s_mu``, ``ab_n_mu``, or a result / posterior ``.npz`` of this package."""

    def __init__(self, means_or_idata, start: int, end: int, cohort_data, device: int = -1):
        self.start, self.end, self.cohort_data, self.device = int(start), int(end), cohort_data, device
        self._src = means_or_idata  # ``draws`` reads the recorded draws from it
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
        return self._windowed(SurvivalModel(self.infected, self.exposure, [titer], (antigen,), device=self.device))

    def model_alone_groups(self, antigen: str, groups, group_name: str = "group") -> SurvivalGroupsModel:
        """The reference's ``model_alone_groups``: ``groups`` holds one label per individual (any sortable values); the model's
        ``groups`` are the sorted unique labels and ``a`` has one entry per label in that order."""
        if antigen not in ("S", "N"):
            raise ValueError(f"antigen must be 'S' or 'N', got {antigen!r}")
        titer = self.s_titer if antigen == "S" else self.n_titer
        return self._windowed(SurvivalGroupsModel(self.infected, self.exposure, titer, antigen, groups, group_name, device=self.device))

    def model_alone_periods(self, antigen: str, periods=None, period_name: Optional[str] = None) -> SurvivalPeriodsModel:
        """One midpoint ``a`` per period of time, one slope ``b``.  ``periods=None``: monthly, every interval its own period, and
        ``a`` carries the reference's dimension ``intervals`` (what ``plotting.plot_protection(interval=)`` reads).  Otherwise
        ``periods`` holds one label per interval (any sortable values, need not be monotone; ``periods_from_splits`` gives the
        variant eras); the model's ``periods`` are the sorted unique labels and ``a`` has one entry per label in that order."""
        if antigen not in ("S", "N"):
            raise ValueError(f"antigen must be 'S' or 'N', got {antigen!r}")
        titer = self.s_titer if antigen == "S" else self.n_titer
        if periods is None:
            periods, period_name = self.intervals, "intervals" if period_name is None else period_name
        name = "period" if period_name is None else period_name
        return self._windowed(SurvivalPeriodsModel(self.infected, self.exposure, titer, antigen, periods, name, device=self.device))

    def periods_from_splits(self, splits) -> np.ndarray:
        """(n_int,) labels: interval t, which covers gap ``start + 1 + t``, gets the number of ``splits`` (gaps, as
        ``TiterData.calculate_splits`` gives them) that are <= that gap -- 0 before the first split, 1 from it on, ..."""
        splits = np.asarray(list(splits), dtype=np.int64).reshape(-1)
        gaps = self.start + 1 + self.intervals
        return (splits[None, :] <= gaps[:, None]).sum(axis=1).astype(np.int64)

    def model_combined(self) -> SurvivalModel:
        return self._windowed(SurvivalModel(self.infected, self.exposure, [self.s_titer, self.n_titer], ("S", "N"), device=self.device))

    def draws(self, n_datasets: Optional[int] = None, index=None) -> "SurvivalDraws":
        """The per-draw datasets of this cohort and window: ``risk.survival_arrays`` of one recorded draw's binary ``i`` with its own
        titers, in event-time form (``event_time``), for M draws of the flattened chain x draw axis -- all of them by default,
        ``n_datasets`` of them spaced evenly (``np.linspace(0, n - 1, M)`` rounded), or those of ``index``.  Needs a posterior with
        recorded draws (``posterior_draws``)."""
        d = posterior_draws(self._src)
        C, Dn, G, N = d["i"].shape
        if index is not None and n_datasets is not None:
            raise ValueError("give n_datasets or index, not both")
        if index is not None:
            idx = np.asarray(index, dtype=np.int64).reshape(-1)
        elif n_datasets is not None:
            if not 1 <= int(n_datasets) <= C * Dn:
                raise ValueError(f"n_datasets must be in [1, {C * Dn}] (chains x draws recorded), got {n_datasets}")
            idx = np.rint(np.linspace(0, C * Dn - 1, int(n_datasets))).astype(np.int64)
        else:
            idx = np.arange(C * Dn)
        if idx.size < 1 or idx.min() < 0 or idx.max() >= C * Dn:
            raise ValueError(f"index must hold draws in [0, {C * Dn}) of the flattened chain x draw axis")
        last_gap = getattr(self.cohort_data, "last_gap", None)
        T = self.n_int
        n_risk, event = np.empty((idx.size, N), np.int32), np.empty((idx.size, N), np.int32)
        s_titer, n_titer = np.empty((idx.size, T, N)), np.empty((idx.size, T, N))
        for m, k in enumerate(idx):
            c, dr = divmod(int(k), Dn)
            arr = risk.survival_arrays(d["i"][c, dr], d["ab_s_mu"][c, dr], d["ab_n_mu"][c, dr], last_gap, self.start, self.end)
            try:
                n_risk[m], event[m] = event_time(arr["infected"], arr["exposure"])
            except ValueError as e:
                raise ValueError(f"chain {c}, draw {dr}: {e}") from None
            s_titer[m], n_titer[m] = d["ab_s_mu"][c, dr, self.start:self.end - 1], d["ab_n_mu"][c, dr, self.start:self.end - 1]
        return SurvivalDraws(n_risk, event, s_titer, n_titer, np.stack(np.divmod(idx, Dn), axis=1))

    def model_alone_draws(self, antigen: str, draws: "SurvivalDraws") -> "SurvivalDrawsModel":
        if antigen not in ("S", "N"):
            raise ValueError(f"antigen must be 'S' or 'N', got {antigen!r}")
        return self._windowed(SurvivalDrawsModel(draws, [draws.s_titer if antigen == "S" else draws.n_titer], (antigen,), device=self.device))

    def model_combined_draws(self, draws: "SurvivalDraws") -> "SurvivalDrawsModel":
        return self._windowed(SurvivalDrawsModel(draws, [draws.s_titer, draws.n_titer], ("S", "N"), device=self.device))

    def model_alone_groups_draws(self, antigen: str, groups, draws: "SurvivalDraws", group_name: str = "group") -> "SurvivalDrawsGroupsModel":
        """``model_alone_groups`` over the per-draw datasets ``draws``: one label per individual, shared by all datasets."""
        if antigen not in ("S", "N"):
            raise ValueError(f"antigen must be 'S' or 'N', got {antigen!r}")
        titer = draws.s_titer if antigen == "S" else draws.n_titer
        return self._windowed(SurvivalDrawsGroupsModel(draws, titer, antigen, groups, group_name, device=self.device))

    def model_alone_periods_draws(self, antigen: str, draws: "SurvivalDraws", periods=None,
                                  period_name: Optional[str] = None) -> "SurvivalDrawsPeriodsModel":
        """``model_alone_periods`` over the per-draw datasets ``draws``; ``periods=None`` is monthly, as there."""
        if antigen not in ("S", "N"):
            raise ValueError(f"antigen must be 'S' or 'N', got {antigen!r}")
        titer = draws.s_titer if antigen == "S" else draws.n_titer
        if periods is None:
            periods, period_name = self.intervals, "intervals" if period_name is None else period_name
        name = "period" if period_name is None else period_name
        return self._windowed(SurvivalDrawsPeriodsModel(draws, titer, antigen, periods, name, device=self.device))

    def _windowed(self, model):
        model.start, model.end = self.start, self.end  # what ``waic`` records in a fit, and ``compare`` checks
        return model


def _chain_gen(dim: int, tune: int, draws: int, rng: np.random.Generator, target_accept: float = 0.8, q0: Optional[np.ndarray] = None,
               adapt: bool = True, step_size: Optional[float] = None):
    """One chain of ``sampler.Nuts`` with ``sampler.WindowedAdaptation`` (what ``sampler.sample_chain`` tunes with), from ``q0`` (the
    origin by default) plus a start jitter U(-1, 1), as a generator: it yields every point it needs evaluated, is sent ``(logp, grad)``
    for it, and returns (draws (draws, dim), stats).  ``adapt=False`` keeps the unit metric and ``step_size`` (tests)."""
    q = (np.zeros(dim) if q0 is None else np.asarray(q0, dtype=np.float64)) + rng.uniform(-1, 1, size=dim)
    nuts = Nuts(None, dim, rng, target_accept=target_accept)
    adaptation = WindowedAdaptation(nuts, tune, target=target_accept)
    lp, g = yield q
    if adapt:
        yield from adaptation.restart(q, lp, g)
    else:
        nuts.eps = float(step_size)
    out = np.empty((draws, dim))
    stats = {k: np.empty(draws) for k in ("lp", "tree_depth", "mean_tree_accept", "step_size", "n_steps", "diverging")}
    for it in range(tune + draws):
        tuning = it < tune
        q, lp, g, st = yield from nuts.step_gen(q, lp, g, adapt=tuning and adapt)
        if tuning and adapt:
            yield from adaptation.update(it, q, lp, g)
        elif not tuning:
            k = it - tune
            out[k] = q
            stats["lp"][k] = lp
            for name in ("tree_depth", "mean_tree_accept", "step_size", "n_steps", "diverging"):
                stats[name][k] = st[name]
    return out, stats


def _chain(fn: Callable, dim: int, tune: int, draws: int, rng: np.random.Generator, target_accept: float = 0.8,
           q0: Optional[np.ndarray] = None, adapt: bool = True, step_size: Optional[float] = None):
    """``_chain_gen`` driven against ``fn(q) -> (logp, grad)``.  Returns (draws (draws, dim), stats)."""
    return drive(_chain_gen(dim, tune, draws, rng, target_accept, q0, adapt, step_size), fn)


def _fit_arrays(model, per_chain) -> Dict[str, np.ndarray]:
    """What ``sample`` and ``sample_draws`` make of their chains' (draws, stats): the unconstrained entries under ``model.names``,
    the constrained ones, ``stat_*`` and ``antigens``, each with the chains on the leading axis."""
    q = np.stack([p[0] for p in per_chain])
    res = {name: q[:, :, k].copy() for k, name in enumerate(model.names)}
    res.update(model.constrain(q) if hasattr(model, "constrain") else constrain(q, model.K))
    for name in per_chain[0][1]:
        res["stat_" + name] = np.stack([p[1][name] for p in per_chain])
    res["antigens"] = np.array(getattr(model, "antigens", ("S", "N")[:model.K]))
    return res


def sample(model, tune: int = 1000, draws: int = 1000, chains: int = 4, seed: int = 0, target_accept: float = 0.8,
           evaluator: Optional[Callable] = None) -> Dict[str, np.ndarray]:
    """NUTS on ``model`` (a ``SurvivalModel``, or anything with ``dim``, ``names``, ``K``): (chains, draws) arrays of the
    unconstrained entries under ``model.names``, of ``a``, ``b``, ``lam0``, ``_lam0_raw_mu``, ``_lam0_raw_sd``, and ``stat_*``.
    A model that offers ``initial_point()`` and ``constrain(q)`` (``SurvivalGroupsModel``) is started and read through them; its
    fit also holds ``groups`` and ``group_name``, or ``periods``, ``period_name`` and ``period_index``, where the model has them.
    ``evaluator``: a callable ``q -> (logp, grad)`` in place of the device (tests)."""
    fn = evaluator if evaluator is not None else model.logp_dlogp
    q0 = _initial_point(model)
    res = _fit_arrays(model, [_chain(fn, model.dim, tune, draws, np.random.default_rng([seed, c]), target_accept, q0) for c in range(chains)])
    res.update(_label_keys(model))
    return res


def _label_keys(model) -> Dict[str, np.ndarray]:
    """What a fit of ``sample`` or ``sample_draws`` records of a model's labels: ``groups`` and ``group_name``, or ``periods``,
    ``period_name`` and ``period_index``, where the model has them -- what ``protection``, ``report_line`` and ``draws_summary`` know
    a fit by group or by period by."""
    res = {}
    if hasattr(model, "groups"):
        res["groups"] = np.asarray(model.groups)
        res["group_name"] = np.array(getattr(model, "group_name", "group"))
    if hasattr(model, "periods"):
        res["periods"] = np.asarray(model.periods)
        res["period_name"] = np.array(getattr(model, "period_name", "period"))
        res["period_index"] = np.asarray(model.period_index, dtype=np.int32)
    return res


def _initial_point(model) -> np.ndarray:
    """The point ``sample`` starts every chain's jitter from."""
    if hasattr(model, "initial_point"):
        return np.asarray(model.initial_point(), dtype=np.float64)
    K = model.K
    q0 = np.zeros(model.dim)
    pri = getattr(model, "priors", PRIORS[K])
    q0[2 * K], q0[2 * K + 1] = pri[1], -math.log(pri[3])  # PyMC's initial point: the prior means of _lam0_raw_mu and _lam0_raw_sd
    return q0


MAX_BATCH = 16  # ABD_MAX_BATCH: the points of one launch, and the chains ``sample_draws`` keeps in flight


def sample_draws(model, tune: int = 1000, draws: int = 1000, chains_per_dataset: int = 1, seed: int = 0, target_accept: float = 0.8,
                 evaluator: Optional[Callable] = None) -> Dict[str, np.ndarray]:
    """NUTS on every dataset of ``model`` (a ``SurvivalDrawsModel``, or anything with ``dim``, ``names``, ``K``, ``n_datasets``):
    M x ``chains_per_dataset`` chains, chain (m, c) exactly ``_chain`` on dataset m with ``np.random.default_rng([seed, m, c])`` from
    ``sample``'s initial point.  The chains are generators (``_chain_gen``) that hand out the point they need; up to ``MAX_BATCH`` of
    them are in flight, and every call of the evaluator carries one point of each -- on the device one launch for up to 16 chains
    of different datasets.  A finished chain's slot goes to the next waiting chain at once.

    Returns the keys of ``sample`` with a leading axis of M x c "chains", dataset-major (``protection``, ``summary`` and
    ``report_line`` read it as they read a fit of ``sample``, by group or by period too: the label keys of ``sample`` are recorded
    where the model has them), and ``dataset`` (M c,) the dataset of every chain, ``source`` (M, 2)
    where the model has it, ``n_evaluations`` and ``n_calls``.
    ``evaluator``: a callable ``(datasets (n,), q (n, D)) -> (logp (n,), grad (n, D))`` in place of the device (tests)."""
    fn = evaluator if evaluator is not None else model.logp_dlogp
    dim, M, c = model.dim, int(model.n_datasets), int(chains_per_dataset)
    if M < 1 or c < 1:
        raise ValueError(f"at least one dataset and one chain per dataset, got {M} and {c}")
    q0 = _initial_point(model)
    jobs = [(m, k) for m in range(M) for k in range(c)]
    per_chain = [None] * len(jobs)
    waiting = iter(range(len(jobs)))
    flight = []  # [job, generator, the point it waits for]

    def start():
        """the next waiting chain into flight, up to its first point"""
        job = next(waiting, None)
        if job is None:
            return
        m, k = jobs[job]
        gen = _chain_gen(dim, tune, draws, np.random.default_rng([seed, m, k]), target_accept, q0)
        flight.append([job, gen, next(gen)])

    for _ in range(min(MAX_BATCH, len(jobs))):
        start()
    n_eval = n_calls = 0
    while flight:
        lp, g = fn(np.array([jobs[f[0]][0] for f in flight], dtype=np.int32), np.stack([f[2] for f in flight]))
        n_eval, n_calls = n_eval + len(flight), n_calls + 1
        done = []
        for i, f in enumerate(flight):
            try:
                f[2] = f[1].send((float(lp[i]), np.array(g[i], dtype=np.float64)))
            except StopIteration as fin:
                per_chain[f[0]] = fin.value
                done.append(i)
        for i in reversed(done):
            del flight[i]
        for _ in done:
            start()
    res = _fit_arrays(model, per_chain)
    res.update(_label_keys(model))
    res["dataset"] = np.array([m for m, _ in jobs], dtype=np.int64)
    if hasattr(model, "source"):
        res["source"] = np.asarray(model.source, dtype=np.int64)
    res["n_evaluations"], res["n_calls"] = np.array(n_eval, dtype=np.int64), np.array(n_calls, dtype=np.int64)
    return res


DRAWS_TITERS = (0.0, 2.0, 4.0)  # where ``draws_summary`` (and ``report_line``) read the protection


DRAWS_CONTRAST_LABELS = (2, 8)  # with this many groups or periods ``draws_summary`` also gives every midpoint against the first


def _fit_labels(fit):
    """The labels of a fit by group or by period (``_label_keys``), as ``_report_line_groups`` prints them; None for any other fit."""
    for key in ("groups", "periods"):
        if key in fit:
            labels = np.asarray(fit[key]).tolist()
            a, b = np.shape(fit["a"]), np.shape(fit["b"])
            if len(a) != 3 or a[-1] != len(labels) or len(b) != 2:
                raise ValueError(f"a fit with {len(labels)} labels needs a (chains, draws, {len(labels)}) and b (chains, draws), got {a} and {b}")
            return labels
    return None


def _protection_of_draws(a, b, x):
    with np.errstate(over="ignore"):
        return 1.0 - 1.0 / (1.0 + np.exp(-b * (x - a)))  # ``protection``'s formula, per draw


def _draws_quantities(fit) -> Dict[str, np.ndarray]:
    """(chains, draws) arrays of a, b and the protection at ``DRAWS_TITERS``, per antigen: ``a[S]``, ``b[S]``, ``protection[S]@0`` ...
    Of a fit by group or by period, whose ``a`` is (chains, draws, labels) of one antigen: ``a[S|label]`` per label, ``b[S]``,
    ``protection[S|label]@0`` ..."""
    names = [str(v) for v in np.asarray(fit["antigens"])]
    a, b = np.asarray(fit["a"], dtype=np.float64), np.asarray(fit["b"], dtype=np.float64)
    out = {}
    labels = _fit_labels(fit)
    if labels is not None:
        ag = names[0]
        for k, label in enumerate(labels):
            out[f"a[{ag}|{label}]"] = a[..., k]
        out[f"b[{ag}]"] = b
        for k, label in enumerate(labels):
            for x in DRAWS_TITERS:
                out[f"protection[{ag}|{label}]@{x:g}"] = _protection_of_draws(a[..., k], b, x)
        return out
    for k, ag in enumerate(names):
        ak, bk = (a[..., k], b[..., k]) if a.ndim == 3 else (a, b)
        out[f"a[{ag}]"], out[f"b[{ag}]"] = ak, bk
        for x in DRAWS_TITERS:
            out[f"protection[{ag}]@{x:g}"] = _protection_of_draws(ak, bk, x)
    return out


def _draws_contrasts(fit) -> Dict[str, np.ndarray]:
    """(chains, draws) arrays ``a[S|label] - a[S|first label]`` of a fit by group or by period with 2 to 8 labels: did the midpoint
    move?  Empty for any other fit."""
    labels = _fit_labels(fit)
    if labels is None or not DRAWS_CONTRAST_LABELS[0] <= len(labels) <= DRAWS_CONTRAST_LABELS[1]:
        return {}
    ag = str(np.asarray(fit["antigens"])[0])
    a = np.asarray(fit["a"], dtype=np.float64)
    return {f"a[{ag}|{label}] - a[{ag}|{labels[0]}]": a[..., k] - a[..., 0] for k, label in enumerate(labels) if k > 0}


def draws_summary(fit, plug_in=None, prob: float = 0.95) -> Dict[str, Dict[str, object]]:
    """The pooled read-out of a fit of ``sample_draws`` (multiple imputation over the datasets): for ``a``, ``b`` and the protection
    at titers 0, 2 and 4 of every antigen -- keys ``a[S]``, ``b[S]``, ``protection[S]@0``, ... -- a dict with

        median, lower, upper   of all draws of all datasets pooled (``prob`` equal-tailed)
        sd                     of the pooled draws (ddof = 1)
        W                      the mean over the datasets of the variance within a dataset (ddof = 1, its chains pooled)
        B                      the variance of the datasets' means (ddof = 1; 0 for one dataset)
        frac_between           B / (B + W): the share of the variance that the plug-in fit cannot see (0 where B + W = 0)
        dataset_median         (M,) the median within every dataset
        n_negative, n_positive the datasets whose median is below / above 0 -- for ``b``, where the model's flat second mode
                                shows as datasets on either side
        sd_ratio               with ``plug_in=`` (a fit of ``sample`` on the posterior means): pooled sd over the plug-in fit's sd

    A fit by group or by period (it holds ``groups`` or ``periods``) has the keys ``a[S|label]`` per label, ``b[S]`` and
    ``protection[S|label]@0``, ...; with 2 to 8 labels also the contrasts ``a[S|label] - a[S|first label]``, whose dicts hold
    one entry more,

        p_positive             the share of the pooled draws above 0: did the midpoint move, with ``frac_between`` beside it saying
                               how much of the contrast's variance lies between the datasets
    """
    ds = np.asarray(fit["dataset"]).reshape(-1)
    labels = np.unique(ds)
    contrasts = _draws_contrasts(fit)
    plug = {**_draws_quantities(plug_in), **_draws_contrasts(plug_in)} if plug_in is not None else None
    out = {}
    for name, x in {**_draws_quantities(fit), **contrasts}.items():
        if x.shape[0] != ds.size:
            raise ValueError(f"{name}: {x.shape[0]} chains for {ds.size} entries of dataset")
        per = [x[ds == m].reshape(-1) for m in labels]
        W = float(np.mean([np.var(v, ddof=1) for v in per]))
        B = float(np.var([v.mean() for v in per], ddof=1)) if len(per) > 1 else 0.0
        med = np.array([np.median(v) for v in per])
        iv = interval(x.reshape(-1), prob)
        row = dict(median=float(iv["median"]), lower=float(iv["lower"]), upper=float(iv["upper"]), sd=float(np.std(x.reshape(-1), ddof=1)),
                   W=W, B=B, frac_between=B / (B + W) if B + W > 0 else 0.0, dataset_median=med,
                   n_negative=int((med < 0).sum()), n_positive=int((med > 0).sum()))
        if name in contrasts:
            row["p_positive"] = float((x > 0).mean())
        if plug is not None:
            if name not in plug:
                raise ValueError(f"the plug-in fit has no {name}: it is of other antigens")
            row["sd_ratio"] = row["sd"] / float(np.std(plug[name].reshape(-1), ddof=1))
        out[name] = row
    return out


# what a fit of ``sample_draws`` holds beyond one of ``sample``, and what ``--per_draw`` adds to it (``draws_fit_keys``)
DRAWS_FIT_KEYS = ("dataset", "source", "n_evaluations", "n_calls", "draws_quantity", "draws_W", "draws_B", "draws_frac_between", "draws_dataset_median")


def draws_fit_keys(summary_) -> Dict[str, np.ndarray]:
    """What ``--per_draw`` adds to the output file: per quantity of ``draws_summary`` (rows in the order of ``draws_quantity``) W, B,
    frac_between and the datasets' medians."""
    names = list(summary_)
    return {"draws_quantity": np.array(names), "draws_W": np.array([summary_[k]["W"] for k in names]),
            "draws_B": np.array([summary_[k]["B"] for k in names]), "draws_frac_between": np.array([summary_[k]["frac_between"] for k in names]),
            "draws_dataset_median": np.stack([summary_[k]["dataset_median"] for k in names])}


WAIC_FIT_KEYS = ("elpd_waic_ind", "p_waic_ind", "waic_n_cells", "waic_n_draws")  # what ``waic`` records in a fit


def fit_points(model, fit) -> np.ndarray:
    """(chains x draws, D): the unconstrained points of a fit under ``model.names``, chain after chain."""
    q = np.stack([np.asarray(fit[name], dtype=np.float64) for name in model.names], axis=-1)
    return np.ascontiguousarray(q.reshape(-1, q.shape[-1]))


def waic(model, fit, pointwise: Optional[Callable] = None) -> Dict[str, object]:
    """WAIC by individual of a fitted survival model over all draws of ``fit``: ``compare.waic_from_individual_stats`` of the
    statistics the device accumulates (``model.waic_reset`` / ``waic_accumulate`` / ``waic_stats``), the draws folded chain after
    chain.  ``elpd_i`` / ``p_waic_i`` have one entry per individual, an exact 0 without follow-up; ``n_readings_i`` holds the
    followed cells.  The entries ``WAIC_FIT_KEYS`` (and ``start`` / ``end`` where the model knows its window) are recorded in
    ``fit``: ``write`` stores them and ``compare`` reads them.
    ``pointwise``: a host callable (n, D) -> (n, N) in the device's place (tests); the model then needs ``names`` and ``n_cells``."""
    q = fit_points(model, fit)
    if pointwise is not None:
        stats, n_cells = _compare.stats_from_matrix(np.asarray(pointwise(q), dtype=np.float64)), np.asarray(model.n_cells)
    else:
        model.waic_reset()
        model.waic_accumulate(q)
        stats, n_cells = model.waic_stats()
    w = _compare.waic_from_individual_stats(stats, n_cells)
    fit["elpd_waic_ind"], fit["p_waic_ind"] = w["elpd_i"], w["p_waic_i"]
    fit["waic_n_cells"], fit["waic_n_draws"] = w["n_readings_i"], np.array(w["n_draws"], dtype=np.int64)
    for k in ("start", "end"):
        if hasattr(model, k):
            fit[k] = np.array(getattr(model, k), dtype=np.int64)
    return w


def waic_of_fit(fit) -> Dict[str, object]:
    """The dictionary of ``waic`` again from the entries it recorded in a fit (or that ``write`` stored)."""
    lacking = [k for k in WAIC_FIT_KEYS if k not in fit]
    if lacking:
        raise ValueError(f"no WAIC in the fit (waic(model, fit), or --waic): {lacking} missing")
    elpd_i, p_waic_i = np.asarray(fit["elpd_waic_ind"], dtype=np.float64), np.asarray(fit["p_waic_ind"], dtype=np.float64)
    n_cells = np.asarray(fit["waic_n_cells"], dtype=np.int64)
    has = n_cells > 0
    m = int(has.sum())
    return dict(elpd_waic=float(elpd_i.sum()), p_waic=float(p_waic_i.sum()), se=float(np.sqrt(m * np.var(elpd_i[has]))) if m else 0.0,
                elpd_i=elpd_i, p_waic_i=p_waic_i, n_warn=int((p_waic_i > _compare.WARN_P_WAIC).sum()),
                n_draws=int(np.asarray(fit["waic_n_draws"])), n_readings=int(n_cells.sum()), n_individuals=m, n_readings_i=n_cells)


# what ``loo`` records in a fit
LOO_FIT_KEYS = ("elpd_loo_ind", "pareto_k_ind", "lppd_ind", "loo_n_cells", "loo_n_draws")


def loo(model, fit, pointwise: Optional[Callable] = None) -> Dict[str, object]:
    """PSIS-LOO by individual of a fitted survival model over all draws of ``fit``: the device keeps the whole draws x
    individuals matrix of ``individual_loglik`` (``model.loo_reserve`` / ``loo_accumulate``, the draws chain after chain), smooths
    every individual's column there (``loo_stats``) and releases it; ``compare.loo_from_individual`` makes the dictionary --
    ``elpd_loo``, ``p_loo``, ``se``, ``pareto_k`` per individual and the counts of k above 0.7 and above min(1 - 1 / log10(S), 0.7).
    The entries ``LOO_FIT_KEYS`` (and ``start`` / ``end`` where the model knows its window) are recorded in ``fit``.  A fit of more
    than 16384 draws is refused.
    ``pointwise``: a host callable (n, D) -> (n, N) in the device's place, smoothed by ``compare.psis_loo_from_matrix``; the
    model then needs ``names`` and ``n_cells``."""
    q = fit_points(model, fit)
    if pointwise is not None:
        n_cells, n_draws = np.asarray(model.n_cells, dtype=np.int64), q.shape[0]
        elpd, k, lppd, _ = _compare.psis_loo_from_matrix(np.asarray(pointwise(q), dtype=np.float64), n_cells)
    else:
        model.loo_reserve(q.shape[0])
        try:
            model.loo_accumulate(q)
            elpd, k, lppd, _, n_draws, n_cells = model.loo_stats()
        finally:
            model.loo_reserve(0)
    w = _compare.loo_from_individual(elpd, k, lppd, n_cells, n_draws)
    fit["elpd_loo_ind"], fit["pareto_k_ind"], fit["lppd_ind"] = w["elpd_i"], w["pareto_k"], w["lppd_i"]
    fit["loo_n_cells"], fit["loo_n_draws"] = w["n_readings_i"], np.array(w["n_draws"], dtype=np.int64)
    for key in ("start", "end"):
        if hasattr(model, key):
            fit[key] = np.array(getattr(model, key), dtype=np.int64)
    return w


def loo_of_fit(fit) -> Dict[str, object]:
    """The dictionary of ``loo`` again from the entries it recorded in a fit (or that ``write`` stored)."""
    lacking = [k for k in LOO_FIT_KEYS if k not in fit]
    if lacking:
        raise ValueError(f"no PSIS-LOO in the fit (loo(model, fit), or --loo): {lacking} missing")
    return _compare.loo_from_individual(fit["elpd_loo_ind"], fit["pareto_k_ind"], fit["lppd_ind"], fit["loo_n_cells"],
                                        int(np.asarray(fit["loo_n_draws"])))


def loo_line(w) -> str:
    """One line; it ends with a warning that names the worst individual when some k is above 0.7."""
    line = (f"survival PSIS-LOO: elpd_loo {w['elpd_loo']:.3f}  p_loo {w['p_loo']:.3f}  se {w['se']:.3f}  ({w['n_individuals']} individuals, "
            f"{w['n_draws']} draws; {w['n_bad']} with pareto_k > 0.7, {w['n_warn']} above {w['k_threshold']:.2f})")
    if w["n_bad"]:
        j = w["worst"]
        line += f"; warning: the estimate is unreliable for them, worst: individual {j} pareto_k {w['pareto_k'][j]:.2f}"
    return line


def compare(fits, ic: str = "waic") -> Dict[str, Dict[str, float]]:
    """Rank fitted survival models of ONE cohort and window by elpd_waic: ``compare.compare`` (rank, elpd_waic, p_waic, se,
    elpd_diff, dse over the followed individuals) of ``{name: fit}``, every fit with the entries of ``waic``.  Fits that differ
    in ``start`` / ``end``, in the number of individuals or in which of them are followed are a ``ValueError`` that names the
    odd ones out.
    ``ic="loo"``: by elpd_loo, every fit with the entries of ``loo``; the rows hold ``elpd_loo`` / ``p_loo`` in the place of
    ``elpd_waic`` / ``p_waic``, and ``n_warn`` counts the individuals with pareto_k > 0.7."""
    if ic not in ("waic", "loo"):
        raise ValueError(f"ic must be 'waic' or 'loo', got {ic!r}")
    w, window = {}, {}
    for name, fit in fits.items():
        try:
            if ic == "loo":  # in the terms of ``compare.compare``
                v = loo_of_fit(fit)
                w[name] = dict(v, elpd_waic=v["elpd_loo"], p_waic=v["p_loo"], n_warn=v["n_bad"])
            else:
                w[name] = waic_of_fit(fit)
        except ValueError as e:
            raise ValueError(f"{name}: {e}") from None
        span = tuple(int(np.asarray(fit[k])) if k in fit else None for k in ("start", "end"))
        window[name] = (span, w[name]["elpd_i"].size, (w[name]["n_readings_i"] > 0).tobytes())
    kinds = list(window.values())
    usual = max(kinds, key=kinds.count)  # the first of the most frequent
    odd = [name for name, k in window.items() if k != usual]
    if odd:
        what = [("start / end", 0), ("the number of individuals", 1), ("which individuals are followed", 2)]
        raise ValueError("; ".join(f"{name} differs from the others in " + ", ".join(t for t, i in what if window[name][i] != usual[i])
                                   + (f" (start {window[name][0][0]}, end {window[name][0][1]} against {usual[0][0]}, {usual[0][1]})"
                                      if window[name][0] != usual[0] else "") for name in odd))
    table = _compare.compare(w, by="individual")
    if ic == "loo":
        table = {name: {{"elpd_waic": "elpd_loo", "p_waic": "p_loo"}.get(k, k): v for k, v in row.items()} for name, row in table.items()}
    return table


def waic_line(w) -> str:
    return (f"survival WAIC: elpd_waic {w['elpd_waic']:.3f}  p_waic {w['p_waic']:.3f}  se {w['se']:.3f}  ({w['n_individuals']} individuals, "
            f"{w['n_draws']} draws; {w['n_warn']} with p_waic_j > 0.4)")


def compare_lines(table) -> list:
    """One row per model of ``compare``'s table, best first."""
    width = max(len(str(name)) for name in table)
    if all("elpd_loo" in v for v in table.values()):  # compare(..., ic="loo")
        return [f"{str(name):<{width}}  rank {v['rank']}  elpd_loo {v['elpd_loo']:.3f}  p_loo {v['p_loo']:.3f}  se {v['se']:.3f}  "
                f"elpd_diff {v['elpd_diff']:.3f}  dse {v['dse']:.3f}  pareto_k > 0.7: {v['n_warn']}"
                for name, v in sorted(table.items(), key=lambda kv: kv[1]["rank"])]
    return [f"{str(name):<{width}}  rank {v['rank']}  elpd_waic {v['elpd_waic']:.3f}  p_waic {v['p_waic']:.3f}  se {v['se']:.3f}  "
            f"elpd_diff {v['elpd_diff']:.3f}  dse {v['dse']:.3f}" for name, v in sorted(table.items(), key=lambda kv: kv[1]["rank"])]


# ---- model comparison of per-draw fits: WAIC and PSIS-LOO by individual per dataset, pooled by Rubin's rule ----

# what ``waic_draws`` / ``loo_draws`` record in a fit of ``sample_draws``: per dataset (M, N), the draws per dataset (M,)
DRAWS_WAIC_FIT_KEYS = ("draws_elpd_waic_ind", "draws_p_waic_ind", "draws_waic_n_cells", "draws_waic_n_draws")
DRAWS_LOO_FIT_KEYS = ("draws_elpd_loo_ind", "draws_pareto_k_ind", "draws_lppd_ind", "draws_loo_n_cells", "draws_loo_n_draws")


def _draws_rows(model, fit):
    """(datasets (n,), q (n, D)): the points of a fit of ``sample_draws`` chain after chain, each with its chain's dataset."""
    q = fit_points(model, fit)
    chain_ds = np.asarray(fit["dataset"], dtype=np.int64).reshape(-1)
    M = int(model.n_datasets)
    if chain_ds.size < 1 or q.shape[0] % chain_ds.size:
        raise ValueError(f"{q.shape[0]} points for {chain_ds.size} entries of dataset: not a fit of sample_draws")
    if chain_ds.min() < 0 or chain_ds.max() >= M:
        raise ValueError(f"the fit names datasets outside [0, {M}) of the model")
    lacking = sorted(set(range(M)) - set(chain_ds.tolist()))
    if lacking:
        raise ValueError(f"the fit has no chain on the datasets {lacking}")
    return np.repeat(chain_ds, q.shape[0] // chain_ds.size), q


def pool_draws(per, ic: str = "waic") -> Dict[str, object]:
    """The pooled read-out of per-dataset WAIC / PSIS-LOO dictionaries ``per`` (one per dataset: ``waic`` / ``loo``'s), multiple
    imputation over the datasets by Rubin's rule:

        elpd, p          the means over the datasets of elpd_m and p_m
        W                the mean of se_m^2, the variance within a dataset (over its individuals)
        B                the variance of elpd_m over the datasets (ddof = 1; 0 for one dataset)
        se               sqrt(W + (1 + 1 / M) B)
        frac_between     (1 + 1 / M) B over W + (1 + 1 / M) B (0 where that is 0): what the plug-in comparison cannot see
        n_warn           WAIC: the (dataset, individual) pairs with p_waic_j > 0.4
        n_bad            PSIS-LOO: those with pareto_k > 0.7
        worst            (dataset, individual) with the largest p_waic_j / pareto_k (None without a followed individual)
        elpd_m, p_m, se_m  (M,) per dataset; ``datasets``: the list ``per``; ``n_datasets``; ``n_draws`` (M,); ``ic``"""
    if ic not in ("waic", "loo"):
        raise ValueError(f"ic must be 'waic' or 'loo', got {ic!r}")
    M = len(per)
    if M < 1:
        raise ValueError("no datasets")
    ke, kp, kw = ("elpd_waic", "p_waic", "p_waic_i") if ic == "waic" else ("elpd_loo", "p_loo", "pareto_k")
    elpd_m, p_m, se_m = (np.array([float(w[k]) for w in per]) for k in (ke, kp, "se"))
    W = float(np.mean(se_m ** 2))
    B = float(np.var(elpd_m, ddof=1)) if M > 1 else 0.0
    between = (1.0 + 1.0 / M) * B
    total = W + between
    score = np.stack([np.where(np.asarray(w["n_readings_i"]) > 0, np.nan_to_num(np.asarray(w[kw], dtype=np.float64), nan=-np.inf), -np.inf)
                      for w in per])
    worst = tuple(int(v) for v in np.unravel_index(int(np.argmax(score)), score.shape)) if (score > -np.inf).any() else None
    out = dict(ic=ic, elpd=float(np.mean(elpd_m)), p=float(np.mean(p_m)), W=W, B=B, se=float(np.sqrt(total)),
               frac_between=between / total if total > 0 else 0.0, n_warn=int(sum(w["n_warn"] for w in per)), worst=worst,
               elpd_m=elpd_m, p_m=p_m, se_m=se_m, datasets=list(per), n_datasets=M, n_draws=np.array([int(w["n_draws"]) for w in per], dtype=np.int64),
               n_individuals=int(per[0]["elpd_i"].size))
    if ic == "loo":
        out["n_bad"] = int(sum(w["n_bad"] for w in per))
    return out


def _record_window(model, fit):
    for k in ("start", "end"):
        if hasattr(model, k):
            fit[k] = np.array(getattr(model, k), dtype=np.int64)


def waic_draws(model, fit, pointwise: Optional[Callable] = None) -> Dict[str, object]:
    """WAIC by individual of a fit of ``sample_draws``, per dataset and pooled: every draw is scored on the dataset of
    its chain -- the device keeps one set of statistics per dataset (``model.draws_waic_reset`` / ``draws_waic_accumulate`` / ``draws_waic_stats``),
    the chains of a dataset folded chain after chain -- and dataset m gives ``compare.waic_from_individual_stats`` with
    ``n_cells = n_risk[m]``: what ``waic`` returns for the plug-in model of that dataset and those draws.  Returns ``pool_draws``
    of them.  The entries ``DRAWS_WAIC_FIT_KEYS`` (and ``start`` / ``end`` where the model knows its window) are recorded in ``fit``:
    ``write`` stores them and ``compare_draws`` reads them.  The result does not depend on the order of the chains in the fit beyond
    the order of the chains of one dataset.
    ``pointwise``: a host callable (datasets (n,), q (n, D)) -> (n, N) in the device's place (tests); the model then needs ``names``,
    ``n_datasets`` and ``n_risk`` (M, N)."""
    ds, q = _draws_rows(model, fit)
    M = int(model.n_datasets)
    if pointwise is not None:
        n_cells = np.asarray(model.n_risk, dtype=np.int64)
        stats = []
        for m in range(M):
            rows = q[ds == m]
            stats.append(_compare.stats_from_matrix(np.asarray(pointwise(np.full(rows.shape[0], m, dtype=np.int32), rows), dtype=np.float64)))
    else:
        model.draws_waic_reset()
        model.draws_waic_accumulate(ds, q)
        lse, mean, m2, n_draws, n_cells = model.draws_waic_stats()
        stats = [(lse[m], mean[m], m2[m], int(n_draws[m])) for m in range(M)]
    per = [_compare.waic_from_individual_stats(stats[m], n_cells[m]) for m in range(M)]
    fit["draws_elpd_waic_ind"], fit["draws_p_waic_ind"] = np.stack([w["elpd_i"] for w in per]), np.stack([w["p_waic_i"] for w in per])
    fit["draws_waic_n_cells"] = np.stack([w["n_readings_i"] for w in per])
    fit["draws_waic_n_draws"] = np.array([w["n_draws"] for w in per], dtype=np.int64)
    _record_window(model, fit)
    return pool_draws(per, "waic")


def loo_draws(model, fit, pointwise: Optional[Callable] = None) -> Dict[str, object]:
    """PSIS-LOO by individual of a fit of ``sample_draws``, per dataset and pooled: the device keeps one draws x
    individuals matrix per dataset (``model.draws_loo_reserve`` with the largest number of draws of a dataset, ``draws_loo_accumulate``),
    smooths every column of every dataset over that dataset's own draws (``draws_loo_stats``) and releases the room; dataset m gives
    ``compare.loo_from_individual`` with ``n_cells = n_risk[m]``: what ``loo`` returns for the plug-in model of that dataset and
    those draws.  Returns ``pool_draws`` of them and records ``DRAWS_LOO_FIT_KEYS`` in ``fit``.  More than 16384 draws of one
    dataset are refused.
    ``pointwise``: as in ``waic_draws``, smoothed by ``compare.psis_loo_from_matrix``."""
    ds, q = _draws_rows(model, fit)
    M = int(model.n_datasets)
    n_cells = np.asarray(model.n_risk, dtype=np.int64)
    counts = np.bincount(ds, minlength=M)
    if pointwise is not None:
        vals = []
        for m in range(M):
            rows = q[ds == m]
            ll = np.asarray(pointwise(np.full(rows.shape[0], m, dtype=np.int32), rows), dtype=np.float64)
            vals.append(_compare.psis_loo_from_matrix(ll, n_cells[m])[:3])
        n_draws = counts
    else:
        model.draws_loo_reserve(int(counts.max()))
        try:
            model.draws_loo_accumulate(ds, q)
            elpd, k, lppd, _, n_draws = model.draws_loo_stats()
        finally:
            model.draws_loo_reserve(0)
        vals = [(elpd[m], k[m], lppd[m]) for m in range(M)]
    per = [_compare.loo_from_individual(*vals[m], n_cells[m], int(n_draws[m])) for m in range(M)]
    fit["draws_elpd_loo_ind"], fit["draws_pareto_k_ind"] = np.stack([w["elpd_i"] for w in per]), np.stack([w["pareto_k"] for w in per])
    fit["draws_lppd_ind"], fit["draws_loo_n_cells"] = np.stack([w["lppd_i"] for w in per]), np.stack([w["n_readings_i"] for w in per])
    fit["draws_loo_n_draws"] = np.array([w["n_draws"] for w in per], dtype=np.int64)
    _record_window(model, fit)
    return pool_draws(per, "loo")


def draws_ic_of_fit(fit, ic: str = "waic") -> Dict[str, object]:
    """The dictionary of ``waic_draws`` / ``loo_draws`` again from the entries it recorded in a fit (or that ``write`` stored)."""
    if ic not in ("waic", "loo"):
        raise ValueError(f"ic must be 'waic' or 'loo', got {ic!r}")
    keys = DRAWS_WAIC_FIT_KEYS if ic == "waic" else DRAWS_LOO_FIT_KEYS
    lacking = [k for k in keys if k not in fit]
    if lacking:
        what = "waic_draws(model, fit), or --per_draw_ic waic" if ic == "waic" else "loo_draws(model, fit), or --per_draw_ic loo"
        raise ValueError(f"no per-draw {'WAIC' if ic == 'waic' else 'PSIS-LOO'} in the fit ({what}): {lacking} missing")
    n_cells, n_draws = np.asarray(fit[keys[-2]], dtype=np.int64), np.asarray(fit[keys[-1]], dtype=np.int64).reshape(-1)
    if n_cells.ndim != 2 or n_draws.size != n_cells.shape[0]:
        raise ValueError(f"{keys[-2]} must be (M, N) with one entry of {keys[-1]} per dataset, got {n_cells.shape} and {n_draws.shape}")
    per = []
    for m in range(n_cells.shape[0]):
        if ic == "waic":
            per.append(waic_of_fit({"elpd_waic_ind": fit[keys[0]][m], "p_waic_ind": fit[keys[1]][m], "waic_n_cells": n_cells[m],
                                    "waic_n_draws": n_draws[m]}))
        else:
            per.append(_compare.loo_from_individual(fit[keys[0]][m], fit[keys[1]][m], fit[keys[2]][m], n_cells[m], int(n_draws[m])))
    return pool_draws(per, ic)


def compare_draws(fits, ic: str = "waic") -> Dict[str, Dict[str, float]]:
    """Rank per-draw fits of ONE ``SurvivalDraws`` (``{name: fit}``, every fit with the entries of ``waic_draws``, or of ``loo_draws``
    for ``ic="loo"``) by their pooled elpd.  Fits without those entries (a plug-in fit among them), or that differ in ``source``, in
    the number of datasets, in ``start`` / ``end``, in the number of individuals or in which of them are followed in which dataset,
    are a ``ValueError`` that names the odd ones out.  Per model:

        rank, elpd, p, se, frac_between   ``pool_draws``' values (rank 0 = the largest pooled elpd)
        elpd_diff       the mean over the datasets of elpd_diff_m = elpd_m of the top-ranked model minus this one's
        dse             sqrt(mean dse_m^2 + (1 + 1 / M) var_m(elpd_diff_m)) (ddof = 1; 0 for one dataset), dse_m the paired standard
                        error over the individuals followed in dataset m, sqrt(n Var_j(elpd_j^top - elpd_j^this)) (ddof 0), as
                        ``compare.compare(..., by="individual")`` computes it
        dse_frac_between  the share of dse^2 that lies between the datasets
        p_ahead         the share of the datasets in which this model's elpd_m is above the top-ranked one's
        n_warn          the (dataset, individual) pairs with p_waic_j > 0.4 (``ic="loo"``: with pareto_k > 0.7)
        elpd_diff_m, dse_m   (M,) per dataset
    With ``ic="loo"`` the rows hold ``elpd_loo`` / ``p_loo`` beside ``elpd`` / ``p``, else ``elpd_waic`` / ``p_waic``."""
    if ic not in ("waic", "loo"):
        raise ValueError(f"ic must be 'waic' or 'loo', got {ic!r}")
    if not fits:
        raise ValueError("no fits")
    w, kind = {}, {}
    for name, fit in fits.items():
        try:
            w[name] = draws_ic_of_fit(fit, ic)
        except ValueError as e:
            raise ValueError(f"{name}: {e}") from None
        if "source" not in fit:
            raise ValueError(f"{name}: no source in the fit (the (chain, draw) of every dataset: a fit of sample_draws records it)")
        span = tuple(int(np.asarray(fit[k])) if k in fit else None for k in ("start", "end"))
        followed = np.stack([np.asarray(v["n_readings_i"]) > 0 for v in w[name]["datasets"]])
        kind[name] = (np.asarray(fit["source"], dtype=np.int64).tobytes(), w[name]["n_datasets"], span, followed.shape[1], followed.tobytes())
    kinds = list(kind.values())
    usual = max(kinds, key=kinds.count)  # the first of the most frequent
    odd = [name for name, k in kind.items() if k != usual]
    if odd:
        what = ("source", "the number of datasets", "start / end", "the number of individuals", "which individuals are followed")
        raise ValueError("; ".join(f"{name} differs from the others in " + ", ".join(t for t, a, b in zip(what, kind[name], usual) if a != b)
                                   for name in odd))
    order = sorted(w, key=lambda k: -w[k]["elpd"])
    top = w[order[0]]
    M = top["n_datasets"]
    out = {}
    for rank, name in enumerate(order):
        v = w[name]
        diff_m, dse_m = np.zeros(M), np.zeros(M)
        for m in range(M):
            a, b = top["datasets"][m], v["datasets"][m]
            d = (a["elpd_i"] - b["elpd_i"])[b["n_readings_i"] > 0]
            diff_m[m] = top["elpd_m"][m] - v["elpd_m"][m]
            dse_m[m] = float(np.sqrt(d.size * np.var(d))) if d.size else 0.0
        within = float(np.mean(dse_m ** 2))
        between = (1.0 + 1.0 / M) * (float(np.var(diff_m, ddof=1)) if M > 1 else 0.0)
        row = dict(rank=rank, elpd=v["elpd"], p=v["p"], se=v["se"], frac_between=v["frac_between"], elpd_diff=float(np.mean(diff_m)),
                   dse=float(np.sqrt(within + between)), dse_frac_between=between / (within + between) if within + between > 0 else 0.0,
                   p_ahead=float(np.mean(v["elpd_m"] > top["elpd_m"])), n_warn=v["n_bad"] if ic == "loo" else v["n_warn"],
                   elpd_diff_m=diff_m, dse_m=dse_m, n_datasets=M)
        row["elpd_loo" if ic == "loo" else "elpd_waic"], row["p_loo" if ic == "loo" else "p_waic"] = v["elpd"], v["p"]
        out[name] = row
    return out


def draws_ic_line(w) -> str:
    """One line of ``waic_draws`` / ``loo_draws``: the pooled elpd, p, se, the share between the datasets and the warnings."""
    if w["ic"] == "loo":
        line = (f"survival per-draw PSIS-LOO: elpd_loo {w['elpd']:.3f}  p_loo {w['p']:.3f}  se {w['se']:.3f}  frac_between {w['frac_between']:.3f}  "
                f"({w['n_datasets']} datasets, {w['n_individuals']} individuals; {w['n_bad']} with pareto_k > 0.7)")
        if w["n_bad"]:
            m, j = w["worst"]
            line += f"; warning: the estimate is unreliable for them, worst: dataset {m} individual {j} pareto_k {w['datasets'][m]['pareto_k'][j]:.2f}"
        return line
    return (f"survival per-draw WAIC: elpd_waic {w['elpd']:.3f}  p_waic {w['p']:.3f}  se {w['se']:.3f}  frac_between {w['frac_between']:.3f}  "
            f"({w['n_datasets']} datasets, {w['n_individuals']} individuals; {w['n_warn']} with p_waic_j > 0.4)")


def draws_compare_lines(table) -> list:
    """One row per model of ``compare_draws``' table, best first."""
    width = max(len(str(name)) for name in table)
    loo_ = all("elpd_loo" in v for v in table.values())
    e, p, warn = ("elpd_loo", "p_loo", "pareto_k > 0.7") if loo_ else ("elpd_waic", "p_waic", "p_waic_j > 0.4")
    return [f"{str(name):<{width}}  rank {v['rank']}  {e} {v['elpd']:.3f}  {p} {v['p']:.3f}  se {v['se']:.3f}  frac_between {v['frac_between']:.3f}  "
            f"elpd_diff {v['elpd_diff']:.3f}  dse {v['dse']:.3f}  p_ahead {v['p_ahead']:.2f}  {warn}: {v['n_warn']}  ({v['n_datasets']} datasets)"
            for name, v in sorted(table.items(), key=lambda kv: kv[1]["rank"])]


# ---- posterior predictive checks (abd_survival_predictive_*) ----

PPC_MAX_EDGES = 7  # up to 8 bins per binning variable
PPC_FLAG = 0.025   # a bin is flagged where min(p_low, p_high) is below this
# what ``predictive`` records in a fit (the variables stacked in the order of ``ppc_variables``; bins past a variable's own hold
# NaN in the float arrays and 0 in the integer ones)
PPC_FIT_KEYS = ("ppc_variables", "ppc_edges", "ppc_n_bins", "ppc_observed", "ppc_person_time", "ppc_n_cells", "ppc_expected", "ppc_replicate",
                "ppc_p_low", "ppc_p_high", "ppc_expected_ind", "ppc_p_infected_ind", "ppc_replicate_mean_ind", "ppc_observed_ind",
                "ppc_n_draws", "ppc_seed")


def default_edges(titer, followed) -> np.ndarray:
    """The seven octiles of the followed cells' titers as bin edges, made strictly ascending: each is a titer of the data (the
    lower of the two beside a quantile), repeated values are dropped and so is an edge at the smallest titer, so that with the rule
    bin = #{edges <= x} every bin holds a followed cell.  Fewer than seven edges where the titers repeat."""
    x, m = np.asarray(titer, dtype=np.float64), np.asarray(followed, dtype=bool)
    if x.shape != m.shape:
        raise ValueError(f"titer {x.shape} and followed {m.shape} must share a shape")
    v = x[m]
    if v.size == 0:
        raise ValueError("no followed cell: no default edges")
    if not np.isfinite(v).all():
        raise ValueError("titer of a followed cell must be finite")
    q = np.unique(np.quantile(v, np.arange(1, PPC_MAX_EDGES + 1) / (PPC_MAX_EDGES + 1), method="lower"))
    return q[q > v.min()]


def check_edges(edges) -> np.ndarray:
    """``edges`` as a float64 vector of at most 7 finite, strictly ascending values (``ValueError`` otherwise)."""
    e = np.asarray(edges, dtype=np.float64).reshape(-1)
    if e.size > PPC_MAX_EDGES:
        raise ValueError(f"{e.size} edges: at most {PPC_MAX_EDGES} (8 bins)")
    if not np.isfinite(e).all():
        raise ValueError("edges must be finite")
    if (np.diff(e) <= 0).any():
        raise ValueError("edges must be strictly ascending")
    return e


def _bin_sums(values, bins, nb):
    """(n, N, T) values summed over the cells of each bin: (n, nb); ``bins`` (N, T) holds -1 for cells that belong to no bin"""
    return np.stack([values[:, bins == b].sum(axis=1) for b in range(nb)], axis=1)


def predictive(model, fit, by, edges=None, seed: int = 0, replicate: Optional[Callable] = None, prob: float = 0.95) -> Dict[str, object]:
    """Posterior predictive check of a fitted survival model over all draws of ``fit``, folded chain after chain: does the model
    reproduce the infections the cohort saw at low, middle and high titers?  ``by`` maps one or two names to titer arrays (N, T),
    the binning variables -- free of the model's own predictor: an S-only fit binned by the N titer is the residual check against
    the omitted variable.  ``edges`` maps a name to up to 7 strictly ascending edges (bin = #{edges <= x}, ``risk.bin_of``'s rule);
    a name without edges gets ``default_edges`` of the model's followed cells.  Draw d's replicates depend on (``seed``, d, the
    individual, the interval) alone.

    Returns ``variables[name]`` with ``edges``, ``observed``, ``person_time``, ``n_cells`` (nb,), ``expected`` and ``replicate``
    (n_draws, nb), ``expected_median`` / ``_lower`` / ``_upper``, ``ratio`` = observed / expected per draw as ``ratio_median`` /
    ``_lower`` / ``_upper``, ``p_low`` = mean(R <= O), ``p_high`` = mean(R >= O) and ``flagged``, the bins with
    min(p_low, p_high) < 0.025; and per individual ``expected_i``, ``p_infected_i`` (the share of draws with a replicated
    infection), ``replicate_mean_i`` and ``observed_i``.  The entries ``PPC_FIT_KEYS`` are recorded in ``fit``; ``write`` stores
    them.
    ``replicate``: a host callable ``(q, draw0) -> (mu, r)``, both (n, N, T), in the device's place (tests); the model then needs
    ``names``, ``infected`` and ``exposure``."""
    names = [str(k) for k in by]
    if len(names) not in (1, 2):
        raise ValueError(f"one or two binning variables, got {len(names)}")
    titers = [np.asarray(by[k], dtype=np.float64) for k in by]
    edges = dict(edges or {})
    unknown = [k for k in edges if str(k) not in names]
    if unknown:
        raise ValueError(f"edges for {unknown}, which are not binning variables ({names})")
    edge_list = []
    for name, x in zip(names, titers):
        if edges.get(name) is not None:
            edge_list.append(check_edges(edges[name]))
        else:
            if not hasattr(model, "followed"):
                raise ValueError(f"no edges for {name} and the model has no followed cells to take the default from")
            edge_list.append(default_edges(x, model.followed))
    q = fit_points(model, fit)
    n, nv = q.shape[0], len(names)
    if n < 1:
        raise ValueError("the fit holds no draws")
    if replicate is not None:
        y, e = np.asarray(model.infected, dtype=np.float64), np.asarray(model.exposure, dtype=np.float64)
        m = followed_mask(y, e)
        mu, r = replicate(q, 0)
        mu, r = np.asarray(mu, dtype=np.float64), np.asarray(r, dtype=np.int64)
        if mu.shape != (n,) + y.shape or r.shape != mu.shape:
            raise ValueError(f"replicate must return two arrays of shape {(n,) + y.shape}")
        obs, pt, cells = np.zeros((nv, 8)), np.zeros((nv, 8)), np.zeros((nv, 8), np.int64)
        E, R = np.zeros((n, nv, 8)), np.zeros((n, nv, 8), np.int64)
        for v, (x, ed) in enumerate(zip(titers, edge_list)):
            if not np.isfinite(x[m]).all():
                raise ValueError(f"{names[v]}: titer of a followed cell must be finite")
            bins = np.where(m, risk.bin_of(np.where(m, x, 0.0), ed), -1)
            for b in range(ed.size + 1):
                sel = bins == b
                obs[v, b], pt[v, b], cells[v, b] = math.fsum(y[sel]), math.fsum(e[sel]), int(sel.sum())
            E[:, v, :ed.size + 1], R[:, v, :ed.size + 1] = _bin_sums(mu, bins, ed.size + 1), _bin_sums(r, bins, ed.size + 1)
        mu_f, r_f = np.where(m, mu, 0.0), np.where(m, r, 0)
        sum_e, sum_r, n_pos = mu_f.sum(axis=2).sum(axis=0), r_f.sum(axis=2).sum(axis=0), (r_f.sum(axis=2) >= 1).sum(axis=0)
        obs_i = np.array([math.fsum(row[mk]) for row, mk in zip(y, m)])
    else:
        model.predictive_configure(titers, edge_list, seed)
        model.predictive_reset()
        E, R = model.predictive_accumulate(q)
        sum_e, sum_r, n_pos, n_folded = model.predictive_stats()
        assert n_folded == n
        obs, pt, cells, obs_i = model.predictive_observed()
    out = {"n_draws": n, "seed": int(seed), "variables": {}, "expected_i": sum_e / n, "p_infected_i": n_pos / n, "replicate_mean_i": sum_r / n,
           "observed_i": obs_i}
    p_low, p_high = np.full((nv, 8), np.nan), np.full((nv, 8), np.nan)
    for v, (name, ed) in enumerate(zip(names, edge_list)):
        nb = ed.size + 1
        Ev, Rv, Ov = E[:, v, :nb], R[:, v, :nb], obs[v, :nb]
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(Ev > 0, Ov[None, :] / Ev, np.nan)
        ie, ir = _interval_of_draws(Ev, prob), _interval_of_draws(ratio, prob)
        p_low[v, :nb], p_high[v, :nb] = (Rv <= Ov[None, :]).mean(axis=0), (Rv >= Ov[None, :]).mean(axis=0)
        tail = np.minimum(p_low[v, :nb], p_high[v, :nb])
        out["variables"][name] = dict(
            edges=ed, observed=Ov, person_time=pt[v, :nb], n_cells=cells[v, :nb], expected=Ev, replicate=Rv, expected_median=ie["median"],
            expected_lower=ie["lower"], expected_upper=ie["upper"], ratio_median=ir["median"], ratio_lower=ir["lower"], ratio_upper=ir["upper"],
            p_low=p_low[v, :nb], p_high=p_high[v, :nb], flagged=np.flatnonzero((tail < PPC_FLAG) & (cells[v, :nb] > 0)))
    pad = np.full((nv, PPC_MAX_EDGES), np.nan)
    for v, ed in enumerate(edge_list):
        pad[v, :ed.size] = ed
    past = np.arange(8)[None, :] >= np.array([ed.size + 1 for ed in edge_list])[:, None]
    fit["ppc_variables"], fit["ppc_edges"], fit["ppc_n_bins"] = np.array(names), pad, np.array([ed.size + 1 for ed in edge_list], dtype=np.int64)
    fit["ppc_observed"], fit["ppc_person_time"], fit["ppc_n_cells"] = np.where(past, np.nan, obs), np.where(past, np.nan, pt), np.asarray(cells, np.int64)
    fit["ppc_expected"], fit["ppc_replicate"] = np.where(past[None], np.nan, E), np.asarray(R, dtype=np.int64)
    fit["ppc_p_low"], fit["ppc_p_high"] = p_low, p_high
    fit["ppc_expected_ind"], fit["ppc_p_infected_ind"] = out["expected_i"], out["p_infected_i"]
    fit["ppc_replicate_mean_ind"], fit["ppc_observed_ind"] = out["replicate_mean_i"], np.asarray(obs_i, dtype=np.float64)
    fit["ppc_n_draws"], fit["ppc_seed"] = np.array(n, dtype=np.int64), np.array(int(seed), dtype=np.int64)
    return out


def sample_posterior_predictive(model, fit, draws=None, seed: int = 0) -> np.ndarray:
    """(n, N, T) int32: the per-cell replicated infections of the draws ``draws`` of ``fit`` (indices into its points chain after
    chain; all of them by default), through ``abd_survival_replicate``: for the same ``seed`` exactly the replicates ``predictive``
    sums for those draws.  A model that ``predictive`` has not configured is configured with one bin (and one that it has loses its
    folded draws: the configuration carries the seed)."""
    q = fit_points(model, fit)
    idx = np.arange(q.shape[0]) if draws is None else np.asarray(draws, dtype=np.int64).reshape(-1)
    if idx.size and (idx.min() < 0 or idx.max() >= q.shape[0]):
        raise ValueError(f"draws must be indices in [0, {q.shape[0]})")
    N = model.followed.shape[0]
    model.predictive_configure([np.zeros(model.followed.shape)], [np.empty(0)], seed)
    out = np.empty((idx.size, N, model.T), dtype=np.int32)
    start = 0
    while start < idx.size:  # runs of consecutive draws share a call
        stop = start + 1
        while stop < idx.size and idx[stop] == idx[stop - 1] + 1:
            stop += 1
        out[start:stop] = model.replicate(q[idx[start]:idx[start] + stop - start], draw0=int(idx[start]))
        start = stop
    return out


def predictive_line(p) -> str:
    """One line per binning variable: observed over expected (the median over the draws) of every bin, and the worst bin with its
    tail probability min(p_low, p_high), marked where it is flagged."""
    lines = []
    for name, v in p["variables"].items():
        cells = " ".join(f"{o:.1f}/{m:.1f}" for o, m in zip(v["observed"], v["expected_median"]))
        tail = np.where(v["n_cells"] > 0, np.minimum(v["p_low"], v["p_high"]), np.inf)
        k = int(np.argmin(tail))
        side = "p_low" if v["p_low"][k] <= v["p_high"][k] else "p_high"
        lines.append(f"survival PPC by {name}: observed/expected per bin {cells}; worst bin {k} ({side} {tail[k]:.4f}"
                     + (", FLAGGED" if k in v["flagged"] else "") + f"); {len(v['flagged'])} of {len(v['observed'])} bins flagged ({p['n_draws']} draws)")
    return "\n".join(lines)


def protection(res, x, antigen: Optional[str] = None, prob: float = 0.95, group=None, period=None, interval=None) -> Dict[str, np.ndarray]:
    """``1 - 1 / (1 + exp(-b (x - a)))`` at titers ``x`` per draw, over all draws of all chains: ``mean``, ``median``, ``lower``,
    ``upper`` (each of ``x``'s shape).  ``antigen``: which titer of a combined fit ('S' or 'N'; the other held at its midpoint).
    ``group``: which group's ``a`` of a grouped fit (one of ``res["groups"]``).  Of a fit by period either ``period``, one of
    ``res["periods"]``, or ``interval``, an index in [0, T): the ``a`` of the period that interval belongs to."""
    a, b = np.asarray(res["a"], dtype=np.float64), np.asarray(res["b"], dtype=np.float64)
    if "periods" in res:
        labels, index = np.asarray(res["periods"]), np.asarray(res["period_index"])
        if (period is None) == (interval is None):
            raise ValueError(f"a fit by period: give period= (one of {labels.tolist()}) or interval= (0 to {len(index) - 1})")
        if interval is not None:
            if not (isinstance(interval, (int, np.integer)) and 0 <= interval < len(index)):
                raise ValueError(f"a fit by period: interval must be an index from 0 to {len(index) - 1}, got {interval!r}")
            k = int(index[interval])
        else:
            hit = np.flatnonzero(labels == period)
            if len(hit) != 1:
                raise ValueError(f"a fit by period: period must be one of {labels.tolist()}, got {period!r}")
            k = int(hit[0])
        a = a[..., k]
    elif period is not None or interval is not None:
        raise ValueError("period= and interval= are for a fit by period (model_alone_periods)")
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
    out = _interval_of_draws(p, prob)
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
    if "periods" in res:
        return _report_line_groups(res, prob, pct, names[0], labels="periods", label_name="period_name", by="period")
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


def _report_line_groups(res, prob: float, pct: int, ag: str, labels: str = "groups", label_name: str = "group_name", by: str = "group") -> str:
    """A grouped fit's line: per group ``a`` with its interval and the protection at titers 0 / 2 / 4, ``b`` once, the largest
    R-hat of the ``a_g`` and ``b``.  A fit by period has the same line over its periods (``labels="periods"``, ...)."""
    gname = str(np.asarray(res.get(label_name, by)))
    parts = []
    for k, label in enumerate(np.asarray(res[labels]).tolist()):
        iv = interval(np.asarray(res["a"])[..., k].reshape(-1), prob)
        pr = protection(res, np.array([0.0, 2.0, 4.0]), prob=prob, **{by: label})
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


def read_periods(path: str, n_intervals: int) -> np.ndarray:
    """One label per interval from ``.npy`` or a text file, read as ``read_groups`` reads its labels."""
    try:
        return read_groups(path, n_intervals)
    except ValueError as e:
        raise ValueError(str(e).replace("individuals", "intervals")) from None


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m abdpymc_amd.survival", description="Fit a survival model of a finished run.  Prints one line on stdout: medians and intervals of a and b, "
                                 "the protection at titers 0, 2 and 4, the largest R-hat of a and b.  With --compare: rank fits written with --waic.")
    ap.add_argument("--compare", nargs="+", metavar="FIT", help="Rank these fits of one cohort and window (.npz written with --waic) by WAIC over the "
                    "individuals: one row per model on stdout (rank, elpd_waic, p_waic, se, elpd_diff, dse).  Needs neither a cohort nor a GPU.")
    ap.add_argument("--ic", choices=("waic", "loo"), help="With --compare: rank by WAIC (the default) or by PSIS-LOO (fits written with --loo).")
    ap.add_argument("--posterior", help="A posterior .npz of abdpymc-infer (mean_i, mean_ab_s_mu, mean_ab_n_mu, or draws).")
    ap.add_argument("--ititers_data", help="The cohort directory the run was made from.")
    ap.add_argument("--start", type=int, help="First gap of the analysis (titers from here).")
    ap.add_argument("--end", type=int, help="One past the last gap of the analysis.")
    ap.add_argument("--model", choices=("s", "n", "combined", "s_groups", "n_groups", "s_periods", "n_periods"), default="combined")
    ap.add_argument("--groups", help="With --model s_groups / n_groups: a .npy or text file, one label per individual in cohort order.")
    ap.add_argument("--group_name", default="group", help="What the labels of --groups are (the reference's coordinate name).")
    ap.add_argument("--periods", default="monthly", help="With --model s_periods / n_periods: 'monthly' (one midpoint per interval, the default), "
                    "'splits' (one per variant era, from --split_delta / --split_omicron as abdpymc-infer takes them), or a .npy or text "
                    "file with one label per interval.")
    ap.add_argument("--split_delta", action="store_true", help="With --periods splits: a new period where delta started to circulate.")
    ap.add_argument("--split_omicron", action="store_true", help="With --periods splits: a new period where omicron started to circulate.")
    ap.add_argument("--period_name", help="What the labels of --periods are (default: 'intervals' for monthly, else 'period').")
    ap.add_argument("--out", help="Output file (.npz; NetCDF where ArviZ imports and the name does not end in .npz).")
    ap.add_argument("--waic", action="store_true", help="Score the fit by WAIC over the individuals on the device: a second line on stdout, and "
                    "elpd_waic_ind, p_waic_ind, waic_n_cells, waic_n_draws, start, end in the output (what --compare reads).")
    ap.add_argument("--loo", action="store_true", help="Score the fit by PSIS-LOO over the individuals on the device (at most 16384 draws): a line on "
                    "stdout after the WAIC line (elpd_loo, p_loo, se, the individuals with Pareto k above 0.7), and elpd_loo_ind, pareto_k_ind, "
                    "lppd_ind, loo_n_cells, loo_n_draws, start, end in the output (what --compare --ic loo reads).")
    ap.add_argument("--ppc", action="store_true", help="Posterior predictive check on the device: per titer bin the observed infections against the "
                    "expected and replicated ones of every draw; one more line on stdout per binning variable, and the ppc_* entries in the output.")
    ap.add_argument("--ppc_edges_s", help="With --ppc: comma-separated bin edges of the S titer (up to 7, ascending; default: the octiles).")
    ap.add_argument("--ppc_edges_n", help="With --ppc: comma-separated bin edges of the N titer (up to 7, ascending; default: the octiles).")
    ap.add_argument("--ppc_seed", type=int, help="With --ppc: the seed of the replicates (default: --seed).")
    ap.add_argument("--per_draw", type=int, metavar="M", help="Per-draw fits (multiple imputation) with --model s | n | combined: fit the model to M "
                    "recorded draws of the posterior, each with its own infections and titers, spaced evenly over chains x draws, and pool "
                    "them.  The line on stdout is of the pooled draws and ends with the share of the variance of a and b that lies between "
                    "the datasets; the output also holds dataset, source, n_evaluations and the draws_* entries.  Needs a posterior with "
                    "recorded draws (abdpymc-infer --thin).")
    ap.add_argument("--per_draw_chains", type=int, metavar="C", help="With --per_draw: chains per dataset (default 1); --chains is not used then.")
    ap.add_argument("--per_draw_ic", choices=("waic", "loo", "both"), help="With --per_draw: score every dataset's draws on that dataset by WAIC "
                    "and / or PSIS-LOO over the individuals on the device and pool them by Rubin's rule: one more line on stdout per criterion "
                    "(pooled elpd, p, se, the share between the datasets, the warnings), and the draws_elpd_waic_ind ... / draws_elpd_loo_ind ... "
                    "entries, start and end in the output (what --compare reads for per-draw fits).")
    ap.add_argument("--tune", type=int, default=1000)
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--chains", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", type=int, default=-1)
    args = ap.parse_args(argv)
    if args.compare:
        return _main_compare(args.compare, args.ic or "waic")
    if args.ic is not None:
        ap.error("--ic goes with --compare")
    missing = [f"--{k}" for k in ("posterior", "ititers_data", "start", "end", "out") if getattr(args, k) is None]
    if missing:
        ap.error("the following arguments are required: " + ", ".join(missing))
    by_period = args.model.endswith("_periods")
    if by_period and args.periods == "splits" and not (args.split_delta or args.split_omicron):
        ap.error("--periods splits needs --split_delta and / or --split_omicron")
    if (args.split_delta or args.split_omicron) and not (by_period and args.periods == "splits"):
        ap.error("--split_delta / --split_omicron go with --model s_periods | n_periods --periods splits")
    if not by_period and (args.periods != "monthly" or args.period_name is not None):
        ap.error("--periods / --period_name go with --model s_periods | n_periods")
    if not args.ppc and (args.ppc_edges_s is not None or args.ppc_edges_n is not None or args.ppc_seed is not None):
        ap.error("--ppc_edges_s / --ppc_edges_n / --ppc_seed go with --ppc")
    if args.per_draw is None and args.per_draw_chains is not None:
        ap.error("--per_draw_chains goes with --per_draw")
    if args.per_draw is None and args.per_draw_ic is not None:
        ap.error("--per_draw_ic goes with --per_draw")
    if args.per_draw is not None:
        if args.model not in ("s", "n", "combined"):
            ap.error(f"--per_draw fits --model s | n | combined here; per-draw fits of --model {args.model} are in Python: "
                     "SurvivalAnalysis.model_alone_groups_draws / model_alone_periods_draws with sample_draws and draws_summary")
        if args.waic or args.ppc:
            ap.error("--per_draw does not go with --waic / --ppc: WAIC of a per-draw fit is --per_draw_ic waic (per dataset, pooled); "
                     "predictive checks of a per-draw fit are not built")
        if args.loo:
            ap.error("--per_draw does not go with --loo: PSIS-LOO of a per-draw fit is --per_draw_ic loo (per dataset, pooled)")
        if args.per_draw < 1 or (args.per_draw_chains is not None and args.per_draw_chains < 1):
            ap.error("--per_draw and --per_draw_chains must be >= 1")
    ppc_edges = {}
    for name, text in (("S", args.ppc_edges_s), ("N", args.ppc_edges_n)):
        if text is not None:
            try:
                ppc_edges[name] = check_edges([float(v) for v in text.split(",")])
            except ValueError as e:
                ap.error(f"--ppc_edges_{name.lower()}: {e}")
    from .data import TiterData

    data = TiterData.from_disk(args.ititers_data)
    try:
        sa = SurvivalAnalysis(args.posterior, args.start, args.end, data, device=args.device)
        if args.per_draw is not None:
            return _main_per_draw(args, sa)
        if by_period:
            if args.periods == "monthly":
                periods = None
            elif args.periods == "splits":
                periods = sa.periods_from_splits(data.calculate_splits(delta=args.split_delta, omicron=args.split_omicron))
            else:
                periods = read_periods(args.periods, sa.n_int)
            model = sa.model_alone_periods(args.model[0].upper(), periods, args.period_name)
        elif args.model.endswith("_groups"):
            if not args.groups:
                raise ValueError(f"--model {args.model} needs --groups FILE")
            model = sa.model_alone_groups(args.model[0].upper(), read_groups(args.groups, sa.infected.shape[0]), args.group_name)
        else:
            model = sa.model_combined() if args.model == "combined" else sa.model_alone(args.model.upper())
    except ValueError as e:
        raise SystemExit(f"survival: {e}")
    res = sample(model, tune=args.tune, draws=args.draws, chains=args.chains, seed=args.seed)
    w = waic(model, res) if args.waic else None
    try:
        lo = loo(model, res) if args.loo else None
    except ValueError as e:  # more draws than the device keeps
        raise SystemExit(f"survival: {e}")
    try:  # both titers, whatever the model's own predictor is
        ppc = predictive(model, res, {"S": sa.s_titer, "N": sa.n_titer}, edges=ppc_edges,
                         seed=args.seed if args.ppc_seed is None else args.ppc_seed) if args.ppc else None
    except ValueError as e:
        raise SystemExit(f"survival: {e}")
    model.close()
    print(report_line(res))  # the one line, on stdout; progress and the file's name go to stderr
    if w is not None:
        print(waic_line(w))  # --waic: and this one
    if lo is not None:
        print(loo_line(lo))  # --loo: after it
    if ppc is not None:
        print(predictive_line(ppc))  # --ppc: and one per binning variable
    out = write(res, args.out, sa)
    print(f"wrote {out}", file=sys.stderr)
    return 0


def _main_per_draw(args, sa) -> int:
    """--per_draw: ``sample_draws`` on M datasets, the pooled line, the file.  A ``ValueError`` (a posterior without draws) is the
    caller's to report."""
    datasets = sa.draws(n_datasets=args.per_draw)
    model = sa.model_combined_draws(datasets) if args.model == "combined" else sa.model_alone_draws(args.model.upper(), datasets)
    scores = []
    try:
        res = sample_draws(model, tune=args.tune, draws=args.draws, chains_per_dataset=args.per_draw_chains or 1, seed=args.seed)
        if args.per_draw_ic in ("waic", "both"):
            scores.append(waic_draws(model, res))
        if args.per_draw_ic in ("loo", "both"):
            scores.append(loo_draws(model, res))  # (a ValueError -- more draws of a dataset than the device keeps -- is the caller's)
    finally:
        model.close()
    sm = draws_summary(res)
    res.update(draws_fit_keys(sm))
    between = ", ".join(f"{k} {sm[k]['frac_between']:.3f}" for k in sm if k[0] in "ab")
    print(f"{report_line(res)}; per-draw fits of {datasets.n_datasets} datasets, share of the variance between datasets: {between}")
    for w in scores:
        print(draws_ic_line(w))  # --per_draw_ic: one line per criterion after the pooled line
    out = write(res, args.out, sa)
    print(f"wrote {out}", file=sys.stderr)
    return 0


def _main_compare(paths, ic: str = "waic") -> int:
    import os

    fits = {}
    for path in paths:
        name = os.path.splitext(os.path.basename(str(path)))[0]
        if name in fits:
            raise SystemExit(f"survival: two fits are called {name}")
        with np.load(path, allow_pickle=False) as f:
            fits[name] = {k: f[k] for k in WAIC_FIT_KEYS + LOO_FIT_KEYS + DRAWS_WAIC_FIT_KEYS + DRAWS_LOO_FIT_KEYS + ("start", "end", "source")
                          if k in f.files}
    # per-draw fits (written with --per_draw_ic) get the pooled table; a mixture of per-draw and plug-in fits is an error
    keys = DRAWS_WAIC_FIT_KEYS if ic == "waic" else DRAWS_LOO_FIT_KEYS
    per_draw = [name for name, fit in fits.items() if all(k in fit for k in keys)]
    if per_draw and len(per_draw) < len(fits):
        rest = [name for name in fits if name not in per_draw]
        raise SystemExit(f"survival: {', '.join(per_draw)} hold the per-draw entries {keys[0]} ... (--per_draw_ic) and {', '.join(rest)} "
                         f"{'does' if len(rest) == 1 else 'do'} not: compare per-draw fits with per-draw fits")
    try:
        lines = draws_compare_lines(compare_draws(fits, ic=ic)) if per_draw else compare_lines(compare(fits, ic=ic))
    except ValueError as e:
        raise SystemExit(f"survival: {e}")
    for line in lines:
        print(line)
    return 0


def write(res, path: str, sa: "SurvivalAnalysis") -> str:
    """``.npz``; NetCDF through ``cli.write_posterior`` where ArviZ imports and the name does not end in ``.npz`` (no test covers
    that branch: ArviZ is optional and the suite does not require it).  A fit that ``waic`` has scored is stored with its
    ``elpd_waic_ind``, ``p_waic_ind``, ``waic_n_cells``, ``waic_n_draws`` (one that ``loo`` has scored with ``LOO_FIT_KEYS``) and the window ``start`` / ``end`` -- in the ``.npz`` form,
    which is what ``--compare`` reads; the NetCDF form holds the draws alone.  The same goes for a fit of ``sample_draws`` that ``waic_draws`` /
    ``loo_draws`` have scored (``DRAWS_WAIC_FIT_KEYS``, ``DRAWS_LOO_FIT_KEYS``).  Likewise ``groups`` / ``group_name`` and ``periods`` /
    ``period_name`` / ``period_index`` are stored in the ``.npz`` form only: ``protection(group= / period= / interval=)`` needs a fit
    written as ``.npz``.  So are the entries ``PPC_FIT_KEYS`` of a fit that ``predictive`` has checked."""
    path = str(path)
    if any(k in res for k in ("elpd_waic_ind", "elpd_loo_ind", "draws_elpd_waic_ind", "draws_elpd_loo_ind")):
        res = dict(res, start=np.array(sa.start, dtype=np.int64), end=np.array(sa.end, dtype=np.int64))
    if not path.endswith(".npz"):
        try:
            import arviz  # noqa: F401

            from .cli import write_posterior

            data = {k: v for k, v in res.items() if k not in ("antigens", "groups", "group_name", "periods", "period_name", "period_index", "start", "end") + WAIC_FIT_KEYS + LOO_FIT_KEYS + PPC_FIT_KEYS + DRAWS_FIT_KEYS + DRAWS_WAIC_FIT_KEYS + DRAWS_LOO_FIT_KEYS}
            return write_posterior(data, path, dict(gap=sa.intervals, ind=np.arange(sa.infected.shape[0])))
        except ImportError:
            path += ".npz"
    np.savez_compressed(path, **res, intervals=sa.intervals, t0=np.array(sa.t0 or ""))
    return path


if __name__ == "__main__":
    raise SystemExit(main())
