"""
PSIS-LOO by individual for the titer model: the joint log-likelihood of every individual's OD readings,
T_sj = S_sj + N_sj (``Context.individual_loglik``: ll_s + ll_n), of every kept draw of every chain stays on the device in one
individual-major matrix, and every individual's column over all chains is Pareto-smoothed there by the estimator of DESIGN.md §27
(``compare.psis_loo_from_matrix`` is its host restatement): Vehtari et al. 2024 with r_eff = 1.

    elpd_loo_j = log sum_s w_sj exp(T_sj),  w_sj the smoothed, normalised weights of exp(-T_sj)
    lppd_j     = log( (1 / S) sum_s exp(T_sj) ),   p_loo_j = lppd_j - elpd_loo_j
    pareto_k_j : the shape of the generalised Pareto fitted to the largest M = min(S / 5, ceil(3 sqrt(S))) weights

Against WAIC by individual (``compare``: ``waic_by="individual"``) it gives the same kind of sum, with a Pareto k per individual
that says for whom the number can be trusted: above min(1 - 1 / log10(S), 0.7) the S draws are too few.

``sample(..., loo=True)`` returns the ``loo_*`` keys, ``loo`` reads them, ``compare.compare(..., ic="loo")`` ranks variants.
NumPy only.
"""
from __future__ import annotations

import warnings
from typing import Dict, Mapping

import numpy as np

from . import compare as _compare
from .summaries import Summary

MAX_DRAWS = 16384  # ABD_SAMPLER_LOO_MAX_DRAWS: the kept draws of all chains together
RESULT_KEYS = ("loo_elpd_i", "loo_pareto_k", "loo_lppd_i", "loo_n_tail", "loo_n_readings", "loo_n_draws")
IND_KEYS = ("elpd_loo_ind", "p_loo_ind", "pareto_k_ind")  # what the CLI adds per individual


def kept_draws(draws: int, thin: int) -> int:
    """C, the draws 0, thin, 2 thin, ... of ``draws``."""
    return -(-int(draws) // int(thin))


def loo(res) -> Dict[str, object]:
    """PSIS-LOO by individual of a ``sample(..., loo=True)`` result, or of a posterior file it was written to and loaded from (the
    mapping of an ``.npz``, or an InferenceData whose ``constant_data`` holds the keys): the dictionary of
    ``compare.loo_from_individual``."""
    if not isinstance(res, Mapping) and not hasattr(res, "files") and hasattr(res, "constant_data"):
        res = {k: np.asarray(v) for k, v in res.constant_data.data_vars.items()}
    return _compare.loo_from_result(res)


def line(w, ids=None) -> str:
    """The report line of ``loo``'s dictionary; ``ids``: the individuals' names."""
    out = (f"LOO by individual: elpd_loo {w['elpd_loo']:.3f}  p_loo {w['p_loo']:.3f}  se {w['se']:.3f}  ({w['n_individuals']} individuals, "
           f"{w['n_draws']} draws; {w['n_bad']} with k > 0.7, {w['n_warn']} above {w['k_threshold']:.2f}")
    if w["worst"] is not None:
        j = w["worst"]
        out += f"; worst: individual {j if ids is None else ids[j]} k {w['pareto_k'][j]:.2f}"
    return out + ")"


class _Loo(Summary):
    """``loo``: keep T_j of draws 0, ``loo_thin``, 2 ``loo_thin``, ... of every chain on the device (``thin`` does not apply) and
    smooth every individual's column there after the last draw.  Pooled over the chains, in chain-major draw order: ``loo_elpd_i``,
    ``loo_pareto_k`` (+inf where the tail has at most 4 draws; NaN without readings), ``loo_lppd_i`` (N,), ``loo_n_tail`` (N,) int32,
    ``loo_n_readings`` (N,) int64, and ``loo_n_draws`` (1,) = chains * ceil(draws / loo_thin), at most 16384.  ``loo`` reads them.
    The per-individual launch of a draw is shared with ``waic_by="individual"``, whose accumulators keep their bits; the
    trajectories do not change."""

    name = "loo"
    options = {"loo": False, "loo_thin": 1}
    prefix = "loo_"
    derived_keys = IND_KEYS
    dims = dict({k: ["ind"] for k in IND_KEYS}, **{k: ["ind"] for k in RESULT_KEYS[:5]})
    native_only = ("loo needs the native sampler (sample(native=True)): the per-individual log-likelihood is kept and smoothed "
                   "inside it")

    def plan(self, opts, draws, chains, G, N):
        p = super().plan(opts, draws, chains, G, N)
        if p is None:
            return None
        thin = p["loo_thin"]
        if not isinstance(thin, (int, np.integer)) or isinstance(thin, bool) or thin < 1:
            raise ValueError(f"loo_thin must be an integer >= 1, got {thin!r}")
        if draws < 1:
            raise ValueError("loo needs at least one draw")
        C = kept_draws(draws, thin)
        if chains * C > MAX_DRAWS:
            room = MAX_DRAWS // chains  # kept draws per chain that fit
            raise ValueError(f"loo keeps {chains} chains x {C} draws = {chains * C} columns per individual, over the {MAX_DRAWS} the "
                             f"device smooths" + (f": a larger loo_thin fits (loo_thin >= {kept_draws(draws, room)})" if room else ""))
        p["kept"] = C
        return p

    def enable(self, smp, plan):
        smp.enable_loo(plan["draws"], plan["loo_thin"])

    def collect(self, smp, plan, last_gap):
        st = smp.loo_stats()
        return {"loo_elpd_i": st["elpd_loo"], "loo_pareto_k": st["pareto_k"], "loo_lppd_i": st["lppd"], "loo_n_tail": st["n_tail"],
                "loo_n_readings": st["n_readings"], "loo_n_draws": np.array([st["n_draws"]], dtype=np.int64)}

    def add_arguments(self, parser):
        parser.add_argument("--loo", help="Keep the joint log-likelihood of each individual's readings at every draw on the device and "
                            "report PSIS-LOO by individual (elpd_loo, p_loo, se, the individuals whose Pareto k says the estimate "
                            "cannot be trusted; elpd_loo_ind / p_loo_ind / pareto_k_ind in the output).", action="store_true")
        parser.add_argument("--loo_thin", help="With --loo: keep every T-th draw (at most 16384 kept draws over all chains).", type=int,
                            default=None, metavar="T")

    def cli_options(self, args, data, chains, world):
        """Chains sharded over processes would need the columns of the other GPUs' chains on one device: refused."""
        if args.loo_thin is not None and not args.loo:
            raise SystemExit("--loo_thin needs --loo")
        if args.loo and world > 1:
            raise SystemExit(f"--loo smooths the draws of all chains on one device: it does not run over {world} processes")
        return {"loo": args.loo, "loo_thin": 1 if args.loo_thin is None else args.loo_thin}

    def report(self, res, data):
        """The per-individual values go into ``res`` (keys IND_KEYS)."""
        w = loo(res)
        res["elpd_loo_ind"], res["p_loo_ind"], res["pareto_k_ind"] = w["elpd_i"], w["p_loo_i"], w["pareto_k"]
        if w["n_bad"]:
            warnings.warn(f"LOO by individual: {w['n_bad']} of {w['n_individuals']} individuals have a Pareto k above "
                          f"{_compare.WARN_PARETO_K}: their elpd_loo cannot be trusted", stacklevel=2)
        return [line(w, getattr(data, "coords", {}).get("ind"))]


SUMMARY = _Loo()
