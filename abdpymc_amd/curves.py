"""
Epidemic curves with posterior uncertainty: infections per gap, the cumulative attack rate, seroprevalence and the mean
titer of the population, one curve per draw.

The native sampler reduces every draw's Deterministics over the individuals on the device (``sample(..., curves=True)``,
``Context.curves``; csrc/abd_curves.hpp), so a draw costs a row of 6 G + 8 numbers instead of three (G, N) arrays and every
draw is kept whatever ``thin`` is.  ``from_deterministics`` is the same definition as literal NumPy, for recorded (G, N)
arrays; ``summary`` turns the per-draw curves into medians and credible intervals.

Definition.  ``last_gap[j]`` in [-1, G-1] is the end of individual j's follow-up, its last serum sample (``TiterData.last_gap``;
-1: never followed; default G-1 for everyone), and cell (g, j) is *followed* iff ``g <= last_gap[j]``: an individual is not
counted after its follow-up ended (as the reference's timelines and survival code stop there).  Per draw:

    counts (4, G)        infected       #{j followed at g: i[g, j] = 1}
                         ever_infected  #{j followed at g: i[g', j] = 1 for some g' <= g}
                         seropos_s      #{j followed at g: ab_s_mu[g, j] >= thr_s}
                         seropos_n      #{j followed at g: ab_n_mu[g, j] >= thr_n}
    n_infections (8,)    individuals with last_gap[j] >= 0 by their number of infections in gaps 0 .. last_gap[j]; [7]: 7 or more
    titer_sums (2, G)    sums over the followed j of ab_s_mu[g, j], of ab_n_mu[g, j]

NumPy only.
"""
from __future__ import annotations

from typing import Dict, Sequence

import numpy as np

from .summaries import Summary, interval

COUNT_NAMES = ("infected", "ever_infected", "seropos_s", "seropos_n")
N_BINS = 8
# what sample(..., curves=True) returns: (chains, draws, G) each, n_infections (chains, draws, 8), n_followed (chains, G)
RESULT_KEYS = tuple(f"curves_{n}" for n in COUNT_NAMES) + ("curves_titer_s", "curves_titer_n", "curves_n_infections",
                                                           "curves_n_followed")


def _last_gap(last_gap, G: int, N: int) -> np.ndarray:
    if last_gap is None:
        return np.full(N, G - 1, dtype=np.int64)
    lg = np.asarray(last_gap)
    if lg.shape != (N,) or not np.issubdtype(lg.dtype, np.integer):
        raise ValueError(f"last_gap must be an integer array of shape ({N},)")
    if lg.size and (lg.min() < -1 or lg.max() >= G):
        raise ValueError(f"last_gap outside [-1, {G})")
    return lg.astype(np.int64)


def n_followed(last_gap, G: int) -> np.ndarray:
    """(G,) int64: the individuals followed at every gap, #{j: g <= last_gap[j]}."""
    lg = np.asarray(last_gap)
    return (np.arange(int(G))[:, None] <= lg[None, :]).sum(axis=1).astype(np.int64)


def from_deterministics(i, ab_s_mu, ab_n_mu, last_gap=None, thr_s: float = np.inf, thr_n: float = np.inf) -> Dict[str, np.ndarray]:
    """The curves of recorded Deterministics: ``i``, ``ab_s_mu``, ``ab_n_mu`` are (..., G, N); returns ``counts`` (..., 4, G)
    int64, ``n_infections`` (..., 8) int64 and ``titer_sums`` (..., 2, G) as defined in the module's docstring."""
    i, ab_s_mu, ab_n_mu = np.asarray(i), np.asarray(ab_s_mu, dtype=np.float64), np.asarray(ab_n_mu, dtype=np.float64)
    if i.ndim < 2 or i.shape != ab_s_mu.shape or i.shape != ab_n_mu.shape:
        raise ValueError("i, ab_s_mu, ab_n_mu must share a shape (..., G, N)")
    G, N = i.shape[-2:]
    lg = _last_gap(last_gap, G, N)
    followed = np.arange(G)[:, None] <= lg[None, :]  # (G, N)
    inf = i != 0
    ever = np.cumsum(inf, axis=-2) > 0
    counts = np.stack([(inf & followed).sum(axis=-1), (ever & followed).sum(axis=-1),
                       ((ab_s_mu >= thr_s) & followed).sum(axis=-1), ((ab_n_mu >= thr_n) & followed).sum(axis=-1)],
                      axis=-2).astype(np.int64)
    per_ind = (inf & followed).sum(axis=-2)  # (..., N): infections in gaps 0 .. last_gap[j]
    binned = np.minimum(per_ind, N_BINS - 1)
    n_inf = np.stack([((binned == k) & (lg >= 0)).sum(axis=-1) for k in range(N_BINS)], axis=-1).astype(np.int64)
    sums = np.stack([np.where(followed, ab_s_mu, 0.0).sum(axis=-1), np.where(followed, ab_n_mu, 0.0).sum(axis=-1)], axis=-2)
    return {"counts": counts, "n_infections": n_inf, "titer_sums": sums}


def as_result(counts, n_infections, titer_sums, followed) -> Dict[str, np.ndarray]:
    """The ``curves_*`` keys of a sampler result from arrays with leading (chains, draws) axes -- ``counts`` (chains, draws, 4,
    G), ``n_infections`` (chains, draws, 8), ``titer_sums`` (chains, draws, 2, G) -- and ``followed`` (G,) = ``n_followed``."""
    counts, sums = np.asarray(counts), np.asarray(titer_sums)
    res = {f"curves_{name}": counts[:, :, k, :] for k, name in enumerate(COUNT_NAMES)}
    res["curves_titer_s"], res["curves_titer_n"] = sums[:, :, 0, :], sums[:, :, 1, :]
    res["curves_n_infections"] = np.asarray(n_infections)
    res["curves_n_followed"] = np.tile(np.asarray(followed, dtype=np.int64), (counts.shape[0], 1))
    return res


def _curves_of(res) -> Dict[str, np.ndarray]:
    missing = [k for k in RESULT_KEYS if k not in res]
    if missing:
        raise ValueError(f"no curves in this result (sample(..., curves=True)): {missing[0]} is missing")
    return {k: np.asarray(res[k]) for k in RESULT_KEYS}


def merge_chains(parts: Sequence[dict]) -> Dict[str, np.ndarray]:
    """Curves of several runs over the SAME cohort and follow-up as one result: concatenated along the chain axis."""
    cs = [_curves_of(p) for p in parts]
    return {k: np.concatenate([c[k] for c in cs], axis=0) for k in RESULT_KEYS}


def merge_individual_shards(parts: Sequence[dict]) -> Dict[str, np.ndarray]:
    """Curves of the same chains and draws over disjoint slices of the individuals (``distributed.IndividualShards``) as the
    whole cohort's: every key is a sum over individuals, so the shards add elementwise -- counts and n_followed exactly, the
    titer sums to rounding."""
    cs = [_curves_of(p) for p in parts]
    out = {k: cs[0][k].copy() for k in RESULT_KEYS}
    for c in cs[1:]:
        for k in RESULT_KEYS:
            if c[k].shape != out[k].shape:
                raise ValueError(f"{k}: shards differ in shape, {c[k].shape} against {out[k].shape}")
            out[k] = out[k] + c[k]
    return out


def summary(res, prob: float = 0.95) -> Dict[str, object]:
    """Medians and equal-tailed ``prob`` intervals of the curves, chains and draws pooled.  Per gap, each a dict of
    ``median`` / ``lower`` / ``upper`` (G,), as shares of the individuals followed at the gap (NaN where nobody is):

        incidence        infected / n_followed
        attack_rate      ever_infected / n_followed, the cumulative attack rate
        first_incidence  diff of attack_rate along the gaps (its first entry is attack_rate[0]): first infections per gap;
                         where follow-up ends for some it compares two slightly different sets of individuals
        seroprev_s, seroprev_n   seropos_* / n_followed
        mean_titer_s, mean_titer_n   titer sums / n_followed

    and ``n_infections``: (8,) the posterior mean share of the followed individuals with k infections (7: 7 or more),
    ``n_followed`` (G,), ``n_draws`` (pooled) and ``prob``.  ``res``: a ``sample(..., curves=True)`` result or any dict with
    the ``curves_*`` keys (``as_result``, ``merge_chains``, ``merge_individual_shards``)."""
    if not 0.0 < prob < 1.0:
        raise ValueError(f"prob must be in (0, 1), got {prob}")
    c = _curves_of(res)
    nf = c["curves_n_followed"]
    if nf.ndim != 2 or (nf != nf[:1]).any():
        raise ValueError("curves_n_followed differs between chains: pool chains of one cohort and follow-up only")
    G = nf.shape[1]
    denom = np.where(nf[0] > 0, nf[0], np.nan).astype(np.float64)

    def share(key):
        return c[key].reshape(-1, G).astype(np.float64) / denom

    attack = share("curves_ever_infected")
    out: Dict[str, object] = {
        "incidence": interval(share("curves_infected"), prob),
        "attack_rate": interval(attack, prob),
        "first_incidence": interval(np.diff(attack, axis=1, prepend=0.0), prob),
        "seroprev_s": interval(share("curves_seropos_s"), prob),
        "seroprev_n": interval(share("curves_seropos_n"), prob),
        "mean_titer_s": interval(share("curves_titer_s"), prob),
        "mean_titer_n": interval(share("curves_titer_n"), prob),
    }
    bins = c["curves_n_infections"].reshape(-1, N_BINS).astype(np.float64)
    tot = bins.sum(axis=1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        out["n_infections"] = (bins / np.where(tot > 0, tot, np.nan)).mean(axis=0) if bins.shape[0] else np.full(N_BINS, np.nan)
    out["n_followed"] = nf[0].copy()
    out["n_draws"] = int(bins.shape[0])
    out["prob"] = float(prob)
    return out


def summary_arrays(sm: dict) -> Dict[str, np.ndarray]:
    """``summary`` flattened to named arrays (``curves_summary_<quantity>``: rows lower, median, upper) for a posterior file."""
    out = {f"curves_summary_{k}": np.stack([v["lower"], v["median"], v["upper"]]) for k, v in sm.items() if isinstance(v, dict)}
    out["curves_summary_n_infections"] = np.asarray(sm["n_infections"])
    return out


class _Curves(Summary):
    """``curves``: keep the epidemic curves of EVERY draw, reduced over the individuals on the device (``thin`` does not apply):
    ``curves_infected`` / ``curves_ever_infected`` / ``curves_seropos_s`` / ``curves_seropos_n`` (counts) and ``curves_titer_s`` /
    ``curves_titer_n`` (titer sums), each (chains, draws, G), ``curves_n_infections`` (chains, draws, 8) and ``curves_n_followed``
    (chains, G); ``summary`` reads them.  An individual counts up to its last serum sample (``model.data.last_gap`` where the
    model's data has one, else every gap); ``sero_thresholds`` = (thr_s, thr_n) on the titer scale switch the seropositive counts
    on.  The arrays are not counted against the host budget.  The trajectories do not change."""

    name = "curves"
    options = {"curves": False, "sero_thresholds": None}
    prefix = "curves_"
    draw_keys = RESULT_KEYS[:-1]  # one row per draw; the number followed and the summary have no draw axis
    dims = {**{k: ["gap"] for k in RESULT_KEYS[:-2]}, "curves_n_followed": ["chain", "gap"]}
    follow_up = True
    native_only = "curves need the native sampler (sample(native=True)): every draw is reduced on the device inside it"

    def enable(self, smp, plan):
        smp.enable_curves(plan["draws"], plan["sero_thresholds"])

    def collect(self, smp, plan, last_gap):
        per_chain = [smp.curves(c) for c in range(plan["chains"])]
        G, N = plan["G"], plan["N"]
        return as_result(*(np.stack([pc[k] for pc in per_chain]) for k in ("counts", "n_infections", "titer_sums")),
                         n_followed(np.full(N, G - 1) if last_gap is None else last_gap, G))

    def add_arguments(self, parser):
        parser.add_argument("--curves", help="Keep the epidemic curves of every draw (infections per gap, cumulative attack rate, "
                            "seroprevalence, mean titers; reduced over the individuals on the device, --thin does not apply) and report "
                            "the final cumulative attack rate and the peak monthly incidence with 95 %% intervals (curves_* in the "
                            "output).  An individual counts up to its last serum sample.", action="store_true")
        parser.add_argument("--sero_threshold_s", help="With --curves: S titer from which an individual counts as seropositive.",
                            type=float, default=float("inf"))
        parser.add_argument("--sero_threshold_n", help="With --curves: N titer from which an individual counts as seropositive.",
                            type=float, default=float("inf"))

    def cli_options(self, args, data, chains, world):
        return {"curves": args.curves, "sero_thresholds": (args.sero_threshold_s, args.sero_threshold_n)}

    def report(self, res, data):
        """``summary``'s arrays go into ``res`` (``curves_summary_*``: rows lower, median, upper per gap)."""
        sm = summary(res)
        res.update(summary_arrays(sm))
        followed = np.flatnonzero(sm["n_followed"] > 0)
        if not (followed.size and sm["n_draws"]):
            return []
        g, inc = followed[-1], sm["incidence"]
        peak = followed[np.argmax(inc["median"][followed])]
        ar = sm["attack_rate"]
        pct = int(round(100 * sm["prob"]))
        return [f"curves: cumulative attack rate at gap {g} {100 * ar['median'][g]:.1f} % ({pct} % interval "
                f"{100 * ar['lower'][g]:.1f}-{100 * ar['upper'][g]:.1f}; {sm['n_followed'][g]} followed); peak monthly incidence "
                f"{100 * inc['median'][peak]:.1f} % ({100 * inc['lower'][peak]:.1f}-{100 * inc['upper'][peak]:.1f}) at gap {peak}; "
                f"{sm['n_draws']} draws"]


SUMMARY = _Curves()
