"""
Convergence diagnostics per cell over ALL draws: split R-hat and a batch-means effective sample size of the Deterministics
``i``, ``ab_n_mu``, ``ab_s_mu``, for runs that never keep their draws.

The native sampler accumulates, per chain and cell, the second moments of either half of the chain and the moments of the
means of batches of ``L`` draws (``sample(..., diagnostics=True)``; csrc/abd_diag.hpp; include/abd_hip.h has the definition in
full).  ``from_draws`` is the same definition as literal NumPy, for draws that were kept; ``rhat`` and ``ess`` read either.

Definition.  ``D`` draws, ``H = D // 2``: half 0 is draws ``0 .. H-1``, half 1 draws ``H .. 2H-1``; a draw ``>= 2H`` is ignored.
Each half is cut into ``B = H // L`` whole batches from its start; the trailing ``H % L`` draws of a half enter its moments
but no batch.  Per chain (all start at 0)::

    mean_h, M2_h    Welford over half h, n the draw's 1-based place in it:  d = x - mean; mean += d * (1.0 / n); M2 += d * (x - mean)
    cur             cur = x on the first draw of a batch, else cur += x
    bm_mean, bm_M2  when a batch closes, b the batches closed so far in the chain (both halves pooled), this one included:
                    bm = cur * (1.0 / L); e = bm - bm_mean; bm_mean += e * (1.0 / b); bm_M2 += e * (bm - bm_mean)

For integer input (``i``: 0 or 1) every moment is a function of counts, so counts are kept: ``c_h0``, ``c_h1`` (ones in either
half), ``sum_cb`` (the sum of the closed batches' counts) and ``sum_cb2`` (the sum of their squares).

A set of MOMENTS is a dict with ``info`` (chains, 4) int64 = draws in half 0, draws in half 1, batches closed, L, and either
``moments`` (chains, 6, ...) float64 = mean_h0, M2_h0, mean_h1, M2_h1, bm_mean, bm_M2 or ``counts`` (chains, 4, ...) int64 =
c_h0, c_h1, sum_cb, sum_cb2.

NumPy only.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence

import numpy as np

from .summaries import Summary

# what sample(..., diagnostics=True) returns: (chains, 4, G, N) int64, (chains, 6, G, N) twice, (chains, 4) int64
RESULT_KEYS = ("diag_i_counts", "diag_ab_n_mu", "diag_ab_s_mu", "diag_info")
VARIABLES = {"i": "diag_i_counts", "ab_n_mu": "diag_ab_n_mu", "ab_s_mu": "diag_ab_s_mu"}
THRESHOLDS = (1.01, 1.05, 1.1)


def default_batch(draws: int) -> int:
    """The batch length ``sample`` uses: ``max(1, floor(sqrt(H)))`` with ``H = draws // 2``."""
    return max(1, math.isqrt(max(0, int(draws) // 2)))


def result_bytes(chains: int, G: int, N: int) -> int:
    """Host bytes of the ``diag_*`` arrays of a result: (4 + 6 + 6) planes of 8 bytes per cell and chain."""
    return int(chains) * (4 + 6 + 6) * 8 * int(G) * int(N)


def from_draws(x, L: int) -> Dict[str, np.ndarray]:
    """The moments of kept draws ``x`` of shape (chains, D, ...) with batches of ``L``, by the recurrences of the module's
    docstring in float64 -- for integer (or boolean) input the integer counts."""
    x = np.asarray(x)
    if x.ndim < 2:
        raise ValueError("x must have shape (chains, D, ...)")
    L = int(L)
    if L < 1:
        raise ValueError(f"the batch length must be >= 1, got {L}")
    chains, D = x.shape[:2]
    if D < 2:
        raise ValueError(f"at least 2 draws are needed, got {D}")
    H = D // 2
    B = H // L
    cell = x.shape[2:]
    info = np.tile(np.array([H, H, 2 * B, L], dtype=np.int64), (chains, 1))
    if x.dtype.kind in "biu":
        counts = np.zeros((chains, 4) + cell, dtype=np.int64)
        cur = np.zeros((chains,) + cell, dtype=np.int64)
        for d in range(2 * H):
            h, p = divmod(d, H)
            v = (x[:, d] != 0).astype(np.int64) if x.dtype.kind == "b" else x[:, d].astype(np.int64)
            counts[:, h] += v
            if p < B * L:
                cur = v.copy() if p % L == 0 else cur + v
                if p % L == L - 1:
                    counts[:, 2] += cur
                    counts[:, 3] += cur * cur
        return {"counts": counts, "info": info}
    x = x.astype(np.float64, copy=False)
    m = np.zeros((chains, 6) + cell)
    cur = np.zeros((chains,) + cell)
    inv_L = 1.0 / L
    for d in range(2 * H):
        h, p = divmod(d, H)
        v = x[:, d]
        inv_n = 1.0 / (p + 1)
        dl = v - m[:, 2 * h]
        m[:, 2 * h] += dl * inv_n
        m[:, 2 * h + 1] += dl * (v - m[:, 2 * h])
        if p < B * L:
            cur = v.copy() if p % L == 0 else cur + v
            if p % L == L - 1:
                inv_b = 1.0 / (h * B + p // L + 1)
                bm = cur * inv_L
                e = bm - m[:, 4]
                m[:, 4] += e * inv_b
                m[:, 5] += e * (bm - m[:, 4])
    return {"moments": m, "info": info}


def moments_of(res, var: str) -> Dict[str, np.ndarray]:
    """The moments of variable ``var`` (``i``, ``ab_n_mu``, ``ab_s_mu``) of a ``sample(..., diagnostics=True)`` result."""
    key = VARIABLES[var]
    if key not in res or "diag_info" not in res:
        raise ValueError(f"no diagnostics in this result (sample(..., diagnostics=True)): {key} is missing")
    return {"counts" if var == "i" else "moments": np.asarray(res[key]), "info": np.asarray(res["diag_info"])}


def _shape(mo):
    """(H, batches per chain, L, the six float moments) of complete moments: every chain has both halves of H draws."""
    info = np.asarray(mo["info"], dtype=np.int64)
    if info.ndim != 2 or info.shape[1] != 4 or info.shape[0] < 1:
        raise ValueError("info must have shape (chains, 4)")
    if (info != info[:1]).any() or info[0, 0] != info[0, 1]:
        raise ValueError("the chains' halves differ in length: the run has not reached its planned draws, or chains of "
                         "different runs were merged")
    H, nb, L = (int(v) for v in info[0, [0, 2, 3]])
    if H < 1:
        raise ValueError("no draws")
    if "counts" in mo:
        c = np.asarray(mo["counts"])
        c0, c1, scb, scb2 = (c[:, k].astype(np.float64) for k in range(4))
        with np.errstate(invalid="ignore", divide="ignore"):
            bm_mean = scb / (L * nb) if nb else np.zeros_like(scb)
            bm_m2 = (scb2 - scb * scb / nb) / (L * L) if nb else np.zeros_like(scb)
        m = np.stack([c0 / H, c0 * (H - c0) / H, c1 / H, c1 * (H - c1) / H, bm_mean, bm_m2], axis=1)
    else:
        m = np.asarray(mo["moments"], dtype=np.float64)
    if m.shape[0] != info.shape[0] or m.shape[1] != 6:
        raise ValueError("moments must have shape (chains, 6, ...)")
    return H, nb, L, m


def rhat(moments) -> np.ndarray:
    """Split R-hat (BDA3 section 11.4) over the ``m = 2 x chains`` half-sequences of length H: ``W`` the mean of their
    variances ``M2_h / (H - 1)``, ``B_over_H`` the variance (ddof 1) of their means, ``var_plus = (H-1)/H W + B_over_H``,
    ``rhat = sqrt(var_plus / W)``.  NaN where ``W = 0`` and ``B_over_H = 0`` (a constant cell), ``inf`` where
    ``W = 0 < B_over_H``.  No rank normalisation: that needs the draws."""
    H, _, _, m = _shape(moments)
    if H < 2:
        return np.full(m.shape[2:], np.nan)
    means = np.concatenate([m[:, 0], m[:, 2]], axis=0)
    W = np.concatenate([m[:, 1], m[:, 3]], axis=0).mean(axis=0) / (H - 1)
    b_over_h = means.var(axis=0, ddof=1)
    var_plus = (H - 1) / H * W + b_over_h
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.sqrt(var_plus / W)
    r = np.where((W == 0) & (b_over_h > 0), np.inf, r)
    return np.where((W == 0) & (b_over_h == 0), np.nan, r)


def _chain_s2(H, m):
    """Per chain the variance of its 2H draws: the halves' M2 merged (Chan et al.) over 2H - 1."""
    delta = m[:, 2] - m[:, 0]
    return (m[:, 1] + m[:, 3] + delta * delta * (H / 2.0)) / (2 * H - 1)


def ess(moments, with_mcse: bool = False):
    """Effective sample size by batch means (as mcmcse's ``ess`` with method "bm"): per chain ``sigma2_k = L bm_M2 / (2B - 1)``
    estimates the asymptotic variance from the chain's ``2B`` batch means and ``s2_k`` is the variance of its 2H draws;
    ``ess = chains 2H mean_k s2_k / mean_k sigma2_k``, ``mcse = sqrt(mean_k sigma2_k / (chains 2H))``; both NaN where
    ``2B < 2`` or ``mean_k sigma2_k = 0``.

    This is a WITHIN-chain estimate: it measures how fast each chain moves through what it visits, and chains stuck in
    different places each look fine to it.  The between-chain part is R-hat's: read the two together.

    ``with_mcse``: return ``(ess, mcse)``."""
    H, nb, L, m = _shape(moments)
    chains = m.shape[0]
    if nb < 2:
        e = np.full(m.shape[2:], np.nan)
        return (e, e.copy()) if with_mcse else e
    sigma2 = (L * m[:, 5] / (nb - 1)).mean(axis=0)
    s2 = _chain_s2(H, m).mean(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.where(sigma2 > 0, chains * 2 * H * s2 / sigma2, np.nan)
        se = np.where(sigma2 > 0, np.sqrt(sigma2 / (chains * 2 * H)), np.nan)
    return (e, se) if with_mcse else e


def posterior_sd(moments) -> np.ndarray:
    """The standard deviation (ddof 1) of all ``chains x 2H`` accumulated draws pooled."""
    H, _, _, m = _shape(moments)
    means = np.concatenate([m[:, 0], m[:, 2]], axis=0)
    m2 = np.concatenate([m[:, 1], m[:, 3]], axis=0).sum(axis=0) + H * ((means - means.mean(axis=0)) ** 2).sum(axis=0)
    n = means.shape[0] * H
    return np.sqrt(m2 / (n - 1)) if n > 1 else np.full(m.shape[2:], np.nan)


def _diag_of(res) -> Dict[str, np.ndarray]:
    missing = [k for k in RESULT_KEYS if k not in res]
    if missing:
        raise ValueError(f"no diagnostics in this result (sample(..., diagnostics=True)): {missing[0]} is missing")
    return {k: np.asarray(res[k]) for k in RESULT_KEYS}


def merge_chains(parts: Sequence[dict]) -> Dict[str, np.ndarray]:
    """Diagnostics of several runs over the SAME cohort, planned draws and batch length as one result: concatenated along the
    chain axis."""
    ds = [_diag_of(p) for p in parts]
    return {k: np.concatenate([d[k] for d in ds], axis=0) for k in RESULT_KEYS}


def merge_individual_shards(parts: Sequence[dict]) -> Dict[str, np.ndarray]:
    """Diagnostics of the same chains and draws over disjoint slices of the individuals (``distributed.IndividualShards``) as
    the whole cohort's: a cell belongs to one shard, so the (G, N) arrays are concatenated along the individuals."""
    ds = [_diag_of(p) for p in parts]
    for d in ds[1:]:
        if not np.array_equal(d["diag_info"], ds[0]["diag_info"]):
            raise ValueError("diag_info differs between the shards")
    out = {k: np.concatenate([d[k] for d in ds], axis=-1) for k in RESULT_KEYS[:3]}
    out["diag_info"] = ds[0]["diag_info"].copy()
    return out


def _figures(r, e, mask) -> Dict[str, object]:
    """Counts and extremes of R-hat ``r`` and ESS ``e`` over the cells of ``mask``."""
    const = np.isnan(r) & mask
    live = mask & ~np.isnan(r)
    out: Dict[str, object] = {"n_cells": int(mask.sum()), "n_constant": int(const.sum())}
    for t in THRESHOLDS:
        out[f"n_rhat_above_{t}"] = int((live & (r > t)).sum())
    out["max_rhat"] = float(r[live].max()) if live.any() else float("nan")
    out["share_rhat_above_1.01"] = (out["n_rhat_above_1.01"] / int(live.sum())) if live.any() else float("nan")
    ok = mask & np.isfinite(e)
    if ok.any():
        at = np.unravel_index(np.argmin(np.where(ok, e, np.inf)), e.shape)
        out["min_ess"], out["min_ess_cell"] = float(e[at]), tuple(int(v) for v in at)
    else:
        out["min_ess"], out["min_ess_cell"] = float("nan"), None
    flat = np.where(live, r, -np.inf).ravel()
    worst = np.argsort(-flat, kind="stable")[:10]
    worst = worst[flat[worst] > -np.inf]
    out["worst_cells"] = np.stack(np.unravel_index(worst, r.shape), axis=1).astype(np.int64) if r.ndim else np.zeros((0, 0), np.int64)
    out["worst_rhat"] = flat[worst]
    return out


def summary(res, last_gap=None) -> Dict[str, object]:
    """Per variable ``i`` / ``ab_n_mu`` / ``ab_s_mu`` of a ``sample(..., diagnostics=True)`` result a dict with ``rhat``, ``ess``,
    ``mcse`` and the posterior ``sd`` as (G, N) arrays and, over all cells, ``n_cells``, ``n_constant`` (cells that never
    changed: R-hat NaN), ``n_rhat_above_1.01`` / ``_1.05`` / ``_1.1``, ``share_rhat_above_1.01`` (of the non-constant cells),
    ``max_rhat``, ``min_ess`` with ``min_ess_cell`` = (g, j), and the ten worst cells by R-hat (``worst_cells`` (<= 10, 2),
    ``worst_rhat``).  With ``last_gap`` (N,) the same figures restricted to the followed cells (``g <= last_gap[j]``) under
    ``followed``.  ``scalars``: name -> {rhat, ess, mcse} of the 17 value variables and ``lp`` from their fully kept draws through
    ``from_draws`` with the result's batch length (those present in ``res``)."""
    d = _diag_of(res)
    G, N = d["diag_i_counts"].shape[-2:]
    followed = None
    if last_gap is not None:
        lg = np.asarray(last_gap)
        if lg.shape != (N,):
            raise ValueError(f"last_gap must have shape ({N},)")
        followed = np.arange(G)[:, None] <= lg[None, :]
    out: Dict[str, object] = {"info": d["diag_info"].copy()}
    everything = np.ones((G, N), dtype=bool)
    for var in VARIABLES:
        mo = moments_of(d, var)
        r = rhat(mo)
        e, se = ess(mo, with_mcse=True)
        v: Dict[str, object] = {"rhat": r, "ess": e, "mcse": se, "sd": posterior_sd(mo)}
        v.update(_figures(r, e, everything))
        if followed is not None:
            v["followed"] = _figures(r, e, followed)
        out[var] = v
    from .model import THETA_NAMES

    L = int(d["diag_info"][0, 3])
    scalars: Dict[str, Dict[str, float]] = {}
    for name, key in [(n, n) for n in THETA_NAMES] + [("lp", "stat_lp")]:
        if key not in res:
            continue
        x = np.asarray(res[key], dtype=np.float64)
        if x.ndim != 2 or x.shape[1] < 2:
            continue
        mo = from_draws(x, L)
        e, se = ess(mo, with_mcse=True)
        scalars[name] = {"rhat": float(rhat(mo)), "ess": float(e), "mcse": float(se)}
    out["scalars"] = scalars
    return out


def summary_arrays(sm: dict) -> Dict[str, np.ndarray]:
    """``summary`` flattened to named arrays for a posterior file: ``diag_summary_<var>_rhat`` / ``_ess`` / ``_mcse`` / ``_sd``
    (G, N), ``diag_summary_<var>_worst_cells`` / ``_worst_rhat``, and ``diag_summary_scalars`` (rows rhat, ess, mcse; columns
    in the order of ``diag_summary_scalar_names``)."""
    out: Dict[str, np.ndarray] = {}
    for var in VARIABLES:
        for k in ("rhat", "ess", "mcse", "sd", "worst_cells", "worst_rhat"):
            out[f"diag_summary_{var}_{k}"] = np.asarray(sm[var][k])
    names = list(sm["scalars"])
    out["diag_summary_scalar_names"] = np.array(names)
    out["diag_summary_scalars"] = np.array([[sm["scalars"][n][k] for n in names] for k in ("rhat", "ess", "mcse")]).reshape(3, len(names))
    return out


class _Diagnostics(Summary):
    """``diagnostics``: accumulate per cell, over ALL draws on the device, what split R-hat and a batch-means effective sample
    size of ``i``, ``ab_n_mu``, ``ab_s_mu`` need (``thin`` does not apply): ``diag_i_counts`` (chains, 4, G, N) int64,
    ``diag_ab_n_mu`` / ``diag_ab_s_mu`` (chains, 6, G, N) and ``diag_info`` (chains, 4); ``rhat`` / ``ess`` / ``summary`` read them.
    ``diag_batch`` is the batch length (default ``default_batch(draws)``).  Needs ``draws >= 2``; the arrays' host bytes count
    against ``budget_bytes``.  The trajectories do not change."""

    name = "diagnostics"
    options = {"diagnostics": False, "diag_batch": None}
    prefix = "diag_"
    native_only = "diagnostics need the native sampler (sample(native=True)): the moments of every draw are accumulated inside it"

    def plan(self, opts, draws, chains, G, N):
        p = super().plan(opts, draws, chains, G, N)
        if p is None:
            return None
        if draws < 2:
            raise ValueError(f"diagnostics need draws >= 2 (two half-chains), got {draws}")
        p["batch"] = default_batch(draws) if p["diag_batch"] is None else int(p["diag_batch"])
        if p["batch"] < 1:
            raise ValueError(f"diag_batch must be >= 1, got {p['batch']}")
        return p

    def host_bytes(self, plan):
        return result_bytes(plan["chains"], plan["G"], plan["N"])

    def over_budget(self, plan, own, before, budget):
        return (f"the diagnostics of {plan['chains']} chains x ({plan['G']}, {plan['N']}) take {own / 2 ** 30:.2f} GiB of host arrays "
                f"(16 planes of 8 bytes per cell and chain) and the recorded draws {before / 2 ** 30:.2f} GiB, over the budget of "
                f"{budget / 2 ** 30:.2f} GiB: record fewer draws (thin, no_deterministics / record_discrete=False) or raise "
                f"ABD_RECORD_BUDGET_GB")

    def enable(self, smp, plan):
        smp.enable_diagnostics(plan["draws"], plan["batch"])

    def collect(self, smp, plan, last_gap):
        per_chain = [smp.diagnostics(c) for c in range(plan["chains"])]
        return {"diag_" + key: np.stack([pc[key] for pc in per_chain]) for key in ("i_counts", "ab_n_mu", "ab_s_mu", "info")}

    def add_arguments(self, parser):
        parser.add_argument("--diagnostics", help="Accumulate per cell of i / ab_n_mu / ab_s_mu, over all draws on the device, what split "
                            "R-hat and a batch-means effective sample size need (--thin does not apply) and report the largest R-hat, the "
                            "share of cells above 1.01 and the smallest ESS per variable, and the worst of the 17 scalars (diag_* and "
                            "diag_summary_* in the output).", action="store_true")
        parser.add_argument("--diag_batch", help="With --diagnostics: draws per batch of the batch-means ESS (default: the square root of "
                            "half the draws).", type=int)

    def report(self, res, data):
        """``summary``'s arrays go into ``res`` (``diag_summary_*``); the line: per variable over the followed cells, then the worst
        scalar."""
        sm = summary(res, getattr(data, "last_gap", None))
        res.update(summary_arrays(sm))
        parts = []
        for var in ("i", "ab_n_mu", "ab_s_mu"):
            f = sm[var].get("followed", sm[var])
            parts.append(f"{var} max R-hat {f['max_rhat']:.3f}, {100 * f['share_rhat_above_1.01']:.1f} % of {f['n_cells'] - f['n_constant']} "
                         f"non-constant followed cells above 1.01, min ESS {f['min_ess']:.0f}")
        sc = {k: v["rhat"] for k, v in sm["scalars"].items() if np.isfinite(v["rhat"])}
        worst = max(sc, key=sc.get) if sc else None
        parts.append(f"worst scalar {worst} R-hat {sc[worst]:.3f}" if worst else "no scalar with a finite R-hat")
        return ["diagnostics: " + "; ".join(parts)]

    def group(self, key):
        return None if key == "diag_summary_scalar_names" else "constant_data"  # (strings; nothing here has a draw axis)


SUMMARY = _Diagnostics()
