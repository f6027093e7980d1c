"""
Per-individual timelines over ALL draws: the arrays the reference's per-individual figure (timelines.py: plot_individual) draws
from the posterior -- the spread of the two titers of a cell, its infection probability and the probability of at least one
infection so far inside the cell's time chunk -- for runs that never keep their draws.

The native sampler accumulates them per chain and cell on the device (``sample(..., timelines=True)``; csrc/abd_timeline.hpp;
include/abd_hip.h has the definition in full).  ``from_draws`` is the same definition as literal NumPy, for draws that were
kept; ``quantiles`` is the definition the device's read-out kernel shares.

Definition.  Titer histograms: per cell 64 counters for ``ab_n_mu`` over ``[lo_n, hi_n)`` and 64 for ``ab_s_mu`` over ``[lo_s,
hi_s)``.  With ``inv_w = 62 / (hi - lo)`` a draw's titer ``x`` goes to bin 0 if ``x < lo``, to bin 63 if ``x >= hi`` or ``x`` is
NaN, else to ``1 + min(61, floor((x - lo) * inv_w))``: 62 interior bins of width ``w = (hi - lo) / 62``.  Infection timing: per
cell ``inf``, the draws with ``i[g, j] = 1``, and ``cum``, the draws with ``i[g', j] = 1`` for some ``g' <= g`` in the same chunk
as ``g`` (chunk borders ``0, splits..., G``); per individual ``ninf[8]``, the draws by the number of infections at gaps ``<=
last_gap[j]`` (``[7]``: 7 or more; no ``last_gap``: every gap; ``last_gap[j] = -1``: the row stays 0).  The cell planes ignore
the follow-up.

Quantile ``q`` of a histogram ``c[0..63]`` with inclusive cumulative sums ``C`` and total ``n``: NaN if ``n = 0``; else ``t = q n``
and ``b`` the smallest bin with ``c[b] > 0`` and ``C[b] >= t``; ``lo`` if ``b = 0``, ``hi`` if ``b = 63``, else
``lo + w ((b - 1) + (t - C[b-1]) / c[b])``.

NumPy only.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

from .summaries import Summary

N_BINS = 64      # counters per histogram: underflow, 62 interior bins, overflow
N_NINF = 8       # bins of the number of infections
MAX_DRAWS = 65535  # per chain: 16-bit counters
MAX_Q = 8        # quantiles per device read-out
DEFAULT_RANGES = ((-4.0, 8.0), (-4.0, 8.0))  # (ab_n_mu, ab_s_mu): the reference's plot range
DEFAULT_Q = (0.025, 0.5, 0.975)

# what sample(..., timelines=True) returns: (chains, G, N) int64 twice, (chains, N, 8) int64, (chains, 1) int64 draws per chain,
# (chains, 2, 2) the ranges (ab_n_mu, ab_s_mu) x (lo, hi), (chains, Q) the quantile levels -- and, pooled over the chains on the
# device, (Q, G, N) twice
RESULT_KEYS = ("tl_inf", "tl_cum", "tl_ninf", "tl_info", "tl_range", "tl_q", "tl_q_n", "tl_q_s")
CHAIN_KEYS = RESULT_KEYS[:6]   # those with a leading chain axis
POOLED_KEYS = RESULT_KEYS[6:]  # those without
HIST_KEYS = ("tl_hist_n", "tl_hist_s")  # (chains, G, N, 64) uint16, with timelines_hist=True


def result_bytes(chains: int, G: int, N: int, n_q: int = len(DEFAULT_Q), hist: bool = False) -> int:
    """Host bytes of the ``tl_*`` arrays of a result: two int64 planes per cell and chain, 8 int64 per individual and chain, two
    planes of float64 per quantile, and with ``hist`` two histograms of 64 uint16 per cell and chain."""
    cells = int(G) * int(N)
    return int(chains) * (2 * 8 * cells + N_NINF * 8 * int(N)) + 2 * int(n_q) * 8 * cells + (int(chains) * 2 * N_BINS * 2 * cells if hist else 0)


def check_range(lo: float, hi: float):
    lo, hi = float(lo), float(hi)
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi and np.isfinite(hi - lo)):
        raise ValueError(f"the range [{lo}, {hi}) is not finite and ascending")
    return lo, hi


def bins(x, lo: float, hi: float) -> np.ndarray:
    """The bin of every titer in ``x`` (the module's rule) as int64."""
    lo, hi = check_range(lo, hi)
    x = np.asarray(x, dtype=np.float64)
    inv_w = (N_BINS - 2) / (hi - lo)
    with np.errstate(invalid="ignore", over="ignore"):
        k = np.floor((x - lo) * inv_w)
        inner = 1 + np.where(k < N_BINS - 3, k, N_BINS - 3)
        b = np.where(x < lo, 0, np.where(~(x < hi), N_BINS - 1, inner))
    return np.nan_to_num(b, nan=N_BINS - 1).astype(np.int64)


def _borders(G: int, splits) -> list:
    sp = [] if splits is None else [int(s) for s in splits]
    if any(s < 0 or s > G for s in sp) or sp != sorted(sp):
        raise ValueError(f"splits {tuple(sp)} are not ascending inside [0, {G}]")
    return [0, *sp, G]


def from_draws(i, ab_n_mu, ab_s_mu, ranges=DEFAULT_RANGES, splits=None, last_gap=None) -> Dict[str, np.ndarray]:
    """The counters of kept draws: ``i``, ``ab_n_mu``, ``ab_s_mu`` of shape (chains, D, G, N) (either titer may be ``None``: no
    histogram of it), ``ranges`` = ((lo_n, hi_n), (lo_s, hi_s)) -> ``tl_inf``, ``tl_cum`` (chains, G, N) int64, ``tl_ninf`` (chains,
    N, 8) int64, ``tl_info`` (chains, 1) int64, ``tl_range`` (chains, 2, 2) and ``tl_hist_n`` / ``tl_hist_s`` (chains, G, N, 64)
    uint16."""
    i = np.asarray(i)
    if i.ndim != 4:
        raise ValueError("i must have shape (chains, D, G, N)")
    chains, D, G, N = i.shape
    if D > MAX_DRAWS:
        raise ValueError(f"{D} draws per chain do not fit 16-bit counters (at most {MAX_DRAWS})")
    ones = i != 0
    out: Dict[str, np.ndarray] = {"tl_inf": ones.sum(axis=1, dtype=np.int64)}
    cum = np.zeros((chains, G, N), dtype=np.int64)
    b = _borders(G, splits)
    for lo, hi in zip(b[:-1], b[1:]):
        if hi > lo:
            cum[:, lo:hi] = (np.cumsum(ones[:, :, lo:hi], axis=2) > 0).sum(axis=1, dtype=np.int64)
    out["tl_cum"] = cum
    last = np.full(N, G - 1, dtype=np.int64) if last_gap is None else np.asarray(last_gap, dtype=np.int64)
    if last.shape != (N,):
        raise ValueError(f"last_gap must have shape ({N},)")
    followed = np.arange(G)[:, None] <= last[None, :]  # (G, N)
    k = np.minimum((ones & followed).sum(axis=2), N_NINF - 1)  # (chains, D, N)
    ninf = (k[..., None] == np.arange(N_NINF)).sum(axis=1, dtype=np.int64)  # (chains, N, 8)
    ninf[:, last < 0] = 0
    out["tl_ninf"] = ninf
    out["tl_info"] = np.full((chains, 1), D, dtype=np.int64)
    out["tl_range"] = np.tile(np.array([check_range(*r) for r in ranges]), (chains, 1, 1))
    for key, x, (lo, hi) in (("tl_hist_n", ab_n_mu, ranges[0]), ("tl_hist_s", ab_s_mu, ranges[1])):
        if x is None:
            continue
        x = np.asarray(x)
        if x.shape != i.shape:
            raise ValueError(f"{key[3:]}: shape {x.shape} is not that of i, {i.shape}")
        bx = bins(x, lo, hi)
        out[key] = (bx[..., None] == np.arange(N_BINS)).sum(axis=1).astype(np.uint16)
    return out


def merge(parts) -> Dict[str, np.ndarray]:
    """The counters of one result, or of several over the SAME cohort, ranges and follow-up (other processes' chains), summed over
    all their chains -- exact, they are integers: ``inf``, ``cum`` (G, N), ``ninf`` (N, 8), ``draws`` (int), ``range`` (2, 2) and,
    where every part has them, ``hist_n`` / ``hist_s`` (G, N, 64), all int64."""
    if isinstance(parts, dict):
        parts = [parts]
    parts = list(parts)
    for p in parts:
        missing = [k for k in ("tl_inf", "tl_cum", "tl_ninf", "tl_info") if k not in p]
        if missing:
            raise ValueError(f"no timelines in this result (sample(..., timelines=True)): {missing[0]} is missing")
    out: Dict[str, np.ndarray] = {}
    for key in ("inf", "cum", "ninf"):
        out[key] = sum(np.asarray(p["tl_" + key], dtype=np.int64).sum(axis=0) for p in parts)
    out["draws"] = int(sum(np.asarray(p["tl_info"], dtype=np.int64).sum() for p in parts))
    if all("tl_range" in p for p in parts):
        rs = [np.asarray(p["tl_range"], dtype=np.float64).reshape(-1, 2, 2) for p in parts]
        if any((r != rs[0][0]).any() for r in rs):
            raise ValueError("tl_range differs between the chains")
        out["range"] = rs[0][0].copy()
    for key in ("hist_n", "hist_s"):
        if all("tl_" + key in p for p in parts):
            out[key] = sum(np.asarray(p["tl_" + key]).sum(axis=0, dtype=np.int64) for p in parts)
    return out


def quantiles(hist, q, lo: float, hi: float) -> np.ndarray:
    """Quantiles ``q`` (numbers in [0, 1]) of histograms ``hist`` (..., 64) of integer counts over ``[lo, hi)`` -> (len(q), ...)
    float64, by the module's definition."""
    lo, hi = check_range(lo, hi)
    c = np.asarray(hist)
    if c.shape[-1] != N_BINS or c.dtype.kind not in "iu":
        raise ValueError(f"hist must hold integer counts with a last axis of {N_BINS}")
    c = c.astype(np.int64)
    qa = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if qa.ndim != 1 or not ((qa >= 0) & (qa <= 1)).all():
        raise ValueError("q must be numbers in [0, 1]")
    w = (hi - lo) / (N_BINS - 2)
    C = np.cumsum(c, axis=-1)
    n = C[..., -1]
    out = np.empty((qa.size,) + c.shape[:-1])
    for k, qk in enumerate(qa):
        t = qk * n.astype(np.float64)
        ok = (c > 0) & (C.astype(np.float64) >= t[..., None])
        b = np.argmax(ok, axis=-1)  # the first such bin (0 where there is none: n = 0)
        cb = np.take_along_axis(c, b[..., None], axis=-1)[..., 0]
        before = np.take_along_axis(C, b[..., None], axis=-1)[..., 0] - cb
        with np.errstate(invalid="ignore", divide="ignore"):
            inner = lo + w * ((b - 1).astype(np.float64) + (t - before.astype(np.float64)) / cb.astype(np.float64))
        v = np.where(b == 0, lo, np.where(b == N_BINS - 1, hi, inner))
        out[k] = np.where(n == 0, np.nan, v)
    return out


def compute_chunked_cum_p(p, splits=None) -> np.ndarray:
    """Cumulative probabilities from a 1-D array of probabilities, per chunk of time: ``splits`` are the borders between the
    chunks of ``p``, the sum starts again at each of them, and a sum above 1 counts as 1.  The approximation the reference makes
    of P(infected at least once by gap g) from the marginal means; ``summary``'s ``cum_p`` is the exact value."""
    p = np.asarray(p)
    if p.ndim != 1:
        raise ValueError("p is not 1D")
    edges = [0, *([] if splits is None else splits), p.size]
    out = np.empty(p.size, dtype=np.result_type(p.dtype, np.float64))
    for a, b in zip(edges[:-1], edges[1:]):
        out[a:b] = np.minimum(np.cumsum(p[a:b]), 1.0)
    return out


def band_levels(q) -> tuple:
    """The three levels ``summary`` reads as lower, median and upper out of the levels ``q`` of a result: the smallest, the one
    nearest 0.5 and the largest (``DEFAULT_Q`` is its own band)."""
    qa = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if qa.ndim != 1 or qa.size < 1:
        raise ValueError("q must hold at least one level")
    order = np.argsort(qa, kind="stable")
    mid = order[int(np.argmin(np.abs(qa[order] - 0.5)))]
    return int(order[0]), int(mid), int(order[-1])


def _bands(res, m, q):
    """levels (3,) and, per titer, (3, G, N) lower / median / upper: from the histograms where the result has them (levels ``q``,
    default DEFAULT_Q), else from the device's quantiles, whose levels are the result's ``tl_q``"""
    if "hist_n" in m and "hist_s" in m and "range" in m:
        q = DEFAULT_Q if q is None else tuple(np.asarray(q, dtype=np.float64)[list(band_levels(q))])
        return q, {"ab_n_mu": quantiles(m["hist_n"], q, *m["range"][0]), "ab_s_mu": quantiles(m["hist_s"], q, *m["range"][1])}
    if "tl_q_n" not in res or "tl_q_s" not in res or "tl_q" not in res:
        raise ValueError("no titer quantiles in this result: neither tl_hist_n / tl_hist_s nor tl_q_n / tl_q_s with tl_q")
    if q is not None:
        raise ValueError("this result holds no histograms: its bands have the levels it was sampled with (tl_q)")
    have = np.asarray(res["tl_q"], dtype=np.float64)
    have = have.reshape(-1, have.shape[-1])[0]
    at = list(band_levels(have))
    return tuple(float(x) for x in have[at]), {"ab_n_mu": np.asarray(res["tl_q_n"])[at], "ab_s_mu": np.asarray(res["tl_q_s"])[at]}


def summary(res, last_gap=None, q=None) -> Dict[str, object]:
    """Of a ``sample(..., timelines=True)`` result (or a ``from_draws`` one), pooled over its chains: ``draws``; per cell ``p_inf`` =
    P(i = 1) and the exact ``cum_p`` = P(infected at least once so far in the chunk) (G, N); per titer ``ab_n_mu`` / ``ab_s_mu`` a
    dict with ``lower``, ``median``, ``upper`` and ``touches_edge`` (the band reaches the under- or overflow bin), each (G, N); per
    individual ``n_infections`` (N, 8), the distribution of the number of infections within follow-up, and ``p_ever`` (N,) = P(at
    least one).  ``q``: the three levels of the band, (lower, median, upper).  A result with histograms (``timelines_hist=True``,
    ``from_draws``) gives any levels, by default ``DEFAULT_Q``, the median and a 95 % band; one without gives those of the
    quantiles it was sampled with: of its ``tl_q`` the smallest level, the one nearest 0.5 and the largest (``band_levels``; the
    default ``timeline_q`` is ``DEFAULT_Q``).  With ``last_gap``: ``followed`` (G, N), the cells at or before it."""
    m = merge(res)
    D = m["draws"]
    G, N = m["inf"].shape
    levels, bands = _bands(res, m, q)
    with np.errstate(invalid="ignore", divide="ignore"):
        out: Dict[str, object] = {"draws": D, "q": levels, "p_inf": m["inf"] / D, "cum_p": m["cum"] / D}
        tot = m["ninf"].sum(axis=1, keepdims=True)
        out["n_infections"] = np.where(tot > 0, m["ninf"] / np.maximum(tot, 1), np.nan)
    out["p_ever"] = 1.0 - out["n_infections"][:, 0]
    rng = m.get("range", np.asarray(res["tl_range"]).reshape(-1, 2, 2)[0] if "tl_range" in res else None)
    for k, (var, band) in enumerate(bands.items()):
        d = {"lower": band[0], "median": band[1], "upper": band[2]}
        if rng is not None:
            d["touches_edge"] = (band[0] <= rng[k][0]) | (band[2] >= rng[k][1])
            d["range"] = (float(rng[k][0]), float(rng[k][1]))
        out[var] = d
    if last_gap is not None:
        out["followed"] = np.arange(G)[:, None] <= np.asarray(last_gap, dtype=np.int64)[None, :]
    return out


def summary_arrays(sm) -> Dict[str, np.ndarray]:
    """``summary`` flattened to named arrays for a posterior file: ``tl_summary_p_inf``, ``tl_summary_cum_p`` (G, N),
    ``tl_summary_ab_n_mu`` / ``tl_summary_ab_s_mu`` (3, G, N) = lower, median, upper, ``tl_summary_n_infections`` (N, 8)."""
    out = {"tl_summary_p_inf": np.asarray(sm["p_inf"]), "tl_summary_cum_p": np.asarray(sm["cum_p"]),
           "tl_summary_n_infections": np.asarray(sm["n_infections"])}
    for var in ("ab_n_mu", "ab_s_mu"):
        out[f"tl_summary_{var}"] = np.stack([sm[var][k] for k in ("lower", "median", "upper")])
    return out


def individual(res, j: int, last_gap=None) -> Dict[str, np.ndarray]:
    """The arrays of individual ``j`` cut at their follow-up (gaps ``0 .. last_gap[j]``; every gap without ``last_gap``): ``gaps``,
    ``p_inf``, ``cum_p`` (n,), ``ab_n_mu`` / ``ab_s_mu`` (3, n) = lower, median, upper, ``n_infections`` (8,) -- everything the
    reference's plot_individual draws from the posterior.  ``res``: a result, or a ``summary`` of one."""
    sm = res if "p_inf" in res else summary(res, last_gap)
    G, N = sm["p_inf"].shape
    j = int(j)
    if not 0 <= j < N:
        raise ValueError(f"individual {j} outside [0, {N})")
    n = G if last_gap is None else int(np.asarray(last_gap)[j]) + 1
    n = max(0, min(G, n))
    out = {"gaps": np.arange(n), "p_inf": sm["p_inf"][:n, j].copy(), "cum_p": sm["cum_p"][:n, j].copy(),
           "n_infections": sm["n_infections"][j].copy()}
    for var in ("ab_n_mu", "ab_s_mu"):
        out[var] = np.stack([sm[var][k][:n, j] for k in ("lower", "median", "upper")])
    return out


def line(sm) -> str:
    """The CLI's one line about the timelines."""
    f = sm.get("followed")
    n_ever = int(np.nansum(sm["p_ever"] > 0.5))
    pct = f"{100 * (sm['q'][2] - sm['q'][0]):.3g}"
    parts = [f"{n_ever} of {sm['p_ever'].size} individuals with P(ever infected within follow-up) > 0.5"]
    touched = total = 0
    for name, var in (("S", "ab_s_mu"), ("N", "ab_n_mu")):
        width = sm[var]["upper"] - sm[var]["lower"]
        sel = np.isfinite(width) if f is None else (np.isfinite(width) & f)
        parts.append(f"median width of the {pct} % {name} band {np.median(width[sel]) if sel.any() else float('nan'):.3f}")
        if "touches_edge" in sm[var]:
            touched += int(sm[var]["touches_edge"][sel].sum())
            total += int(sel.sum())
    parts.append(f"{100 * touched / max(total, 1):.2f} % of cell bands touch an under- or overflow bin")
    return "timelines: " + "; ".join(parts) + f"; {sm['draws']} draws"


def add_summary(res: dict, last_gap=None) -> dict:
    """``summary`` of a gathered ``timelines=True`` result: its arrays go into ``res`` (``tl_summary_*``), the summary is returned.
    A result gathered from several ranks carries the histograms and no pooled quantiles (``timeline_q=None``): they are pooled
    here (``merge`` / ``quantiles`` at ``DEFAULT_Q``) and the histograms are dropped from ``res``."""
    sm = summary(res, last_gap)
    if "tl_q_n" not in res:
        m = merge(res)
        q = np.array(DEFAULT_Q)
        res["tl_q"] = np.tile(q, (np.asarray(res["tl_inf"]).shape[0], 1))
        res["tl_q_n"] = quantiles(m["hist_n"], q, *m["range"][0])
        res["tl_q_s"] = quantiles(m["hist_s"], q, *m["range"][1])
        for k in HIST_KEYS:
            res.pop(k)
    res.update(summary_arrays(sm))
    return sm


class _Timelines(Summary):
    """``timelines``: accumulate per cell, over ALL draws on the device, what a per-individual timeline needs (``thin`` does not
    apply): histograms of the two titers over ``timeline_ranges`` = ((lo_n, hi_n), (lo_s, hi_s)) (default: the reference's plot
    range) and the infection timing counters.  Per chain ``tl_inf`` / ``tl_cum`` (chains, G, N) int64 -- draws with an infection in
    the cell; with one so far in the cell's time chunk --, ``tl_ninf`` (chains, N, 8) int64 -- draws by the number of infections
    within follow-up (the curves') --, ``tl_info`` (chains, 1) the draws, ``tl_range`` (chains, 2, 2) and ``tl_q`` (chains, Q); pooled
    over the chains by a device kernel ``tl_q_n`` / ``tl_q_s`` (Q, G, N), the quantiles ``timeline_q`` (1 to 8 levels; ``summary``
    reads the smallest, the one nearest 0.5 and the largest as lower, median and upper; ``None``: no pooled quantiles, none of the
    three keys -- for a caller that pools the histograms of several processes itself) of ``ab_n_mu`` / ``ab_s_mu``; with
    ``timelines_hist`` also the histograms ``tl_hist_n`` / ``tl_hist_s`` (chains, G, N, 64) uint16.  ``summary`` / ``individual``
    read them.  At most 65535 draws per chain; the arrays' host bytes count against ``budget_bytes``.  The trajectories do not
    change."""

    name = "timelines"
    options = {"timelines": False, "timeline_ranges": ((-4, 8), (-4, 8)), "timeline_q": DEFAULT_Q, "timelines_hist": False}
    prefix = "tl_"
    follow_up = True
    native_only = "timelines need the native sampler (sample(native=True)): the counters of every draw are accumulated inside it"

    def plan(self, opts, draws, chains, G, N):
        p = super().plan(opts, draws, chains, G, N)
        if p is None:
            return None
        ranges = tuple(check_range(*r) for r in p["timeline_ranges"])
        if len(ranges) != 2:
            raise ValueError("timeline_ranges must be ((lo_n, hi_n), (lo_s, hi_s))")
        q = p["timeline_q"]  # (None: the device's pooled quantiles are not read out)
        if q is not None:
            q = np.atleast_1d(np.asarray(q, dtype=np.float64))
            if q.ndim != 1 or not 1 <= q.size <= MAX_Q or not ((q >= 0) & (q <= 1)).all():
                raise ValueError(f"timeline_q must be 1 to {MAX_Q} numbers in [0, 1]")
        if not 1 <= draws <= MAX_DRAWS:
            raise ValueError(f"timelines count in 16 bits: 1 to {MAX_DRAWS} draws per chain, got {draws}")
        p.update(ranges=ranges, q=q, hist=bool(p["timelines_hist"]))
        return p

    def host_bytes(self, plan):
        return result_bytes(plan["chains"], plan["G"], plan["N"], 0 if plan["q"] is None else plan["q"].size, plan["hist"])

    def over_budget(self, plan, own, before, budget):
        return (f"the timelines of {plan['chains']} chains x ({plan['G']}, {plan['N']}) take {own / 2 ** 30:.2f} GiB ({own} bytes) of "
                f"host arrays{' (the histograms: 256 bytes per cell and chain)' if plan['hist'] else ''} and the other recorded arrays "
                f"{before / 2 ** 30:.2f} GiB, over the budget of {budget / 2 ** 30:.2f} GiB: record less (thin, "
                f"no_deterministics / record_discrete=False) or raise ABD_RECORD_BUDGET_GB")

    def enable(self, smp, plan):
        smp.enable_timelines(plan["draws"], *plan["ranges"])

    def collect(self, smp, plan, last_gap):
        chains, q = plan["chains"], plan["q"]
        per_chain = [smp.timelines(c, hist=plan["hist"]) for c in range(chains)]
        res = {"tl_" + key: np.stack([pc[key] for pc in per_chain])
               for key in ("inf", "cum", "ninf") + (("hist_n", "hist_s") if plan["hist"] else ())}
        res["tl_info"] = np.array([[pc["n_draws"]] for pc in per_chain], dtype=np.int64)
        res["tl_range"] = np.tile(np.array(plan["ranges"], dtype=np.float64), (chains, 1, 1))
        if q is not None:
            res["tl_q"] = np.tile(q, (chains, 1))
            res["tl_q_n"], res["tl_q_s"] = smp.timeline_quantiles(q)
        return res

    def add_arguments(self, parser):
        parser.add_argument("--timelines", help="Accumulate per cell, over all draws on the device, what a per-individual timeline needs "
                            "(--thin does not apply): histograms of the S and N titers, from which the median and a 95 %% band are read, "
                            "the infection probability and the exact probability of at least one infection so far in the cell's time "
                            "chunk, and per individual the distribution of the number of infections (tl_* and tl_summary_* in the "
                            "output).  Reports the individuals more likely infected than not, the median width of the bands and the share "
                            "of bands that touch the ends of the range.", action="store_true")
        parser.add_argument("--timeline_range_s", help="With --timelines: the S titer range of the histograms, --timeline_range_s=lo,hi.", default="-4,8")
        parser.add_argument("--timeline_range_n", help="With --timelines: the N titer range of the histograms, --timeline_range_n=lo,hi.", default="-4,8")

    def cli_options(self, args, data, chains, world):
        """Over several processes every rank hands its chains' histograms to rank 0, which pools them (``add_summary``): no pooled
        quantiles from the device then, and the run is refused (by every rank alike, before anything runs) when what rank 0 holds
        after the gather -- the histograms and counters of all chains beside their recorded draws -- would not fit its host
        budget."""
        opts = {"timelines": args.timelines, "timeline_q": None if world > 1 else DEFAULT_Q, "timelines_hist": args.timelines and world > 1}
        if not args.timelines:
            return opts
        ranges = []
        for flag, text in (("--timeline_range_n", args.timeline_range_n), ("--timeline_range_s", args.timeline_range_s)):
            try:
                lo, hi = (float(x) for x in text.split(","))
                ranges.append(check_range(lo, hi))
            except ValueError as e:
                raise SystemExit(f"{flag}: need lo,hi with lo < hi, got {text!r} ({e})")
        opts["timeline_ranges"] = tuple(ranges)
        if world > 1:
            from .sampler import record_budget_bytes, record_bytes

            K = (len(data.s) + len(data.n)) if (args.log_likelihood or args.posterior_predictive) else 0
            own = result_bytes(chains, data.n_gaps, data.n_inds, n_q=0, hist=True)
            rest = record_bytes(chains, -(-args.draws // args.thin), data.n_gaps, data.n_inds, not args.no_deterministics, not args.no_discrete,
                                n_readings=K if args.log_likelihood else 0, n_replicates=K if args.posterior_predictive else 0)
            if own + rest > record_budget_bytes():
                raise SystemExit(f"--timelines over {world} processes gathers the histograms of {chains} chains on one rank: {own} bytes "
                                 f"beside {rest} bytes of recorded draws, over the host budget of {record_budget_bytes()} bytes "
                                 f"(ABD_RECORD_BUDGET_GB raises it; --thin, --no_deterministics, --no_discrete record less; one process "
                                 f"needs no histograms on the host)")
        return opts

    def report(self, res, data):
        return [line(add_summary(res, getattr(data, "last_gap", None)))]


SUMMARY = _Timelines()
