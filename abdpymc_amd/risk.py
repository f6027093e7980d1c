"""
Infection risk by titer with posterior uncertainty: does the S or N titer of gap g - 1 predict infection in gap g?

For a binary draw the sufficient statistic of every Poisson / Cox-type model of that question with a piecewise-constant titer
effect is a small integer table: person-gaps at risk and infections, by gap and by titer bin.  The native sampler reduces every
draw to that table on the device (``sample(..., risk=spec)``, ``Context.risk``; csrc/abd_risk.hpp), so every draw is kept
whatever ``thin`` is.  ``from_deterministics`` is the same definition as literal NumPy, for recorded (G, N) arrays; ``summary``
turns the per-draw tables into a hazard-versus-titer curve and a calendar-time-adjusted rate ratio per bin with credible
intervals.  ``survival_arrays`` builds, from posterior means, the arrays the reference's plug-in survival models take.

Definition (one draw).  ``last_gap[j]`` is the follow-up the curves use (``curves.py``; -1: never followed).  With a window
``(start, end)``, ``0 <= start``, ``end <= G``, ``end - start >= 2``:

    cell (g, j) is at risk   iff start < g < end, g <= last_gap[j] and, when ``first_only``, i[g', j] == 0 for every
                             start < g' < g (at most one infection per individual inside the window)
    cell (g, j) is an event  iff it is at risk and i[g, j] == 1
    table (2, 2, G, 8)       antigen (S, N) x (at risk, events) x gap x bin; a cell is counted in the bin
                             #{e in edges: x >= e} of the titer of the PREVIOUS gap, x = ab_s_mu[g - 1, j] / ab_n_mu[g - 1, j]

Up to 7 finite, strictly ascending edges per antigen; bins above ``len(edges)`` stay empty; a NaN titer lands in bin 0.

NumPy only.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

from .summaries import Summary, interval

N_BINS = 8
MAX_EDGES = N_BINS - 1
ANTIGENS = ("s", "n")
KINDS = ("at_risk", "events")
# what sample(..., risk=spec) returns: the table (chains, draws, 2, 2, G, 8) and the spec, one row per chain: the edges padded
# with NaN to 7, and (start, end, first_only)
RESULT_KEYS = ("risk_table", "risk_edges_s", "risk_edges_n", "risk_window")
QUANTITIES = ("person_gaps", "events", "rate", "rate_ratio", "protection")


def _edges(e, name: str) -> np.ndarray:
    e = np.atleast_1d(np.asarray(e if e is not None else (), dtype=np.float64))
    if e.ndim != 1:
        raise ValueError(f"{name} must be one-dimensional")
    if e.size > MAX_EDGES:
        raise ValueError(f"{name}: {e.size} edges, at most {MAX_EDGES}")
    if not np.isfinite(e).all():
        raise ValueError(f"{name} must be finite")
    if e.size > 1 and not (np.diff(e) > 0).all():
        raise ValueError(f"{name} must be strictly ascending")
    return e


def spec(start: int = 0, end: Optional[int] = None, edges_s=(), edges_n=(), first_only=True, n_gaps: Optional[int] = None) -> Dict[str, object]:
    """A checked risk specification {"start", "end", "first_only", "edges_s", "edges_n"}: the rules of ``abd_risk`` (abd_hip.h).
    ``end=None`` is ``n_gaps``; with ``n_gaps`` given the window is checked against it, otherwise where the spec is used.
    ``ValueError`` for a bad window, more than 7 edges, edges that are non-finite or not strictly ascending, and a
    ``first_only`` that is not 0 / 1 / a bool."""
    if end is None:
        if n_gaps is None:
            raise ValueError("end=None needs n_gaps")
        end = n_gaps
    for name, v in (("start", start), ("end", end)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} must be an integer, got {v!r}")
    if isinstance(first_only, (bool, np.bool_)):
        first_only = int(first_only)
    if not isinstance(first_only, (int, np.integer)) or first_only not in (0, 1):
        raise ValueError(f"first_only must be 0 or 1, got {first_only!r}")
    start, end = int(start), int(end)
    if start < 0 or end - start < 2 or (n_gaps is not None and end > int(n_gaps)):
        raise ValueError(f"window ({start}, {end}) needs 0 <= start, end <= n_gaps"
                         f"{'' if n_gaps is None else ' = %d' % int(n_gaps)} and end - start >= 2")
    return {"start": start, "end": end, "first_only": int(first_only), "edges_s": _edges(edges_s, "edges_s"),
            "edges_n": _edges(edges_n, "edges_n")}


def _checked(sp, G: int) -> Dict[str, object]:
    return spec(sp["start"], sp["end"], sp["edges_s"], sp["edges_n"], sp["first_only"], n_gaps=G)


def bin_of(x, edges) -> np.ndarray:
    """#{e in edges: x >= e}; NaN fails every comparison: bin 0."""
    x = np.asarray(x, dtype=np.float64)
    b = np.zeros(x.shape, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for e in np.asarray(edges, dtype=np.float64):
            b += x >= e
    return b


def from_deterministics(i, ab_s_mu, ab_n_mu, last_gap, spec) -> np.ndarray:
    """The table of recorded Deterministics: ``i``, ``ab_s_mu``, ``ab_n_mu`` are (..., G, N), ``last_gap`` (N,) or ``None`` (G - 1
    for everyone); returns (..., 2, 2, G, 8) int64 as defined in the module's docstring."""
    from .curves import _last_gap

    i, ab_s_mu, ab_n_mu = np.asarray(i), np.asarray(ab_s_mu, dtype=np.float64), np.asarray(ab_n_mu, dtype=np.float64)
    if i.ndim < 2 or i.shape != ab_s_mu.shape or i.shape != ab_n_mu.shape:
        raise ValueError("i, ab_s_mu, ab_n_mu must share a shape (..., G, N)")
    G, N = i.shape[-2:]
    sp = _checked(spec, G)
    lg = _last_gap(last_gap, G, N)
    g = np.arange(G)
    in_window = (g > sp["start"]) & (g < sp["end"])
    at_risk = in_window[:, None] & (g[:, None] <= lg[None, :])  # (G, N)
    inf = i != 0
    if sp["first_only"]:
        inside = inf & (g > sp["start"])[:, None]
        before = np.cumsum(inside, axis=-2) - inside  # infections in (start, g)
        at_risk = at_risk & (before == 0)
    else:
        at_risk = np.broadcast_to(at_risk, inf.shape)
    events = at_risk & inf
    out = np.zeros(i.shape[:-2] + (2, 2, G, N_BINS), dtype=np.int64)
    for a, (mu, edges) in enumerate(((ab_s_mu, sp["edges_s"]), (ab_n_mu, sp["edges_n"]))):
        prev = np.empty_like(mu)
        prev[..., 1:, :] = mu[..., :-1, :]
        prev[..., 0, :] = np.nan  # (gap 0 has no predecessor and is never in a window)
        b = bin_of(prev, edges)
        for k in range(N_BINS):
            hit = b == k
            out[..., a, 0, :, k] = (at_risk & hit).sum(axis=-1)
            out[..., a, 1, :, k] = (events & hit).sum(axis=-1)
    return out


def as_result(table, spec, chains: Optional[int] = None) -> Dict[str, np.ndarray]:
    """The ``risk_*`` keys of a sampler result from ``table`` (chains, draws, 2, 2, G, 8) and the spec it was counted under."""
    table = np.asarray(table)
    if table.ndim != 6 or table.shape[2:4] != (2, 2) or table.shape[5] != N_BINS:
        raise ValueError(f"table must be (chains, draws, 2, 2, G, {N_BINS}), got {table.shape}")
    sp = _checked(spec, table.shape[4])
    c = table.shape[0] if chains is None else int(chains)

    def padded(e):
        p = np.full(MAX_EDGES, np.nan)
        p[: e.size] = e
        return np.tile(p, (c, 1))

    return {"risk_table": table.astype(np.int64, copy=False), "risk_edges_s": padded(sp["edges_s"]), "risk_edges_n": padded(sp["edges_n"]),
            "risk_window": np.tile(np.array([sp["start"], sp["end"], sp["first_only"]], dtype=np.int64), (c, 1))}


def _risk_of(res) -> Dict[str, np.ndarray]:
    missing = [k for k in RESULT_KEYS if k not in res]
    if missing:
        raise ValueError(f"no risk table in this result (sample(..., risk=spec)): {missing[0]} is missing")
    return {k: np.asarray(res[k]) for k in RESULT_KEYS}


def _same_spec(cs) -> None:
    for k in RESULT_KEYS[1:]:
        rows = np.concatenate([c[k] for c in cs], axis=0)
        if not np.array_equal(rows, np.broadcast_to(rows[:1], rows.shape), equal_nan=True):
            raise ValueError(f"{k} differs between the parts: pool tables counted under one spec only")


def merge_chains(parts: Sequence[dict]) -> Dict[str, np.ndarray]:
    """Tables of several runs over the SAME cohort, follow-up and spec as one result: concatenated along the chain axis."""
    cs = [_risk_of(p) for p in parts]
    _same_spec(cs)
    return {k: np.concatenate([c[k] for c in cs], axis=0) for k in RESULT_KEYS}


def merge_individual_shards(parts: Sequence[dict]) -> Dict[str, np.ndarray]:
    """Tables of the same chains and draws over disjoint slices of the individuals as the whole cohort's: every count is a sum
    over individuals, so the shards add elementwise and exactly."""
    cs = [_risk_of(p) for p in parts]
    _same_spec(cs)
    out = {k: cs[0][k].copy() for k in RESULT_KEYS}
    for c in cs[1:]:
        if c["risk_table"].shape != out["risk_table"].shape:
            raise ValueError(f"risk_table: shards differ in shape, {c['risk_table'].shape} against {out['risk_table'].shape}")
        out["risk_table"] = out["risk_table"] + c["risk_table"]
    return out


def rate_ratio(at_risk, events, reference_bin: int = 0) -> np.ndarray:
    """Mantel-Haenszel rate ratio of every bin against ``reference_bin``, stratified by gap: ``at_risk`` T and ``events`` e are
    (..., G, 8); returns (..., 8)

        RR_b = sum_g e[g, b] T[g, r] / (T[g, b] + T[g, r])  /  sum_g e[g, r] T[g, b] / (T[g, b] + T[g, r])

    over the gaps where T[g, b] + T[g, r] > 0; NaN where the lower sum is 0.  The gap plays the part of the baseline hazard
    of a calendar month: a bin is compared with the reference inside each gap only."""
    T, e = np.asarray(at_risk, dtype=np.float64), np.asarray(events, dtype=np.float64)
    if T.shape != e.shape or T.ndim < 2 or T.shape[-1] != N_BINS:
        raise ValueError(f"at_risk and events must share a shape (..., G, {N_BINS})")
    r = int(reference_bin)
    if not 0 <= r < N_BINS:
        raise ValueError(f"reference_bin={reference_bin} outside [0, {N_BINS})")
    Tr, er = T[..., r:r + 1], e[..., r:r + 1]
    tot = T + Tr
    with np.errstate(invalid="ignore", divide="ignore"):
        inv = np.where(tot > 0, 1.0 / np.where(tot > 0, tot, 1.0), 0.0)
        num = (e * Tr * inv).sum(axis=-2)
        den = (er * T * inv).sum(axis=-2)
        return np.where(den > 0, num / np.where(den > 0, den, 1.0), np.nan)


def per_draw(table, reference_bin: int = 0) -> Dict[str, np.ndarray]:
    """Per-draw quantities of ``table`` (..., 2, 2, G, 8): ``by_bin`` (..., 2, 2, 8) the table summed over the gaps, ``rate``
    (..., 2, 8) events / person-gaps (NaN for an empty bin), ``rate_ratio`` (..., 2, 8) (``rate_ratio``)."""
    t = np.asarray(table)
    by_bin = t.sum(axis=-2)
    pg, ev = by_bin[..., 0, :].astype(np.float64), by_bin[..., 1, :].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        rate = np.where(pg > 0, ev / np.where(pg > 0, pg, 1.0), np.nan)
    return {"by_bin": by_bin, "rate": rate, "rate_ratio": rate_ratio(t[..., 0, :, :], t[..., 1, :, :], reference_bin)}


def summary(res, prob: float = 0.95, reference_bin: int = 0) -> Dict[str, object]:
    """Medians and equal-tailed ``prob`` intervals over the pooled draws of all chains.  Per antigen (``"s"``, ``"n"``) and bin,
    each a dict of ``median`` / ``lower`` / ``upper`` / ``n_defined`` (8,) -- NaN draws are ignored and ``n_defined`` counts the
    others:

        person_gaps  person-gaps at risk, pooled over the gaps
        events       infections, pooled over the gaps
        rate         events / person_gaps, the crude hazard per gap (NaN in a draw whose bin is empty)
        rate_ratio   the Mantel-Haenszel rate ratio against ``reference_bin``, stratified by gap (``rate_ratio``)
        protection   1 - rate_ratio

    and ``n_draws`` (pooled), ``prob``, ``reference_bin``, ``edges_s``, ``edges_n``, ``window`` (start, end, first_only).
    ``res``: a ``sample(..., risk=spec)`` result or any dict with the ``risk_*`` keys (``as_result``, the merges)."""
    if not 0.0 < prob < 1.0:
        raise ValueError(f"prob must be in (0, 1), got {prob}")
    c = _risk_of(res)
    _same_spec([c])
    t = c["risk_table"]
    t = t.reshape((-1,) + t.shape[2:])  # (chains x draws, 2, 2, G, 8)
    pd = per_draw(t, reference_bin)
    out: Dict[str, object] = {}
    for a, name in enumerate(ANTIGENS):
        rr = pd["rate_ratio"][:, a]
        out[name] = {k: interval(x, prob, count_defined=True) for k, x in (
            ("person_gaps", pd["by_bin"][:, a, 0].astype(np.float64)), ("events", pd["by_bin"][:, a, 1].astype(np.float64)),
            ("rate", pd["rate"][:, a]), ("rate_ratio", rr), ("protection", 1.0 - rr))}
    out["n_draws"] = int(t.shape[0])
    out["prob"], out["reference_bin"] = float(prob), int(reference_bin)
    for k in ("edges_s", "edges_n"):
        e = c[f"risk_{k}"][0] if c[f"risk_{k}"].shape[0] else np.full(MAX_EDGES, np.nan)
        out[k] = e[np.isfinite(e)]
    out["window"] = tuple(int(v) for v in c["risk_window"][0]) if c["risk_window"].shape[0] else None
    return out


def summary_arrays(sm: dict) -> Dict[str, np.ndarray]:
    """``summary`` flattened to named arrays for a posterior file: ``risk_summary_<antigen>_<quantity>`` (4, 8) with rows lower,
    median, upper, n_defined."""
    out = {}
    for name in ANTIGENS:
        for q in QUANTITIES:
            v = sm[name][q]
            out[f"risk_summary_{name}_{q}"] = np.stack([v["lower"], v["median"], v["upper"], v["n_defined"].astype(np.float64)])
    return out


def survival_arrays(i_mean, ab_s_mu_mean, ab_n_mu_mean, last_gap, start: int, end: int) -> Dict[str, np.ndarray]:
    """The inputs of the reference's plug-in survival models from posterior means (``abd_sampler_means``; each (G, N)):
    ``infected``, ``exposure``, ``s_titer``, ``n_titer``, each (n_ind, end - start - 1), column t for gap start + 1 + t.

        infected   the mean infection probability of gaps start + 1 .. end - 1, NaN after the individual's last sample, and cut
                   off where its running sum along the window passes 1 (the entry that passes it keeps what was left to 1, the
                   later ones are 0): at most one infection per individual
        exposure   1 minus the sum of ``infected`` over the window's earlier gaps, with the NaNs of ``infected``
        s_titer, n_titer   the mean titers of gaps start .. end - 2: the titer of the gap before

    An individual with ``last_gap`` -1 is NaN throughout.  As in the reference, an individual whose running sum has passed 1
    before its last sample gets one 0 (with exposure 0) in the first gap after it and NaN from there on.  ``exposure`` is kept in [0, 1] (the sum can pass 1 by a rounding)."""
    from .curves import _last_gap

    i_mean = np.asarray(i_mean, dtype=np.float64)
    s_mu, n_mu = np.asarray(ab_s_mu_mean, dtype=np.float64), np.asarray(ab_n_mu_mean, dtype=np.float64)
    if i_mean.ndim != 2 or s_mu.shape != i_mean.shape or n_mu.shape != i_mean.shape:
        raise ValueError("i_mean, ab_s_mu_mean, ab_n_mu_mean must share a shape (G, N)")
    G, N = i_mean.shape
    sp = spec(start, end, n_gaps=G)
    start, end = sp["start"], sp["end"]
    lg = _last_gap(last_gap, G, N)
    raw = i_mean.T.copy()  # (N, G)
    raw[np.arange(G)[None, :] > lg[:, None]] = np.nan
    raw = raw[:, start + 1:end]
    if (raw < 0).any():
        raise ValueError("infection probabilities must not be negative")
    infected = np.empty_like(raw)
    run = np.zeros(N)
    with np.errstate(invalid="ignore"):
        for t in range(raw.shape[1]):
            v = raw[:, t]
            infected[:, t] = np.where(run > 1.0, 0.0, np.where(run + v > 1.0, 1.0 - run, v))
            run = run + v
    exposure = np.ones_like(infected)
    exposure[:, 1:] -= np.cumsum(infected, axis=1)[:, :-1]
    exposure = np.clip(exposure, 0.0, 1.0)
    exposure[np.isnan(infected)] = np.nan
    return {"infected": infected, "exposure": exposure, "s_titer": s_mu.T[:, start:end - 1].copy(), "n_titer": n_mu.T[:, start:end - 1].copy()}


class _Risk(Summary):
    """``risk`` = a ``spec``: keep the infection-risk-by-titer table of EVERY draw, reduced over the individuals on the device
    (``thin`` does not apply): ``risk_table`` (chains, draws, 2, 2, G, 8) int64 -- antigen (S, N) x (at risk, events) x gap x bin of
    the previous gap's titer -- and the spec, one row per chain: ``risk_edges_s`` / ``risk_edges_n`` (chains, 7), NaN beyond the
    edges given, and ``risk_window`` (chains, 3) = (start, end, first_only); ``summary`` reads them.  The follow-up is the curves'.
    The table's host bytes count against ``budget_bytes``.  The trajectories do not change."""

    name = "risk"
    options = {"risk": None}
    prefix = "risk_"
    draw_keys = ("risk_table", "risk_by_bin", "risk_rate_ratio")
    follow_up = True
    native_only = "risk needs the native sampler (sample(native=True)): every draw is reduced on the device inside it"

    def on(self, opts):
        return opts["risk"] is not None

    def plan(self, opts, draws, chains, G, N):
        p = super().plan(opts, draws, chains, G, N)
        if p is not None:
            p["spec"] = _checked(p["risk"], G)
        return p

    def host_bytes(self, plan):
        return plan["chains"] * plan["draws"] * 4 * plan["G"] * N_BINS * 8

    def over_budget(self, plan, own, before, budget):
        return (f"the risk tables of {plan['chains']} chains x {plan['draws']} draws x {plan['G']} gaps take {own / 2 ** 30:.2f} GiB of "
                f"host arrays (32 counts of 8 bytes per gap and draw) and the other recorded arrays {before / 2 ** 30:.2f} GiB, over "
                f"the budget of {budget / 2 ** 30:.2f} GiB: fewer draws, record less (thin, no_deterministics / record_discrete=False) "
                f"or raise ABD_RECORD_BUDGET_GB")

    def enable(self, smp, plan):
        smp.enable_risk(plan["draws"], plan["spec"])

    def collect(self, smp, plan, last_gap):
        return as_result(np.stack([smp.risk(c) for c in range(plan["chains"])]), plan["spec"])

    def add_arguments(self, parser):
        parser.add_argument("--risk", help="Keep the infection-risk-by-titer table of every draw (person-gaps at risk and infections by gap "
                            "and by bin of the previous gap's titer; reduced over the individuals on the device, --thin does not apply) "
                            "and report per antigen the protection (1 - the rate ratio stratified by gap) of the highest populated bin "
                            "against bin 0 with its 95 %% interval (risk_* in the output).  An individual counts up to its last serum "
                            "sample and, without --risk_all_infections, up to its first infection inside the window.", action="store_true")
        parser.add_argument("--risk_edges_s", help="With --risk: up to 7 ascending S titer bin edges, separated by commas.", default="")
        parser.add_argument("--risk_edges_n", help="With --risk: up to 7 ascending N titer bin edges, separated by commas.", default="")
        parser.add_argument("--risk_start", help="With --risk: the window's first gap; risk is counted from the gap after it.", type=int,
                            default=0)
        parser.add_argument("--risk_end", help="With --risk: the end of the window, one past its last gap (default: the number of gaps).",
                            type=int)
        parser.add_argument("--risk_all_infections", help="With --risk: count every infection of an individual inside the window, not "
                            "only the first.", action="store_true")

    def cli_options(self, args, data, chains, world):
        """The ``spec`` the --risk flags ask for (``None`` without --risk); ``SystemExit`` for what ``spec`` refuses."""
        if not args.risk:
            return {"risk": None}
        try:
            edges = [[float(x) for x in text.split(",") if x.strip()] for text in (args.risk_edges_s, args.risk_edges_n)]
            return {"risk": spec(args.risk_start, args.risk_end, edges[0], edges[1], not args.risk_all_infections, n_gaps=data.n_gaps)}
        except ValueError as e:
            raise SystemExit(f"--risk: {e}")

    def report(self, res, data):
        """The per-draw table is replaced in ``res`` by what a posterior file keeps of it: ``risk_by_bin`` (chains, draws, 2, 2, 8)
        the table summed over the gaps, ``risk_rate_ratio`` (chains, draws, 2, 8) the per-draw rate ratios against bin 0,
        ``risk_table_sum`` (chains, 2, 2, G, 8) the table summed over the draws, and ``risk_summary_*``.  The line: per antigen the
        highest populated bin against bin 0."""
        sm = summary(res)
        table = res.pop("risk_table")
        pd = per_draw(table)
        res["risk_by_bin"], res["risk_rate_ratio"] = pd["by_bin"], pd["rate_ratio"]
        res["risk_table_sum"] = table.sum(axis=1)
        res.update(summary_arrays(sm))
        pct = int(round(100 * sm["prob"]))
        parts = []
        for name in ANTIGENS:
            a = sm[name]
            used = np.flatnonzero(np.nan_to_num(a["person_gaps"]["median"]) > 0)
            top = int(used[-1]) if used.size else 0
            if top == 0:
                parts.append(f"{name.upper()} no populated bin above bin 0")
                continue
            p = a["protection"]
            parts.append(f"{name.upper()} protection of bin {top} against bin 0 {100 * p['median'][top]:.1f} % ({pct} % interval "
                         f"{100 * p['lower'][top]:.1f} to {100 * p['upper'][top]:.1f}; defined in {int(p['n_defined'][top])} of "
                         f"{sm['n_draws']} draws)")
        return ["risk: " + "; ".join(parts)]


SUMMARY = _Risk()
