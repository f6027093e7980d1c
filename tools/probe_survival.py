"""
What the survival evaluator costs: microseconds per ``logp_dlogp`` call for 1 and 4 points per launch, the wall time
of a 1000 + 1000 x 4-chain fit of the combined model, and the NumPy restatement's time per evaluation on this host beside them,
at N x T = 1 520 x 30 and 10 000 x 199.  Data are simulated from the model (seeded).  ``--groups Gr [Gr]`` times the model by
group instead, with Gr groups at every size or one Gr per size, beside the ungrouped K = 1 model on the same data in
the same run: microseconds per call for 1 and 4 points, the tile counts, and the ratio.

``--leg waic`` times what scoring a fit costs: ``waic_accumulate`` of ``--points`` jittered points of the combined model
(launches of 16, a host clock around calls that end in a synchronise) beside ``logp_dlogp`` at one point per call on the same
handle, alternating, ``--reps`` times; per repeat and at its best, microseconds per draw, per single-point evaluation, the ratio.

``--leg ppc`` times the posterior predictive check in the same way: ``predictive_accumulate`` of ``--points`` jittered points of
the combined model, binned by both titers in octiles, beside ``waic_accumulate`` of the same points on the same handle,
alternating, ``--reps`` times; per repeat and at its best, microseconds per draw of each and the ratio.

``--leg loo`` times PSIS-LOO by individual: reserve + ``loo_accumulate`` + ``loo_stats`` + release of ``--points``
jittered points of the combined model beside ``waic_accumulate`` + ``waic_stats`` of the same points on the same handle,
alternating, ``--reps`` times, and ``compare.psis_loo_from_matrix`` on this host over ``--host_columns`` individuals of the same
matrix, scaled to the cohort.

``--leg draws_ic`` times the model comparison of per-draw fits for the combined model: (a) the ensemble WAIC fold and the
ensemble PSIS-LOO of ``--datasets`` x ``--draws_per_dataset`` draws on one ``SurvivalDrawsModel`` against (b) what there was before it,
a loop over the datasets of creating ``SurvivalModel(*d.arrays(m))`` and calling ``survival.waic`` / ``survival.loo`` on it, creation
included; both in this process, alternating, ``--reps`` times; and the plug-in fold of one dataset's draws on a resident handle, for
the per-row kernel time.

``--periods P [P]`` times the model by period in the same way, with P periods of equal length (0: monthly, P = T),
every P at both sizes, beside the ungrouped K = 1 model on the same data in the same run; ``--fit`` adds the wall time of a
``--tune`` + ``--draws`` x 4-chain fit of each of them and of the K = 1 model.

    python tools/probe_survival.py [--out FILE] [--tune 1000] [--draws 1000] [--no_fit]
    python tools/probe_survival.py --groups 4 8 [--out FILE]
    python tools/probe_survival.py --periods 3 0 [--fit] [--out FILE]
    python tools/probe_survival.py --leg waic [--points 4000] [--reps 3] [--out FILE]
    python tools/probe_survival.py --leg ppc [--points 4000] [--reps 3] [--out FILE]
    python tools/probe_survival.py --leg loo [--points 4000] [--reps 5] [--host_columns 500] [--out FILE]
    python tools/probe_survival.py --leg draws_ic [--datasets 64] [--draws_per_dataset 1000] [--reps 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from abdpymc_amd import survival  # noqa: E402
from tests import survival_restatement as R  # noqa: E402

SIZES = ((1520, 30), (10000, 199))


def simulate(N, T, seed=0):
    """(y, e, [x_s, x_n]) from the combined model at a = (1.5, 1), b = (1.5, 0.5), lam0 in [0.02, 0.08]; one infection at most,
    exposure 1 until it, no follow-up (NaN) after a random last interval."""
    rng = np.random.default_rng([seed, N, T])
    xs = [rng.uniform(0.0, 4.0, size=(N, T)) for _ in range(2)]
    lam0 = rng.uniform(0.02, 0.08, size=T)
    eta = 1.5 * (xs[0] - 1.5) + 0.5 * (xs[1] - 1.0)
    event = rng.random((N, T)) < lam0[None, :] / (1.0 + np.exp(-eta))
    y = (event & (np.cumsum(event, axis=1) == 1)).astype(np.float64)
    e = np.ones_like(y)
    e[:, 1:] -= np.cumsum(y, axis=1)[:, :-1]
    gone = np.arange(T)[None, :] >= rng.integers(max(1, T // 2), T + 1, size=N)[:, None]
    y[gone], e[gone] = np.nan, np.nan
    return y, e, xs


def per_call(fn, q, seconds=1.0):
    fn(q)
    n, t0 = 0, time.perf_counter()
    while True:
        for _ in range(20):
            fn(q)
        n += 20
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return 1e6 * dt / n


def probe_groups(N, T, Gr):
    """One row: the grouped model (labels ``j % Gr``: groups of equal size, interleaved) and the ungrouped K = 1 model on the S titer
    of ``simulate(N, T)``, timed one after the other, twice, the smaller figure kept."""
    y, e, xs = simulate(N, T)
    groups = np.arange(N) % Gr
    alone = survival.SurvivalModel(y, e, xs[:1], ("S",))
    grouped = survival.SurvivalGroupsModel(y, e, xs[0], "S", groups)
    rng = np.random.default_rng(1)
    qg = np.tile(grouped.initial_point(), (4, 1)) + rng.uniform(-0.5, 0.5, size=(4, grouped.dim))
    q1 = np.zeros((4, alone.dim))
    q1[:, 2], q1[:, 3] = -3.0, np.log(0.5)
    q1 += rng.uniform(-0.5, 0.5, size=q1.shape)
    sizes = np.bincount(groups, minlength=Gr)
    row = {"N": N, "T": T, "Gr": Gr, "dim": grouped.dim, "tiles_ungrouped": (N + 63) // 64, "tiles_grouped": int(((sizes + 63) // 64).sum())}
    row["tile_ratio"] = row["tiles_grouped"] / row["tiles_ungrouped"]
    for _ in range(2):
        for name, fn, q in (("ungrouped_us_per_call_n1", alone.logp_dlogp, q1[0]), ("grouped_us_per_call_n1", grouped.logp_dlogp, qg[0]),
                            ("ungrouped_us_per_call_n4", alone.logp_dlogp, q1), ("grouped_us_per_call_n4", grouped.logp_dlogp, qg)):
            row[name] = min(row.get(name, np.inf), per_call(fn, q))
    row["ratio_n1"] = row["grouped_us_per_call_n1"] / row["ungrouped_us_per_call_n1"]
    row["ratio_n4"] = row["grouped_us_per_call_n4"] / row["ungrouped_us_per_call_n4"]
    alone.close()
    grouped.close()
    return row


def timed_fit(model, tune, draws):
    """wall time, evaluations, mean tree depth and the largest R-hat of a and b of a tune + draws x 4-chain fit"""
    count = [0]

    def counted(x):
        count[0] += 1
        return model.logp_dlogp(x)

    t0 = time.perf_counter()
    fit = survival.sample(model, tune=tune, draws=draws, chains=4, seed=0, evaluator=counted)
    wall = time.perf_counter() - t0
    sm = survival.summary(fit)
    return {"fit_wall_s": wall, "fit_evaluations": count[0], "fit_mean_tree_depth": float(fit["stat_tree_depth"].mean()),
            "fit_rhat_max_ab": float(max(np.max(sm["a"]["rhat"]), np.max(sm["b"]["rhat"])))}


def probe_periods(N, T, P, fit, tune, draws):
    """One row: the model by period (P periods of equal length; P = T: monthly) and the ungrouped K = 1 model on the S titer of
    ``simulate(N, T)``, timed one after the other, twice, the smaller figure kept; with ``fit`` a fit of each."""
    y, e, xs = simulate(N, T)
    periods = np.arange(T) * P // T
    alone = survival.SurvivalModel(y, e, xs[:1], ("S",))
    by_period = survival.SurvivalPeriodsModel(y, e, xs[0], "S", periods)
    rng = np.random.default_rng(1)
    qp = np.tile(by_period.initial_point(), (4, 1)) + rng.uniform(-0.5, 0.5, size=(4, by_period.dim))
    q1 = np.zeros((4, alone.dim))
    q1[:, 2], q1[:, 3] = -3.0, np.log(0.5)
    q1 += rng.uniform(-0.5, 0.5, size=q1.shape)
    row = {"N": N, "T": T, "P": P, "dim": by_period.dim, "tiles": (N + 63) // 64}
    for _ in range(2):
        for name, fn, q in (("ungrouped_us_per_call_n1", alone.logp_dlogp, q1[0]), ("periods_us_per_call_n1", by_period.logp_dlogp, qp[0]),
                            ("ungrouped_us_per_call_n4", alone.logp_dlogp, q1), ("periods_us_per_call_n4", by_period.logp_dlogp, qp)):
            row[name] = min(row.get(name, np.inf), per_call(fn, q))
    row["ratio_n1"] = row["periods_us_per_call_n1"] / row["ungrouped_us_per_call_n1"]
    row["ratio_n4"] = row["periods_us_per_call_n4"] / row["ungrouped_us_per_call_n4"]
    if fit:
        row.update({"fit_tune": tune, "fit_draws": draws, "fit_chains": 4})
        row.update({"periods_" + k: v for k, v in timed_fit(by_period, tune, draws).items()})
        row.update({"ungrouped_" + k: v for k, v in timed_fit(alone, tune, draws).items()})
    alone.close()
    by_period.close()
    return row


def probe_waic(N, T, points, reps):
    """One row: ``waic_accumulate`` of ``points`` draws against ``logp_dlogp`` at one point per call, on one handle of the combined
    model of ``simulate(N, T)``."""
    y, e, xs = simulate(N, T)
    model = survival.SurvivalModel(y, e, xs, ("S", "N"))
    rng = np.random.default_rng(1)
    q = np.zeros((points, model.dim))
    q[:, 4], q[:, 5] = -3.0, np.log(0.5)
    q += rng.uniform(-0.5, 0.5, size=q.shape)
    row = {"N": N, "T": T, "K": 2, "points": points, "launches": (points + 15) // 16, "waves_per_launch": ((N + 63) // 64) * min(16, points),
           "accumulate_us_per_draw": [], "logp_dlogp_us_per_call_n1": []}
    model.waic_accumulate(q[:64])  # warm up: the buffers of the first call, the code objects
    model.logp_dlogp(q[0])
    for _ in range(reps):
        model.waic_reset()
        t0 = time.perf_counter()
        model.waic_accumulate(q)
        row["accumulate_us_per_draw"].append(1e6 * (time.perf_counter() - t0) / points)
        row["logp_dlogp_us_per_call_n1"].append(per_call(model.logp_dlogp, q[0]))
    (lse, mean, m2, n), cells = model.waic_stats()
    w = survival.waic(model, {name: q[None, :, k] for k, name in enumerate(model.names)})
    row["n_draws"], row["elpd_waic"], row["p_waic"] = n, w["elpd_waic"], w["p_waic"]
    row["best_accumulate_us_per_draw"] = min(row["accumulate_us_per_draw"])
    row["best_logp_dlogp_us_per_call_n1"] = min(row["logp_dlogp_us_per_call_n1"])
    row["draw_over_single_evaluation"] = row["best_accumulate_us_per_draw"] / row["best_logp_dlogp_us_per_call_n1"]
    model.close()
    return row


def probe_ppc(N, T, points, reps):
    """One row: ``predictive_accumulate`` of ``points`` draws, binned by both titers, against ``waic_accumulate`` of the same draws, on
    one handle of the combined model of ``simulate(N, T)``."""
    y, e, xs = simulate(N, T)
    model = survival.SurvivalModel(y, e, xs, ("S", "N"))
    rng = np.random.default_rng(1)
    q = np.zeros((points, model.dim))
    q[:, 4], q[:, 5] = -3.0, np.log(0.5)
    q += rng.uniform(-0.5, 0.5, size=q.shape)
    edges = [survival.default_edges(x, model.followed) for x in xs]
    model.predictive_configure(xs, edges, 0)
    row = {"N": N, "T": T, "K": 2, "points": points, "launches": (points + 15) // 16, "waves_per_launch": ((N + 63) // 64) * min(16, points),
           "n_bins": [len(ed) + 1 for ed in edges], "ppc_us_per_draw": [], "waic_us_per_draw": []}
    model.predictive_accumulate(q[:64])  # warm up: the buffers of the first call, the code objects
    model.waic_accumulate(q[:64])
    for _ in range(reps):
        model.predictive_reset()
        t0 = time.perf_counter()
        E, Rr = model.predictive_accumulate(q)
        row["ppc_us_per_draw"].append(1e6 * (time.perf_counter() - t0) / points)
        model.waic_reset()
        t0 = time.perf_counter()
        model.waic_accumulate(q)
        row["waic_us_per_draw"].append(1e6 * (time.perf_counter() - t0) / points)
    row["n_draws"] = model.predictive_stats()[3]
    row["expected_total_mean"], row["replicate_total_mean"] = float(E[:, 0].sum(axis=1).mean()), float(Rr[:, 0].sum(axis=1).mean())
    row["observed_total"] = float(model.predictive_observed()[0][0].sum())
    row["best_ppc_us_per_draw"], row["best_waic_us_per_draw"] = min(row["ppc_us_per_draw"]), min(row["waic_us_per_draw"])
    row["ppc_fold_ms"], row["waic_fold_ms"] = 1e-3 * points * row["best_ppc_us_per_draw"], 1e-3 * points * row["best_waic_us_per_draw"]
    row["ppc_over_waic"] = row["best_ppc_us_per_draw"] / row["best_waic_us_per_draw"]
    model.close()
    return row


def probe_loo(N, T, points, reps, host_columns):
    """One row: PSIS-LOO of ``points`` draws (reserve, ``loo_accumulate``, ``loo_stats``, release) against ``waic_accumulate`` +
    ``waic_stats`` of the same draws on one handle of the combined model of ``simulate(N, T)``, alternating; the parts of the LOO
    on their own; and ``compare.psis_loo_from_matrix`` on this host over the first ``host_columns`` followed individuals of the
    matrix read back, scaled to all of them (0: all)."""
    from abdpymc_amd import compare

    y, e, xs = simulate(N, T)
    model = survival.SurvivalModel(y, e, xs, ("S", "N"))
    rng = np.random.default_rng(1)
    q = np.zeros((points, model.dim))
    q[:, 4], q[:, 5] = -3.0, np.log(0.5)
    q += rng.uniform(-0.5, 0.5, size=q.shape)
    row = {"N": N, "T": T, "K": 2, "points": points, "matrix_bytes": 8 * 64 * ((N + 63) // 64) * points, "loo_ms": [], "loo_accumulate_ms": [],
           "loo_stats_ms": [], "waic_ms": []}
    model.loo_reserve(64)  # warm up: the buffers of the first call, the code objects
    model.loo_accumulate(q[:64])
    model.loo_stats()
    model.waic_accumulate(q[:64])
    for _ in range(reps):
        t0 = time.perf_counter()
        model.loo_reserve(points)
        model.loo_accumulate(q)
        t1 = time.perf_counter()
        stats = model.loo_stats()
        t2 = time.perf_counter()
        model.loo_reserve(0)
        row["loo_ms"].append(1e3 * (time.perf_counter() - t0))
        row["loo_accumulate_ms"].append(1e3 * (t1 - t0))
        row["loo_stats_ms"].append(1e3 * (t2 - t1))
        model.waic_reset()
        t0 = time.perf_counter()
        model.waic_accumulate(q)
        model.waic_stats()
        row["waic_ms"].append(1e3 * (time.perf_counter() - t0))
    model.loo_reserve(points)  # once more, untimed, for the host path's matrix
    model.loo_accumulate(q)
    ll = model.loo_rows(0, points)
    model.close()
    w = compare.loo_from_individual(stats[0], stats[1], stats[2], stats[5], stats[4])
    row.update({k: w[k] for k in ("elpd_loo", "p_loo", "se", "n_bad", "n_warn", "n_individuals")})
    cols = np.flatnonzero(stats[5] > 0)
    cols = cols[:host_columns] if host_columns else cols
    t0 = time.perf_counter()
    host = compare.psis_loo_from_matrix(ll[:, cols])
    row["host_columns"] = int(cols.size)
    row["host_ms_all_individuals"] = 1e3 * (time.perf_counter() - t0) * w["n_individuals"] / cols.size
    row["host_max_gap_elpd"] = float(np.abs(host[0] - stats[0][cols]).max())
    row["host_max_gap_k"] = float(np.abs(host[1] - stats[1][cols]).max())
    for k in ("loo_ms", "loo_accumulate_ms", "loo_stats_ms", "waic_ms"):
        row["best_" + k], row["median_" + k] = min(row[k]), float(np.median(row[k]))
    row["loo_over_waic"] = row["best_loo_ms"] / row["best_waic_ms"]
    row["host_over_device_stats"] = row["host_ms_all_individuals"] / row["best_loo_stats_ms"]
    return row


def simulate_draws(M, N, T, seed=0):
    """M event-time datasets from the combined model of ``simulate``: per dataset its own titers, one infection at most, at risk
    until it or until a random last interval."""
    n_risk, event = np.empty((M, N), np.int32), np.empty((M, N), np.int32)
    xs, xn = np.empty((M, T, N)), np.empty((M, T, N))
    for m in range(M):
        rng = np.random.default_rng([seed, m, N, T])
        xs[m], xn[m] = rng.uniform(0.0, 4.0, size=(T, N)), rng.uniform(0.0, 4.0, size=(T, N))
        lam0 = rng.uniform(0.02, 0.08, size=T)
        hit = rng.random((T, N)) < lam0[:, None] / (1.0 + np.exp(-(1.5 * (xs[m] - 1.5) + 0.5 * (xn[m] - 1.0))))
        first = np.where(hit.any(axis=0), hit.argmax(axis=0), T)
        last = rng.integers(max(1, T // 2), T + 1, size=N)
        n_risk[m] = np.minimum(first + 1, last)
        event[m] = np.where(first < last, first, -1)
    return survival.SurvivalDraws(n_risk, event, xs, xn, np.stack([np.zeros(M, np.int64), np.arange(M)], axis=1))


def probe_draws_ic(N, T, M, S, reps):
    """One row: WAIC and PSIS-LOO of M x S draws, every draw on its own dataset -- (a) on the ensemble handle, (b) by a loop over M
    plug-in handles, creation included -- alternating, ``reps`` times; host clocks around calls that end in a synchronise."""
    d = simulate_draws(M, N, T)
    rng = np.random.default_rng(1)
    ens = survival.SurvivalDrawsModel(d, [d.s_titer, d.n_titer], ("S", "N"))
    q = np.zeros((M * S, ens.dim))
    q[:, 4], q[:, 5] = -3.0, np.log(0.5)
    q += rng.uniform(-0.5, 0.5, size=q.shape)
    ds = np.repeat(np.arange(M, dtype=np.int32), S)  # dataset-major, as waic_draws hands a fit of sample_draws over
    fit_of = lambda rows: {name: rows[None, :, k] for k, name in enumerate(ens.names)}  # noqa: E731
    row = {"N": N, "T": T, "K": 2, "datasets": M, "draws_per_dataset": S, "launches": (M * S + 15) // 16,
           "titer_bytes": 2 * 8 * M * T * 64 * ((N + 63) // 64), "loo_matrix_bytes": 8 * M * 64 * ((N + 63) // 64) * S,
           "ensemble_waic_ms": [], "ensemble_loo_ms": [], "loop_waic_ms": [], "loop_loo_ms": [], "loop_create_ms": [], "resident_waic_ms": []}
    ens.draws_waic_accumulate(ds[:64], q[:64])  # warm up: the buffers of the first call, the code objects
    ens.draws_loo_reserve(64)
    ens.draws_loo_accumulate(ds[:64], q[:64])
    ens.draws_loo_stats()
    ens.draws_loo_reserve(0)

    def plug_in(m):
        y, e, xs, xn = d.arrays(m)
        return survival.SurvivalModel(y, e, [xs, xn], ("S", "N"))

    resident = plug_in(0)
    resident.waic_accumulate(q[:64])
    for _ in range(reps):
        t0 = time.perf_counter()
        ens.draws_waic_reset()
        ens.draws_waic_accumulate(ds, q)
        a_waic = ens.draws_waic_stats()
        row["ensemble_waic_ms"].append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        ens.draws_loo_reserve(S)
        ens.draws_loo_accumulate(ds, q)
        a_loo = ens.draws_loo_stats()
        ens.draws_loo_reserve(0)
        row["ensemble_loo_ms"].append(1e3 * (time.perf_counter() - t0))
        create = 0.0
        t0 = time.perf_counter()
        for m in range(M):
            t1 = time.perf_counter()
            sm = plug_in(m)
            create += time.perf_counter() - t1
            b_waic = survival.waic(sm, fit_of(q[m * S:(m + 1) * S]))
            sm.close()
        row["loop_waic_ms"].append(1e3 * (time.perf_counter() - t0))
        row["loop_create_ms"].append(1e3 * create)
        t0 = time.perf_counter()
        for m in range(M):
            sm = plug_in(m)
            b_loo = survival.loo(sm, fit_of(q[m * S:(m + 1) * S]))
            sm.close()
        row["loop_loo_ms"].append(1e3 * (time.perf_counter() - t0))
        resident.waic_reset()
        t0 = time.perf_counter()
        resident.waic_accumulate(q[:S])
        resident.waic_stats()
        row["resident_waic_ms"].append(1e3 * (time.perf_counter() - t0))
    # the last dataset's result of both paths: the same bits
    w_last = survival._compare.waic_from_individual_stats((a_waic[0][M - 1], a_waic[1][M - 1], a_waic[2][M - 1], int(a_waic[3][M - 1])), a_waic[4][M - 1])
    row["same_bits_waic"] = bool(np.array_equal(w_last["elpd_i"], b_waic["elpd_i"]))
    row["same_bits_loo"] = bool(np.array_equal(a_loo[0][M - 1], b_loo["elpd_i"]) and np.array_equal(a_loo[1][M - 1], b_loo["pareto_k"], equal_nan=True))
    resident.close()
    ens.close()
    for k in ("ensemble_waic_ms", "ensemble_loo_ms", "loop_waic_ms", "loop_loo_ms", "loop_create_ms", "resident_waic_ms"):
        row["best_" + k], row["median_" + k] = min(row[k]), float(np.median(row[k]))
    row["ensemble_waic_us_per_draw"] = 1e3 * row["best_ensemble_waic_ms"] / (M * S)
    row["ensemble_loo_us_per_draw"] = 1e3 * row["best_ensemble_loo_ms"] / (M * S)
    row["loop_waic_us_per_draw"] = 1e3 * row["best_loop_waic_ms"] / (M * S)
    row["loop_loo_us_per_draw"] = 1e3 * row["best_loop_loo_ms"] / (M * S)
    row["resident_waic_us_per_draw"] = 1e3 * row["best_resident_waic_ms"] / S
    row["loop_over_ensemble_waic"] = row["best_loop_waic_ms"] / row["best_ensemble_waic_ms"]
    row["loop_over_ensemble_loo"] = row["best_loop_loo_ms"] / row["best_ensemble_loo_ms"]
    row["ensemble_over_resident_per_draw"] = row["ensemble_waic_us_per_draw"] / row["resident_waic_us_per_draw"]
    return row


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("eval", "waic", "ppc", "loo", "draws_ic"), default="eval",
                    help="eval: the evaluator and a fit (the default); waic: scoring a fit; ppc: the posterior predictive check beside the WAIC fold; "
                    "loo: PSIS-LOO beside the WAIC fold and beside the host path; draws_ic: WAIC and PSIS-LOO of per-draw fits on the ensemble "
                    "handle beside a loop over plug-in handles")
    ap.add_argument("--datasets", type=int, default=64, help="--leg draws_ic: datasets of the ensemble")
    ap.add_argument("--draws_per_dataset", type=int, default=1000, help="--leg draws_ic: draws scored on every dataset")
    ap.add_argument("--host_columns", type=int, default=500, help="--leg loo: individuals the host path is timed on (0: all)")
    ap.add_argument("--points", type=int, default=4000, help="--leg waic / ppc: draws folded per repeat")
    ap.add_argument("--reps", type=int, default=3, help="--leg waic / ppc: repeats")
    ap.add_argument("--groups", type=int, nargs="+", help="time the model by group with this many groups (one figure, or one per size)")
    ap.add_argument("--periods", type=int, nargs="+", help="time the model by period with this many periods (0: monthly), each at every size")
    ap.add_argument("--fit", action="store_true", help="--periods: also time a fit of the model by period and of the K = 1 model")
    ap.add_argument("--out")
    ap.add_argument("--tune", type=int, default=1000)
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--no_fit", action="store_true")
    args = ap.parse_args(argv)
    rows = []
    if args.leg == "waic":
        for N, T in SIZES:
            rows.append(probe_waic(N, T, args.points, args.reps))
            print(json.dumps(rows[-1]), flush=True)
    if args.leg == "ppc":
        for N, T in SIZES:
            rows.append(probe_ppc(N, T, args.points, args.reps))
            print(json.dumps(rows[-1]), flush=True)
    if args.leg == "loo":
        for N, T in SIZES:
            rows.append(probe_loo(N, T, args.points, args.reps, args.host_columns))
            print(json.dumps(rows[-1]), flush=True)
    if args.leg == "draws_ic":
        for N, T in SIZES:
            rows.append(probe_draws_ic(N, T, args.datasets, args.draws_per_dataset, args.reps))
            print(json.dumps(rows[-1]), flush=True)
            if args.out:  # kept row by row: a run that is cut short leaves what it measured
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    json.dump(rows, f, indent=1)
    if args.groups:
        if len(args.groups) not in (1, len(SIZES)):
            ap.error(f"--groups takes one figure or {len(SIZES)}")
        for (N, T), Gr in zip(SIZES, args.groups * (len(SIZES) if len(args.groups) == 1 else 1)):
            rows.append(probe_groups(N, T, Gr))
            print(json.dumps(rows[-1]), flush=True)
    for N, T in SIZES if args.periods else ():
        for P in args.periods:
            if not 0 <= P <= T:
                ap.error(f"--periods: {P} outside [0, {T}]")
            rows.append(probe_periods(N, T, P or T, args.fit, args.tune, args.draws))
            print(json.dumps(rows[-1]), flush=True)
            if args.out:  # kept row by row: a long run that is cut short leaves what it measured
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    json.dump(rows, f, indent=1)
    for N, T in SIZES if not args.groups and not args.periods and args.leg == "eval" else ():
        y, e, xs = simulate(N, T)
        rs = R.Restatement(y, e, xs)
        model = survival.SurvivalModel(y, e, xs, ("S", "N"))
        rng = np.random.default_rng(1)
        q = np.zeros((4, model.dim))
        q[:, 4], q[:, 5] = -3.0, np.log(0.5)
        q += rng.uniform(-0.5, 0.5, size=q.shape)
        row = {"N": N, "T": T, "K": 2, "dim": model.dim, "cells": N * T, "data_bytes": 32 * N * T}
        row["device_us_per_call_n1"] = per_call(model.logp_dlogp, q[0])
        row["device_us_per_call_n4"] = per_call(model.logp_dlogp, q)
        row["numpy_us_per_evaluation"] = per_call(rs.logp_dlogp, q[0])
        lp_d, g_d = model.logp_dlogp(q[0])
        lp_r, g_r = rs.logp_dlogp(q[0])
        row["logp_device"], row["logp_numpy"] = lp_d, lp_r
        row["grad_max_rel_diff"] = float(np.abs(g_d - g_r).max() / np.abs(g_r).max())
        print(json.dumps(row), flush=True)
        if not args.no_fit:
            t0 = time.perf_counter()
            count = [0]

            def counted(x):  # (a sign of life every 50 000 evaluations)
                count[0] += 1
                if count[0] % 50000 == 0:
                    print(f"  {count[0]} evaluations, {time.perf_counter() - t0:.0f} s", file=sys.stderr, flush=True)
                return model.logp_dlogp(x)

            fit = survival.sample(model, tune=args.tune, draws=args.draws, chains=4, seed=0, evaluator=counted)
            row["fit_evaluations"] = count[0]
            row["fit_wall_s"] = time.perf_counter() - t0
            row["fit_tune"], row["fit_draws"], row["fit_chains"] = args.tune, args.draws, 4
            row["fit_leapfrogs_kept_draws"] = int(fit["stat_n_steps"].sum())
            row["fit_mean_tree_depth"] = float(fit["stat_tree_depth"].mean())
            sm = survival.summary(fit)
            row["fit_rhat_max_ab"] = float(max(np.max(sm["a"]["rhat"]), np.max(sm["b"]["rhat"])))
            row["fit_a_median"] = np.median(fit["a"], axis=(0, 1)).tolist()
            row["fit_b_median"] = np.median(fit["b"], axis=(0, 1)).tolist()
            print(json.dumps({k: v for k, v in row.items() if k.startswith("fit_")}), flush=True)
        model.close()
        rows.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
