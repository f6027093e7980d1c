"""
What per-draw survival fits cost, two legs in one run on one device, each alternated with its yardstick, best of
``--reps``, for every ``--form``: ``combined`` (K = 2, the default), ``groups`` (S titer, four interleaved groups) and ``periods``
(S titer, three eras of equal length):

(a) a 16-point launch of the ensemble kernel of the form on 16 datasets (``logp_dlogp`` of the per-draw model) against a 16-point
    launch of the plug-in kernel of the same form on one handle, at N x T = 1 520 x 30 and 10 000 x 199: microseconds per call.
    The probe checks that 16 points on dataset 0 are the bits the plug-in handle of dataset 0 returns, logp and gradient.
(b) an M = ``--datasets`` fit by ``sample_draws`` (up to 16 chains of different datasets share every launch) against the same M
    chains run as a loop of ``_chain`` over M plug-in handles of the form -- the paths a caller had before -- at 1 520 x 30:
    wall time, evaluations, evaluator calls, and where the wall time went: inside the evaluator (the device and its call) and
    outside it (the host's NUTS).  The two legs run the same chains bit for bit; the probe checks it.

Data are simulated from the model, one seed per dataset (``tools/probe_survival.py: simulate``): they have event-time form.  The
exit status is 1 where a bit check failed.

    python tools/probe_survival_draws.py [--out FILE] [--datasets 64] [--tune 100] [--draws 50] [--reps 3] [--leg a|b|both]
                                         [--form combined|groups|periods|all]
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
from tools.probe_survival import SIZES, per_call, simulate  # noqa: E402


def ensemble(M, N, T):
    """(SurvivalDraws, the (y, e, xs) of every dataset)"""
    data = [simulate(N, T, seed=m) for m in range(M)]
    pairs = [survival.event_time(y, e) for y, e, _ in data]
    d = survival.SurvivalDraws(np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]), np.stack([xs[0].T for _, _, xs in data]),
                               np.stack([xs[1].T for _, _, xs in data]), np.stack([np.zeros(M, np.int64), np.arange(M)], axis=1))
    return d, data


FORMS = ("combined", "groups", "periods")
N_GROUPS, N_PERIODS = 4, 3


def models(form, d, data):
    """(the per-draw model of ``form`` over the ensemble ``d``, a function m -> the plug-in model of dataset m, K)"""
    N, T = d.n_inds, d.n_int
    if form == "groups":
        groups = np.arange(N) % N_GROUPS
        return (survival.SurvivalDrawsGroupsModel(d, d.s_titer, "S", groups),
                lambda m: survival.SurvivalGroupsModel(data[m][0], data[m][1], data[m][2][0], "S", groups), 1)
    if form == "periods":
        periods = np.arange(T) * N_PERIODS // T
        return (survival.SurvivalDrawsPeriodsModel(d, d.s_titer, "S", periods),
                lambda m: survival.SurvivalPeriodsModel(data[m][0], data[m][1], data[m][2][0], "S", periods), 1)
    return (survival.SurvivalDrawsModel(d, [d.s_titer, d.n_titer], ("S", "N")),
            lambda m: survival.SurvivalModel(data[m][0], data[m][1], data[m][2], ("S", "N")), 2)


def points(n, model, seed=1):
    q = np.tile(survival._initial_point(model), (n, 1))  # the prior means of lam0's hyperparameters, the rest 0
    return q + np.random.default_rng(seed).uniform(-0.5, 0.5, size=q.shape)


def leg_a(form, N, T, reps):
    d, data = ensemble(16, N, T)
    ens, plug_in, K = models(form, d, data)
    one = plug_in(0)
    q, ds = points(16, ens), np.arange(16, dtype=np.int32)
    ld = d.n_inds if form != "groups" else 64 * int(((np.bincount(np.arange(N) % N_GROUPS) + 63) // 64).sum())  # columns of a plane
    row = {"leg": "a", "form": form, "N": N, "T": T, "K": K, "points": 16, "datasets": 16, "ensemble_bytes": int(16 * (8 * K * T * ld + 8 * ld)),
           "plug_in_bytes_16_handles": int(16 * 8 * (2 + K) * ld * T), "ensemble_us_per_call": [], "plug_in_us_per_call": []}
    lp_e, g_e = ens.logp_dlogp(ds * 0, q)
    lp_p, g_p = one.logp_dlogp(q)
    row["same_bits_on_dataset_0"] = bool(np.array_equal(lp_e, lp_p) and np.array_equal(g_e, g_p))
    for _ in range(reps):
        row["ensemble_us_per_call"].append(per_call(lambda x: ens.logp_dlogp(ds, x), q, 0.5))
        row["plug_in_us_per_call"].append(per_call(one.logp_dlogp, q, 0.5))
    row["best_ensemble_us_per_call"], row["best_plug_in_us_per_call"] = min(row["ensemble_us_per_call"]), min(row["plug_in_us_per_call"])
    row["ensemble_over_plug_in"] = row["best_ensemble_us_per_call"] / row["best_plug_in_us_per_call"]
    ens.close()
    one.close()
    return row


class Clocked:
    """an evaluator with the time spent inside it, its calls and its points"""

    def __init__(self, fn):
        self.fn, self.s, self.calls, self.points = fn, 0.0, 0, 0

    def __call__(self, *args):
        t0 = time.perf_counter()
        out = self.fn(*args)
        self.s += time.perf_counter() - t0
        self.calls += 1
        self.points += 1 if np.ndim(args[-1]) == 1 else len(args[-1])
        return out


def leg_b(form, N, T, M, tune, draws, reps, seed=0):
    d, data = ensemble(M, N, T)
    ens, plug_in, K = models(form, d, data)
    handles = [plug_in(m) for m in range(M)]
    q0 = survival._initial_point(ens)
    row = {"leg": "b", "form": form, "N": N, "T": T, "K": K, "datasets": M, "tune": tune, "draws": draws, "batched": [], "loop": []}
    for _ in range(reps):
        ev = Clocked(ens.logp_dlogp)
        t0 = time.perf_counter()
        fit = survival.sample_draws(ens, tune=tune, draws=draws, seed=seed, evaluator=ev)
        wall = time.perf_counter() - t0
        row["batched"].append({"wall_s": wall, "evaluator_s": ev.s, "host_s": wall - ev.s, "calls": ev.calls, "evaluations": ev.points})
        t0 = time.perf_counter()
        spent, calls, alone = 0.0, 0, []
        for m, h in enumerate(handles):
            ev1 = Clocked(h.logp_dlogp)
            alone.append(survival._chain(ev1, ens.dim, tune, draws, np.random.default_rng([seed, m, 0]), 0.8, q0)[0])
            spent, calls = spent + ev1.s, calls + ev1.calls
        wall = time.perf_counter() - t0
        row["loop"].append({"wall_s": wall, "evaluator_s": spent, "host_s": wall - spent, "calls": calls, "evaluations": calls})
        got = np.stack([fit[name] for name in ens.names], axis=-1)
        row["same_chains"] = bool(np.array_equal(got, np.stack(alone)))
    best = {k: min(row[k], key=lambda r: r["wall_s"]) for k in ("batched", "loop")}
    row["best_batched_wall_s"], row["best_loop_wall_s"] = best["batched"]["wall_s"], best["loop"]["wall_s"]
    row["loop_over_batched"] = row["best_loop_wall_s"] / row["best_batched_wall_s"]
    for k, b in best.items():
        row[k + "_us_per_evaluation"] = {"wall": 1e6 * b["wall_s"] / b["evaluations"], "evaluator": 1e6 * b["evaluator_s"] / b["evaluations"],
                                         "host": 1e6 * b["host_s"] / b["evaluations"]}
    row["mean_points_per_call"] = best["batched"]["evaluations"] / best["batched"]["calls"]
    sm = survival.draws_summary(fit)
    row["frac_between"] = {k: v["frac_between"] for k, v in sm.items() if k[0] in "ab"}
    row["p_positive"] = {k: v["p_positive"] for k, v in sm.items() if "p_positive" in v}
    ens.close()
    for h in handles:
        h.close()
    return row


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("a", "b", "both"), default="both")
    ap.add_argument("--datasets", type=int, default=64)
    ap.add_argument("--tune", type=int, default=100)
    ap.add_argument("--draws", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--form", choices=FORMS + ("all",), default="combined")
    ap.add_argument("--out")
    args = ap.parse_args(argv)
    rows = []

    def keep(row):
        rows.append(row)
        print(json.dumps(row), flush=True)
        if args.out:  # row by row: a run that is cut short leaves what it measured
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(rows, f, indent=1)

    for form in FORMS if args.form == "all" else (args.form,):
        if args.leg in ("a", "both"):
            for N, T in SIZES:
                keep(leg_a(form, N, T, args.reps))
        if args.leg in ("b", "both"):
            keep(leg_b(form, SIZES[0][0], SIZES[0][1], args.datasets, args.tune, args.draws, args.reps))
    return 0 if all(r.get("same_bits_on_dataset_0", True) and r.get("same_chains", True) for r in rows) else 1


if __name__ == "__main__":
    raise SystemExit(main())
