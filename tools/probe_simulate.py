"""
Cost of the device cohort simulator (abd_simulate): wall time of ``Context.simulate`` on the default cohort (191 x 31, lists) and
on BASELINE config 3 (dense, 10 000 individuals x 200 gaps) for 1, 16 and 256 replicates, with every output and with
infections + n_infected only -- one warm-up call, then the median of ``--reps`` calls -- and, on the same box's CPU, the two
baselines for scale: ``synthetic.make_cohort`` for one cohort (the only generator there was; a simpler process) and the NumPy
restatement's loop on the default cohort (tests/sim_restatement.py, standing in for the reference's Python loop).
``--profile COHORT R`` makes three calls of R replicates with every output and nothing else, for
``rocprofv3 --kernel-trace --stats -- python tools/probe_simulate.py --profile config3 16``: the kernels' own times.
Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from abdpymc_amd import synthetic  # noqa: E402
from abdpymc_amd._native import SIM_OUTPUTS, Context  # noqa: E402
from abdpymc_amd.simulation import Antibodies  # noqa: E402


def cohorts(which):
    out = {}
    if "default" in which:
        from tests.test_data_loader import default_cohort

        td = default_cohort(os.path.join(ROOT, "tests", "golden"))
        out["default"] = (td.n_gaps, td.n_inds, td.s.obs, td.n.obs, td.vacs, td.pcrpos)
    if "config3" in which:
        sc = synthetic.make_cohort(10000, 200, seed=3)
        out["config3"] = (sc.n_gaps, sc.n_inds, sc.s_obs, sc.n_obs, sc.vacs, sc.pcrpos)
    return out


def timed(f, reps):
    f()  # warm-up: code objects, the first touch of the output pages
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append(time.perf_counter() - t0)
    return statistics.median(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cohorts", nargs="+", default=["default", "config3"], choices=("default", "config3"))
    ap.add_argument("--replicates", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--profile", nargs=2, metavar=("COHORT", "R"))
    a = ap.parse_args()
    params = Antibodies().as_native()
    if a.profile:
        name, R = a.profile[0], int(a.profile[1])
        G, N, s_obs, n_obs, vacs, pcr = cohorts([name])[name]
        ctx = Context(G, N, s_obs, n_obs, vacs, pcr)
        for _ in range(3):
            ctx.simulate(params, np.full(G, 0.04), seed=1, n_replicates=R)
        print(json.dumps(dict(profile=name, replicates=R, n_inds=N, n_gaps=G, calls=3)))
        ctx.close()
        return
    out = {}
    for name, (G, N, s_obs, n_obs, vacs, pcr) in cohorts(a.cohorts).items():
        ctx = Context(G, N, s_obs, n_obs, vacs, pcr)
        lam0 = np.full(G, 0.04)
        res = dict(n_inds=N, n_gaps=G, dense=ctx.is_dense, readings=ctx.n_obs_s + ctx.n_obs_n)
        for R in a.replicates:
            for leg, outputs in (("all", SIM_OUTPUTS), ("infections", ("infections", "n_infected"))):
                res[f"{leg}_{R}_s"] = timed(lambda: ctx.simulate(params, lam0, seed=1, n_replicates=R, outputs=outputs), a.reps)
        out[name] = res
        ctx.close()
        if not a.no_cpu:
            res["make_cohort_s"] = timed(lambda: synthetic.make_cohort(N, G, seed=3), 3)
    if not a.no_cpu and "default" in a.cohorts:
        from tests import sim_restatement as Rst

        G, N, s_obs, n_obs, vacs, pcr = cohorts(["default"])["default"]
        out["default"]["restatement_s"] = timed(
            lambda: Rst.simulate(params, np.full(G, 0.04), vacs, pcr, 1, 0, s_obs[:3], n_obs[:3]), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
