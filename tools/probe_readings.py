"""
Cost of the per-reading outputs at BASELINE config 3 (dense, 10 000 individuals x 200 gaps, 4 M readings): wall time of a
4-chain compound sampler run with and without on-device WAIC accumulation (``--leg waic``: sample(..., waic=True)) or posterior
predictive check statistics (``--leg ppc``: sample(..., ppc=True)) or the per-individual WAIC accumulation alone (``--leg
individual``: sample(..., waic=True, waic_by="individual"); ``--profile``: waic_by="both", so that abd_individual_dense_kernel runs
beside abd_readings_dense_kernel<LogLik, ...> in one trace) or PSIS-LOO by individual (``--leg loo``: sample(..., loo=True), whose
read-out at the end of the run is abd_psis_kernel over all chains' draws; ``--profile``: with waic_by="individual" as well, so that
the one abd_individual_dense_kernel launch per draw and chain writes the staging rows AND the accumulators, and abd_loo_store runs
once per 16 draws) or the epidemic curves of every draw (``--leg curves``:
sample(..., curves=True); not a per-reading output, but the same question) or the per-cell convergence accumulators
(``--leg diagnostics``: sample(..., diagnostics=True); likewise) or the infection-risk-by-titer table of every draw (``--leg
risk``: sample(..., risk=spec) with 7 edges per antigen, the whole window, first infections only; likewise) or the per-individual
timelines (``--leg timelines``: sample(..., timelines=True) over the default ranges, with the device's quantile read-out at the end
of the run; likewise), alternated.  With two run lengths (``--draws 100 400``) the
fixed (per run) and per-draw costs separate.  ``--profile`` runs one short sample with both on, for
``rocprofv3 --kernel-trace --stats -- python tools/probe_readings.py --profile``: the kernel's own time per draw and chain of
each op (abd_readings_dense_kernel<LogLik, ...>, <Predictive, ...>) in the same run; with ``--leg curves`` the short sample has
the curves on instead (abd_curves_kernel, abd_curves_sum_kernel beside abd_deterministics_kernel with its running sums), with
``--leg diagnostics`` the accumulators (abd_diag_kernel beside the same), with ``--leg risk`` the risk table AND the curves
(abd_risk_kernel, abd_risk_sum_kernel beside abd_curves_kernel, abd_curves_sum_kernel: the two walk the same words), with
``--leg timelines`` the timelines AND the convergence accumulators (abd_timeline_kernel beside abd_diag_kernel, the same walker;
abd_timeline_quantile_kernel is the read-out).  Prints
one JSON line.
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from abdpymc_amd import risk, synthetic  # noqa: E402
from abdpymc_amd.model import AbdModel  # noqa: E402
from abdpymc_amd.sampler import sample  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("waic", "individual", "loo", "ppc", "curves", "diagnostics", "risk", "timelines"), default="waic")
    ap.add_argument("--inds", type=int, default=10000)
    ap.add_argument("--gaps", type=int, default=200)
    ap.add_argument("--chains", type=int, default=4)
    ap.add_argument("--tune", type=int, default=100)
    ap.add_argument("--draws", type=int, nargs="+", default=[100])
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    sc = synthetic.make_cohort(a.inds, a.gaps, seed=3)
    d = SimpleNamespace(n_gaps=sc.n_gaps, n_inds=sc.n_inds, vacs=sc.vacs, pcrpos=sc.pcrpos,
                        coords={"gap": np.arange(sc.n_gaps), "ind": np.arange(sc.n_inds)},
                        s=SimpleNamespace(obs=sc.s_obs), n=SimpleNamespace(obs=sc.n_obs))
    m = AbdModel(d, n_chains=a.chains)
    kw = dict(tune=a.tune, chains=a.chains, seed=1, record_deterministics=False, record_discrete=False)
    spec = risk.spec(0, a.gaps, 0.5 * np.arange(1, 8), 0.5 * np.arange(1, 8), 1)

    def leg_kw(on):  # the option of this leg, switched on or off
        if a.leg == "individual":
            return dict(waic=on, waic_by="individual")
        return dict(risk=spec if on else None) if a.leg == "risk" else {a.leg: on}

    if a.profile:
        t0 = time.perf_counter()
        on = {a.leg: True} if a.leg in ("curves", "diagnostics") else dict(waic=True, ppc=True)
        if a.leg == "risk":
            on = dict(curves=True)
        if a.leg == "timelines":
            on = dict(timelines=True, diagnostics=True)
        if a.leg == "individual":
            on = dict(waic=True, waic_by="both")
        if a.leg == "loo":
            on = dict(waic=True, waic_by="individual", loo=True)
        sample(m, draws=a.draws[0], **on, **(leg_kw(True) if a.leg == "risk" else {}), **kw)
        print(json.dumps(dict(inds=a.inds, gaps=a.gaps, chains=a.chains, tune=a.tune, draws=a.draws[0], **on, risk=a.leg == "risk",
                              wall_s=time.perf_counter() - t0)))
        m.close()
        return
    sample(m, **dict(kw, tune=5), draws=5, **leg_kw(True))  # warm-up: code objects, allocations
    legs = ("plain", a.leg)
    t = {f"{leg}_{n}": [] for n in a.draws for leg in legs}
    for _ in range(a.reps):  # alternated, so that drift hits both legs alike
        for n in a.draws:
            for leg in legs:
                t0 = time.perf_counter()
                sample(m, draws=n, **leg_kw(leg != "plain"), **kw)
                t[f"{leg}_{n}"].append(time.perf_counter() - t0)
    best = {k: min(v) for k, v in t.items()}
    out = dict(leg=a.leg, inds=a.inds, gaps=a.gaps, chains=a.chains, tune=a.tune, draws=a.draws, wall_s=t,
               overhead={str(n): best[f"{a.leg}_{n}"] / best[f"plain_{n}"] - 1.0 for n in a.draws})
    if len(a.draws) == 2 and a.draws[0] != a.draws[1]:
        d0, d1 = a.draws
        extra0, extra1 = best[f"{a.leg}_{d0}"] - best[f"plain_{d0}"], best[f"{a.leg}_{d1}"] - best[f"plain_{d1}"]
        per_draw = (extra1 - extra0) / (d1 - d0)  # seconds per draw (all chains)
        out.update(per_draw_ms=1e3 * per_draw, per_draw_chain_us=1e6 * per_draw / a.chains,
                   fixed_ms=1e3 * (extra0 - per_draw * d0))
    print(json.dumps(out))
    m.close()


if __name__ == "__main__":
    main()
