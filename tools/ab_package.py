#!/usr/bin/env python3
"""A/B of two trees' PYTHON packages on one library: what a refactor of the host side has to leave byte-equal.

    git archive <parent> abdpymc_amd | tar -x -C <dir>                # the parent's package, beside this tree
    ABD_HIP_LIB=$PWD/abdpymc_amd/libabd_hip.so python tools/ab_package.py run <dir> <out A>
    ABD_HIP_LIB=$PWD/abdpymc_amd/libabd_hip.so python tools/ab_package.py run . <out B>
    python tools/ab_package.py compare <out A> <out B>

A refactor of the library's own host side: archive the whole parent (its `tests/` too), build its library there, and give each
`run` its own tree's library in `ABD_HIP_LIB`.

`run` (a process per tree): `sample()` with every summary and record row on (`thin=3`, `timelines_hist`), and with nothing on,
on the dense 67 x 65 cohort and the golden `test_cohort` of `tests/test_gpu_summaries_together.py`, then `abdpymc-infer` with
every flag, each saved as `.npz`; the CLI's stderr is the caller's to keep.  The same pair of `sample()` calls again under
each environment of `LEGS`, which reach what the defaults (observation-list trains; dense trains with units of one) do not: the
sampler's result-row back-end on several host threads and on one with units of two chains, and dense trains that share a launch
(units of two, four chains).  Then the survival models (`survival.npz`): handles
of `_native.Survival` on `tests.survival_restatement.make_data` at (N, T) = (1, 1), (67, 30), (130, 65) with K = 1 and 2, and of
`_native.SurvivalGroups` on `tests.survival_groups_restatement.make_case` at (67, 30, 3) and (130, 65, 4) -- `loglik_sums` at every
point of the restatement's `POINTS`, `logp_dlogp` and `individual_loglik` of 19 stacked points (two launches), the WAIC
accumulators of the same 19 -- and one short `survival.sample` with `survival.waic` per form on 300 x 6 simulated cells.
`compare`: the same sixteen files and key sets, every array equal in dtype, shape and bytes -- the chains are deterministic per seed,
so this is a condition, not a tolerance."""
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "test_cohort")
CHAINS, TUNE, DRAWS = 3, 3, 8
# (file prefix, environment of the library while the leg's samplers are created, chains, cohorts)
LEGS = (("", {}, CHAINS, ("dense", "test")),
        ("rows_", {"ABD_SAMPLER_TRAINS": "0"}, CHAINS, ("dense", "test")),
        ("rows_unit2_", {"ABD_SAMPLER_TRAINS": "0", "ABD_SAMPLER_UNIT": "2", "ABD_SAMPLER_THREADS": "1"}, CHAINS, ("dense", "test")),
        ("unit2_", {"ABD_SAMPLER_UNIT": "2"}, 4, ("dense",)))
N_FILES = 2 * sum(len(leg[3]) for leg in LEGS) + 2  # everything / nothing per leg and cohort, cli.npz, survival.npz


def run(tree, out):
    tree = os.path.abspath(tree)
    sys.path.insert(0, tree)
    import abdpymc_amd
    from abdpymc_amd import _native, cli, risk, synthetic
    from abdpymc_amd.data import TiterData
    from abdpymc_amd.model import AbdModel, model
    from abdpymc_amd.sampler import sample

    assert os.path.dirname(os.path.abspath(abdpymc_amd.__file__)) == os.path.join(tree, "abdpymc_amd"), abdpymc_amd.__file__
    print("package", os.path.relpath(abdpymc_amd.__file__, ROOT), "library", os.path.relpath(_native.LIB_PATH, ROOT), flush=True)
    os.makedirs(out, exist_ok=True)

    def cohort(which, chains):
        if which == "test":
            return model(TiterData.from_disk(GOLDEN), n_chains=chains)
        N, G = 67, 65
        sc = synthetic.make_cohort(N, G, seed=11)
        last = np.full(N, G - 1, dtype=np.int32)
        last[::5] = -1
        last[1::5] = np.arange(len(last[1::5])) * 4 % (G - 1)
        last[2::5] = 63
        d = SimpleNamespace(n_gaps=sc.n_gaps, n_inds=sc.n_inds, vacs=sc.vacs, pcrpos=sc.pcrpos, last_gap=last,
                            coords={"gap": np.arange(sc.n_gaps), "ind": np.arange(sc.n_inds)},
                            s=SimpleNamespace(obs=sc.s_obs), n=SimpleNamespace(obs=sc.n_obs))
        return AbdModel(d, n_chains=chains)

    for prefix, env, chains, which in ((p, e, c, w) for p, e, c, ws in LEGS for w in ws):
        assert not any(k in os.environ for leg in LEGS for k in leg[1]), "the legs set the sampler's environment themselves"
        os.environ.update(env)
        m = cohort(which, chains)
        sp = risk.spec(0, m.n_gaps, 0.5 * np.arange(1, 8), 0.25 * np.arange(1, 8), 1)
        kw = dict(tune=TUNE, draws=DRAWS, chains=chains, seed=7)
        everything = sample(m, log_likelihood=True, posterior_predictive=True, thin=3, waic=True, ppc=True, curves=True,
                            sero_thresholds=(1.0, 0.5), diagnostics=True, diag_batch=2, risk=sp, timelines=True,
                            timeline_ranges=((-3, 7), (-2, 6)), timeline_q=(0.1, 0.5, 0.8, 0.9), timelines_hist=True, **kw)
        np.savez(os.path.join(out, f"{prefix}{which}_everything.npz"), **everything)
        nothing = sample(m, **kw)
        np.savez(os.path.join(out, f"{prefix}{which}_nothing.npz"), **nothing)
        print(prefix + which, "everything", len(everything), "keys; nothing", len(nothing), "keys", flush=True)
        m.close()
        for k in env:
            del os.environ[k]
    rc = cli.main(["--tune", "6", "--draws", "8", "--cores", "1", "--chains", "2", "--seed", "5", "--ititers_data", GOLDEN, "--thin", "3",
                   "--waic", "--log_likelihood", "--posterior_predictive", "--ppc", "--curves", "--sero_threshold_s", "2.0",
                   "--sero_threshold_n", "1.0", "--diagnostics", "--diag_batch", "2", "--risk", "--risk_edges_s", "0.5,1.5,2.5",
                   "--risk_edges_n", "0.5,1.0", "--risk_start", "1", "--risk_all_infections", "--timelines", "--timeline_range_s=-2,6",
                   "--timeline_range_n=-3,7", "--netcdf", os.path.join(out, "cli.npz")])
    assert rc == 0
    run_survival(out)


def run_survival(out):
    """The survival leg of `run`, through API that every tree since DESIGN 21 has."""
    from abdpymc_amd import _native, survival
    from tests import survival_groups_restatement as RG
    from tests import survival_restatement as R
    from tests.test_gpu_survival import _simulated
    from tests.test_survival_groups_cpu import simulate

    res = {}

    def handle(tag, h, points):
        for name, q in points.items():
            res[f"{tag}/{name}/sums"] = h.loglik_sums(q)
        q19 = np.stack([list(points.values())[k % len(points)] for k in range(19)])
        res[f"{tag}/logp"], res[f"{tag}/grad"] = h.logp_dlogp(q19)
        res[f"{tag}/ll"] = h.individual_loglik(q19)
        h.waic_reset()
        h.waic_accumulate(q19)
        (res[f"{tag}/lse"], res[f"{tag}/mean"], res[f"{tag}/m2"], n), res[f"{tag}/n_cells"] = h.waic_stats()
        res[f"{tag}/n_draws"] = np.array(n)
        h.close()

    for N, T in ((1, 1), (67, 30), (130, 65)):
        for K in (1, 2):
            y, e, xs = R.make_data(N, T, K)
            handle(f"N{N}_T{T}_K{K}", _native.Survival(y, e, xs, R.PRIORS[K]), {name: R.make_point(name, T, K) for name in R.POINTS})
    for N, T, Gr in ((67, 30, 3), (130, 65, 4)):
        y, e, x, group = RG.make_case(N, T, Gr)
        handle(f"N{N}_T{T}_G{Gr}", _native.SurvivalGroups(y, e, x, group, Gr, RG.PRIORS), {name: RG.make_point(name, T, Gr) for name in RG.POINTS})
    y, e, xs = _simulated()
    yg, eg, xg, group = simulate(N=300, T=6, seed=3, a=(0.5, 1.5, 2.5), b=2.0)
    for tag, model in (("fit", survival.SurvivalModel(y, e, xs, ("S",))), ("fit_groups", survival.SurvivalGroupsModel(yg, eg, xg, "S", group))):
        fit = survival.sample(model, tune=20, draws=20, chains=2, seed=0)
        w = survival.waic(model, fit)  # records its arrays in the fit
        model.close()
        res.update({f"{tag}/{k}": np.asarray(v) for k, v in fit.items()})
        res.update({f"{tag}/waic_{k}": np.asarray(w[k]) for k in ("elpd_waic", "p_waic", "se")})
    np.savez(os.path.join(out, "survival.npz"), **res)
    print("survival", len(res), "arrays", flush=True)


def compare(a, b):
    files = sorted(os.listdir(a))
    assert files == sorted(os.listdir(b)) and len(files) == N_FILES, (files, sorted(os.listdir(b)))
    bad = n = nbytes = 0
    for f in files:
        za, zb = np.load(os.path.join(a, f), allow_pickle=False), np.load(os.path.join(b, f), allow_pickle=False)
        same_keys = set(za.files) == set(zb.files)
        bad += not same_keys
        eq = 0
        for k in sorted(set(za.files) & set(zb.files)):
            x, y = za[k], zb[k]
            ok = x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
            eq, n, nbytes = eq + ok, n + 1, nbytes + x.nbytes
            if not ok:
                bad += 1
                print("DIFFERS", f, k, x.dtype, y.dtype, x.shape, y.shape)
        print(f"{f}: {len(za.files)} keys A, {len(zb.files)} keys B, key sets {'equal' if same_keys else 'DIFFER: ' + str(set(za.files) ^ set(zb.files))}, "
              f"{eq} arrays equal in dtype, shape and bytes; order of keys {'the same' if za.files == zb.files else 'differs'}")
    print(f"{n} arrays, {nbytes} bytes compared: {'ALL BYTE-EQUAL' if not bad else str(bad) + ' DIFFERENCES'}")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 4 or sys.argv[1] not in ("run", "compare"):
        raise SystemExit(__doc__)
    raise SystemExit(run(*sys.argv[2:]) if sys.argv[1] == "run" else compare(*sys.argv[2:]))
