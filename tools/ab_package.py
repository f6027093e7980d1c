#!/usr/bin/env python3
"""A/B of two trees' PYTHON packages on one library: what a refactor of the host side has to leave byte-equal.

    git archive <parent> abdpymc_amd | tar -x -C <dir>                # the parent's package, beside this tree
    ABD_HIP_LIB=$PWD/abdpymc_amd/libabd_hip.so python tools/ab_package.py run <dir> <out A>
    ABD_HIP_LIB=$PWD/abdpymc_amd/libabd_hip.so python tools/ab_package.py run . <out B>
    python tools/ab_package.py compare <out A> <out B>

`run` (a process per tree): `sample()` with every summary and record row on (`thin=3`, `timelines_hist`), and with nothing on,
on the dense 67 x 65 cohort and the golden `test_cohort` of `tests/test_gpu_summaries_together.py`, then `abdpymc-infer` with
every flag, each saved as `.npz`; the CLI's stderr is the caller's to keep.  `compare`: the same files and key sets, every array
equal in dtype, shape and bytes -- the chains are deterministic per seed, so this is a condition, not a tolerance."""
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "test_cohort")
CHAINS, TUNE, DRAWS = 3, 3, 8


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

    def cohort(which):
        if which == "test":
            return model(TiterData.from_disk(GOLDEN), n_chains=CHAINS)
        N, G = 67, 65
        sc = synthetic.make_cohort(N, G, seed=11)
        last = np.full(N, G - 1, dtype=np.int32)
        last[::5] = -1
        last[1::5] = np.arange(len(last[1::5])) * 4 % (G - 1)
        last[2::5] = 63
        d = SimpleNamespace(n_gaps=sc.n_gaps, n_inds=sc.n_inds, vacs=sc.vacs, pcrpos=sc.pcrpos, last_gap=last,
                            coords={"gap": np.arange(sc.n_gaps), "ind": np.arange(sc.n_inds)},
                            s=SimpleNamespace(obs=sc.s_obs), n=SimpleNamespace(obs=sc.n_obs))
        return AbdModel(d, n_chains=CHAINS)

    for which in ("dense", "test"):
        m = cohort(which)
        sp = risk.spec(0, m.n_gaps, 0.5 * np.arange(1, 8), 0.25 * np.arange(1, 8), 1)
        kw = dict(tune=TUNE, draws=DRAWS, chains=CHAINS, seed=7)
        everything = sample(m, log_likelihood=True, posterior_predictive=True, thin=3, waic=True, ppc=True, curves=True,
                            sero_thresholds=(1.0, 0.5), diagnostics=True, diag_batch=2, risk=sp, timelines=True,
                            timeline_ranges=((-3, 7), (-2, 6)), timeline_q=(0.1, 0.5, 0.8, 0.9), timelines_hist=True, **kw)
        np.savez(os.path.join(out, f"{which}_everything.npz"), **everything)
        nothing = sample(m, **kw)
        np.savez(os.path.join(out, f"{which}_nothing.npz"), **nothing)
        print(which, "everything", len(everything), "keys; nothing", len(nothing), "keys", flush=True)
        m.close()
    rc = cli.main(["--tune", "6", "--draws", "8", "--cores", "1", "--chains", "2", "--seed", "5", "--ititers_data", GOLDEN, "--thin", "3",
                   "--waic", "--log_likelihood", "--posterior_predictive", "--ppc", "--curves", "--sero_threshold_s", "2.0",
                   "--sero_threshold_n", "1.0", "--diagnostics", "--diag_batch", "2", "--risk", "--risk_edges_s", "0.5,1.5,2.5",
                   "--risk_edges_n", "0.5,1.0", "--risk_start", "1", "--risk_all_infections", "--timelines", "--timeline_range_s=-2,6",
                   "--timeline_range_n=-3,7", "--netcdf", os.path.join(out, "cli.npz")])
    assert rc == 0


def compare(a, b):
    files = sorted(os.listdir(a))
    assert files == sorted(os.listdir(b)) and len(files) == 5, (files, sorted(os.listdir(b)))
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
