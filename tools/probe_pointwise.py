"""
Cost of the pointwise log-likelihood at BASELINE config 3 (dense, 10 000 individuals x 200 gaps, 4 M readings): wall time of a
4-chain compound sampler run with and without on-device WAIC accumulation (sample(..., waic=True)).  Run under
``rocprofv3 --kernel-trace --stats -- python tools/probe_pointwise.py`` for the kernel's own time per draw and chain
(abd_pointwise_dense_kernel).  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from abdpymc_amd import synthetic  # noqa: E402
from abdpymc_amd.model import AbdModel  # noqa: E402
from abdpymc_amd.sampler import sample  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inds", type=int, default=10000)
    ap.add_argument("--gaps", type=int, default=200)
    ap.add_argument("--chains", type=int, default=4)
    ap.add_argument("--tune", type=int, default=100)
    ap.add_argument("--draws", type=int, default=100)
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    sc = synthetic.make_cohort(a.inds, a.gaps, seed=3)
    d = SimpleNamespace(n_gaps=sc.n_gaps, n_inds=sc.n_inds, vacs=sc.vacs, pcrpos=sc.pcrpos,
                        coords={"gap": np.arange(sc.n_gaps), "ind": np.arange(sc.n_inds)},
                        s=SimpleNamespace(obs=sc.s_obs), n=SimpleNamespace(obs=sc.n_obs))
    m = AbdModel(d, n_chains=a.chains)
    kw = dict(tune=a.tune, draws=a.draws, chains=a.chains, seed=1, record_deterministics=False, record_discrete=False)
    sample(m, **dict(kw, tune=5, draws=5), waic=True)  # warm-up: code objects, allocations
    t = {"plain": [], "waic": []}
    for _ in range(a.reps):  # alternated, so that drift hits both legs alike
        for leg in ("plain", "waic"):
            t0 = time.perf_counter()
            sample(m, waic=leg == "waic", **kw)
            t[leg].append(time.perf_counter() - t0)
    best = {k: min(v) for k, v in t.items()}
    print(json.dumps(dict(inds=a.inds, gaps=a.gaps, chains=a.chains, iterations=a.tune + a.draws, draws=a.draws,
                          wall_s=t, overhead=best["waic"] / best["plain"] - 1.0)))
    m.close()


if __name__ == "__main__":
    main()
