"""
Writes tests/golden/survival_predictive_reference.npz from the case table of tests/survival_predictive_restatement.py: per case of
the expected tables ``<case>/E`` (n_var, 8), the 40-digit statement rounded to float64; per replicate case
``<shape>_rep/r`` (3, N, T) int8, the float64 restatement's per-cell replicates of the three replicate points as the draws
draw0 .. draw0 + 2 under the case's seed, and ``<shape>_rep/boundary``, the number of boundary cells (0: the seeds were chosen so).
Needs mpmath; about a minute on eight processes.

    python -m tests.golden.make_survival_predictive_fixtures
"""
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import survival_predictive_restatement as R  # noqa: E402


def one(case):
    key, shape, name = case
    rs, _, variables, edges = R.model_of(shape)
    return key, R.mp_expected(rs, R.point_of(shape, name), variables, edges)[0]


def replicate_case(shape, seed, draw0):
    """(r (3, N, T) int8, boundary cells) of one replicate case"""
    rs = R.model_of(shape)[0]
    got = [R.replicates(rs, R.point_of(shape, name), seed, draw0 + d) for d, name in enumerate(R.REPLICATE_POINTS)]
    r = np.stack([g[0] for g in got])
    assert r.max() <= 127
    return r.astype(np.int8), sum(g[1] for g in got)


def main():
    table = sorted(R.cases(), key=lambda c: -c[1][1] * c[1][2])  # the long ones first
    out = {}
    with ProcessPoolExecutor(min(8, os.cpu_count() or 1)) as ex:
        for key, E in ex.map(one, table):
            out[f"{key}/E"] = np.asarray(E, dtype=np.float64)
    for shape, seed, draw0 in R.REPLICATE_CASES:
        r, boundary = replicate_case(shape, seed, draw0)
        out[f"{R.tag(shape)}_rep/r"], out[f"{R.tag(shape)}_rep/boundary"] = r, np.array(boundary, dtype=np.int64)
    np.savez_compressed(os.path.join(HERE, R.FIXTURE), **out)
    print(f"{len(table)} cases, {len(R.REPLICATE_CASES)} replicate cases -> {R.FIXTURE}")


if __name__ == "__main__":
    main()
