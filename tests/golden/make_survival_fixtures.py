"""
Writes tests/golden/survival_reference_k1.npz and _k2.npz: the case table of tests/survival_restatement.py evaluated by its 40-digit statement,
rounded to float64, with the sum of the absolute addends S of every output.  Needs mpmath; about ten minutes on eight processes.

    python -m tests.golden.make_survival_fixtures
"""
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import survival_restatement as R  # noqa: E402


def one(case):
    key, N, T, K, name = case
    y, e, xs = R.make_data(N, T, K)
    r = R.mp_evaluate(y, e, xs, R.make_point(name, T, K))
    return key, r


def main():
    table = sorted(R.cases(), key=lambda c: -c[1] * c[2])  # the long ones first
    out = {}
    with ProcessPoolExecutor(min(8, os.cpu_count() or 1)) as ex:
        for key, r in ex.map(one, table):
            for name, v in r.items():
                out[f"{key}/{name}"] = np.asarray(v, dtype=np.float64)
    for K, name in R.FIXTURES.items():
        np.savez_compressed(os.path.join(HERE, name), **{k: v for k, v in out.items() if f"_K{K}_" in k})
    print(f"{len(table)} cases -> {sorted(R.FIXTURES.values())}")


if __name__ == "__main__":
    main()
