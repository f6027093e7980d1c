"""
Writes tests/golden/survival_pointwise_reference.npz: the case table of tests/survival_pointwise_restatement.py evaluated by its
40-digit statement, rounded to float64: per case ll_j and the sum of the absolute addends S_j of every individual.  Needs mpmath;
about a minute on eight processes.

    python -m tests.golden.make_survival_pointwise_fixtures
"""
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import survival_pointwise_restatement as R  # noqa: E402


def one(case):
    key, N, T, K, Gr, name = case
    rs, _ = R.model_of(N, T, K, Gr)
    return key, R.mp_pointwise(rs, R.point_of(name, T, K, Gr))


def main():
    table = sorted(R.cases(), key=lambda c: -c[1] * c[2])  # the long ones first
    out = {}
    with ProcessPoolExecutor(min(8, os.cpu_count() or 1)) as ex:
        for key, r in ex.map(one, table):
            for name, v in r.items():
                out[f"{key}/{name}"] = np.asarray(v, dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, R.FIXTURE), **out)
    print(f"{len(table)} cases -> {R.FIXTURE}")


if __name__ == "__main__":
    main()
