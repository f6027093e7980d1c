"""
Writes tests/golden/survival_periods_reference.npz: the case table of tests/survival_periods_restatement.py evaluated by its
40-digit statement, rounded to float64, with the sum of the absolute addends S of every output; the cases of the two pointwise
shapes also hold every individual's log-likelihood.  Needs mpmath; some ten minutes on eight processes.

    python -m tests.golden.make_survival_periods_fixtures
"""
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import survival_periods_restatement as R  # noqa: E402


def one(case):
    key, N, T, P, name = case
    y, e, x, period = R.make_case(N, T, P)
    return key, R.mp_evaluate_periods(y, e, x, period, P, R.make_point(name, T, P), pointwise=(N, T, P) in R.SHAPES_POINTWISE)


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
