"""
Writes tests/golden/psis_wide_reference.npz: the 40-digit PSIS-LOO statistics of the matrices of
tests/survival_loo_restatement.WIDE_CASES -- tails past 256 draws, the dispatch edges of abd_psis_kernel and the cap of 16 384
draws -- by ``psis_column_mp`` of that file, rounded to float64.

    python tests/golden/make_psis_wide_fixtures.py [out.npz]

Per case `<name>` of WIDE_CASES, over the columns of its matrix (an unfollowed column: elpd = lppd = 0, k = NaN, n_tail = 0):

    <name>.elpd    (columns,) float64
    <name>.k       (columns,) float64   +inf where the tail has at most 4 draws
    <name>.lppd    (columns,) float64
    <name>.n_tail  (columns,) int64

The matrices are not in the file: whoever reads it rebuilds them from the seeds (``wide_case``).  The members are written in sorted
order with a fixed date, so the same inputs give the same bytes.  All thirteen cases take about 20 s of mpmath on one core (5 s at
S = 16 384); tests/test_psis_wide_cpu.py regenerates every one and compares it bit for bit.

The program also prints, per case, the gap of the fp64 loop restatement ``psis_column`` to the values it has just computed, and
their worst: `g_wide` of tests/golden/NOTICE_survival_loo.md.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import survival_loo_restatement as R  # noqa: E402

FIXTURE = "psis_wide_reference.npz"
WHAT = ("elpd", "k", "lppd", "n_tail")


def generate(name):
    """{member: array} of one case"""
    ll, unfollowed = R.wide_case(name)
    return {f"{name}.{what}": v for what, v in zip(WHAT, R.matrix_of(R.psis_column_mp, ll, unfollowed))}


def load(path=None):
    """{member: array} of the committed file"""
    with np.load(path or os.path.join(ROOT, "tests", "golden", FIXTURE)) as f:
        return {k: f[k] for k in f.files}


def reference(fixture, name):
    """(elpd, k, lppd, n_tail) of one case from ``load()``"""
    return tuple(fixture[f"{name}.{what}"] for what in WHAT)


if __name__ == "__main__":
    import time

    from tests.golden.make_fused_fixtures import write  # sorted members, a fixed date

    path =sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", FIXTURE)
    t0 = time.time()
    arrays, worst = {}, {}
    for name in R.WIDE_CASES:
        arrays.update(generate(name))
        ll, unfollowed = R.wide_case(name)
        ref = reference(arrays, name)
        got = R.matrix_of(R.psis_column, ll, unfollowed)
        assert np.array_equal(got[3], ref[3])
        gaps = [R.rel_gap(got[i], ref[i]) for i in range(3)]
        print(name, "elpd %.3g  k %.3g  lppd %.3g" % tuple(gaps), "n_tail", ref[3].tolist(), "k", np.round(ref[1], 3).tolist(), flush=True)
        for key, g in zip(WHAT, gaps):
            worst[key] = max(worst.get(key, 0.0), g)
    write(path, arrays)
    print("worst", worst)
    print(path, os.path.getsize(path), "bytes,", f"{time.time() - t0:.0f} s")
