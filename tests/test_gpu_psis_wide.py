"""
abd_psis_kernel where the suite had never asked it for anything (abd_psis.hpp; DESIGN.md §27, "Past a tail of 256"): tails above
256 draws, which alone take the 512-slot sort; 16 384 draws, every register slot of ``abd_psis_kernel<64>`` live; the last and the
first S of every instantiation; a tail that fills its sort array; positive and very large values, a constant column, a tail of
equal values, k < 0 and k > 1.

The statistics are held to the committed 40-digit values of tests/golden/psis_wide_reference.npz with the bound of
tests/test_psis_wide_cpu.py: n_tail and the inf / NaN pattern exactly, the values within max(64 g_wide, S 2^-53) relative to
max(1, |value|).  The matrices go in through ``loo_append_rows`` of a one-interval handle; the pointwise kernels play no part but in
the last test, which ties a dataset's block of a per-draw handle to the plug-in handle at a tail of 257.
"""
import numpy as np
import pytest

from abdpymc_amd import _native, compare
from tests import survival_loo_restatement as R
from tests import survival_predictive_restatement as RS
from tests import survival_restatement as R1
from tests.survival_draws_cases import datasets
from tests.test_gpu_survival_loo import _plain_handle
from tests.golden import make_psis_wide_fixtures as F
from tests.test_psis_wide_cpu import check_against_the_fixture
from tests.test_survival_loo_cpu import bound

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture():
    return F.load()  # a file: no mpmath on the GPU machine


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _same_bits(got, want, what=""):
    """two results of ``loo_stats``"""
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        a, b = np.asarray(a), np.asarray(b)
        np.testing.assert_array_equal(_bits(a) if a.dtype == np.float64 else a, _bits(b) if b.dtype == np.float64 else b, err_msg=f"{what}: output {i}")


def _stats(ll, unfollowed, capacity=None, calls=None):
    """``loo_stats`` of the rows ``ll`` in a handle reserved at ``capacity`` (default: the rows), appended in ``calls`` (default: one)"""
    h = _plain_handle(ll.shape[1], unfollowed)
    try:
        h.loo_reserve(ll.shape[0] if capacity is None else capacity)
        at = 0
        for n in calls or (ll.shape[0],):
            h.loo_append_rows(ll[at:at + n])
            at += n
        assert at == ll.shape[0]
        return h.loo_stats()
    finally:
        h.close()


@pytest.mark.parametrize("name", R.WIDE_CASES)
def test_stats_against_the_40_digit_fixture(name, fixture):
    ll, unfollowed = R.wide_case(name)
    S, N = ll.shape
    elpd, k, lppd, n_tail, n_draws, cells = _stats(ll, unfollowed)
    assert n_draws == S and cells.tolist() == [0 if j in unfollowed else 1 for j in range(N)]
    check_against_the_fixture((elpd, k, lppd, n_tail), name, fixture, "device")


def test_capacity_above_the_draws_held():
    """The row stride is the capacity, not S: 7 282 draws (a tail of 257, the 512-slot sort) in a matrix reserved for 16 384 give
    the bits of the matrix reserved for 7 282."""
    ll, unfollowed = R.wide_case("wide_7282")
    tight = _stats(ll, unfollowed)
    assert tight[4] == 7282 and tight[3].tolist() == [257, 257, 0, 85, 257, 257, 0]
    _same_bits(_stats(ll, unfollowed, capacity=_native.Survival.LOO_MAX_DRAWS), tight, "capacity 16384")


def test_fill_order_at_the_cap():
    """16 384 draws in one call and in calls of 1, 4 095, 4 097 and 8 191 rows, and both again after ``loo_reset``: the same bits."""
    ll, unfollowed = R.wide_case("wide_16384")
    split = (1, 4095, 4097, 8191)
    assert sum(split) == ll.shape[0] == _native.Survival.LOO_MAX_DRAWS
    once = _stats(ll, unfollowed)
    assert once[4] == 16384 and once[3].tolist() == [384, 384, 0, 128, 384, 384, 0]
    h = _plain_handle(ll.shape[1], unfollowed)
    try:
        h.loo_reserve(ll.shape[0])
        for calls in (split, (ll.shape[0],), split):
            at = 0
            for n in calls:
                h.loo_append_rows(ll[at:at + n])
                at += n
            _same_bits(h.loo_stats(), once, f"calls {calls}")
            h.loo_reset()
    finally:
        h.close()


def test_ensemble_block_equals_the_plug_in_at_a_wide_tail():
    """Dataset m of a per-draw handle reserved at 7 282 draws starts m * ld * 7282 doubles into the matrix: its statistics are the
    bits of the plug-in handle of that dataset, whose rows the host path confirms, with a tail of 257 in the 512-slot sort."""
    S, N, T, M = 7282, 65, 3, 2
    d = datasets(M, N, T)
    shape = ("k", N, T, 1)
    p0 = RS.point_of(shape, "typical")
    q = p0 + 0.1 * np.random.default_rng(7).normal(size=(S, p0.size))
    h = _native.SurvivalDraws(d.n_risk, d.event, [d.s_titer], R1.PRIORS[1])
    try:
        h.draws_loo_reserve(S)
        for m in range(M):
            h.draws_loo_accumulate(m, q)
        got = h.draws_loo_stats()
    finally:
        h.close()
    np.testing.assert_array_equal(got[4], [S, S])
    for m in range(M):
        y, e, xs, _ = d.arrays(m)
        p = _native.Survival(y, e, [xs], R1.PRIORS[1])
        try:
            p.loo_reserve(S)
            p.loo_accumulate(q)
            elpd, k, lppd, n_tail, n, cells = p.loo_stats()
            rows = p.loo_rows(0, S)
        finally:
            p.close()
        followed = cells > 0
        assert n == S and followed.sum() > 32 and not followed.all()
        np.testing.assert_array_equal(cells, d.n_risk[m])
        assert (n_tail[followed] == 257).all() and (n_tail[~followed] == 0).all()  # the 512-slot sort, or this test checks nothing
        np.testing.assert_array_equal(n_tail, got[3][m])
        for a, b, what in zip((elpd, k, lppd), (got[0][m], got[1][m], got[2][m]), ("elpd", "k", "lppd")):
            np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=f"{what} of dataset {m}")
        host = compare.psis_loo_from_matrix(rows, cells)
        np.testing.assert_array_equal(n_tail, host[3])
        for a, b, what in zip((elpd, k, lppd), host[:3], ("elpd", "k", "lppd")):
            gap = R.rel_gap(a, b)
            print(f"dataset {m}: {what} device against host {gap:.3g} (bound {bound(what, S):.3g})")
            assert gap <= bound(what, S), (m, what, gap)
