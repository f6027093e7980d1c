"""
PSIS-LOO where the tail passes 256 draws and at the cap of 16 384, without a GPU ("Past a tail of 256"): the
committed 40-digit values of tests/golden/psis_wide_reference.npz are what tests/golden/make_psis_wide_fixtures.py computes, the
matrices of ``survival_loo_restatement.WIDE_CASES`` reach what they were made to reach (asserted from the reference's n_tail and
k, before any kernel is involved), the fp64 loop restatement stays within its recorded gap ``G_WIDE`` and the host path within
the bound.

The bound on a value, relative to max(1, |value|), against the 40-digit one: max(64 g_wide, S 2^-53), the rule of
tests/test_survival_loo_cpu.py with ``g_wide``, the loop restatement's worst gap over these matrices
(tests/golden/NOTICE_survival_loo.md): its sequential S-term sums grow with S, so these cases have a figure of their own and
``G`` of the old cases is not raised.
"""
import functools

import numpy as np
import pytest

from abdpymc_amd import _native, compare
from tests import survival_loo_restatement as R
from tests.golden import make_psis_wide_fixtures as F

# the fp64 restatement's own worst gap to the 40-digit values over WIDE_CASES (python tests/golden/make_psis_wide_fixtures.py)
G_WIDE = dict(elpd=2.2e-13, k=1.7e-14, lppd=7.4e-15)


def bound_wide(what, S):
    return max(64.0 * G_WIDE[what], S * 2.0 ** -53)


@pytest.fixture(scope="module")
def fixture():
    return F.load()


def check_against_the_fixture(got, name, fixture, tag):
    """``got`` = (elpd, k, lppd, n_tail) of the case's matrix against the committed 40-digit values: n_tail and the inf / NaN
    pattern exactly, the values within ``bound_wide``.  Prints every figure, then asserts.  Returns the gaps."""
    S = R.wide_case(name)[0].shape[0]
    ref = F.reference(fixture, name)
    np.testing.assert_array_equal(np.asarray(got[3]), ref[3])
    gaps = {}
    for i, what in enumerate(("elpd", "k", "lppd")):
        gaps[what] = R.rel_gap(got[i], ref[i])  # asserts the inf / NaN pattern
        print(f"case {name} (S {S}): {tag} {what} gap {gaps[what]:.3g} bound {bound_wide(what, S):.3g}")
    for what, gap in gaps.items():
        assert gap <= bound_wide(what, S), (name, what, gap)
    return gaps


@functools.lru_cache(maxsize=None)
def _fp64(name):
    ll, unfollowed = R.wide_case(name)
    return R.matrix_of(R.psis_column, ll, unfollowed)


@pytest.mark.parametrize("name", R.WIDE_CASES)
def test_fixture_is_the_40_digit_statement(name, fixture):
    import mpmath  # noqa: F401  (no skip: this test is what ties the committed file to psis_column_mp)

    today = F.generate(name)
    assert sorted(today) == sorted(k for k in fixture if k.startswith(name + "."))
    for key, v in today.items():
        assert v.dtype == fixture[key].dtype == (np.int64 if key.endswith(".n_tail") else np.float64)
        np.testing.assert_array_equal(v, fixture[key], err_msg=key)


def test_fixture_holds_the_cases_and_nothing_else(fixture):
    assert len(R.WIDE_CASES) == 13 and sorted(fixture) == sorted(f"{name}.{what}" for name in R.WIDE_CASES for what in F.WHAT)
    assert [R.tail_len(S) for S in R.S_WIDE_VALUES] == [8, 48, 64, 96, 97, 128, 192, 256, 257, 384]
    assert R.tail_len(R.S_TIES_WIDE) == 261 and R.S_WIDE_VALUES[-1] == _native.Survival.LOO_MAX_DRAWS
    assert all(compare.psis_tail_len(S) == R.tail_len(S) for S in R.S_WIDE_VALUES + (R.S_TIES_WIDE,))


@pytest.mark.parametrize("S", R.S_WIDE_VALUES)
def test_matrix_wide_reaches_what_it_was_made_for(S, fixture):
    """From the reference alone: the four random columns fill the tail (a full sort array of 8, 64, 128, 256; 257 and 384 in the
    512-slot one), ``few_high`` has a tail of equal values with a finite negative k, ``constant`` has none."""
    name = f"wide_{S}"
    ll, unfollowed = R.wide_case(name)
    elpd, k, lppd, n_tail = F.reference(fixture, name)
    M, few = R.tail_len(S), R.n_few_high(S)
    col = {c: j for j, c in enumerate(R.COLUMNS_WIDE)}
    assert ll.shape == (S, 7) and unfollowed == (col["unfollowed"],) and (ll[:, 6] == 0).all()
    for c in ("positive", "huge", "uniform", "heavy"):
        assert n_tail[col[c]] == M and np.isfinite(k[col[c]]), c
    assert few == (5, 16, 21, 32, 32, 42, 64, 85, 85, 128)[R.S_WIDE_VALUES.index(S)] < M
    assert n_tail[col["few_high"]] == few and np.isfinite(k[col["few_high"]]) and k[col["few_high"]] < 0
    x = -ll[:, col["few_high"]] - (-ll[:, col["few_high"]]).max()
    assert np.unique(x).tolist() == [-1.0, 0.0] and (x == 0.0).sum() == few  # the tail's members are equal: t_q == t_max
    assert n_tail[col["constant"]] == 0 and np.isposinf(k[col["constant"]])
    assert elpd[col["constant"]] == lppd[col["constant"]] == -1.25
    assert n_tail[col["unfollowed"]] == 0 and np.isnan(k[col["unfollowed"]]) and elpd[col["unfollowed"]] == lppd[col["unfollowed"]] == 0.0
    assert (ll[:, col["positive"]] > 0).all() and elpd[col["positive"]] > 0 and lppd[col["positive"]] > 0
    assert 1.9e4 < -elpd[col["huge"]] < 2.1e4
    if S >= 256:  # at S = 40 the prior of the fit (10 pseudo-draws at k = 0.5) outweighs a tail of 8
        assert k[col["uniform"]] < 0 and k[col["heavy"]] > 1


def test_plain_and_tied_matrices_reach_the_512_slot_sort(fixture):
    assert F.reference(fixture, "plain_7282")[3].tolist() == [257, 257, 257, 257, 128, 0]
    assert F.reference(fixture, "plain_16384")[3].tolist() == [384, 384, 384, 384, 192, 0]
    ll, _ = R.wide_case("ties_wide")
    assert ll.shape == (7512, 6) and all((ll[:1878] == ll[1878 * r:1878 * (r + 1)]).all() for r in range(4))
    assert F.reference(fixture, "ties_wide")[3].tolist() == [260, 260, 260, 260, 260, 0]  # below M = 261, above 256
    for name in ("plain_7282", "plain_16384", "ties_wide"):
        k = F.reference(fixture, name)[1]
        assert np.isfinite(k[:5]).all() and np.isnan(k[5])


@pytest.mark.parametrize("name", R.WIDE_CASES)
def test_restatement_is_within_its_recorded_gap(name, fixture):
    """Both restatements agree on n_tail and on the inf / NaN pattern (``rel_gap`` asserts it); the values within ``G_WIDE``."""
    got, ref = _fp64(name), F.reference(fixture, name)
    np.testing.assert_array_equal(got[3], ref[3])
    for i, what in enumerate(("elpd", "k", "lppd")):
        gap = R.rel_gap(got[i], ref[i])
        print(f"case {name}: psis_column {what} gap {gap:.3g} (g_wide {G_WIDE[what]:.3g})")
        assert gap <= G_WIDE[what], (name, what, gap)


@pytest.mark.parametrize("name", R.WIDE_CASES)
def test_host_path_against_the_fixture(name, fixture):
    ll, unfollowed = R.wide_case(name)
    got = compare.psis_loo_from_matrix(ll)  # the unfollowed column is found by its zeros
    fp64 = _fp64(name)
    np.testing.assert_array_equal(got[3], fp64[3])  # the tail is decided by exact operations
    np.testing.assert_array_equal(np.isposinf(got[1]), np.isposinf(fp64[1]))
    np.testing.assert_array_equal(np.isnan(got[1]), np.isnan(fp64[1]))
    check_against_the_fixture(got, name, fixture, "host path")
