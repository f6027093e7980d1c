"""
PSIS-LOO by individual of the survival models on the device (abd_survival_loo_*; abd_psis.hpp): the stored rows
against abd_survival_individual_loglik bit for bit on all four kinds of handle, the statistics' independence of how the matrix
was filled, the statistics against the 40-digit restatement of tests/survival_loo_restatement.py with the bound of
tests/test_survival_loo_cpu.py, the known tail shapes, capacity and release, and ``survival.loo`` end to end.
"""
import os

import numpy as np
import pytest

from abdpymc_amd import _native, compare, survival
from abdpymc_amd.data import TiterData
from tests import survival_loo_restatement as R
from tests import survival_predictive_restatement as RS
from tests.test_gpu_survival_predictive import _handle
from tests.test_survival_loo_cpu import bound, check_against_40_digits

pytestmark = pytest.mark.gpu

# one cell; a second tile with one live lane; three tiles ending in a partial one -- of every kind of handle (the grouped labels
# are interleaved: the slots are a permutation of the caller's order)
KINDS = [("k", 1), ("k", 2), ("groups", None), ("periods", None)]
SHAPES = [(form, N, T, n if n is not None else {1: 1, 65: 3 if form == "groups" else 2, 130: 4 if form == "groups" else 3}[N])
          for form, n in KINDS for N, T in ((1, 1), (65, 3), (130, 65))]


def _draws(shape, n, seed=7):
    rng = np.random.default_rng(seed)
    q = RS.point_of(shape, "typical")
    return q + 0.1 * rng.normal(size=(n, q.size))


@pytest.mark.parametrize("shape", SHAPES, ids=RS.tag)
def test_stored_rows_are_the_bits_of_individual_loglik(shape):
    h = _handle(RS.model_of(shape)[1])
    try:
        q = _draws(shape, 19)
        ll = h.individual_loglik(q)
        h.loo_reserve(24)
        h.loo_accumulate(q)  # launches of 16 + 3
        np.testing.assert_array_equal(h.loo_rows(0, 19), ll)
        np.testing.assert_array_equal(h.loo_rows(15, 3), ll[15:18])
        assert h.loo_rows(19, 0).shape == (0, shape[1])
        with pytest.raises(ValueError, match="outside the 19 draws held"):
            h.loo_rows(18, 2)
        assert h.loo_stats()[4] == 19
    finally:
        h.close()


@pytest.mark.parametrize("shape", [("k", 130, 65, 2), ("groups", 130, 65, 4), ("periods", 130, 65, 3)], ids=RS.tag)
def test_stats_do_not_depend_on_how_the_matrix_was_filled(shape):
    h = _handle(RS.model_of(shape)[1])
    try:
        q = _draws(shape, 70)
        h.loo_reserve(70)
        with pytest.raises(ValueError, match="no draws held"):
            h.loo_stats()
        h.loo_accumulate(q)
        once = h.loo_stats()
        ll = h.loo_rows(0, 70)
        assert once[4] == 70 and (once[3][once[5] > 0] > 4).all() and np.isfinite(once[1][once[5] > 0]).all()
        assert (ll.std(axis=0)[once[5] > 0] > 1e-4).all()  # the draws differ
        h.loo_reset()
        at = 0
        for n in (1, 16, 19, 34):
            h.loo_accumulate(q[at:at + n])
            at += n
        split = h.loo_stats()
        h.loo_reset()
        h.loo_append_rows(ll[:33])
        h.loo_append_rows(ll[33:])
        np.testing.assert_array_equal(h.loo_rows(0, 70), ll)
        rows = h.loo_stats()
        for other in (split, rows, h.loo_stats()):  # _stats consumes nothing
            for a, b in zip(other, once):
                np.testing.assert_array_equal(a, b)
    finally:
        h.close()


def _plain_handle(N, unfollowed=()):
    """N individuals of one interval, those of ``unfollowed`` without a followed cell: rows come from append_rows"""
    e = np.ones((N, 1))
    e[list(unfollowed)] = 0.0
    return _native.Survival(np.zeros((N, 1)), e, [np.zeros((N, 1))], (1.0, -3.0, 0.5, 2.0, 1.0))


@pytest.mark.parametrize("name", R.CASES)
def test_stats_against_the_40_digit_restatement(name):
    """n_tail and the inf / NaN pattern exactly, the values within max(64 g, S 2^-53) relative to max(1, |value|)."""
    ll, _ = R.case(name)
    h = _plain_handle(ll.shape[1], R.UNFOLLOWED)
    try:
        h.loo_reserve(ll.shape[0])
        h.loo_append_rows(ll)
        elpd, k, lppd, n_tail, n_draws, cells = h.loo_stats()
        assert n_draws == ll.shape[0] and cells.tolist() == [1, 1, 1, 1, 1, 0]
        check_against_40_digits((elpd, k, lppd, n_tail), name)
    finally:
        h.close()


@pytest.mark.parametrize("k0", (0.3, 0.7))
def test_known_tail_shape(k0):
    ll = R.known_k(k0)
    h = _plain_handle(ll.shape[1])
    try:
        h.loo_reserve(ll.shape[0])
        h.loo_append_rows(ll)
        k = h.loo_stats()[1]
    finally:
        h.close()
    print(f"k0 {k0}: the device's median k {np.median(k):.4f}")
    assert abs(float(np.median(k)) - k0) <= 0.1
    host = compare.psis_loo_from_matrix(ll)[1]
    assert np.abs(k - host).max() <= 2 * bound("k", ll.shape[0])


def test_capacity_and_release():
    shape = ("k", 65, 3, 1)
    h = _handle(RS.model_of(shape)[1])
    try:
        q = _draws(shape, 21)
        with pytest.raises(_native.AbdError, match="no matrix reserved"):
            h.loo_accumulate(q[:1])
        with pytest.raises(ValueError, match="outside"):
            h.loo_reserve(_native.Survival.LOO_MAX_DRAWS + 1)
        with pytest.raises(ValueError, match="outside"):
            h.loo_reserve(-1)
        h.loo_reserve(20)
        h.loo_accumulate(q[:16])
        before = h.loo_rows(0, 16)
        for call in (lambda: h.loo_accumulate(q[16:]), lambda: h.loo_append_rows(np.ones((5, 65)))):
            with pytest.raises(_native.AbdError, match="would pass the capacity of 20"):
                call()
            assert h.loo_stats()[4] == 16  # nothing stored
            np.testing.assert_array_equal(h.loo_rows(0, 16), before)
        h.loo_accumulate(q[16:20])
        first = h.loo_stats()
        assert first[4] == 20
        h.loo_reserve(0)  # released
        with pytest.raises(ValueError, match="no draws held"):
            h.loo_stats()
        with pytest.raises(_native.AbdError, match="no matrix reserved"):
            h.loo_accumulate(q[:1])
        h.loo_reserve(32)  # and again, wider
        h.loo_accumulate(q[:20])
        for a, b in zip(h.loo_stats(), first):
            np.testing.assert_array_equal(a, b)
        h.loo_reserve(_native.Survival.LOO_MAX_DRAWS)  # the cap itself is served
        h.loo_accumulate(q[:20])
        for a, b in zip(h.loo_stats(), first):
            np.testing.assert_array_equal(a, b)
    finally:
        h.close()


def test_loo_of_a_fit_of_the_golden_cohort(golden_dir, capsys):
    """``survival.loo`` on the device against ``compare.psis_loo_from_matrix`` of the rows read back, within the bound."""
    from abdpymc_amd.model import model
    from abdpymc_amd.sampler import sample

    data = TiterData.from_disk(os.path.join(golden_dir, "test_cohort"))
    m = model(data, n_chains=2)
    res = sample(m, tune=20, draws=20, chains=2, seed=1, record_deterministics=False, record_discrete=False)
    m.close()
    sa = survival.SurvivalAnalysis(res, 0, data.n_gaps, data)
    sm = sa.model_combined()
    try:
        fit = survival.sample(sm, tune=100, draws=100, chains=2, seed=0)
        w = survival.loo(sm, fit)
        with pytest.raises(ValueError, match="no draws held"):
            sm.loo_stats()  # released
        q = survival.fit_points(sm, fit)
        sm.loo_reserve(q.shape[0])
        sm.loo_accumulate(q)
        rows = sm.loo_rows(0, q.shape[0])
        sm.loo_reserve(0)
        np.testing.assert_array_equal(rows, sm.individual_loglik(q))
        waic = survival.waic(sm, fit)
    finally:
        sm.close()
    assert all(key in fit for key in survival.LOO_FIT_KEYS + survival.WAIC_FIT_KEYS) and (int(fit["start"]), int(fit["end"])) == (0, data.n_gaps)
    elpd, k, lppd, n_tail = compare.psis_loo_from_matrix(rows, sm.n_cells)
    host = compare.loo_from_individual(elpd, k, lppd, sm.n_cells, 200)
    followed = sm.n_cells > 0
    assert w["n_draws"] == 200 and w["n_individuals"] == int(followed.sum()) > 0 and (n_tail[followed] > 4).all() and n_tail.max() == 40
    np.testing.assert_array_equal(np.isnan(w["pareto_k"]), ~followed)
    assert (w["elpd_i"][~followed] == 0).all() and (w["p_loo_i"][~followed] == 0).all()
    for key, what in (("elpd_i", "elpd"), ("lppd_i", "lppd"), ("pareto_k", "k")):
        gap = R.rel_gap(w[key], host[key])
        print(f"{key}: device against host {gap:.3g} (bound {bound(what, 200):.3g})")
        assert gap <= bound(what, 200)
    assert abs(w["elpd_loo"] - host["elpd_loo"]) <= bound("elpd", 200) * max(1.0, abs(host["elpd_loo"])) and w["p_loo"] > 0
    assert (w["n_bad"], w["n_warn"], w["worst"]) == (host["n_bad"], host["n_warn"], host["worst"])
    print(survival.waic_line(waic))
    print(survival.loo_line(w))
    assert abs(w["elpd_loo"] - waic["elpd_waic"]) < 0.05 * abs(waic["elpd_waic"])  # two estimates of one quantity
