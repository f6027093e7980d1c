"""
The per-individual log-likelihood of the survival model by period on the device (MODE 3 of abd_survival_individual_kernel;
DESIGN 24): parity with the 40-digit per-individual reference in tests/golden/survival_periods_reference.npz, its sum against the
data part of logp, bit-reproducibility across launches, and the WAIC statistics however the draws are batched.
"""
import numpy as np
import pytest

from abdpymc_amd import _native, compare
from tests import survival_periods_restatement as R
from tests import survival_pointwise_restatement as RP
from tests.test_survival_periods_cpu import _priors_logp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def reference(golden_dir):
    return R.load_fixture(golden_dir)


def _handle(N, T, P):
    y, e, x, period = R.make_case(N, T, P)
    return _native.SurvivalPeriods(y, e, x, period, P, R.PRIORS)


@pytest.mark.parametrize("N,T,P", R.SHAPES_POINTWISE)
def test_parity_with_the_40_digit_reference(reference, N, T, P):
    """Every ll_j finite and within C u S_j of the reference, C = R.c_device_pointwise(class of point) = 4 E_NP[class] of the
    pointwise table (fixed before the kernel ran), at every point, all points of a shape in one call; an individual with S_j = 0
    exactly 0.  sum_j ll_j against the data part of the device's own logp (logp minus the priors' closed form): within the two
    budgets added, C u sum_j S_j and C' u S_logp.  Measured on an MI355X, worst over the two shapes per class (against C):
    typical 2.18 (28), b_plus_50 3.32 (44), b_minus_50 3.96 (20), eta_800 3.43 (40), r_plus_800 4.01 (44), r_minus_800 2.56 (16),
    sd_e10 3.35 (28), sd_em10 2.94 (28), a_spread 3.67 (32)."""
    h = _handle(N, T, P)
    try:
        pts = np.stack([R.make_point(name, T, P) for name in R.POINTS])
        ll = h.individual_loglik(pts)
        lp, _ = h.logp_dlogp(pts)
        assert ll.shape == (len(R.POINTS), N)
        for row, name, q, logp in zip(ll, R.POINTS, pts, lp):
            key = f"N{N}_T{T}_P{P}_{name}"
            ref, S = reference[key + "/ll"], reference[key + "/ll_S"]
            assert np.isfinite(row).all(), key
            assert (row[S == 0] == 0).all() and (S == 0).any(), key
            worst = float((np.abs(row - ref)[S > 0] / S[S > 0] / R.U).max())
            total = abs(row.sum() - (logp - _priors_logp(q, T, P)))
            budget = R.U * (R.c_device_pointwise(name) * S.sum() + R.c_device(name) * float(reference[key + "/logp_S"]))
            print(f"{key}: worst {worst:.2f} u S_j (C = {R.c_device_pointwise(name):.0f}); |sum_j ll_j - data logp| = {total:.3g} (budget {budget:.3g})")
            assert worst <= R.c_device_pointwise(name), (key, worst)
            assert total <= budget, (key, total, budget)
    finally:
        h.close()


def test_bits_do_not_depend_on_the_launch():
    N, T, P = 130, 65, 65
    h = _handle(N, T, P)
    try:
        pts = np.stack([R.make_point(name, T, P, seed=s) for s in (0, 1) for name in R.POINTS[:8]])  # 16 points
        ll = h.individual_loglik(pts)
        np.testing.assert_array_equal(ll, h.individual_loglik(pts))
        assert np.isfinite(ll).all() and len(np.unique(ll[:, 0])) == 16
        for row in (0, 5, 15):
            np.testing.assert_array_equal(h.individual_loglik(pts[row])[0], ll[row])  # alone
            for at in (0, 7, 15):  # as row 0 / 7 / 15 of a 16-point launch among other points
                np.testing.assert_array_equal(h.individual_loglik(np.roll(pts, at - row, axis=0))[at], ll[row])
        both = h.individual_loglik(np.concatenate([pts[13:], pts]))  # 19 points: launches of 16 + 3
        np.testing.assert_array_equal(both, np.concatenate([ll[13:], ll]))
        assert h.individual_loglik(np.empty((0, h.dim))).shape == (0, N)
    finally:
        h.close()


@pytest.mark.parametrize("N,T,P", R.SHAPES_POINTWISE)
def test_waic_statistics_do_not_depend_on_the_batching(N, T, P):
    """19 draws that really differ (jittered typical points) folded in one call, in 19 calls, in 5 + 14, and again after a reset:
    the same bits.  Against compare.stats_from_matrix of the device's own (19, N) matrix: the bounds of
    tests/test_gpu_survival_pointwise.py for the same fold."""
    h = _handle(N, T, P)
    try:
        with pytest.raises(ValueError, match="no draws accumulated"):
            h.waic_stats()
        rng = np.random.default_rng(7)
        q = R.make_point("typical", T, P) + 0.1 * rng.normal(size=(19, h.dim))
        h.waic_accumulate(q)
        (lse, mean, m2, n), cells = h.waic_stats()
        assert n == 19
        np.testing.assert_array_equal(cells, RP.constants(R.model_of(N, T, P)[0])[1])
        h.waic_reset()
        for row in q:
            h.waic_accumulate(row)
        one_by_one = h.waic_stats()
        h.waic_reset()
        h.waic_accumulate(q[:5])
        h.waic_accumulate(q[5:])
        split = h.waic_stats()
        for (s2, c2) in (one_by_one, split):
            assert s2[3] == 19
            np.testing.assert_array_equal(c2, cells)
            for a, b in zip(s2[:3], (lse, mean, m2)):
                np.testing.assert_array_equal(a, b)
        ll = h.individual_loglik(q)
        r_lse, r_mean, r_m2, r_n = compare.stats_from_matrix(ll)
        assert (ll.std(axis=0)[cells > 0] > 1e-3).all()  # the draws differ
        assert (np.abs(lse - r_lse) <= 1e-12 * np.abs(r_lse)).all()
        assert (np.abs(mean - r_mean) <= 1e-12 * np.abs(r_mean)).all()
        assert (np.abs(m2 - r_m2) <= 1e-9 * r_m2).all()
        assert (mean[cells == 0] == 0).all() and (m2[cells == 0] == 0).all() and (cells == 0).any()
    finally:
        h.close()
