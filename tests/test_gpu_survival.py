"""
The survival evaluator on the device (abd_survival_*; abdpymc_amd.survival): parity with the 40-digit reference of
tests/golden/survival_reference_k1.npz / _k2.npz over the whole case table of tests/survival_restatement.py, bit-reproducibility, a NUTS
trajectory against the NumPy restatement, and one fit end to end on the golden cohort.
"""
import os

import numpy as np
import pytest

from abdpymc_amd import _native, survival
from abdpymc_amd.data import TiterData
from tests import survival_restatement as R
from tests.survival_restatement import _worst

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def reference(golden_dir):
    return R.load_fixtures(golden_dir)


def _handle(N, T, K):
    y, e, xs = R.make_data(N, T, K)
    return _native.Survival(y, e, xs, R.PRIORS[K])


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("N,T", R.SHAPES)
def test_parity_with_the_40_digit_reference(reference, N, T, K):
    """Every output of loglik_sums and logp_dlogp within C u S_k of the reference, C = R.c_device(class of point) = 4 E_np[class]
    (derived in DESIGN 19, not from the kernel's output), at all eight points of every shape; every output finite.  Measured on
    an MI355X, worst over the table per class (raw sums / logp / gradient, against C): typical 11.0 / 2.3 / 4.5 (44), b_plus_50
    319 / 3.0 / 4.2 (1096), b_minus_50 881 / 3.9 / 5.4 (2516), eta_800 962 / 5.1 / 4.7 (3228), r_plus_800 21.4 / 1.6 / 1.8 (72),
    r_minus_800 13.7 / 1.7 / 6.5 (56), sd_e10 15.1 / 1.5 / 14.8 (64), sd_em10 20.5 / 2.2 / 5.0 (88)."""
    h = _handle(N, T, K)
    try:
        assert h.dim == 2 * K + 2 + T
        for name in R.points_of(N, T):
            key = f"N{N}_T{T}_K{K}_{name}"
            q = R.make_point(name, T, K)
            sums = h.loglik_sums(q)
            lp, g = h.logp_dlogp(q)
            worst = {"sums": _worst(sums, reference[key + "/sums"], reference[key + "/sums_S"], key),
                     "logp": _worst(lp, reference[key + "/logp"], reference[key + "/logp_S"], key),
                     "grad": _worst(g, reference[key + "/grad"], reference[key + "/grad_S"], key)}
            print(key, {k: round(v, 2) for k, v in worst.items()})
            for what, v in worst.items():
                assert v <= R.c_device(name), (key, what, v, R.c_device(name))
    finally:
        h.close()


@pytest.mark.parametrize("N,T,K", [(1, 1, 1), (130, 65, 2), (1000, 199, 1), (1000, 199, 2), (67, 511, 2)])
def test_bits_do_not_depend_on_the_launch(N, T, K):
    h = _handle(N, T, K)
    try:
        pts = np.stack([R.make_point(name, T, K, seed=s) for s in (0, 1) for name in R.POINTS])  # 16 points
        lp, g = h.logp_dlogp(pts)
        lp2, g2 = h.logp_dlogp(pts)
        np.testing.assert_array_equal(lp, lp2)
        np.testing.assert_array_equal(g, g2)
        assert np.isfinite(lp).all() and np.isfinite(g).all()
        for row in (0, 5, 15):
            one_lp, one_g = h.logp_dlogp(pts[row])  # alone
            assert one_lp == lp[row]
            np.testing.assert_array_equal(one_g, g[row])
            for at in (0, 7, 15):  # as any row of a 16-point launch among other points
                mixed = np.roll(pts, at - row, axis=0)
                m_lp, m_g = h.logp_dlogp(mixed)
                assert m_lp[at] == lp[row]
                np.testing.assert_array_equal(m_g[at], g[row])
        both_lp, _ = h.logp_dlogp(np.concatenate([pts, pts[:3]]))  # 19 points: two launches
        np.testing.assert_array_equal(both_lp, np.concatenate([lp, lp[:3]]))
        np.testing.assert_array_equal(h.loglik_sums(pts[3]), h.loglik_sums(pts[3]))
    finally:
        h.close()


def _simulated(N=300, T=6, seed=3, a=1.5, b=2.0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 4.0, size=(N, T))
    lam0 = rng.uniform(0.15, 0.3, size=T)
    e = rng.uniform(0.3, 1.0, size=(N, T))
    y = rng.poisson(e * lam0[None, :] / (1.0 + np.exp(-b * (x - a)))).astype(np.float64)
    return y, e, [x]


# 25 transitions at step size 0.05 with the unit metric from the same seed.  Measured on an MI355X: every tree_depth and n_steps
# equal (depths 2 to 6), worst |q_device - q_restatement| / max |q| = TRAJ_MEASURED; the tolerance leaves a factor of about 150
# above it (on the CPU, an evaluator perturbed by 1e-15 relative noise deviates by 8e-16 over the same run: the dynamics do not
# amplify rounding here).
TRAJ_MEASURED = 6.4e-16
TRAJ_TOL = 1e-13


def test_trajectory_follows_the_restatement():
    y, e, xs = _simulated()
    h = _native.Survival(y, e, xs, R.PRIORS[1])
    try:
        rs = R.Restatement(y, e, xs)
        q0 = np.zeros(rs.dim)
        q0[2], q0[3] = -3.0, np.log(0.5)
        runs = [survival._chain(fn, rs.dim, 0, 25, np.random.default_rng(5), q0=q0, adapt=False, step_size=0.05)
                for fn in (h.logp_dlogp, rs.logp_dlogp)]
        (qd, sd), (qr, sr) = runs
        np.testing.assert_array_equal(sd["tree_depth"], sr["tree_depth"])
        np.testing.assert_array_equal(sd["n_steps"], sr["n_steps"])
        dev = float(np.abs(qd - qr).max() / np.abs(qr).max())
        print("trajectory: worst relative deviation", dev, "tree depths", sr["tree_depth"].tolist())
        assert sr["tree_depth"].max() >= 3  # the run builds real trees
        assert dev <= TRAJ_TOL
    finally:
        h.close()


def test_fit_of_the_golden_cohort_end_to_end(golden_dir):
    from abdpymc_amd.model import model
    from abdpymc_amd.sampler import sample

    data = TiterData.from_disk(os.path.join(golden_dir, "test_cohort"))
    m = model(data, n_chains=2)
    res = sample(m, tune=20, draws=20, chains=2, seed=1, record_deterministics=False, record_discrete=False)
    m.close()
    G = data.n_gaps
    sa = survival.SurvivalAnalysis(res, 0, G, data)
    assert sa.infected.shape == (data.n_inds, G - 1) and sa.n_int == G - 1
    sm = sa.model_combined()
    try:
        assert sm.dim == 6 + sa.n_int and len(sm.names) == sm.dim
        fit = survival.sample(sm, tune=100, draws=100, chains=2, seed=0)
    finally:
        sm.close()
    assert fit["a"].shape == (2, 100, 2) and fit["b"].shape == (2, 100, 2) and fit["lam0"].shape == (2, 100, sa.n_int)
    assert fit["stat_lp"].shape == (2, 100)
    for k, v in fit.items():
        if k != "antigens":
            assert np.isfinite(v).all(), k
    assert ((fit["lam0"] > 0) & (fit["lam0"] < 1)).all()
    for ag in ("S", "N"):
        p = survival.protection(fit, np.linspace(-2.0, 6.0, 9), antigen=ag)
        for k in ("mean", "median", "lower", "upper"):
            assert ((p[k] >= 0) & (p[k] <= 1)).all(), (ag, k)
    assert "survival: a[S]" in survival.report_line(fit)


def test_cli_fits_a_posterior_file(tmp_path, golden_dir, capsys):
    from abdpymc_amd.model import model
    from abdpymc_amd.sampler import sample

    cohort = os.path.join(golden_dir, "test_cohort")
    data = TiterData.from_disk(cohort)
    m = model(data, n_chains=2)
    res = sample(m, tune=20, draws=20, chains=2, seed=1, record_deterministics=False, record_discrete=False)
    m.close()
    post = tmp_path / "posterior.npz"
    np.savez(post, **{k: res[k] for k in ("mean_i", "mean_ab_s_mu", "mean_ab_n_mu")})
    out = tmp_path / "fit.npz"
    for which, K in (("combined", 2), ("s", 1)):
        rc = survival.main(["--posterior", str(post), "--ititers_data", cohort, "--start", "2", "--end", "20", "--model", which,
                            "--out", str(out), "--tune", "50", "--draws", "40", "--chains", "2"])
        assert rc == 0
        cap = capsys.readouterr()
        line = cap.out.splitlines()  # stdout holds the one line and nothing else
        assert len(line) == 1 and line[0].startswith("survival: ") and "wrote " in cap.err
        assert "a[S]" in line[0] and "b[S]" in line[0] and "at titer 0 / 2 / 4" in line[0] and "max R-hat of a, b" in line[0], cap.out
        assert ("a[N]" in line[0]) == (K == 2)
        with np.load(out) as f:
            assert f["a"].shape == ((2, 40, 2) if K == 2 else (2, 40)) and f["lam0"].shape == (2, 40, 17)
            assert list(f["intervals"]) == list(range(17)) and str(f["t0"]) == survival._month_add(data.t0, 3)
            assert np.isfinite(f["b"]).all() and f["stat_tree_depth"].shape == (2, 40)
    with pytest.raises(SystemExit):
        survival.main(["--posterior", str(post), "--ititers_data", cohort, "--start", "5", "--end", "6", "--model", "n", "--out", str(out)])
