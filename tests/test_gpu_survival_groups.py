"""
The grouped survival evaluator on the device (abd_survival_create_groups; SurvivalAnalysis.model_alone_groups): parity
with the 40-digit reference of tests/golden/survival_groups_reference.npz over the case table of
tests/survival_groups_restatement.py, bit-reproducibility, the ungrouped kernel as a yardstick at Gr = 1, a NUTS trajectory against
the NumPy restatement, one fit end to end on the golden cohort and one run of the command-line tool.
"""
import os

import numpy as np
import pytest

from abdpymc_amd import _native, survival
from abdpymc_amd.data import TiterData
from tests import survival_groups_restatement as R
from tests import survival_restatement as R1
from tests.survival_restatement import _worst
from tests.test_survival_groups_cpu import simulate

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def reference(golden_dir):
    return R.load_fixture(golden_dir)


def _handle(N, T, Gr):
    y, e, x, group = R.make_case(N, T, Gr)
    return _native.SurvivalGroups(y, e, x, group, Gr, R.PRIORS)


@pytest.mark.parametrize("N,T,Gr", R.SHAPES)
def test_parity_with_the_40_digit_reference(reference, N, T, Gr):
    """Every output of loglik_sums and logp_dlogp finite and within C u S_k of the reference, C = R.c_device(class of point)
    = 4 E_NP_GROUPS[class] (fixed before the kernel ran), at all nine points of every shape; an output with S_k = 0 (an empty
    group, a group or an interval without follow-up) exactly 0.  Measured on an MI355X, worst over the table per class
    (raw sums / logp / gradient, against C): typical 1.1 / 0.0 / 0.4 (16), b_plus_50 153.8 / 2.3 / 2.7 (860), b_minus_50
    133.2 / 1.6 / 13.2 (840), eta_800 423.9 / 1.8 / 424.0 (1300), r_plus_800 3.9 / 1.6 / 2.6 (20), r_minus_800 6.6 / 1.6 / 3.1 (24),
    sd_e10 3.1 / 0.0 / 3.4 (24), sd_em10 5.7 / 1.3 / 4.2 (16), a_spread 7.5 / 1.8 / 2.1 (20)."""
    h = _handle(N, T, Gr)
    try:
        assert h.dim == T + Gr + 5
        for name in R.POINTS:
            key = f"N{N}_T{T}_G{Gr}_{name}"
            q = R.make_point(name, T, Gr)
            sums = h.loglik_sums(q)
            lp, g = h.logp_dlogp(q)
            assert sums.shape == (T + 2 + Gr,)
            worst = {"sums": _worst(sums, reference[key + "/sums"], reference[key + "/sums_S"], key),
                     "logp": _worst(lp, reference[key + "/logp"], reference[key + "/logp_S"], key),
                     "grad": _worst(g, reference[key + "/grad"], reference[key + "/grad_S"], key)}
            print(key, {k: round(v, 2) for k, v in worst.items()})
            for what, v in worst.items():
                assert v <= R.c_device(name), (key, what, v, R.c_device(name))
    finally:
        h.close()


@pytest.mark.parametrize("N,T,Gr", [(1, 1, 1), (130, 65, 4), (1000, 199, 5)])
def test_bits_do_not_depend_on_the_launch(N, T, Gr):
    h = _handle(N, T, Gr)
    try:
        pts = np.stack([R.make_point(name, T, Gr, seed=s) for s in (0, 1) for name in R.POINTS[:8]])  # 16 points
        lp, g = h.logp_dlogp(pts)
        lp2, g2 = h.logp_dlogp(pts)
        np.testing.assert_array_equal(lp, lp2)
        np.testing.assert_array_equal(g, g2)
        assert np.isfinite(lp).all() and np.isfinite(g).all()
        for row in (0, 5, 15):
            one_lp, one_g = h.logp_dlogp(pts[row])  # alone
            assert one_lp == lp[row]
            np.testing.assert_array_equal(one_g, g[row])
            for at in (0, 7, 15):  # as row 0 / 7 / 15 of a 16-point launch among other points
                mixed = np.roll(pts, at - row, axis=0)
                m_lp, m_g = h.logp_dlogp(mixed)
                assert m_lp[at] == lp[row]
                np.testing.assert_array_equal(m_g[at], g[row])
        both_lp, both_g = h.logp_dlogp(np.concatenate([pts, pts[:3]]))  # 19 points: two launches
        np.testing.assert_array_equal(both_lp, np.concatenate([lp, lp[:3]]))
        np.testing.assert_array_equal(both_g, np.concatenate([g, g[:3]]))
        np.testing.assert_array_equal(h.loglik_sums(pts[3]), h.loglik_sums(pts[3]))
    finally:
        h.close()


@pytest.mark.parametrize("N,T", [(67, 30), (1000, 199)])
def test_one_group_is_the_ungrouped_model(N, T):
    """Gr = 1 with the same data and the same a: S_t, L, W_x and W0 within the budget that holds for the ungrouped kernel's S_t, L,
    W_1, W_0 -- C u S_k of the ungrouped 40-digit fixture, C = 4 E_NP[class] of tests/survival_restatement.py.  Whether the two
    kernels' sums are bit-equal is printed, not asserted; measured on an MI355X: equal at 5 of these 16 points (S_t, L and W_x
    are summed in one order by both, W0 over the waves in another)."""
    ref = R1.load_fixtures(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    y, e, (x,) = R1.make_data(N, T, 1)
    h1 = _native.Survival(y, e, [x], R1.PRIORS[1])
    hg = _native.SurvivalGroups(y, e, x, np.zeros(N, dtype=np.int32), 1, R.PRIORS)
    try:
        for name in R1.POINTS:
            q1 = R1.make_point(name, T, 1)  # a, b, m, s, z
            a, b = q1[0], q1[1]
            qg = np.concatenate([q1[2:], [a, -30.0, 0.0], [b]])  # a_mu = a, _a_z = 0: a_g = a exactly
            s1, sg = h1.loglik_sums(q1), hg.loglik_sums(qg)
            order = np.concatenate([np.arange(T + 1), [T + 2, T + 1]])  # S_t, L, W_1 (= W_x), W_0: the grouped order
            truth, S = ref[f"N{N}_T{T}_K1_{name}/sums"][order], ref[f"N{N}_T{T}_K1_{name}/sums_S"][order]
            print(f"N{N}_T{T}_{name}: bit-equal to the ungrouped sums {bool((s1[order] == sg).all())}")
            for got in (sg, s1[order]):
                assert _worst(got, truth, S, name) <= R1.c_device(name), name
    finally:
        h1.close()
        hg.close()


# 25 transitions at step size 0.05 with the unit metric from the same seed, on data simulated from the grouped model (N 300, T 6,
# Gr 3).  On the CPU, the restatement against itself with 1e-15 relative noise on logp and gradient deviates by TRAJ_NOISE over the
# same run (worst |q - q'| / max |q|): the dynamics do not amplify rounding here.  TRAJ_TOL allows about 100 times that, as DESIGN 19
# set its TRAJ_TOL; measured on an MI355X: TRAJ_MEASURED, every tree_depth and n_steps equal (depths 3 to 6).
TRAJ_NOISE = 1.4e-15
TRAJ_MEASURED = 1.7e-15
TRAJ_TOL = 1.5e-13
TRAJ_SIM = dict(N=300, T=6, seed=3, a=(0.5, 1.5, 2.5), b=2.0)


def trajectory(fn, dim, T, Gr):
    return survival._chain(fn, dim, 0, 25, np.random.default_rng(5), q0=survival.initial_point_groups(T, Gr), adapt=False, step_size=0.05)


def test_trajectory_follows_the_restatement():
    y, e, x, group = simulate(**TRAJ_SIM)
    h = _native.SurvivalGroups(y, e, x, group, 3, R.PRIORS)
    try:
        rs = R.GroupsRestatement(y, e, x, group, 3)
        (qd, sd), (qr, sr) = (trajectory(fn, rs.dim, 6, 3) for fn in (h.logp_dlogp, rs.logp_dlogp))
        np.testing.assert_array_equal(sd["tree_depth"], sr["tree_depth"])
        np.testing.assert_array_equal(sd["n_steps"], sr["n_steps"])
        dev = float(np.abs(qd - qr).max() / np.abs(qr).max())
        print("trajectory: worst relative deviation", dev, "tree depths", sr["tree_depth"].tolist())
        assert sr["tree_depth"].max() >= 3  # the run builds real trees
        assert dev <= TRAJ_TOL
    finally:
        h.close()


def _posterior_means(golden_dir):
    from abdpymc_amd.model import model
    from abdpymc_amd.sampler import sample

    data = TiterData.from_disk(os.path.join(golden_dir, "test_cohort"))
    m = model(data, n_chains=2)
    res = sample(m, tune=20, draws=20, chains=2, seed=1, record_deterministics=False, record_discrete=False)
    m.close()
    return data, res


def test_fit_of_the_golden_cohort_end_to_end(golden_dir):
    data, res = _posterior_means(golden_dir)
    G, N = data.n_gaps, data.n_inds
    sa = survival.SurvivalAnalysis(res, 0, G, data)
    sm = sa.model_alone_groups("S", np.arange(N) % 3)
    try:
        assert sm.dim == sa.n_int + 3 + 5 and len(sm.names) == sm.dim and list(sm.groups) == [0, 1, 2] and sm.group_name == "group"
        q0 = sm.initial_point()
        lp, g = sm.logp_dlogp(q0)
        assert np.isfinite(lp) and np.isfinite(g).all() and sm.loglik_sums(q0).shape == (sa.n_int + 2 + 3,)
        fit = survival.sample(sm, tune=100, draws=100, chains=2, seed=0)
    finally:
        sm.close()
    assert fit["a"].shape == (2, 100, 3) and fit["b"].shape == (2, 100) and fit["lam0"].shape == (2, 100, sa.n_int)
    assert fit["a_mu"].shape == (2, 100) and fit["a_sd"].shape == (2, 100) and fit["_a_z_1"].shape == (2, 100)
    assert list(fit["groups"]) == [0, 1, 2] and str(fit["group_name"]) == "group"
    for k, v in fit.items():
        if k not in ("antigens", "groups", "group_name"):
            assert np.isfinite(v).all(), k
    assert ((fit["lam0"] > 0) & (fit["lam0"] < 1)).all() and (fit["a_sd"] > 0).all()
    np.testing.assert_array_equal(fit["a"][..., 1], fit["a_mu"] + fit["a_sd"] * fit["_a_z_1"])
    for label in (0, 1, 2):
        p = survival.protection(fit, np.linspace(-2.0, 6.0, 9), group=label)
        for k in ("mean", "median", "lower", "upper"):
            assert ((p[k] >= 0) & (p[k] <= 1)).all(), (label, k)
    assert survival.summary(fit)["a"]["rhat"].shape == (3,)
    assert "survival: a[S, group 0]" in survival.report_line(fit)


def test_cli_fits_a_grouped_model(tmp_path, golden_dir, capsys):
    data, res = _posterior_means(golden_dir)
    cohort = os.path.join(golden_dir, "test_cohort")
    post = tmp_path / "posterior.npz"
    np.savez(post, **{k: res[k] for k in ("mean_i", "mean_ab_s_mu", "mean_ab_n_mu")})
    labels = tmp_path / "arms.txt"
    labels.write_text("\n".join("vaccinated" if j % 3 else "not" for j in range(data.n_inds)) + "\n")
    out = tmp_path / "fit.npz"
    rc = survival.main(["--posterior", str(post), "--ititers_data", cohort, "--start", "2", "--end", "20", "--model", "s_groups",
                        "--groups", str(labels), "--group_name", "arm", "--out", str(out), "--tune", "50", "--draws", "40", "--chains", "2"])
    assert rc == 0
    cap = capsys.readouterr()
    line = cap.out.splitlines()  # stdout holds the one line and nothing else
    assert len(line) == 1 and line[0].startswith("survival: a[S, arm not] ") and "wrote " in cap.err
    assert "a[S, arm vaccinated] " in line[0] and line[0].count("b[S] ") == 1 and line[0].count("at titer 0 / 2 / 4") == 2
    assert "max R-hat of a, b" in line[0]
    with np.load(out) as f:
        assert f["a"].shape == (2, 40, 2) and f["b"].shape == (2, 40) and f["lam0"].shape == (2, 40, 17)
        assert list(f["groups"]) == ["not", "vaccinated"] and str(f["group_name"]) == "arm"
        assert list(f["intervals"]) == list(range(17)) and np.isfinite(f["a"]).all()
