"""
The survival evaluator by period on the device (abd_survival_create_periods; SurvivalAnalysis.model_alone_periods):
parity with the 40-digit reference of tests/golden/survival_periods_reference.npz over the case table of
tests/survival_periods_restatement.py, bit-reproducibility, the identity with the grouped handle of one group, a NUTS trajectory
against the NumPy restatement, fits of the golden cohort by era and by month compared with the plain fit end to end, and one run
of the command-line tool.
"""
import math
import os

import numpy as np
import pytest

from abdpymc_amd import _native, survival
from abdpymc_amd.data import TiterData
from tests import survival_groups_restatement as RG
from tests import survival_periods_restatement as R
from tests.survival_restatement import _worst
from tests.test_gpu_survival_groups import TRAJ_TOL
from tests.test_survival_periods_cpu import SIM, simulate

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def reference(golden_dir):
    return R.load_fixture(golden_dir)


def _handle(N, T, P):
    y, e, x, period = R.make_case(N, T, P)
    return _native.SurvivalPeriods(y, e, x, period, P, R.PRIORS)


@pytest.mark.parametrize("N,T,P", R.SHAPES)
def test_parity_with_the_40_digit_reference(reference, N, T, P):
    """Every output of loglik_sums and logp_dlogp finite and within C u S_k of the reference, C = R.c_device(class of point)
    = 4 E_NP_PERIODS[class] (fixed before the kernel ran), at all nine points of every shape; an output with S_k = 0 (an interval
    without follow-up, a period without intervals) exactly 0.  Measured on an MI355X, worst over the table per class
    (raw sums / logp / gradient, against C): typical 5.4 / 1.5 / 3.7 (24), b_plus_50 182.3 / 1.4 / 2.2 (860), b_minus_50
    174.7 / 3.0 / 3.8 (948), eta_800 411.1 / 1.3 / 106.1 (1312), r_plus_800 4.5 / 1.6 / 1.8 (16), r_minus_800 5.4 / 1.5 / 3.8 (24),
    sd_e10 5.6 / 1.5 / 4.8 (28), sd_em10 5.5 / 1.3 / 2.7 (28), a_spread 40.6 / 1.1 / 3.8 (288)."""
    h = _handle(N, T, P)
    try:
        assert h.dim == T + P + 5
        for name in R.POINTS:
            key = f"N{N}_T{T}_P{P}_{name}"
            q = R.make_point(name, T, P)
            sums = h.loglik_sums(q)
            lp, g = h.logp_dlogp(q)
            assert sums.shape == (2 * T + 2,)
            worst = {"sums": _worst(sums, reference[key + "/sums"], reference[key + "/sums_S"], key),
                     "logp": _worst(lp, reference[key + "/logp"], reference[key + "/logp_S"], key),
                     "grad": _worst(g, reference[key + "/grad"], reference[key + "/grad_S"], key)}
            print(key, {k: round(v, 2) for k, v in worst.items()})
            for what, v in worst.items():
                assert v <= R.c_device(name), (key, what, v, R.c_device(name))
    finally:
        h.close()


@pytest.mark.parametrize("N,T,P", [(1, 1, 1), (130, 65, 65), (67, 511, 4), (2100, 129, 4)])
def test_bits_do_not_depend_on_the_launch(N, T, P):
    h = _handle(N, T, P)
    try:
        pts = np.stack([R.make_point(name, T, P, seed=s) for s in (0, 1) for name in R.POINTS[:8]])  # 16 points
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


@pytest.mark.parametrize("N,T,P", [(67, 30, 3), (130, 65, 65), (2100, 129, 4)])
def test_equal_midpoints_are_the_grouped_model_with_one_group(N, T, P):
    """At points whose _a_z are all equal every interval reads the same a, as the grouped handle of the same data with one group
    does: S_t, L and W_x are the same bits (the same cell function, tiles, ranges and finalize order), and sum_t W0_t agrees with
    the group's W0_0 within the device budget C u S -- C = 4 E_np[class], the smaller of this model's and the grouped model's
    (16 to 1300); S = the sum of |addends| of W0 over all cells (float64, from the restatement's arrays).  Measured on an
    MI355X: the bits of S_t, L and W_x equal at all 27 points; the two W0 differ by at most 1.95 u S."""
    y, e, x, period = R.make_case(N, T, P)
    hp = _native.SurvivalPeriods(y, e, x, period, P, R.PRIORS)
    hg = _native.SurvivalGroups(y, e, x, np.zeros(N, dtype=np.int32), 1, R.PRIORS)
    rs = R.PeriodsRestatement(y, e, x, period, P)
    try:
        for name in R.POINTS:
            q = R.make_point(name, T, P)
            q[T + 4:T + 4 + P] = q[T + 4]  # all _a_z equal
            qg = np.concatenate([q[:T + 5], [q[T + 4 + P]]])
            sp, sg = hp.loglik_sums(q), hg.loglik_sums(qg)
            np.testing.assert_array_equal(sp[:T + 2], sg[:T + 2], err_msg=name)
            m, s, z, a_mu, a_sl, az, b = rs.split(q)
            with np.errstate(over="ignore", under="ignore"):
                eta = b * (rs.x - rs.a_t(q)[None, :])
                sig, oms = R._invlogit(eta), R._invlogit(-eta)
                S = float((rs.y * oms).sum() + (R._invlogit(m + np.exp(s) * z)[None, :] * rs.e * sig * oms).sum())
            diff = abs(math.fsum(sp[T + 2:]) - sg[T + 2])
            budget = min(R.c_device(name), RG.c_device(name))
            print(f"N{N}_T{T}_P{P}_{name}: |sum_t W0_t - W0_0| = {diff / (R.U * S) if S else 0.0:.2f} u S (C = {budget:.0f})")
            assert diff <= budget * R.U * S, name
    finally:
        hp.close()
        hg.close()


# 25 transitions at step size 0.05 with the unit metric from the same seed, on the simulated cohort of
# tests/test_survival_periods_cpu.py (N 400, T 8, two eras).  TRAJ_TOL is that of tests/test_gpu_survival_groups.py; measured on an
# MI355X: TRAJ_MEASURED, every tree_depth and n_steps equal (depths 3 to 6).
TRAJ_MEASURED = 5.9e-15


def trajectory(fn, dim, T, P):
    q0 = survival.initial_point_groups(T, P, survival.PRIORS_PERIODS)
    return survival._chain(fn, dim, 0, 25, np.random.default_rng(5), q0=q0, adapt=False, step_size=0.05)


def test_trajectory_follows_the_restatement():
    y, e, x, period, _ = simulate(**SIM)
    T = SIM["T"]
    h = _native.SurvivalPeriods(y, e, x, period, 2, R.PRIORS)
    try:
        rs = R.PeriodsRestatement(y, e, x, period, 2)
        (qd, sd), (qr, sr) = (trajectory(fn, rs.dim, T, 2) for fn in (h.logp_dlogp, rs.logp_dlogp))
        np.testing.assert_array_equal(sd["tree_depth"], sr["tree_depth"])
        np.testing.assert_array_equal(sd["n_steps"], sr["n_steps"])
        dev = float(np.abs(qd - qr).max() / np.abs(qr).max())
        print("trajectory: worst relative deviation", dev, "tree depths", sr["tree_depth"].tolist())
        assert sr["tree_depth"].max() >= 3  # the run builds real trees
        assert dev <= TRAJ_TOL
    finally:
        h.close()


@pytest.fixture(scope="module")
def golden_fits(golden_dir):
    """The golden cohort's posterior means, and three fits of its whole window at tune 100, draws 100, 2 chains, each scored by
    WAIC on the device: the plain S model, S by era (periods_from_splits) and S by month."""
    from abdpymc_amd.model import model
    from abdpymc_amd.sampler import sample

    data = TiterData.from_disk(os.path.join(golden_dir, "test_cohort"))
    m = model(data, n_chains=2)
    res = sample(m, tune=20, draws=20, chains=2, seed=1, record_deterministics=False, record_discrete=False)
    m.close()
    sa = survival.SurvivalAnalysis(res, 0, data.n_gaps, data)
    eras = sa.periods_from_splits(data.calculate_splits(delta=True, omicron=True))
    models = {"S": sa.model_alone("S"), "S by era": sa.model_alone_periods("S", eras, "era"), "S by month": sa.model_alone_periods("S")}
    fits, scores = {}, {}
    try:
        for name, sm in models.items():
            fits[name] = survival.sample(sm, tune=100, draws=100, chains=2, seed=0)
            scores[name] = survival.waic(sm, fits[name])
        shapes = {name: (sm.dim, len(sm.names), sm.loglik_sums(np.zeros(sm.dim)).shape) for name, sm in models.items()}
    finally:
        for sm in models.values():
            sm.close()
    return data, res, sa, eras, fits, scores, shapes


def test_fits_of_the_golden_cohort_by_era_and_by_month(golden_fits):
    data, res, sa, eras, fits, scores, shapes = golden_fits
    T = sa.n_int
    assert T == 25 and eras.tolist() == [0] * 13 + [1] * 6 + [2] * 6  # the gaps 1 .. 25 against the splits 14 and 20
    for name, P, labels, pname in (("S by era", 3, [0, 1, 2], "era"), ("S by month", T, list(range(T)), "intervals")):
        fit = fits[name]
        assert shapes[name] == (T + P + 5, T + P + 5, (2 * T + 2,))
        assert fit["a"].shape == (2, 100, P) and fit["b"].shape == (2, 100) and fit["lam0"].shape == (2, 100, T)
        assert fit["a_mu"].shape == (2, 100) and fit["a_sd"].shape == (2, 100) and fit[f"_a_z_{P - 1}"].shape == (2, 100)
        assert list(fit["periods"]) == labels and str(fit["period_name"]) == pname
        assert fit["period_index"].tolist() == (eras.tolist() if P == 3 else list(range(T)))
        for k, v in fit.items():
            if k not in ("antigens", "periods", "period_name"):
                assert np.isfinite(v).all(), (name, k)
        assert ((fit["lam0"] > 0) & (fit["lam0"] < 1)).all() and (fit["a_sd"] > 0).all()
        np.testing.assert_array_equal(fit["a"][..., 1], fit["a_mu"] + fit["a_sd"] * fit["_a_z_1"])
        x = np.linspace(-2.0, 6.0, 9)
        for label in labels:
            p = survival.protection(fit, x, period=label)
            for k in ("mean", "median", "lower", "upper"):
                assert ((p[k] >= 0) & (p[k] <= 1)).all(), (name, label, k)
        np.testing.assert_array_equal(survival.protection(fit, x, interval=T - 1)["median"], survival.protection(fit, x, period=labels[-1])["median"])
        assert survival.summary(fit)["a"]["rhat"].shape == (P,)
        assert f"survival: a[S, {pname} 0]" in survival.report_line(fit)


def test_waic_and_compare_give_a_table(golden_fits):
    data, res, sa, eras, fits, scores, shapes = golden_fits
    for name, w in scores.items():
        assert np.isfinite(w["elpd_waic"]) and w["elpd_i"].shape == (data.n_inds,) and w["n_draws"] == 200, name
        assert int(fits[name]["start"]) == 0 and int(fits[name]["end"]) == data.n_gaps
    table = survival.compare(fits)
    print("\n".join(survival.compare_lines(table)))
    assert sorted(v["rank"] for v in table.values()) == [0, 1, 2] and set(table) == {"S", "S by era", "S by month"}
    for v in table.values():
        assert all(np.isfinite(v[k]) for k in ("elpd_waic", "p_waic", "se", "elpd_diff", "dse"))


def test_cli_fits_a_model_by_era(tmp_path, golden_dir, golden_fits, capsys):
    data, res = golden_fits[:2]
    cohort = os.path.join(golden_dir, "test_cohort")
    post = tmp_path / "posterior.npz"
    np.savez(post, **{k: res[k] for k in ("mean_i", "mean_ab_s_mu", "mean_ab_n_mu")})
    out = tmp_path / "fit.npz"
    rc = survival.main(["--posterior", str(post), "--ititers_data", cohort, "--start", "2", "--end", "24", "--model", "s_periods",
                        "--periods", "splits", "--split_delta", "--split_omicron", "--period_name", "era", "--waic", "--out", str(out),
                        "--tune", "50", "--draws", "40", "--chains", "2"])
    assert rc == 0
    cap = capsys.readouterr()
    line = cap.out.splitlines()  # stdout holds the one line and the WAIC line, nothing else
    assert len(line) == 2 and line[0].startswith("survival: a[S, era 0] ") and line[1].startswith("survival WAIC: ") and "wrote " in cap.err
    assert "a[S, era 2] " in line[0] and line[0].count("b[S] ") == 1 and line[0].count("at titer 0 / 2 / 4") == 3
    assert "max R-hat of a, b" in line[0]
    with np.load(out) as f:
        assert f["a"].shape == (2, 40, 3) and f["b"].shape == (2, 40) and f["lam0"].shape == (2, 40, 21)
        assert list(f["periods"]) == [0, 1, 2] and str(f["period_name"]) == "era"
        # the intervals cover the gaps 3 .. 23; the splits are the gaps 14 and 20
        assert f["period_index"].tolist() == [0] * 11 + [1] * 6 + [2] * 4
        assert list(f["intervals"]) == list(range(21)) and np.isfinite(f["a"]).all() and f["elpd_waic_ind"].shape == (data.n_inds,)
    capsys.readouterr()
    assert survival.main(["--compare", str(out)]) == 0  # --compare reads the new fit
    assert capsys.readouterr().out.startswith("fit  rank 0 ")
