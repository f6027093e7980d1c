"""
The posterior predictive checks of the survival models on the device (abd_survival_predictive_*, abd_survival_replicate;
survival.predictive / sample_posterior_predictive): the expected tables against the 40-digit reference of
tests/golden/survival_predictive_reference.npz, the per-cell replicates against the restatement's exactly, bit-reproducibility
however the draws are batched, the refusals, and the check end to end from Python and from the command line.
"""
import os

import numpy as np
import pytest

from abdpymc_amd import _native, survival
from abdpymc_amd.data import TiterData
from tests import survival_groups_restatement as RG
from tests import survival_periods_restatement as RP
from tests import survival_predictive_restatement as R
from tests import survival_restatement as R1
from tests.test_survival_predictive_cpu import check_statements, fit_and_check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def reference(golden_dir):
    return R.load_fixture(golden_dir)


def _handle(made):
    if made[0] == "k":
        _, y, e, xs = made
        return _native.Survival(y, e, xs, R1.PRIORS[len(xs)])
    if made[0] == "groups":
        _, y, e, x, group, Gr = made
        return _native.SurvivalGroups(y, e, x, group, Gr, RG.PRIORS)
    _, y, e, x, period, P = made
    return _native.SurvivalPeriods(y, e, x, period, P, RP.PRIORS)


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.tag)
def test_expected_tables_against_the_40_digit_reference(reference, shape):
    """Every E[v][b] finite and within C u E of the reference, C = R.c_device(class of point) = 4 E_NP[class] (fixed before the kernel
    ran), at every point of every shape, all points of a shape in one call; a bin without followed cells (and every bin at
    r_minus_800, where lambda underflows) exactly 0.  (67, 511), the longest walk, is in this test only.  Measured on an MI355X,
    worst over the table per class (against C): typical 6.02 (28), b_plus_50 129.7 (408), b_minus_50 228.3 (1040), eta_800 775.7
    (3004), r_plus_800 5.75 (44), r_minus_800 0 (4), sd_e10 5.03 (24), sd_em10 5.11 (24), a_spread 2.73 (16)."""
    rs, made, variables, edges = R.model_of(shape)
    names = R.points_of(shape)
    cells = R.constants(rs, variables, edges)[2]
    h = _handle(made)
    try:
        h.predictive_configure(variables, edges, seed=0)
        E, Rr = h.predictive_accumulate(np.stack([R.point_of(shape, name) for name in names]))
        assert E.shape == Rr.shape == (len(names), len(variables), 8)
        for row, rrow, name in zip(E, Rr, names):
            ref = reference[f"{R.tag(shape)}_{name}/E"]
            assert np.isfinite(row).all() and (row[ref == 0] == 0).all() and (row[cells == 0] == 0).all() and (rrow[cells == 0] == 0).all(), name
            m = ref > 0
            worst = float((np.abs(row - ref)[m] / ref[m] / R.U).max()) if m.any() else 0.0
            print(f"{R.tag(shape)}_{name}: worst {worst:.2f} u E (C = {R.c_device(name):.0f})")
            assert worst <= R.c_device(name), (name, worst)
        obs, pt, n_cells, obs_i = h.predictive_observed()
        O, PT, _, O_j = R.constants(rs, variables, edges)
        np.testing.assert_array_equal(n_cells, cells)
        for a, b in ((obs, O), (pt, PT), (obs_i, O_j)):
            assert (np.abs(a - b) <= 2 * R.U * np.abs(b)).all()
    finally:
        h.close()


@pytest.mark.parametrize("case", R.REPLICATE_CASES, ids=lambda c: R.tag(c[0]))
def test_replicates_equal_the_restatements(reference, case):
    """replicate() gives the fixture's per-cell replicates exactly (no boundary cell in any case: tests/test_survival_predictive_cpu.py),
    in the caller's order also where the grouped layout reorders the individuals: the key is the caller's index.  The bin sums and
    the per-individual sums of predictive_accumulate for the same draw indices are the sums of those matrices."""
    shape, seed, draw0 = case
    rs, made, variables, edges = R.model_of(shape)
    want = reference[f"{R.tag(shape)}_rep/r"].astype(np.int64)
    pts = np.stack([R.point_of(shape, name) for name in R.REPLICATE_POINTS])
    bins = R.bins_of(rs, variables, edges)
    h = _handle(made)
    try:
        h.predictive_configure(variables, edges, seed=seed)
        got = h.replicate(pts, draw0=draw0)
        assert got.dtype == np.int32 and got.shape == (3,) + rs.y.shape
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(h.replicate(pts[2], draw0=draw0 + 2)[0], want[2])  # alone
        before = np.zeros(rs.N, np.int64), np.zeros(rs.N, np.int64)
        if draw0:  # the draws before draw0: any points
            h.predictive_accumulate(np.repeat(pts[:1], draw0, axis=0))
            before = h.predictive_stats()[1:3]
        E, Rr = h.predictive_accumulate(pts)
        sum_e, sum_r, n_pos, n = h.predictive_stats()
        assert n == draw0 + 3
        for v in range(len(variables)):
            np.testing.assert_array_equal(Rr[:, v], np.stack([want[:, bins[v] == b].sum(axis=1) for b in range(8)], axis=1))
        np.testing.assert_array_equal(sum_r - before[0], want.sum(axis=(0, 2)))
        np.testing.assert_array_equal(n_pos - before[1], (want.sum(axis=2) >= 1).sum(axis=0))
    finally:
        h.close()


@pytest.mark.parametrize("shape", [("k", 130, 65, 2), ("groups", 130, 65, 4), ("periods", 130, 65, 3)], ids=R.tag)
def test_bits_do_not_depend_on_the_launch(shape):
    """19 draws that differ, folded in one call, one by one, and as 5 + 14 after a reset: expected, replicate and the three
    accumulators have the same bits.  A draw alone is row 0, 7 and 15 of a 16-point launch given the same draw index.  Another seed
    changes the replicates and leaves expected bit-identical.  sum_e is the running sum of the device's own E_j rows in ascending
    draw order (tests/test_gpu_survival_pointwise.py's bound for a running sum in a fixed order: 1e-12 relative)."""
    rs, made, variables, edges = R.model_of(shape)
    h = _handle(made)
    try:
        q = R.point_of(shape, "typical") + 0.1 * np.random.default_rng(7).normal(size=(19, h.dim))
        h.predictive_configure(variables, edges, seed=3)
        E, Rr = h.predictive_accumulate(q)
        stats = h.predictive_stats()
        assert stats[3] == 19 and len(np.unique(E[:, 0, 3])) == 19 and Rr.sum() > 0
        h.predictive_reset()
        with pytest.raises(ValueError, match="no draws accumulated"):
            h.predictive_stats()
        one = [h.predictive_accumulate(row) for row in q]
        ways = [(np.concatenate([o[0] for o in one]), np.concatenate([o[1] for o in one]), h.predictive_stats())]
        h.predictive_reset()
        a, b = h.predictive_accumulate(q[:5]), h.predictive_accumulate(q[5:])
        ways.append((np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]]), h.predictive_stats()))
        for E2, R2, s2 in ways:
            np.testing.assert_array_equal(E2, E)
            np.testing.assert_array_equal(R2, Rr)
            assert s2[3] == 19
            for x, y in zip(s2[:3], stats[:3]):
                np.testing.assert_array_equal(x, y)
        # a draw alone against rows of a 16-point launch
        cells = h.replicate(q[:16], draw0=0)
        for at in (0, 7, 15):
            h.predictive_reset()
            if at:
                h.predictive_accumulate(q[:at])
            alone = h.predictive_accumulate(q[at])
            np.testing.assert_array_equal(alone[0][0], E[at])
            np.testing.assert_array_equal(alone[1][0], Rr[at])
            np.testing.assert_array_equal(h.replicate(q[at], draw0=at)[0], cells[at])
        # sum_e: the running sum of the E_j rows, each read back as the accumulator after one draw
        rows = []
        for row in q:
            h.predictive_reset()
            h.predictive_accumulate(row)
            rows.append(h.predictive_stats()[0])
        run = np.zeros(rs.N)
        for row in rows:
            run = run + row
        assert (np.abs(stats[0] - run) <= 1e-12 * np.abs(run)).all() and (stats[0][rs.e.sum(axis=1) == 0] == 0).all()
        np.testing.assert_allclose(np.array(rows).sum(axis=1), E[:, 0].sum(axis=1), rtol=1e-12)
        # another seed
        h.predictive_configure(variables, edges, seed=4)
        E4, R4 = h.predictive_accumulate(q)
        np.testing.assert_array_equal(E4, E)
        assert (R4 != Rr).any() and (h.replicate(q[:16]) != cells).any()
        np.testing.assert_array_equal(h.predictive_stats()[0], stats[0])
    finally:
        h.close()


def test_refusals_leave_the_handle_usable():
    shape = ("k", 65, 3, 2)
    rs, made, variables, edges = R.model_of(shape)
    q = R.point_of(shape, "typical")
    h = _handle(made)
    try:
        for call in (lambda: h.predictive_accumulate(q), h.predictive_stats, h.predictive_observed, lambda: h.replicate(q)):
            with pytest.raises(ValueError, match="abd_survival_predictive_configure comes first"):
                call()
        j, t = np.argwhere(rs.e > 0)[7]
        bad = [v.copy() for v in variables]
        bad[0][j, t] = np.nan
        for titers, ed, msg in ((variables + variables[:1], edges + edges[:1], "one or two binning variables"), ([], [], "one or two binning variables"),
                                (variables, [edges[0], list(range(8))], "at most 7 edges"), (variables, [edges[0], [0.0, np.inf]], "edges must be finite"),
                                (variables, [[1.0, 1.0], edges[1]], "strictly ascending"), (variables, [[2.0, 1.0], edges[1]], "strictly ascending"),
                                (bad, edges, f"individual {j}, interval {t}: binning titer of a followed cell must be finite")):
            with pytest.raises(ValueError, match=msg):
                h.predictive_configure(titers, ed)
        h.predictive_configure(variables, edges, seed=1)
        with pytest.raises(ValueError, match="no draws accumulated"):
            h.predictive_stats()
        first = h.predictive_accumulate(q)
        with pytest.raises(ValueError, match="strictly ascending"):  # a refused reconfiguration leaves the earlier one standing
            h.predictive_configure(variables, [[2.0, 1.0], edges[1]])
        h.predictive_reset()
        again = h.predictive_accumulate(q)
        np.testing.assert_array_equal(again[0], first[0])
        np.testing.assert_array_equal(again[1], first[1])
        assert h.predictive_accumulate(np.empty((0, h.dim)))[0].shape == (0, 2, 8) and h.replicate(np.empty((0, h.dim))).shape == (0, 65, 3)
        with pytest.raises(ValueError, match="negative"):
            h.replicate(q, draw0=-1)
    finally:
        h.close()
    y, e, xs = made[1:]
    e = np.where(np.isnan(e), np.nan, e * 5.0)  # exposures up to 5: taken by the model, refused by the check
    big = _native.Survival(y, e, xs, R1.PRIORS[2])
    try:
        with pytest.raises(ValueError, match="exposure above 4"):
            big.predictive_configure(variables, edges)
        assert np.isfinite(big.logp_dlogp(q)[0])
    finally:
        big.close()


def test_s_model_fits_and_n_model_misses_the_s_titer_on_the_device():
    """tests/test_survival_predictive_cpu.py's two statements with the fits and the checks on the device."""
    checked = fit_and_check(lambda y, e, xs, ag: survival.SurvivalModel(y, e, xs, ag), use_device=True)
    check_statements(checked)
    p = checked["S"][2]
    assert p["n_draws"] == 300 and p["expected_i"].shape == p["p_infected_i"].shape == (300,)
    assert (p["p_infected_i"] > 0).all() and (p["p_infected_i"] < 1).all()
    np.testing.assert_allclose(p["expected_i"].sum(), p["variables"]["S"]["expected"].sum(axis=1).mean(), rtol=1e-12)
    np.testing.assert_allclose(p["replicate_mean_i"].sum(), p["variables"]["S"]["replicate"].sum(axis=1).mean(), rtol=1e-12)


def test_cli_checks_a_fit_of_the_golden_cohort(golden_dir, tmp_path, capsys):
    cohort = os.path.join(golden_dir, "test_cohort")
    data = TiterData.from_disk(cohort)
    rng = np.random.default_rng(0)
    post = tmp_path / "posterior.npz"
    means = dict(mean_i=rng.random((data.n_gaps, data.n_inds)) * 0.02, mean_ab_s_mu=rng.normal(size=(data.n_gaps, data.n_inds)),
                 mean_ab_n_mu=rng.normal(size=(data.n_gaps, data.n_inds)))
    np.savez(post, **means)
    out = tmp_path / "fit_s.npz"
    rc = survival.main(["--posterior", str(post), "--ititers_data", cohort, "--start", "2", "--end", "20", "--model", "s", "--out", str(out),
                        "--tune", "50", "--draws", "40", "--chains", "2", "--seed", "5", "--waic", "--ppc"])
    assert rc == 0
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 4 and lines[1].startswith("survival WAIC: ") and lines[2].startswith("survival PPC by S: ")
    assert lines[3].startswith("survival PPC by N: ") and "(80 draws)" in lines[2]
    with np.load(out) as f:
        fit = {k: f[k] for k in f.files}
    assert set(survival.PPC_FIT_KEYS) <= set(fit) and int(fit["ppc_seed"]) == 5 and int(fit["ppc_n_draws"]) == 80
    nb = fit["ppc_n_bins"]
    assert fit["ppc_expected"].shape == (80, 2, 8) and np.isfinite(fit["ppc_expected"][:, 0, :nb[0]]).all() and (fit["ppc_n_cells"][0, :nb[0]] > 0).all()
    assert fit["ppc_n_cells"][0].sum() == fit["ppc_n_cells"][1].sum() == fit["waic_n_cells"].sum()
    sa = survival.SurvivalAnalysis(means, 2, 20, data)
    model = sa.model_alone("S")
    try:
        again = dict(fit)
        p = survival.predictive(model, again, {"S": sa.s_titer, "N": sa.n_titer}, seed=5)
        for k in survival.PPC_FIT_KEYS:
            np.testing.assert_array_equal(again[k], fit[k], err_msg=k)
        cells = survival.sample_posterior_predictive(model, fit, draws=[0, 1, 2, 40, 79], seed=5)
        assert cells.shape == (5, data.n_inds, 17) and cells.dtype == np.int32
        np.testing.assert_array_equal(cells.sum(axis=(1, 2)), fit["ppc_replicate"][[0, 1, 2, 40, 79], 0].sum(axis=1))
        np.testing.assert_array_equal(p["observed_i"], fit["ppc_observed_ind"])
    finally:
        model.close()
