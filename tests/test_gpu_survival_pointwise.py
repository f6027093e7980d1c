"""
The per-individual log-likelihood of the survival models on the device and what is built on it (abd_survival_individual_loglik,
abd_survival_waic_*; survival.waic / survival.compare): parity with the 40-digit reference of
tests/golden/survival_pointwise_reference.npz over the case table of tests/survival_pointwise_restatement.py, bit-reproducibility
across launches, the accumulators against the statistics of the device's own matrix, the ranking of the S, N and combined models
on data simulated from an S-only model, and fits of the golden cohort scored and compared end to end, from Python and from the
command line.
"""
import os

import numpy as np
import pytest

from abdpymc_amd import _native, compare, survival
from abdpymc_amd.data import TiterData
from tests import survival_groups_restatement as RG
from tests import survival_pointwise_restatement as P
from tests import survival_restatement as R1
from tests.test_survival_pointwise_cpu import SIM, fit_and_score, simulate, variants

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def reference(golden_dir):
    return P.load_fixture(golden_dir)


def _handle(N, T, K=None, Gr=None):
    made = P.model_of(N, T, K, Gr)[1]
    if made[0] == "k":
        _, y, e, xs = made
        return _native.Survival(y, e, xs, R1.PRIORS[K])
    _, y, e, x, group, Gr = made
    return _native.SurvivalGroups(y, e, x, group, Gr, RG.PRIORS)


SHAPES = [(N, T, K, None) for N, T in P.SHAPES for K in (1, 2)] + [(N, T, None, Gr) for N, T, Gr in P.SHAPES_GROUPS]


@pytest.mark.parametrize("N,T,K,Gr", SHAPES)
def test_parity_with_the_40_digit_reference(reference, N, T, K, Gr):
    """Every ll_j finite and within C u S_j of the reference, C = P.c_device(class of point) = 4 E_NP[class] (fixed before the
    kernel ran), at every point of every shape, all points of a shape in one call; an individual with S_j = 0 (no followed cell)
    exactly 0.  Outputs are in the caller's order of individuals: the grouped shapes' labels are interleaved.  Measured on an
    MI355X, worst over the table per class (against C): typical 2.96 (28), b_plus_50 4.01 (44), b_minus_50 3.72 (20), eta_800 4.75
    (40), r_plus_800 5.27 (44), r_minus_800 3.32 (16), sd_e10 3.17 (28), sd_em10 2.97 (28), a_spread 2.49 (32)."""
    names = P.POINTS if Gr is None else P.POINTS_GROUPS
    tag = f"N{N}_T{T}_" + (f"K{K}" if Gr is None else f"G{Gr}")
    h = _handle(N, T, K, Gr)
    try:
        ll = h.individual_loglik(np.stack([P.point_of(name, T, K, Gr) for name in names]))
        assert ll.shape == (len(names), N)
        for row, name in zip(ll, names):
            ref, S = reference[f"{tag}_{name}/ll"], reference[f"{tag}_{name}/ll_S"]
            assert np.isfinite(row).all(), (tag, name)
            assert (row[S == 0] == 0).all(), (tag, name)
            worst = float((np.abs(row - ref)[S > 0] / S[S > 0] / P.U).max())
            print(f"{tag}_{name}: worst {worst:.2f} u S (C = {P.c_device(name):.0f})")
            assert worst <= P.c_device(name), (tag, name, worst)
    finally:
        h.close()


def _sixteen(T, K, Gr):
    names = P.POINTS[:8]
    return np.stack([P.point_of(name, T, K, Gr, seed=s) for s in (0, 1) for name in names])


@pytest.mark.parametrize("N,T,K,Gr", [(130, 65, 2, None), (130, 65, None, 4)])
def test_bits_do_not_depend_on_the_launch(N, T, K, Gr):
    h = _handle(N, T, K, Gr)
    try:
        pts = _sixteen(T, K, Gr)
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


@pytest.mark.parametrize("N,T,K,Gr", [(130, 65, 2, None), (130, 65, None, 4)])
def test_accumulators_fold_draws_in_order(N, T, K, Gr):
    """19 draws that really differ (jittered typical points) folded in one call, in 19 calls, and again after a reset: the same
    bits.  Against compare.stats_from_matrix of the device's own (19, N) matrix: the bounds of tests/test_gpu_individual_loglik.py
    for the same waic_update with its order term zero (the matrix holds the very values that were folded)."""
    h = _handle(N, T, K, Gr)
    try:
        with pytest.raises(ValueError, match="no draws accumulated"):
            h.waic_stats()  # nothing folded yet
        rng = np.random.default_rng(7)
        q = P.point_of("typical", T, K, Gr) + 0.1 * rng.normal(size=(19, h.dim))
        h.waic_accumulate(q)
        (lse, mean, m2, n), cells = h.waic_stats()
        assert n == 19
        np.testing.assert_array_equal(cells, P.constants(P.model_of(N, T, K, Gr)[0])[1])
        h.waic_reset()
        with pytest.raises(ValueError, match="no draws accumulated"):
            h.waic_stats()
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


def test_s_model_ranks_above_n_model_on_s_only_data():
    """tests/test_survival_pointwise_cpu.py's data and sampler seeds, the fits and the scores on the device: the same ranking."""
    models = variants(*simulate(**SIM), make=lambda y, e, xs, ag: survival.SurvivalModel(y, e, xs, ag))
    try:
        fits, w = fit_and_score(models, use_device=True)
    finally:
        for m in models.values():
            m.close()
    table = survival.compare(fits)
    print({k: (v["rank"], round(v["elpd_diff"], 3), round(v["dse"], 3)) for k, v in table.items()})
    assert table["N"]["rank"] == 2 and table["S"]["rank"] < table["N"]["rank"]
    pair = compare.compare({"S": w["S"], "N": w["N"]}, by="individual")
    assert pair["S"]["rank"] == 0 and pair["N"]["elpd_diff"] > 2.0 * pair["N"]["dse"] > 0.0


@pytest.fixture(scope="module")
def golden_run(golden_dir):
    from abdpymc_amd.model import model
    from abdpymc_amd.sampler import sample

    data = TiterData.from_disk(os.path.join(golden_dir, "test_cohort"))
    m = model(data, n_chains=2)
    res = sample(m, tune=20, draws=20, chains=2, seed=1, record_deterministics=False, record_discrete=False)
    m.close()
    return data, res


def test_fits_of_the_golden_cohort_scored_and_compared(golden_run):
    data, res = golden_run
    sa = survival.SurvivalAnalysis(res, 0, data.n_gaps, data)
    fits, w = {}, {}
    for name, make in (("S", lambda: sa.model_alone("S")), ("N", lambda: sa.model_alone("N")), ("combined", sa.model_combined)):
        sm = make()
        try:
            assert (sm.start, sm.end) == (0, data.n_gaps)
            fits[name] = survival.sample(sm, tune=100, draws=100, chains=2, seed=0)
            w[name] = survival.waic(sm, fits[name])
            (lse, mean, m2, n), cells = sm.waic_stats()
            np.testing.assert_array_equal(cells, sm.n_cells)  # the library's count and the Python layer's
        finally:
            sm.close()
        assert n == 200 and w[name]["n_draws"] == 200 and w[name]["elpd_i"].shape == (data.n_inds,)
        for k, v in w[name].items():
            assert np.isfinite(v).all(), (name, k)
        unfollowed = cells == 0
        assert (w[name]["elpd_i"][unfollowed] == 0).all() and (w[name]["p_waic_i"][unfollowed] == 0).all()
        assert w[name]["n_individuals"] == int((~unfollowed).sum()) > 0 and w[name]["elpd_waic"] < 0 and w[name]["p_waic"] > 0
    table = survival.compare(fits)
    assert sorted(v["rank"] for v in table.values()) == [0, 1, 2]
    for name, v in table.items():
        assert v["elpd_diff"] >= 0 and v["dse"] >= 0 and np.isfinite([v["elpd_waic"], v["p_waic"], v["se"], v["elpd_diff"], v["dse"]]).all()
        assert v["elpd_waic"] == w[name]["elpd_waic"]
    assert [v["elpd_diff"] for v in table.values() if v["rank"] == 0] == [0.0]


def test_cli_scores_fits_and_compares_them(golden_run, golden_dir, tmp_path, capsys):
    data, res = golden_run
    cohort = os.path.join(golden_dir, "test_cohort")
    post = tmp_path / "posterior.npz"
    np.savez(post, **{k: res[k] for k in ("mean_i", "mean_ab_s_mu", "mean_ab_n_mu")})
    for which in ("s", "n", "combined"):
        rc = survival.main(["--posterior", str(post), "--ititers_data", cohort, "--start", "2", "--end", "20", "--model", which,
                            "--out", str(tmp_path / f"fit_{which}.npz"), "--tune", "50", "--draws", "40", "--chains", "2", "--waic"])
        assert rc == 0
        lines = capsys.readouterr().out.splitlines()
        assert len(lines) == 2 and lines[0].startswith("survival: ") and lines[1].startswith("survival WAIC: elpd_waic ")
        assert "individuals, 80 draws; " in lines[1]
        with np.load(tmp_path / f"fit_{which}.npz") as f:
            assert f["elpd_waic_ind"].shape == (data.n_inds,) and int(f["waic_n_draws"]) == 80 and (int(f["start"]), int(f["end"])) == (2, 20)
            assert np.isfinite(f["elpd_waic_ind"]).all() and (f["elpd_waic_ind"][f["waic_n_cells"] == 0] == 0).all()
    assert survival.main(["--compare"] + [str(tmp_path / f"fit_{w}.npz") for w in ("s", "n", "combined")]) == 0
    rows = capsys.readouterr().out.splitlines()
    assert len(rows) == 3 and [f" rank {k} " in r for k, r in enumerate(rows)] == [True] * 3
