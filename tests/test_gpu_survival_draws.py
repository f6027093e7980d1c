"""
Per-draw survival fits on the device (abd_survival_draws_*; abdpymc_amd.survival.sample_draws): the ensemble kernel is
bit for bit the plug-in kernel on every dataset, a point's bits do not depend on the launch, the batched driver is ``_chain`` per
dataset, and one fit end to end on the golden cohort.
"""
import os
import re

import numpy as np
import pytest

from abdpymc_amd import _native, survival
from abdpymc_amd.data import TiterData
from tests import survival_restatement as R
from tests.survival_draws_cases import datasets

pytestmark = pytest.mark.gpu


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _points(T, K):
    return np.stack([R.make_point(name, T, K, seed=s) for s in (0, 1) for name in R.POINTS])  # 16 points


def _ensemble(d, K):
    return _native.SurvivalDraws(d.n_risk, d.event, [d.s_titer, d.n_titer][:K], R.PRIORS[K])


def _plug_in(d, m, K):
    y, e, xs, xn = d.arrays(m)
    return _native.Survival(y, e, [xs, xn][:K], R.PRIORS[K])


# (130, 65, 2, 3): a partial tile and two finalize blocks; (520, 511, 2, 3): seg_len = 2, which no smaller shape reaches
@pytest.mark.parametrize("N,T,K,M", [(1, 1, 1, 1), (130, 65, 2, 3), (520, 511, 2, 3), (1000, 199, 1, 2)])
def test_bit_equal_to_the_plug_in_kernel_on_every_dataset(N, T, K, M):
    """logp, gradient and loglik_sums of 16 points, each on its own dataset, equal BITWISE what an abd_survival handle of that
    dataset's (infected, exposure, titers) returns: the same cell function, the same split and the same finalize in the same order;
    the cells a wave skips add exact +0 there (abd_survival.hpp, beside SurvSource).  The yardstick is the kernel tests/test_gpu_survival.py
    pins to the 40-digit fixture."""
    d = datasets(M, N, T)
    pts = _points(T, K)
    ds = ((np.arange(16) * 5 + 2) % M).astype(np.int32)  # M = 3: 2, 1, 0, 2, ...: not monotone, every dataset more than once
    h = _ensemble(d, K)
    try:
        assert h.dim == 2 * K + 2 + T
        lp, g = h.logp_dlogp(ds, pts)
        assert np.isfinite(lp).all() and np.isfinite(g).all()
        sums = np.stack([h.loglik_sums(int(m), q) for m, q in zip(ds, pts)])
        for m in range(M):
            p = _plug_in(d, m, K)
            try:
                rows = np.flatnonzero(ds == m)
                lp_m, g_m = p.logp_dlogp(pts[rows])
                np.testing.assert_array_equal(_bits(lp[rows]), _bits(lp_m))
                np.testing.assert_array_equal(_bits(g[rows]), _bits(g_m))
                for r in rows:
                    np.testing.assert_array_equal(_bits(sums[r]), _bits(p.loglik_sums(pts[r])))
            finally:
                p.close()
        if M > 1:  # the datasets differ: the index is read
            other, _ = h.logp_dlogp((ds + 1) % M, pts)
            assert (other != lp).any()
    finally:
        h.close()


def test_bits_do_not_depend_on_the_launch_or_the_row():
    N, T, K, M = 130, 65, 2, 3
    d = datasets(M, N, T)
    pts = _points(T, K)
    ds = ((np.arange(16) * 5 + 2) % M).astype(np.int32)
    h = _ensemble(d, K)
    try:
        lp, g = h.logp_dlogp(ds, pts)
        lp2, g2 = h.logp_dlogp(ds, pts)
        np.testing.assert_array_equal(_bits(lp), _bits(lp2))
        np.testing.assert_array_equal(_bits(g), _bits(g2))
        for row in (0, 5, 15):
            one_lp, one_g = h.logp_dlogp(int(ds[row]), pts[row])  # alone
            assert one_lp == lp[row]
            np.testing.assert_array_equal(one_g, g[row])
            for at in (0, 7, 15):  # as any row of a 16-point launch among other datasets
                m_lp, m_g = h.logp_dlogp(np.roll(ds, at - row), np.roll(pts, at - row, axis=0))
                assert m_lp[at] == lp[row]
                np.testing.assert_array_equal(m_g[at], g[row])
        both_lp, both_g = h.logp_dlogp(np.concatenate([ds, ds[:3]]), np.concatenate([pts, pts[:3]]))  # 19 points: two launches
        np.testing.assert_array_equal(both_lp, np.concatenate([lp, lp[:3]]))
        np.testing.assert_array_equal(both_g, np.concatenate([g, g[:3]]))
        np.testing.assert_array_equal(h.loglik_sums(1, pts[3]), h.loglik_sums(1, pts[3]))
        # a dataset index outside [0, M) is refused, and nothing is evaluated
        for bad in (-1, M):
            with pytest.raises(ValueError, match=rf"point 2: dataset {bad} outside \[0, {M}\)"):
                h.logp_dlogp(np.array([0, 1, bad], dtype=np.int32), pts[:3])
            with pytest.raises(ValueError, match="outside"):
                h.loglik_sums(bad, pts[0])
    finally:
        h.close()


def test_driver_on_the_device_is_chain_per_dataset():
    M, N, T, tune, draws, seed = 4, 300, 6, 40, 20, 2
    d = datasets(M, N, T)
    model = survival.SurvivalDrawsModel(d, [d.s_titer], ("S",))
    try:
        calls = []

        def recording(ds, q):
            calls.append(len(ds))
            return model.logp_dlogp(ds, q)

        fit = survival.sample_draws(model, tune=tune, draws=draws, chains_per_dataset=1, seed=seed, evaluator=recording)
        assert int(fit["n_evaluations"]) == sum(calls) and len(calls) < int(fit["n_evaluations"]) / 2
        q0 = survival._initial_point(model)
        for m in range(M):
            out, stats = survival._chain(lambda q: model.logp_dlogp(m, q), model.dim, tune, draws, np.random.default_rng([seed, m, 0]), 0.8, q0)
            np.testing.assert_array_equal(np.stack([fit[name][m] for name in model.names], axis=-1), out)
            for name, v in stats.items():
                np.testing.assert_array_equal(fit["stat_" + name][m], v, err_msg=name)
        unbatched = survival.sample_draws(model, tune=5, draws=3, seed=seed)  # and through the model's own evaluator
        assert unbatched["a"].shape == (M, 3) and np.isfinite(unbatched["stat_lp"]).all()
    finally:
        model.close()


def test_per_draw_fit_of_the_golden_cohort_end_to_end(tmp_path, golden_dir, capsys):
    from abdpymc_amd.model import model
    from abdpymc_amd.sampler import sample

    cohort = os.path.join(golden_dir, "test_cohort")
    data = TiterData.from_disk(cohort)
    m = model(data, n_chains=2)
    res = sample(m, tune=20, draws=20, chains=2, seed=1, record_deterministics=True, record_discrete=False)
    m.close()
    G = data.n_gaps
    sa = survival.SurvivalAnalysis(res, 0, G, data)
    d = sa.draws(n_datasets=4)
    assert d.n_risk.shape == (4, data.n_inds) and d.s_titer.shape == (4, G - 1, data.n_inds) and d.source.tolist() == [[0, 0], [0, 13], [1, 6], [1, 19]]
    sm = sa.model_combined_draws(d)
    try:
        assert sm.dim == 6 + sa.n_int and len(sm.names) == sm.dim and sm.n_datasets == 4
        fit = survival.sample_draws(sm, tune=60, draws=40, seed=0)
    finally:
        sm.close()
    assert fit["a"].shape == (4, 40, 2) and fit["b"].shape == (4, 40, 2) and fit["lam0"].shape == (4, 40, sa.n_int)
    assert fit["dataset"].tolist() == [0, 1, 2, 3] and fit["source"].shape == (4, 2) and int(fit["n_evaluations"]) > 0
    for k, v in fit.items():
        if k != "antigens":
            assert np.isfinite(v).all(), k
    assert ((fit["lam0"] > 0) & (fit["lam0"] < 1)).all()
    for ag in ("S", "N"):
        p = survival.protection(fit, np.linspace(-2.0, 6.0, 9), antigen=ag)
        for k in ("mean", "median", "lower", "upper"):
            assert ((p[k] >= 0) & (p[k] <= 1)).all(), (ag, k)
    summ = survival.draws_summary(fit)
    assert len(summ) == 10
    for name, row in summ.items():
        assert 0.0 <= row["frac_between"] <= 1.0 and row["dataset_median"].shape == (4,), name
        assert row["lower"] <= row["median"] <= row["upper"]
    # the command line: one line, the new keys in the file
    post = tmp_path / "posterior.npz"
    np.savez(post, **{k: res[k] for k in ("i", "ab_s_mu", "ab_n_mu", "mean_i", "mean_ab_s_mu", "mean_ab_n_mu")})
    out = tmp_path / "fit.npz"
    capsys.readouterr()
    rc = survival.main(["--posterior", str(post), "--ititers_data", cohort, "--start", "2", "--end", "20", "--model", "s", "--out", str(out),
                        "--tune", "40", "--draws", "30", "--per_draw", "4", "--per_draw_chains", "2"])
    assert rc == 0
    cap = capsys.readouterr()
    line = cap.out.splitlines()
    assert len(line) == 1 and line[0].startswith("survival: a[S]") and "wrote " in cap.err
    assert "per-draw fits of 4 datasets" in line[0] and re.search(r"between datasets: a\[S\] [01]\.\d{3}, b\[S\] [01]\.\d{3}$", line[0]), line[0]
    with np.load(out) as f:
        assert f["a"].shape == (8, 30) and f["lam0"].shape == (8, 30, 17) and f["dataset"].tolist() == [0, 0, 1, 1, 2, 2, 3, 3]
        assert f["source"].shape == (4, 2) and int(f["n_evaluations"]) > int(f["n_calls"]) > 0
        assert f["draws_quantity"].tolist()[:2] == ["a[S]", "b[S]"] and f["draws_frac_between"].shape == (5,)
        assert ((f["draws_frac_between"] >= 0) & (f["draws_frac_between"] <= 1)).all() and f["draws_dataset_median"].shape == (5, 4)
