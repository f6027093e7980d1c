"""
The per-individual sums of the pointwise log-likelihood (abd_individual_loglik; the native sampler's per-individual WAIC
accumulators, ``waic_by``) against the frozen oracle.  The reference of a row is ``math.fsum`` of the oracle's per-reading
values of that individual and antigen; with n_j terms ll_k the allowed difference per entry is

    sum_k (RTOL |ll_k| + ATOL)          the project's per-reading tolerances (tests/test_gpu_pointwise.py)
  + n_j 2^-52 sum_k |ll_k|              which bounds the rounding of any order of summation

so a row without readings must be exactly 0.0.
"""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest

from abdpymc_amd import compare, synthetic
from abdpymc_amd.data import TiterData
from oracle import abd_oracle as O
from tests.helpers import oracle_cohort_from_synth, random_sparse_cohort
from tests.test_gpu_pointwise import RTOL, ATOL, _cohort_of, _ctx, _same_trajectories, _state, oracle_ll

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52


def by_individual(idx, ll, N):
    """-> (fsum of ll, fsum of |ll|, count) per individual"""
    terms = [[] for _ in range(N)]
    for j, v in zip(np.asarray(idx).tolist(), np.asarray(ll, float).tolist()):
        terms[j].append(v)
    return (np.array([math.fsum(t) for t in terms]), np.array([math.fsum(abs(v) for v in t) for t in terms]),
            np.array([len(t) for t in terms], dtype=np.int64))


def order_term(sabs, cnt):
    return cnt * EPS * sabs


def _within(got, ref, bound):
    bad = np.abs(got - ref) > bound
    assert not bad.any(), (np.flatnonzero(bad)[:5], got[bad][:5], ref[bad][:5], bound[bad][:5])


def _check(coh, ctx, seed, splits=None, ignore=False, ref_coh=None):
    """the rows against the oracle; then against fsum of the device's own per-reading row, within the order term alone"""
    theta, i_raw, w = _state(coh, seed)
    ctx.set_discrete(0, i_raw, w)
    N = coh.n_inds
    rows = ctx.individual_loglik(0, theta)
    dev = ctx.pointwise_loglik(0, theta)
    orc = oracle_ll(ref_coh or coh, theta, i_raw, w, splits, ignore)
    for got, o, d, obs in zip(rows, orc, dev, (coh.s, coh.n)):
        assert got.shape == (N,)
        ref, sabs, cnt = by_individual(obs.idx_ind, o, N)
        _within(got, ref, RTOL * sabs + ATOL * cnt + order_term(sabs, cnt))
        assert np.all(got[cnt == 0] == 0.0)
        dref, dabs, _ = by_individual(obs.idx_ind, d, N)
        _within(got, dref, order_term(dabs, cnt))
    return theta, rows


@pytest.fixture(scope="module")
def test_td(golden_dir):
    return TiterData.from_disk(os.path.join(golden_dir, "test_cohort"))


@pytest.mark.parametrize("splits,ignore", [(None, False), ((14, 20), False), (None, True)])
def test_golden_test_cohort(test_td, splits, ignore):
    coh = _cohort_of(test_td)
    _check(coh, _ctx(coh, splits, ignore), 1, splits, ignore)


@pytest.mark.parametrize("G", [31, 65, 300])  # one, two, and more than ABD_MAXT packed words
def test_random_sparse(G):
    coh = random_sparse_cohort(60, G, 900, 700, seed=G)
    ctx = _ctx(coh)
    assert not ctx.is_dense
    _check(coh, ctx, G)


def test_empty_individuals_and_empty_antigen():
    coh = random_sparse_cohort(50, 31, 20, 0, seed=3)
    ctx = _ctx(coh)
    _, (ll_s, ll_n) = _check(coh, ctx, 1)
    has = np.bincount(coh.s.idx_ind, minlength=50) > 0
    assert (~has).sum() >= 30 and np.all(ll_s[~has] == 0.0) and np.all(ll_s[has] != 0.0)
    np.testing.assert_array_equal(ll_n, np.zeros(50))


def test_more_than_64_readings_of_one_individual():
    """the lanes' stride over a segment: individual 2 has 150 S readings, individual 3 has 70 N readings"""
    coh = random_sparse_cohort(5, 31, 40, 30, seed=11)
    rng = np.random.default_rng(12)

    def more(o, j, k):
        return O.AntigenObs(np.concatenate([o.idx_gap, rng.integers(0, 31, k).astype(np.int32)]),
                            np.concatenate([o.idx_ind, np.full(k, j, np.int32)]),
                            np.concatenate([o.log_dilution, rng.choice(np.array([0.0, 2.0, 4.0]), k)]),
                            np.concatenate([o.od, rng.uniform(0.0, 2.0, k)]))

    coh = O.Cohort(coh.n_gaps, coh.n_inds, coh.vacs, coh.pcrpos, more(coh.s, 2, 150), more(coh.n, 3, 70))
    assert np.bincount(coh.s.idx_ind, minlength=5)[2] > 128 and np.bincount(coh.n.idx_ind, minlength=5)[3] > 64
    ctx = _ctx(coh)
    assert not ctx.is_dense
    _check(coh, ctx, 2)


@pytest.mark.parametrize("G,N", [(64, 65), (65, 70), (300, 40)])
def test_dense_f64(G, N):
    coh = oracle_cohort_from_synth(synthetic.make_cohort(N, G, seed=G + N))
    ctx = _ctx(coh)
    assert ctx.is_dense
    _check(coh, ctx, 0)


def test_dense_f32_storage():
    coh = oracle_cohort_from_synth(synthetic.make_cohort(100, 60, seed=280))
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)  # noqa: E731
    ref = O.Cohort(coh.n_gaps, coh.n_inds, coh.vacs, coh.pcrpos,
                   O.AntigenObs(coh.s.idx_gap, coh.s.idx_ind, f32(coh.s.log_dilution), f32(coh.s.od)),
                   O.AntigenObs(coh.n.idx_gap, coh.n.idx_ind, f32(coh.n.log_dilution), f32(coh.n.od)))
    ctx = _ctx(coh, storage="f32")
    assert ctx.is_dense
    _check(coh, ctx, 2, ref_coh=ref)


def test_dense_kept_as_lists(monkeypatch):
    monkeypatch.setenv("ABD_FORCE_SPARSE", "1")
    coh = oracle_cohort_from_synth(synthetic.make_cohort(70, 65, seed=135))
    ctx = _ctx(coh)
    assert not ctx.is_dense
    _check(coh, ctx, 0)


@pytest.mark.parametrize("dense", [True, False])
def test_rows_are_reproducible_and_either_alone_is_the_pairs_half(dense):
    from abdpymc_amd import _native

    coh = oracle_cohort_from_synth(synthetic.make_cohort(70, 65, seed=135)) if dense else random_sparse_cohort(60, 65, 900, 700, seed=65)
    ctx = _ctx(coh)
    assert ctx.is_dense == dense
    theta, i_raw, w = _state(coh, 7)
    ctx.set_discrete(0, i_raw, w)
    a_s, a_n = ctx.individual_loglik(0, theta)
    b_s, b_n = ctx.individual_loglik(0, theta)
    np.testing.assert_array_equal(a_s, b_s)
    np.testing.assert_array_equal(a_n, b_n)
    t = np.ascontiguousarray(theta, dtype=np.float64)
    for ref, first in ((a_s, True), (a_n, False)):
        one = np.full(coh.n_inds, np.nan)
        p = _native._ptr(one)
        assert ctx._lib.abd_individual_loglik(ctx._h, 0, _native._ptr(t), p if first else None, None if first else p) == 0
        np.testing.assert_array_equal(one, ref)
    assert ctx._lib.abd_individual_loglik(ctx._h, 0, _native._ptr(t), None, None) == -1


def _check_sampler(res, mat_s, mat_n, idx_s, idx_n, N):
    """the per-individual accumulators of every chain against the statistics of its recorded (unthinned) matrix, grouped on
    the host; B_j: the summation-order term of individual j, at its largest over the chain's draws"""
    T = compare.individual_matrix(mat_s, mat_n, idx_s, idx_n, N)
    cnt = np.bincount(idx_s, minlength=N) + np.bincount(idx_n, minlength=N)
    sabs = compare.individual_matrix(np.abs(mat_s), np.abs(mat_n), idx_s, idx_n, N)
    np.testing.assert_array_equal(res["waic_ind_n_readings"], np.tile(cnt, (T.shape[0], 1)))
    for c in range(T.shape[0]):
        lse, mean, m2, n = compare.stats_from_matrix(T[c])
        assert res["waic_n_draws"][c] == n
        B = order_term(sabs[c].max(axis=0), cnt)
        _within(res["waic_ind_lse"][c], lse, 1e-12 * np.abs(lse) + B)
        _within(res["waic_ind_mean"][c], mean, 1e-12 * np.abs(mean) + B)
        _within(res["waic_ind_m2"][c], m2, 1e-9 * m2 + 2.0 * np.sqrt(n * m2) * B + n * B * B)


def test_sampler_accumulates_test_cohort(test_td):
    from abdpymc_amd.model import model
    from abdpymc_amd.sampler import sample

    m = model(test_td, n_chains=3)
    kw = dict(tune=30, draws=40, chains=3, seed=5, record_deterministics=False)
    both = sample(m, thin=3, log_likelihood=True, waic=True, waic_by="both", **kw)
    full = sample(m, thin=1, log_likelihood=True, waic=True, waic_by="both", **kw)
    ind = sample(m, thin=3, waic=True, waic_by="individual", **kw)
    plain = sample(m, thin=3, **kw)
    N = test_td.n_inds
    idx_s, idx_n = np.asarray(test_td.s.obs[1]), np.asarray(test_td.n.obs[1])
    assert both["waic_ind_lse"].shape == (3, N)
    for res in (both, full):
        _check_sampler(res, full["log_likelihood_it_s_lik"], full["log_likelihood_it_n_lik"], idx_s, idx_n, N)
    assert list(both["waic_n_draws"]) == [40, 40, 40] and list(ind["waic_n_draws"]) == [40, 40, 40]
    # alone, the per-individual accumulators are the same bits, and nothing is kept per reading
    assert "waic_lse" not in ind and "waic_lse" in both
    for k in ("waic_ind_lse", "waic_ind_mean", "waic_ind_m2", "waic_ind_n_readings"):
        np.testing.assert_array_equal(ind[k], both[k])
    # the feature changes nothing the chains draw
    _same_trajectories(both, plain)
    _same_trajectories(ind, plain)
    w = compare.waic(both, by="individual")
    wm = compare.waic_from_matrix(np.concatenate([full["log_likelihood_it_s_lik"], full["log_likelihood_it_n_lik"]], axis=-1),
                                  groups=np.concatenate([idx_s, idx_n]), n_groups=N)
    assert abs(w["elpd_waic"] - wm["elpd_waic"]) <= 1e-9 * abs(wm["elpd_waic"]) and np.isfinite(w["se"])
    assert w["n_individuals"] == wm["n_individuals"] == int((np.bincount(idx_s, minlength=N) + np.bincount(idx_n, minlength=N) > 0).sum())


def test_sampler_dense():
    from abdpymc_amd.model import AbdModel
    from abdpymc_amd.sampler import sample

    sc = synthetic.make_cohort(130, 65, seed=31)
    d = SimpleNamespace(n_gaps=sc.n_gaps, n_inds=sc.n_inds, vacs=sc.vacs, pcrpos=sc.pcrpos,
                        coords={"gap": np.arange(sc.n_gaps), "ind": np.arange(sc.n_inds)},
                        s=SimpleNamespace(obs=sc.s_obs), n=SimpleNamespace(obs=sc.n_obs))
    m = AbdModel(d, n_chains=2)
    assert m.ctx.is_dense
    kw = dict(tune=4, draws=6, chains=2, seed=3, record_deterministics=False, record_discrete=False)
    res = sample(m, log_likelihood=True, waic=True, waic_by="both", **kw)
    plain = sample(m, **kw)
    idx = np.asarray(sc.idx_ind)
    _check_sampler(res, res["log_likelihood_it_s_lik"], res["log_likelihood_it_n_lik"], idx, idx, sc.n_inds)
    assert list(res["waic_n_draws"]) == [6, 6]
    _same_trajectories(res, plain, keys=())


def test_cli_waic_by_both(tmp_path, golden_dir, capsys):
    from abdpymc_amd import cli

    out = tmp_path / "post.npz"
    rc = cli.main(["--tune", "6", "--draws", "5", "--cores", "1", "--ititers_data", os.path.join(golden_dir, "test_cohort"),
                   "--waic", "--waic_by", "both", "--netcdf", str(out)])
    assert rc == 0
    err = capsys.readouterr().err
    line = [ln for ln in err.splitlines() if ln.startswith("WAIC:")]
    assert line and math.isfinite(float(line[0].split()[2]))
    by_ind = [ln for ln in err.splitlines() if ln.startswith("WAIC by individual:")]
    assert by_ind and math.isfinite(float(by_ind[0].split()[4])) and "worst: individual" in by_ind[0]
    z = np.load(out)
    td = TiterData.from_disk(os.path.join(golden_dir, "test_cohort"))
    assert z["elpd_waic_ind"].shape == (td.n_inds,) and np.all(np.isfinite(z["elpd_waic_ind"]))
    assert z["p_waic_ind"].shape == (td.n_inds,) and "elpd_waic_i_it_s_lik" in z.files
