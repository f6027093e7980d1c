"""
The pointwise log-likelihood of the OD readings (abd_pointwise_loglik; the native sampler's recorded matrix and WAIC
accumulators) against the frozen oracle: mu from O.deterministics, the logistic curve, an elementwise Normal log-density.
"""
import math
import os

import numpy as np
import pytest

from abdpymc_amd import compare, synthetic
from abdpymc_amd.data import TiterData
from oracle import abd_oracle as O
from tests.helpers import oracle_cohort_from_synth, random_sparse_cohort
from tests.test_data_loader import default_cohort

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-12, 1e-10


def _ctx(coh, splits=None, ignore=False, n_chains=1, storage="f64"):
    from abdpymc_amd._native import Context

    return Context(coh.n_gaps, coh.n_inds, (coh.s.idx_gap, coh.s.idx_ind, coh.s.log_dilution, coh.s.od),
                   (coh.n.idx_gap, coh.n.idx_ind, coh.n.log_dilution, coh.n.od), coh.vacs, None if ignore else coh.pcrpos,
                   splits=splits, n_chains=n_chains, storage=storage)


def _cohort_of(td):
    return O.Cohort(td.n_gaps, td.n_inds, np.asarray(td.vacs, dtype=np.int8), np.asarray(td.pcrpos, dtype=np.int8),
                    O.AntigenObs(*td.s.obs), O.AntigenObs(*td.n.obs))


def oracle_ll(coh, theta, i_raw, w, splits=None, ignore=False):
    c = O.constrained(theta)
    _, mu_n, mu_s = O.deterministics(theta, i_raw, w, coh, splits, ignore)

    def one(o, mu, b, d, sig):
        m = O.logistic(np.asarray(o.log_dilution, float), mu[np.asarray(o.idx_gap), np.asarray(o.idx_ind)], b, d)
        r = (np.asarray(o.od, float) - m) / sig
        return -0.5 * r * r - math.log(sig) - 0.5 * math.log(2 * math.pi)

    return one(coh.s, mu_s, c["b_s"], c["d_s"], c["sigma_s"]), one(coh.n, mu_n, c["b_n"], c["d_n"], c["sigma_n"])


def _state(coh, seed):
    rng = np.random.default_rng(seed)
    i_raw = (rng.random((coh.n_gaps, coh.n_inds)) < 2.0 / coh.n_gaps).astype(np.int8)
    w = (rng.random(coh.n_inds) < 0.5).astype(np.int8)
    theta = synthetic.theta_init(coh.n_gaps) + 0.3 * rng.standard_normal(17)
    return theta, i_raw, w


def _check(coh, ctx, seed, splits=None, ignore=False, ref_coh=None):
    theta, i_raw, w = _state(coh, seed)
    ctx.set_discrete(0, i_raw, w)
    ll_s, ll_n = ctx.pointwise_loglik(0, theta)
    r_s, r_n = oracle_ll(ref_coh or coh, theta, i_raw, w, splits, ignore)
    assert ll_s.shape == r_s.shape and ll_n.shape == r_n.shape
    np.testing.assert_allclose(ll_s, r_s, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(ll_n, r_n, rtol=RTOL, atol=ATOL)
    return theta, ll_s, ll_n


@pytest.fixture(scope="module")
def test_td(golden_dir):
    return TiterData.from_disk(os.path.join(golden_dir, "test_cohort"))


@pytest.mark.parametrize("splits,ignore", [(None, False), ((14, 20), False), (None, True)])
def test_golden_test_cohort(test_td, splits, ignore):
    coh = _cohort_of(test_td)
    ctx = _ctx(coh, splits, ignore)
    for seed in range(3):
        _check(coh, ctx, seed, splits, ignore)


def test_default_cohort_and_the_sum_is_loglik(golden_dir):
    coh = _cohort_of(default_cohort(golden_dir))
    ctx = _ctx(coh)
    assert not ctx.is_dense and coh.s.od.size + coh.n.od.size == 35709
    for seed in range(3):
        theta, ll_s, ll_n = _check(coh, ctx, seed)
        ll, _ = ctx.loglik_dlogp(0, theta)
        assert abs(ll_s.sum() + ll_n.sum() - ll) <= 1e-9 * abs(ll)


@pytest.mark.parametrize("G", [31, 64, 65, 200, 300])
def test_random_sparse(G):
    coh = random_sparse_cohort(60, G, 900, 700, seed=G)
    _check(coh, _ctx(coh), G)


def test_empty_individual_and_empty_antigen():
    coh = random_sparse_cohort(50, 31, 20, 0, seed=3)  # most individuals have no reading, the N antigen none at all
    ctx = _ctx(coh)
    _, ll_s, ll_n = _check(coh, ctx, 1)
    assert ll_n.size == 0 and ll_s.size == 20


@pytest.mark.parametrize("G,N", [(60, 100), (64, 65), (200, 50), (300, 40)])
def test_dense_f64_and_sum(G, N):
    coh = oracle_cohort_from_synth(synthetic.make_cohort(N, G, seed=G + N))
    ctx = _ctx(coh)
    assert ctx.is_dense
    for seed in range(2):
        theta, ll_s, ll_n = _check(coh, ctx, seed)
        ll, _ = ctx.loglik_dlogp(0, theta)
        assert abs(ll_s.sum() + ll_n.sum() - ll) <= 1e-9 * abs(ll)


def test_dense_kept_as_lists(monkeypatch):
    monkeypatch.setenv("ABD_FORCE_SPARSE", "1")
    coh = oracle_cohort_from_synth(synthetic.make_cohort(70, 65, seed=5))
    ctx = _ctx(coh)
    assert not ctx.is_dense
    _check(coh, ctx, 4)


@pytest.mark.parametrize("G,N", [(60, 100), (200, 50)])
def test_dense_f32_storage(G, N):
    coh = oracle_cohort_from_synth(synthetic.make_cohort(N, G, seed=G * 3 + N))
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)  # noqa: E731
    ref = O.Cohort(coh.n_gaps, coh.n_inds, coh.vacs, coh.pcrpos,
                   O.AntigenObs(coh.s.idx_gap, coh.s.idx_ind, f32(coh.s.log_dilution), f32(coh.s.od)),
                   O.AntigenObs(coh.n.idx_gap, coh.n.idx_ind, f32(coh.n.log_dilution), f32(coh.n.od)))
    _check(coh, _ctx(coh, storage="f32"), 2, ref_coh=ref)


@pytest.mark.parametrize("which", ["test", "sparse"])
def test_shuffled_readings_come_back_in_their_order(test_td, which):
    coh = _cohort_of(test_td) if which == "test" else random_sparse_cohort(40, 31, 500, 400, seed=9)
    rng = np.random.default_rng(1)
    ps, pn = rng.permutation(coh.s.od.size), rng.permutation(coh.n.od.size)
    sh = lambda o, p: O.AntigenObs(*(np.asarray(a)[p] for a in (o.idx_gap, o.idx_ind, o.log_dilution, o.od)))  # noqa: E731
    coh2 = O.Cohort(coh.n_gaps, coh.n_inds, coh.vacs, coh.pcrpos, sh(coh.s, ps), sh(coh.n, pn))
    theta, ll_s, ll_n = _check(coh, _ctx(coh), 3)
    _, ll2_s, ll2_n = _check(coh2, _ctx(coh2), 3)
    np.testing.assert_array_equal(ll2_s, ll_s[ps])
    np.testing.assert_array_equal(ll2_n, ll_n[pn])


def _theta_rows(res):
    from abdpymc_amd.model import THETA_NAMES

    return np.stack([res[n] for n in THETA_NAMES], axis=-1)  # (chains, draws, 17)


def _stats_equal(res, mat):
    """the device accumulators of every chain against the statistics of its recorded (unthinned) matrix"""
    for c in range(mat.shape[0]):
        lse, mean, m2, n = compare.stats_from_matrix(mat[c])
        assert res["waic_n_draws"][c] == n
        np.testing.assert_allclose(res["waic_lse"][c], lse, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(res["waic_mean"][c], mean, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(res["waic_m2"][c], m2, rtol=1e-9, atol=1e-12)


def _same_trajectories(a, b, keys=("i_raw", "ab_s_waner")):
    np.testing.assert_array_equal(_theta_rows(a), _theta_rows(b))
    for k in [k for k in a if k.startswith("stat_")]:
        np.testing.assert_array_equal(a[k], b[k])
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k])


def test_sampler_records_and_accumulates_test_cohort(test_td):
    from abdpymc_amd.model import model
    from abdpymc_amd.sampler import sample

    m = model(test_td, n_chains=4)
    kw = dict(tune=30, draws=40, chains=3, seed=5, record_deterministics=False)
    res = sample(m, thin=3, log_likelihood=True, waic=True, **kw)
    full = sample(m, thin=1, log_likelihood=True, waic=True, **kw)
    plain = sample(m, thin=3, **kw)
    K_s, K_n = m.ctx.n_obs_s, m.ctx.n_obs_n
    assert res["log_likelihood_it_s_lik"].shape == (3, 14, K_s) and res["log_likelihood_it_n_lik"].shape == (3, 14, K_n)
    # every recorded row is pointwise_loglik at the recorded draw, on a spare chain slot
    th = _theta_rows(res)
    for c in range(3):
        for r, d in enumerate(res["draw_index"][c]):
            m.ctx.set_discrete(3, res["i_raw"][c, r], res["ab_s_waner"][c, r])
            ll_s, ll_n = m.ctx.pointwise_loglik(3, th[c, d])
            np.testing.assert_allclose(res["log_likelihood_it_s_lik"][c, r], ll_s, rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(res["log_likelihood_it_n_lik"][c, r], ll_n, rtol=1e-12, atol=1e-12)
    # the accumulators hold the statistics of all 40 draws
    mat = np.concatenate([full["log_likelihood_it_s_lik"], full["log_likelihood_it_n_lik"]], axis=-1)
    _stats_equal(res, mat)
    _stats_equal(full, mat)
    np.testing.assert_array_equal(full["log_likelihood_it_s_lik"][:, ::3], res["log_likelihood_it_s_lik"])
    # the feature changes nothing the chains draw
    _same_trajectories(res, plain)
    w = compare.waic(res)
    wm = compare.waic_from_matrix(mat)
    assert abs(w["elpd_waic"] - wm["elpd_waic"]) <= 1e-9 * abs(wm["elpd_waic"]) and np.isfinite(w["se"])


def test_sampler_dense_trains():
    """a dense cohort large enough for leapfrog trains over more than 256 workgroups"""
    from types import SimpleNamespace

    from abdpymc_amd.model import AbdModel
    from abdpymc_amd.sampler import sample

    sc = synthetic.make_cohort(1500, 200, seed=31)
    d = SimpleNamespace(n_gaps=sc.n_gaps, n_inds=sc.n_inds, vacs=sc.vacs, pcrpos=sc.pcrpos,
                        coords={"gap": np.arange(sc.n_gaps), "ind": np.arange(sc.n_inds)},
                        s=SimpleNamespace(obs=sc.s_obs), n=SimpleNamespace(obs=sc.n_obs))
    m = AbdModel(d, n_chains=2)
    assert m.ctx.is_dense
    kw = dict(tune=4, draws=6, chains=2, seed=3, record_deterministics=False, record_discrete=False)
    res = sample(m, log_likelihood=True, waic=True, **kw)
    plain = sample(m, **kw)
    mat = np.concatenate([res["log_likelihood_it_s_lik"], res["log_likelihood_it_n_lik"]], axis=-1)
    assert mat.shape == (2, 6, 2 * 1500 * 200)
    _stats_equal(res, mat)
    _same_trajectories(res, plain, keys=())


def test_cli_waic_and_log_likelihood(tmp_path, golden_dir, capsys):
    from abdpymc_amd import cli

    out = tmp_path / "post.npz"
    rc = cli.main(["--tune", "6", "--draws", "5", "--cores", "1", "--ititers_data", os.path.join(golden_dir, "test_cohort"),
                   "--waic", "--log_likelihood", "--thin", "2", "--netcdf", str(out)])
    assert rc == 0
    err = capsys.readouterr().err
    line = [ln for ln in err.splitlines() if ln.startswith("WAIC:")]
    assert line and math.isfinite(float(line[0].split()[2]))
    z = np.load(out)
    td = TiterData.from_disk(os.path.join(golden_dir, "test_cohort"))
    K_s, K_n = td.s.obs[0].size, td.n.obs[0].size
    assert z["log_likelihood_it_s_lik"].shape == (2, 3, K_s) and z["log_likelihood_it_n_lik"].shape == (2, 3, K_n)
    assert z["elpd_waic_i_it_s_lik"].shape == (K_s,) and z["p_waic_i_it_n_lik"].shape == (K_n,)
    assert np.all(np.isfinite(z["elpd_waic_i_it_s_lik"]))
