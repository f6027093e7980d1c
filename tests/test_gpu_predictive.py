"""
Posterior predictive replicates and check statistics of the OD readings (abd_posterior_predictive; the native sampler's
recorded replicates and accumulators) against the frozen oracle -- mu from O.deterministics, the logistic curve -- and the
numpy restatement of the normals' stream (tests/test_predictive_cpu.py).
"""
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from abdpymc_amd import predictive, synthetic
from abdpymc_amd.data import TiterData
from oracle import abd_oracle as O
from tests.helpers import oracle_cohort_from_synth, random_sparse_cohort
from tests.test_data_loader import default_cohort
from tests.test_gpu_pointwise import _cohort_of, _ctx, _same_trajectories, _state, _theta_rows
from tests.test_predictive_cpu import stream_normals

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-12, 1e-13
SEED, STREAM, DRAW = 0x1234_5678_9ABC, 3, 2 ** 33 + 41
_erfc = np.vectorize(math.erfc, otypes=[float])


def oracle_mean(coh, theta, i_raw, w, splits=None, ignore=False):
    """(m_s, m_n, sigma_s, sigma_n): the noise-free predictive mean of every reading, as oracle_ll of test_gpu_pointwise forms it"""
    c = O.constrained(theta)
    _, mu_n, mu_s = O.deterministics(theta, i_raw, w, coh, splits, ignore)

    def one(o, mu, b, d):
        return O.logistic(np.asarray(o.log_dilution, float), mu[np.asarray(o.idx_gap), np.asarray(o.idx_ind)], b, d)

    return one(coh.s, mu_s, c["b_s"], c["d_s"]), one(coh.n, mu_n, c["b_n"], c["d_n"]), c["sigma_s"], c["sigma_n"]


def _check(coh, ctx, seed, splits=None, ignore=False, ref_coh=None, key=(SEED, STREAM, DRAW)):
    """-> theta, (z_s, z_n) implied by the device's replicates, (m_s, m_n) of the device"""
    theta, i_raw, w = _state(coh, seed)
    ctx.set_discrete(0, i_raw, w)
    y_s, y_n, m_s, m_n = ctx.posterior_predictive(0, theta, *key, mean=True)
    r_s, r_n, sig_s, sig_n = oracle_mean(ref_coh or coh, theta, i_raw, w, splits, ignore)
    assert y_s.shape == m_s.shape == r_s.shape and y_n.shape == m_n.shape == r_n.shape
    np.testing.assert_allclose(m_s, r_s, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(m_n, r_n, rtol=RTOL, atol=ATOL)
    z_s = stream_normals(key[0], key[1], key[2], 0, np.arange(r_s.size))
    z_n = stream_normals(key[0], key[1], key[2], 1, np.arange(r_n.size))
    np.testing.assert_allclose(y_s, r_s + sig_s * z_s, rtol=0, atol=1e-12)
    np.testing.assert_allclose(y_n, r_n + sig_n * z_n, rtol=0, atol=1e-12)
    return theta, ((y_s - m_s) / sig_s, (y_n - m_n) / sig_n), (m_s, m_n)


@pytest.fixture(scope="module")
def test_td(golden_dir):
    return TiterData.from_disk(os.path.join(golden_dir, "test_cohort"))


@pytest.mark.parametrize("splits,ignore", [(None, False), ((14, 20), False), (None, True)])
def test_golden_test_cohort(test_td, splits, ignore):
    coh = _cohort_of(test_td)
    ctx = _ctx(coh, splits, ignore)
    for seed in range(3):
        _check(coh, ctx, seed, splits, ignore)


def test_default_cohort(golden_dir):
    coh = _cohort_of(default_cohort(golden_dir))
    ctx = _ctx(coh)
    assert not ctx.is_dense
    _check(coh, ctx, 1)


@pytest.mark.parametrize("G", [40, 300])
def test_random_sparse(G):
    coh = random_sparse_cohort(60, G, 900, 700, seed=G)
    _check(coh, _ctx(coh), G)


@pytest.mark.parametrize("G,N", [(70, 100), (200, 50)])
def test_dense_f64(G, N):
    coh = oracle_cohort_from_synth(synthetic.make_cohort(N, G, seed=G + N))
    ctx = _ctx(coh)
    assert ctx.is_dense
    _check(coh, ctx, 2)


@pytest.mark.parametrize("G,N", [(60, 100), (200, 50)])
def test_dense_f32_storage(G, N):
    coh = oracle_cohort_from_synth(synthetic.make_cohort(N, G, seed=G * 3 + N))
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)  # noqa: E731
    ref = O.Cohort(coh.n_gaps, coh.n_inds, coh.vacs, coh.pcrpos,
                   O.AntigenObs(coh.s.idx_gap, coh.s.idx_ind, f32(coh.s.log_dilution), f32(coh.s.od)),
                   O.AntigenObs(coh.n.idx_gap, coh.n.idx_ind, f32(coh.n.log_dilution), f32(coh.n.od)))
    _check(coh, _ctx(coh, storage="f32"), 2, ref_coh=ref)


def test_dense_kept_as_lists_draws_the_same_noise(monkeypatch):
    coh = oracle_cohort_from_synth(synthetic.make_cohort(70, 65, seed=5))
    dense = _ctx(coh)
    assert dense.is_dense
    _, z_d, _ = _check(coh, dense, 4)
    monkeypatch.setenv("ABD_FORCE_SPARSE", "1")
    lists = _ctx(coh)
    assert not lists.is_dense
    _, z_l, _ = _check(coh, lists, 4)
    for a, b in zip(z_d, z_l):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-11)


@pytest.mark.parametrize("which", ["test", "sparse"])
def test_shuffled_readings_keep_their_noise_by_caller_index(test_td, which):
    coh = _cohort_of(test_td) if which == "test" else random_sparse_cohort(40, 31, 500, 400, seed=9)
    rng = np.random.default_rng(1)
    ps, pn = rng.permutation(coh.s.od.size), rng.permutation(coh.n.od.size)
    sh = lambda o, p: O.AntigenObs(*(np.asarray(a)[p] for a in (o.idx_gap, o.idx_ind, o.log_dilution, o.od)))  # noqa: E731
    coh2 = O.Cohort(coh.n_gaps, coh.n_inds, coh.vacs, coh.pcrpos, sh(coh.s, ps), sh(coh.n, pn))
    _, z1, m1 = _check(coh, _ctx(coh), 3)
    _, z2, m2 = _check(coh2, _ctx(coh2), 3)
    np.testing.assert_allclose(z2[0], z1[0], rtol=0, atol=1e-11)  # the noise belongs to the caller's index r ...
    np.testing.assert_allclose(z2[1], z1[1], rtol=0, atol=1e-11)
    np.testing.assert_array_equal(m2[0], m1[0][ps])  # ... the means to their readings
    np.testing.assert_array_equal(m2[1], m1[1][pn])


def test_repeatable_and_keyed(test_td):
    coh = _cohort_of(test_td)
    ctx = _ctx(coh)
    theta, i_raw, w = _state(coh, 0)
    ctx.set_discrete(0, i_raw, w)
    a = np.concatenate(ctx.posterior_predictive(0, theta, SEED, STREAM, DRAW))
    b = np.concatenate(ctx.posterior_predictive(0, theta, SEED, STREAM, DRAW))
    np.testing.assert_array_equal(a, b)
    for key in ((SEED + 1, STREAM, DRAW), (SEED, STREAM + 1, DRAW), (SEED, STREAM, DRAW + 1), (SEED, STREAM, DRAW + 2 ** 32)):
        c = np.concatenate(ctx.posterior_predictive(0, theta, *key))
        assert not np.any(a == c)


def test_one_reading_moments():
    coh = random_sparse_cohort(10, 31, 1, 0, seed=2)
    ctx = _ctx(coh)
    theta, i_raw, w = _state(coh, 1)
    ctx.set_discrete(0, i_raw, w)
    m, _, sig, _ = oracle_mean(coh, theta, i_raw, w)
    n = 4000
    y = np.array([ctx.posterior_predictive(0, theta, 9, 0, d)[0][0] for d in range(n)])
    assert abs(y.mean() - m[0]) < 4 * sig / math.sqrt(n)
    assert abs(y.std() - sig) < 4 * sig / math.sqrt(2 * n)


def _oracle_stats(coh, res, tune, seed, splits=None, ignore=False):
    """the accumulators recomputed from the recorded (unthinned) states by the oracle, chains merged"""
    th = _theta_rows(res)
    ys, yn = np.asarray(coh.s.od, float), np.asarray(coh.n.od, float)
    ms, ps = [], []
    for c in range(th.shape[0]):
        for d in range(th.shape[1]):
            r_s, r_n, sig_s, sig_n = oracle_mean(coh, th[c, d], res["i_raw"][c, d], res["ab_s_waner"][c, d], splits, ignore)
            ms.append(np.concatenate([r_s, r_n]))
            ps.append(0.5 * _erfc(np.concatenate([(r_s - ys) / sig_s, (r_n - yn) / sig_n]) / math.sqrt(2.0)))
    return predictive.stats_from_matrix(np.array(ms), np.array(ps))


def _check_sampler(m, coh, kw, rec_slot):
    from abdpymc_amd.sampler import sample

    full = sample(m, thin=1, posterior_predictive=True, ppc=True, **kw)
    half = sample(m, thin=2, posterior_predictive=True, ppc=True, **kw)
    plain = sample(m, thin=1, **kw)
    chains, draws, tune, seed = kw["chains"], kw["draws"], kw["tune"], kw["seed"]
    K_s, K_n = m.ctx.n_obs_s, m.ctx.n_obs_n
    assert full["posterior_predictive_it_s_lik"].shape == (chains, draws, K_s)
    assert half["posterior_predictive_it_n_lik"].shape == (chains, (draws + 1) // 2, K_n)
    # the feature changes nothing the chains draw
    _same_trajectories(full, plain)
    _same_trajectories(half, plain, keys=())
    for k in ("i_raw", "ab_s_waner"):
        np.testing.assert_array_equal(half[k], plain[k][:, ::2])
    # every recorded replicate is abd_posterior_predictive at the recorded draw, bit for bit
    th = _theta_rows(full)
    for c in range(chains):
        for d in range(draws):
            m.ctx.set_discrete(rec_slot, full["i_raw"][c, d], full["ab_s_waner"][c, d])
            y_s, y_n = m.ctx.posterior_predictive(rec_slot, th[c, d], seed=seed, stream=c, draw=tune + d)
            np.testing.assert_array_equal(full["posterior_predictive_it_s_lik"][c, d], y_s)
            np.testing.assert_array_equal(full["posterior_predictive_it_n_lik"][c, d], y_n)
    again = predictive.sample_posterior_predictive(m, full, tune=tune, seed=seed, slot=rec_slot)
    np.testing.assert_array_equal(again["it_s_lik"], full["posterior_predictive_it_s_lik"])
    np.testing.assert_array_equal(again["it_n_lik"], full["posterior_predictive_it_n_lik"])
    for k in ("posterior_predictive_it_s_lik", "posterior_predictive_it_n_lik"):
        np.testing.assert_array_equal(half[k], full[k][:, ::2])
    # the device accumulators: every draw, whatever the thinning
    want = _oracle_stats(coh, full, tune, seed, m.splits or None, m.ignore_pcrpos)
    for r in (full, half):
        assert list(r["ppc_n_draws"]) == [draws] * chains and list(r["ppc_n_obs"][0]) == [K_s, K_n]
        got = predictive.merge(*predictive.chain_stats(r))
        assert got[3] == want[3]
        for g, w in zip(got[:3], want[:3]):
            np.testing.assert_allclose(g, w, rtol=1e-10, atol=1e-10)
    sm = predictive.summary(full)
    assert sm["it_s_lik"]["p"].shape == (K_s,) and sm["it_n_lik"]["hist"].sum() == K_n


def test_sampler_test_cohort(test_td):
    from abdpymc_amd.model import model

    m = model(test_td, n_chains=4)
    assert not m.ctx.is_dense
    _check_sampler(m, _cohort_of(test_td), dict(tune=20, draws=12, chains=3, seed=5, record_deterministics=False), rec_slot=3)


def test_sampler_dense_trains():
    """a dense cohort large enough for leapfrog trains (chains' sweeps and predictive launches on their side streams)"""
    from abdpymc_amd.model import AbdModel

    sc = synthetic.make_cohort(400, 120, seed=31)
    d = SimpleNamespace(n_gaps=sc.n_gaps, n_inds=sc.n_inds, vacs=sc.vacs, pcrpos=sc.pcrpos,
                        coords={"gap": np.arange(sc.n_gaps), "ind": np.arange(sc.n_inds)},
                        s=SimpleNamespace(obs=sc.s_obs), n=SimpleNamespace(obs=sc.n_obs))
    m = AbdModel(d, n_chains=3)
    assert m.ctx.is_dense
    _check_sampler(m, oracle_cohort_from_synth(sc), dict(tune=4, draws=6, chains=2, seed=3, record_deterministics=False),
                   rec_slot=2)


def test_cli_ppc_and_posterior_predictive(tmp_path, golden_dir, capsys, monkeypatch):
    from abdpymc_amd import cli

    monkeypatch.setitem(sys.modules, "arviz", None)  # the .npz output
    out = tmp_path / "post.npz"
    rc = cli.main(["--tune", "6", "--draws", "5", "--cores", "1", "--ititers_data", os.path.join(golden_dir, "test_cohort"),
                   "--ppc", "--posterior_predictive", "--thin", "2", "--netcdf", str(out)])
    assert rc == 0
    err = capsys.readouterr().err
    lines = [ln for ln in err.splitlines() if ln.startswith("PPC ")]
    assert len(lines) == 2 and "it_s_lik" in lines[0] and "it_n_lik" in lines[1]
    z = np.load(out)
    td = TiterData.from_disk(os.path.join(golden_dir, "test_cohort"))
    K_s, K_n = td.s.obs[0].size, td.n.obs[0].size
    assert z["posterior_predictive_it_s_lik"].shape == (2, 3, K_s) and z["posterior_predictive_it_n_lik"].shape == (2, 3, K_n)
    assert z["ppc_p_it_s_lik"].shape == (K_s,) and z["ppc_p_it_n_lik"].shape == (K_n,)
    assert z["ppc_pit"].shape == (2, K_s + K_n) and list(z["ppc_n_draws"]) == [5, 5]
    np.testing.assert_array_equal(z["observed_data_it_s_lik"], td.s.obs[3])
    np.testing.assert_array_equal(z["observed_data_it_n_lik"], td.n.obs[3])
    assert np.all((z["ppc_p_it_s_lik"] >= 0) & (z["ppc_p_it_s_lik"] <= 1))
