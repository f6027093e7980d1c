"""
PSIS-LOO by individual for the titer model on the device (abd_loo.hpp): the rows the sampler keeps against the
recorded pointwise matrices in both layouts, the statistics against the fp64 restatement of DESIGN.md §27 and the host path, the
thinned matrix, what must not move (trajectories, the WAIC accumulators' bits), a run cut into several calls, the refusals of the
C ABI, and the command line.

Every run is made once (module fixtures) and shared; nothing here writes to what a fixture returns.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest

from abdpymc_amd import compare, loo, synthetic
from abdpymc_amd.data import TiterData
from tests.helpers import random_sparse_cohort
from tests.survival_loo_restatement import psis_column, rel_gap
from tests.test_gpu_individual_loglik import _same_trajectories, by_individual, order_term  # noqa: F401

pytestmark = pytest.mark.gpu

# tests/golden/NOTICE_survival_loo.md: the fp64 restatement's own gap to 40 digits, fixed before the kernel ran
G_REF = dict(elpd=7.4e-14, k=4.9e-15, lppd=3.1e-15)


def bound(what, S):
    return max(64.0 * G_REF[what], S * 2.0 ** -53)


def _namespace(n_gaps, n_inds, vacs, pcrpos, s_obs, n_obs):
    return SimpleNamespace(n_gaps=n_gaps, n_inds=n_inds, vacs=vacs, pcrpos=pcrpos, coords={"gap": np.arange(n_gaps), "ind": np.arange(n_inds)},
                           s=SimpleNamespace(obs=s_obs), n=SimpleNamespace(obs=n_obs))


def _direct(m, chains, tune, draws, seed, thin=1, calls=None, waic_ind=False):
    """A run through NativeSampler itself, started as ``sample`` starts it, with the pointwise matrices of every draw recorded:
    -> the open sampler and {"theta" (chains, draws, 17), "ll_s", "ll_n" (chains, draws, K)}"""
    from abdpymc_amd.model import THETA_NAMES

    ctx = m.ctx
    pt = m.initial_point()
    q0 = np.empty((chains, len(THETA_NAMES)))
    for c in range(chains):
        rng = np.random.default_rng([seed, c])
        ctx.set_discrete(c, pt["i_raw"].astype(np.int8), pt["ab_s_waner"].astype(np.int8))
        q0[c] = m.ravel(pt) + rng.uniform(-1, 1, size=len(THETA_NAMES))
    smp = ctx.sampler(np.arange(chains), q0, tune=tune, seed=seed, gibbs=True, accumulate=True)
    smp.enable_loo(draws, thin)
    if waic_ind:
        smp.enable_individual_loglik()
    smp.run(tune)
    out = {"ll_s": np.full((chains, draws, ctx.n_obs_s), np.nan), "ll_n": np.full((chains, draws, ctx.n_obs_n), np.nan)}
    thetas, k = [], 0
    for n in calls or [draws]:
        th, _ = smp.run_record(n, k, ll_s=out["ll_s"], ll_n=out["ll_n"])
        thetas.append(th)
        k += n
    assert k == draws
    out["theta"] = np.concatenate(thetas, axis=1)
    return smp, out


def _check_rows(rows, mat_s, mat_n, idx_s, idx_n, N, kept=slice(None)):
    """a chain's kept rows against its recorded matrices grouped on the host, within 1e-12 |T| + the summation-order term"""
    T = compare.individual_matrix(mat_s, mat_n, idx_s, idx_n, N)[kept]
    sabs = compare.individual_matrix(np.abs(mat_s), np.abs(mat_n), idx_s, idx_n, N)[kept]
    cnt = np.bincount(idx_s, minlength=N) + np.bincount(idx_n, minlength=N)
    assert rows.shape == T.shape, (rows.shape, T.shape)
    lim = 1e-12 * np.abs(T) + order_term(sabs, cnt)
    bad = np.abs(rows - T) > lim
    assert not bad.any(), (np.argwhere(bad)[:5], rows[bad][:5], T[bad][:5], lim[bad][:5])
    assert np.all(rows[:, cnt == 0] == 0.0)
    return cnt


def _check_stats(st, rows_by_chain, cnt):
    """loo_stats() against the restatement per column and the host path, on the device's own rows pooled chain-major"""
    T = np.concatenate(rows_by_chain)
    S, N = T.shape
    assert st["n_draws"] == S
    np.testing.assert_array_equal(st["n_readings"], cnt)
    has = cnt > 0
    ref = [np.zeros(N), np.full(N, np.nan), np.zeros(N), np.zeros(N, dtype=np.int64)]
    for j in np.flatnonzero(has):
        for r, v in zip(ref, psis_column(T[:, j])):
            r[j] = v
    host = compare.psis_loo_from_matrix(T, n_cells=cnt)
    for name, other in (("restatement", ref), ("host", host)):
        np.testing.assert_array_equal(st["n_tail"], other[3])
        for key, what, i in (("elpd_loo", "elpd", 0), ("pareto_k", "k", 1), ("lppd", "lppd", 2)):
            gap = rel_gap(st[key], other[i])  # (asserts that the inf / NaN pattern agrees exactly)
            print(f"S = {S}: {key} against the {name}: {gap:.3g} (bound {bound(what, S):.3g})")
            assert gap <= bound(what, S), (name, key, gap, bound(what, S))
    assert np.all(st["elpd_loo"][~has] == 0.0) and np.all(st["lppd"][~has] == 0.0) and np.all(st["n_tail"][~has] == 0)
    assert np.isnan(st["pareto_k"][~has]).all()
    return has


@pytest.fixture(scope="module")
def test_td(golden_dir):
    return TiterData.from_disk(os.path.join(golden_dir, "test_cohort"))


KW = dict(chains=3, tune=30, draws=40, seed=5)


@pytest.fixture(scope="module")
def list_run(test_td):
    """test_cohort, observation lists: 40 kept rows are two full flushes of the staging block and a remainder of 8"""
    from abdpymc_amd.model import model

    m = model(test_td, n_chains=3)
    assert not m.ctx.is_dense
    smp, out = _direct(m, **KW)
    out["rows"] = [smp.loo_rows(k) for k in range(3)]
    out["stats"], out["stats_again"] = smp.loo_stats(), smp.loo_stats()
    out["last"] = [m.ctx.individual_loglik(k, out["theta"][k, -1]) for k in range(3)]  # (the slots still hold the last draw's state)
    smp.close()
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return m, out


def test_rows_lists(test_td, list_run):
    _, out = list_run
    N = test_td.n_inds
    idx_s, idx_n = np.asarray(test_td.s.obs[1]), np.asarray(test_td.n.obs[1])
    for k in range(3):
        assert out["rows"][k].shape == (40, N)
        _check_rows(out["rows"][k], out["ll_s"][k], out["ll_n"][k], idx_s, idx_n, N)
        # after the run the slot holds the last draw's discrete state (queue_draw comes behind the iteration's sweep, and nothing
        # but a sweep rewrites it): the last row is the bits of the one-point entry, added as IndLogLik::put adds them
        ll_s, ll_n = out["last"][k]
        np.testing.assert_array_equal(out["rows"][k][-1], ll_s + ll_n)


def test_stats_lists(test_td, list_run):
    _, out = list_run
    cnt = np.bincount(np.asarray(test_td.s.obs[1]), minlength=test_td.n_inds) + np.bincount(np.asarray(test_td.n.obs[1]), minlength=test_td.n_inds)
    has = _check_stats(out["stats"], out["rows"], cnt)  # S = 120: M = 24
    assert has.any() and np.isfinite(out["stats"]["pareto_k"][has]).all()  # a test that only saw k = inf would check nothing
    assert (out["stats"]["n_tail"][has] > 4).all() and (out["stats"]["n_tail"][has] <= 24).all()
    for key in ("elpd_loo", "pareto_k", "lppd", "n_tail"):  # the call consumes nothing
        np.testing.assert_array_equal(out["stats"][key], out["stats_again"][key])


def test_rows_and_stats_dense():
    from abdpymc_amd.model import AbdModel

    sc = synthetic.make_cohort(130, 65, seed=31)  # N = 130, G = 65: ld = 192, 62 padding slots, the store kernel's one block partly idle
    m = AbdModel(_namespace(sc.n_gaps, sc.n_inds, sc.vacs, sc.pcrpos, sc.s_obs, sc.n_obs), n_chains=2)
    assert m.ctx.is_dense and sc.n_inds == 130
    smp, out = _direct(m, chains=2, tune=4, draws=20, seed=3)
    rows = [smp.loo_rows(k) for k in range(2)]
    st = smp.loo_stats()
    smp.close()
    idx = np.asarray(sc.idx_ind)
    for k in range(2):
        cnt = _check_rows(rows[k], out["ll_s"][k], out["ll_n"][k], idx, idx, sc.n_inds)
    _check_stats(st, rows, cnt)  # S = 40: M = 8


def test_individuals_without_readings():
    """the cohort of test_gpu_individual_loglik.test_empty_individuals_and_empty_antigen: N = 50, ld = 64, no N reading at all"""
    from abdpymc_amd.model import AbdModel

    coh = random_sparse_cohort(50, 31, 20, 0, seed=3)
    obs = lambda o: (o.idx_gap, o.idx_ind, o.log_dilution, o.od)  # noqa: E731
    m = AbdModel(_namespace(coh.n_gaps, coh.n_inds, coh.vacs, coh.pcrpos, obs(coh.s), obs(coh.n)), n_chains=2)
    smp, out = _direct(m, chains=2, tune=4, draws=20, seed=3)
    rows = [smp.loo_rows(k) for k in range(2)]
    st = smp.loo_stats()
    smp.close()
    has = np.bincount(coh.s.idx_ind, minlength=50) > 0
    assert (~has).sum() >= 30
    for k in range(2):
        cnt = _check_rows(rows[k], out["ll_s"][k], out["ll_n"][k], np.asarray(coh.s.idx_ind), np.asarray(coh.n.idx_ind), 50)
        assert np.all(rows[k][:, ~has] == 0.0) and np.all(rows[k][:, has] != 0.0)
    np.testing.assert_array_equal(cnt > 0, has)
    _check_stats(st, rows, cnt)
    assert np.isnan(st["pareto_k"][~has]).all() and np.all(st["elpd_loo"][~has] == 0.0) and np.all(st["n_tail"][~has] == 0)


def test_thinned_rows_are_every_third_row(list_run):
    m, full = list_run
    smp, out = _direct(m, thin=3, **KW)  # C = 14
    rows = [smp.loo_rows(k) for k in range(3)]
    st = smp.loo_stats()
    smp.close()
    np.testing.assert_array_equal(out["theta"], full["theta"])
    for k in range(3):
        assert rows[k].shape == (14, full["rows"][k].shape[1])
        np.testing.assert_array_equal(rows[k], full["rows"][k][::3])
    assert st["n_draws"] == 3 * 14


def test_nothing_else_moves(list_run):
    from abdpymc_amd.sampler import sample

    m, full = list_run
    kw = dict(tune=30, draws=40, chains=3, seed=5, record_deterministics=False, thin=3)
    plain = sample(m, **kw)
    with_loo = sample(m, loo=True, loo_thin=3, **kw)
    _same_trajectories(with_loo, plain)
    assert with_loo["loo_n_draws"].tolist() == [3 * 14] and not [k for k in plain if k.startswith("loo_")]
    # sample() starts its chains as the direct runs above do: the thinned matrix's statistics are those of that run's rows
    T = np.concatenate([r[::3] for r in full["rows"]])
    elpd, k, lppd, n_tail = compare.psis_loo_from_matrix(T, n_cells=with_loo["loo_n_readings"])
    np.testing.assert_array_equal(with_loo["loo_n_tail"], n_tail)
    assert rel_gap(with_loo["loo_elpd_i"], elpd) <= bound("elpd", 42) and rel_gap(with_loo["loo_pareto_k"], k) <= bound("k", 42)
    w = loo.loo(with_loo)
    assert w["n_draws"] == 42 and np.isfinite(w["elpd_loo"]) and w["p_loo"] > 0
    ind = sample(m, waic=True, waic_by="individual", **kw)
    both = sample(m, waic=True, waic_by="individual", loo=True, **kw)
    _same_trajectories(both, plain)
    for key in ("waic_ind_lse", "waic_ind_mean", "waic_ind_m2", "waic_ind_n_readings", "waic_n_draws"):
        np.testing.assert_array_equal(both[key], ind[key])
    assert both["loo_n_draws"].tolist() == [120]
    np.testing.assert_array_equal(both["loo_elpd_i"], full["stats"]["elpd_loo"])  # one launch serves both: the same rows
    np.testing.assert_array_equal(both["loo_pareto_k"], full["stats"]["pareto_k"])


def test_a_run_cut_into_several_calls(test_td, list_run):
    """draws 7 + 16 + 17: the first call ends with a partly filled staging block, and every later flush starts off a line"""
    m, full = list_run
    smp, out = _direct(m, calls=[7, 16, 17], waic_ind=True, **KW)
    rows = [smp.loo_rows(k) for k in range(3)]
    a, b = smp.loo_stats(), smp.loo_stats()
    part = smp.loo_rows(1, 5, 12)
    smp.close()
    N = test_td.n_inds
    idx_s, idx_n = np.asarray(test_td.s.obs[1]), np.asarray(test_td.n.obs[1])
    for k in range(3):
        _check_rows(rows[k], out["ll_s"][k], out["ll_n"][k], idx_s, idx_n, N)
    np.testing.assert_array_equal(part, rows[1][5:17])
    for key in ("elpd_loo", "pareto_k", "lppd", "n_tail", "n_readings"):
        np.testing.assert_array_equal(a[key], b[key])
    assert a["n_draws"] == b["n_draws"] == 120


def test_refusals_of_the_c_abi(list_run):
    from abdpymc_amd._native import AbdError

    m, _ = list_run
    ctx = m.ctx
    q0 = np.tile(m.ravel(m.initial_point()), (3, 1))
    for c in range(3):
        pt = m.initial_point()
        ctx.set_discrete(c, pt["i_raw"].astype(np.int8), pt["ab_s_waner"].astype(np.int8))
    smp = ctx.sampler(np.arange(3), q0, tune=2, seed=1, gibbs=True)
    with pytest.raises(ValueError, match=r"3 chains x 6000 kept draws = 18000 pass the cap of 16384"):
        smp.enable_loo(6000)
    with pytest.raises(AbdError, match="loo is not enabled"):  # nothing was allocated
        smp.loo_rows(0)
    with pytest.raises(ValueError, match="thin=0"):
        smp.enable_loo(10, 0)
    with pytest.raises(ValueError, match="negative"):
        smp.enable_loo(-1)
    smp.enable_loo(6000, 2)  # 3 x 3000 fits; and again, smaller: the first is released
    smp.enable_loo(10)
    smp.run(2 + 7)
    with pytest.raises(AbdError, match=r"\[-3\] loo: chain 0 holds 7 of its 10 rows"):
        smp.loo_stats()
    assert smp.loo_rows(2).shape == (7, ctx.n_inds)
    with pytest.raises(ValueError, match=r"loo: rows \[5, 8\) are beyond the 7 the chain holds"):
        smp.loo_rows(0, 5, 3)
    with pytest.raises(AbdError, match=r"\[-3\] loo must be enabled before the first"):
        smp.enable_loo(20)
    with pytest.raises(AbdError, match=r"\[-3\] loo: draws up to 11 pass the planned 10"):
        smp.run(4)
    smp.run(3)
    assert smp.loo_stats()["n_draws"] == 30
    smp.close()


@pytest.mark.filterwarnings("ignore:LOO by individual")  # (60 draws of 10 individuals: some k pass 0.7, and the report says so)
def test_cli(tmp_path, golden_dir, capsys):
    from abdpymc_amd import cli

    out = tmp_path / "post.npz"
    rc = cli.main(["--tune", "6", "--draws", "30", "--cores", "1", "--ititers_data", os.path.join(golden_dir, "test_cohort"), "--loo",
                   "--netcdf", str(out)])
    assert rc == 0
    line = [ln for ln in capsys.readouterr().err.splitlines() if ln.startswith("LOO by individual:")]
    assert line and np.isfinite(float(line[0].split()[4])) and "60 draws" in line[0]
    z = np.load(out)
    td = TiterData.from_disk(os.path.join(golden_dir, "test_cohort"))
    assert z["elpd_loo_ind"].shape == (td.n_inds,) and z["pareto_k_ind"].shape == (td.n_inds,) and z["p_loo_ind"].shape == (td.n_inds,)
    assert np.isfinite(z["elpd_loo_ind"]).all()
    np.testing.assert_array_equal(z["elpd_loo_ind"], loo.loo(z)["elpd_i"])
