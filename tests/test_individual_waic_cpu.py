"""
WAIC by individual (abdpymc_amd.compare, ``waic_by``) without a GPU: the regrouping of a pointwise matrix, the formulas over
individuals, the summary's plumbing against a stub sampler, the CLI's refusals and the new entry points' NULL checks.
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from abdpymc_amd import compare, sampler, summaries
from tests.test_summaries_plumbing_cpu import CHAINS, DRAWS, G, K_N, K_S, N, StubContext, StubModel, StubSampler

N_READINGS = np.array([3, 0, 1, 0, 2, 1, 0])  # of the stub's N = 7 individuals


class IndStubSampler(StubSampler):
    def enable_individual_loglik(self):
        self.calls.append(("enable_individual_loglik",))

    def individual_loglik_stats(self, k):
        self.calls.append(("individual_loglik_stats", k))
        return np.zeros((3, N)), DRAWS, N_READINGS.copy()

    def pointwise_stats(self, k):
        self.calls.append(("pointwise_stats", k))
        return super().pointwise_stats(k)


class IndStubContext(StubContext):
    def sampler(self, chains, theta0, **kw):
        self.calls.append(("sampler", sorted(kw)))
        return IndStubSampler(self.calls, len(chains))


class IndStubModel(StubModel):
    def __init__(self):
        self.ctx = IndStubContext()


def run(**kw):
    m = IndStubModel()
    res = sampler.sample(m, tune=2, draws=DRAWS, chains=CHAINS, **kw)
    return res, [c for c in m.ctx.calls if c[0].startswith("enable_")], [c[0] for c in m.ctx.calls if c[0].endswith("_stats")]


def _loop_matrix(ll_s, ll_n, idx_s, idx_n, n):
    out = np.zeros(ll_s.shape[:-1] + (n,))
    for ll, idx in ((ll_s, idx_s), (ll_n, idx_n)):
        for k, j in enumerate(idx):
            out[..., j] += ll[..., k]
    return out


@pytest.mark.parametrize("k_s, k_n", [(40, 30), (25, 0), (0, 0)])
def test_individual_matrix_against_a_loop(k_s, k_n):
    rng = np.random.default_rng(k_s + k_n)
    n = 9
    idx_s, idx_n = rng.integers(0, n - 1, k_s), rng.integers(0, n - 1, k_n)  # shuffled; individual n - 1 has no reading
    ll_s, ll_n = rng.standard_normal((3, 5, k_s)), rng.standard_normal((3, 5, k_n))
    T = compare.individual_matrix(ll_s, ll_n, idx_s, idx_n, n)
    assert T.shape == (3, 5, n) and np.all(T[..., n - 1] == 0.0)
    np.testing.assert_allclose(T, _loop_matrix(ll_s, ll_n, idx_s, idx_n, n), rtol=1e-13, atol=1e-13)
    np.testing.assert_array_equal(compare.individual_matrix(ll_s[0, 0], ll_n[0, 0], idx_s, idx_n, n), T[0, 0])
    p = rng.permutation(k_s)  # the order the readings are given in moves nothing but rounding
    np.testing.assert_allclose(compare.individual_matrix(ll_s[..., p], ll_n, idx_s[p], idx_n, n), T, rtol=1e-13, atol=1e-13)
    with pytest.raises(ValueError):
        compare.individual_matrix(ll_s, ll_n, np.full(k_s, n), idx_n, n) if k_s else compare.individual_matrix(ll_s, ll_n[:1], idx_s, idx_n, n)


def _grouped_case(seed=0, chains=3, draws=30, K=120, n=17):
    rng = np.random.default_rng(seed)
    ll = -1.0 + 0.4 * rng.standard_normal((chains, draws, K))
    groups = rng.integers(0, n - 3, K)  # the last three individuals have no reading
    T = _loop_matrix(ll, ll[..., :0], groups, groups[:0], n)
    cnt = np.bincount(groups, minlength=n)
    per_chain = [compare.stats_from_matrix(T[c]) for c in range(chains)]
    res = {"waic_ind_lse": np.stack([p[0] for p in per_chain]), "waic_ind_mean": np.stack([p[1] for p in per_chain]),
           "waic_ind_m2": np.stack([p[2] for p in per_chain]), "waic_n_draws": np.array([p[3] for p in per_chain]),
           "waic_ind_n_readings": np.tile(cnt, (chains, 1))}
    return ll, groups, T, cnt, res


def test_waic_by_individual_from_merged_statistics_equals_the_grouped_matrix():
    ll, groups, T, cnt, res = _grouped_case()
    n = cnt.size
    w = compare.waic(res, by="individual")
    assert compare.waic(res)["n_individuals"] == w["n_individuals"]  # by=None: per individual where that is all there is
    wm = compare.waic_from_matrix(ll, groups=groups, n_groups=n)
    np.testing.assert_allclose([w["elpd_waic"], w["p_waic"], w["se"]], [wm["elpd_waic"], wm["p_waic"], wm["se"]], rtol=1e-10)
    np.testing.assert_allclose(w["elpd_i"], wm["elpd_i"], rtol=1e-10, atol=1e-13)
    lse, mean, m2, S = compare.merge(*compare.chain_stats(res, by="individual"))
    r = compare.stats_from_matrix(T.reshape(-1, n))
    np.testing.assert_allclose(lse, r[0], rtol=1e-12)
    np.testing.assert_allclose(mean, r[1], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(m2, r[2], rtol=1e-9)
    # the formulas, written out over the individuals with readings only
    has = cnt > 0
    Tp = T.reshape(-1, n)
    elpd = np.log(np.mean(np.exp(Tp), axis=0)) - np.var(Tp, axis=0)
    assert w["elpd_i"].shape == w["p_waic_i"].shape == (n,) and np.all(w["elpd_i"][~has] == 0.0) and np.all(w["p_waic_i"][~has] == 0.0)
    assert w["n_individuals"] == int(has.sum()) == n - 3 and w["n_draws"] == S == 90 and w["n_readings"] == 120
    m = has.sum()
    assert w["se"] == pytest.approx(np.sqrt(m * np.var(elpd[has])), rel=1e-10)
    assert w["se"] != pytest.approx(np.sqrt(n * np.var(np.where(has, elpd, 0.0))), rel=1e-6)  # not over all N
    assert w["elpd_waic"] == pytest.approx(elpd[has].sum(), rel=1e-10)
    assert w["n_warn"] == int((np.var(Tp, axis=0)[has] > 0.4).sum()) > 0
    with pytest.raises(ValueError, match="by"):
        compare.waic(res, by="subject")
    with pytest.raises(ValueError, match="waic_ind"):
        compare.waic({"waic_lse": res["waic_ind_lse"], "waic_mean": res["waic_ind_mean"], "waic_m2": res["waic_ind_m2"],
                      "waic_n_draws": res["waic_n_draws"]}, by="individual")


def test_compare_by_individual_dse_by_hand():
    ll, groups, T, cnt, res_a = _grouped_case(1)
    rng = np.random.default_rng(2)
    ll_b = ll + 0.2 * rng.standard_normal(ll.shape) - 0.05
    n = cnt.size
    res_b = dict(res_a)
    Tb = _loop_matrix(ll_b, ll_b[..., :0], groups, groups[:0], n)
    per_chain = [compare.stats_from_matrix(Tb[c]) for c in range(Tb.shape[0])]
    for j, k in enumerate(("lse", "mean", "m2")):
        res_b["waic_ind_" + k] = np.stack([p[j] for p in per_chain])
    out = compare.compare({"A": res_a, "B": res_b}, by="individual")
    wa, wb = compare.waic(res_a, by="individual"), compare.waic(res_b, by="individual")
    best, other = ("A", "B") if wa["elpd_waic"] >= wb["elpd_waic"] else ("B", "A")
    has = cnt > 0
    d = ((wa if best == "A" else wb)["elpd_i"] - (wb if best == "A" else wa)["elpd_i"])[has]
    dse = np.sqrt(sum((x - sum(d) / len(d)) ** 2 for x in d) / len(d) * len(d))  # sqrt(n var), ddof 0, n individuals with readings
    assert out[best]["rank"] == 0 and out[best]["dse"] == 0.0
    assert out[other]["elpd_diff"] == pytest.approx(float(d.sum()), rel=1e-12)
    assert out[other]["dse"] == pytest.approx(dse, rel=1e-12)
    assert compare.compare({"A": wa, "B": wb})[other]["dse"] == pytest.approx(dse, rel=1e-12)  # dictionaries of waic(), by=None
    # a variant that has only per-reading statistics is named
    per_reading = {"waic_lse": np.zeros((1, 4)), "waic_mean": np.zeros((1, 4)), "waic_m2": np.zeros((1, 4)), "waic_n_draws": np.array([5])}
    with pytest.raises(ValueError, match="plain"):
        compare.compare({"A": res_a, "plain": per_reading}, by="individual")
    with pytest.raises(ValueError, match="A"):
        compare.compare({"A": res_a, "plain": per_reading}, by="reading")
    with pytest.raises(ValueError, match="mix"):
        compare.compare({"A": wa, "plain": compare.waic(per_reading)})


def test_enable_calls_and_keys_of_the_three_values():
    reading = {"waic_lse", "waic_mean", "waic_m2", "waic_n_draws", "waic_n_obs"}
    individual = {"waic_ind_lse", "waic_ind_mean", "waic_ind_m2", "waic_ind_n_readings", "waic_n_draws"}
    res, calls, stats = run(waic=True, waic_by="reading")
    assert calls == [("enable_pointwise",)] and {k for k in res if k.startswith("waic_")} == reading
    assert set(stats) == {"pointwise_stats"}
    res, calls, stats = run(waic=True, waic_by="individual")
    assert calls == [("enable_individual_loglik",)] and {k for k in res if k.startswith("waic_")} == individual
    assert set(stats) == {"individual_loglik_stats"}  # nothing per reading is asked for either
    assert res["waic_ind_lse"].shape == res["waic_ind_n_readings"].shape == (CHAINS, N) and res["waic_n_draws"].shape == (CHAINS,)
    assert res["waic_ind_n_readings"].dtype == np.int64
    res, calls, _ = run(waic=True, waic_by="both")
    assert calls == [("enable_pointwise",), ("enable_individual_loglik",)]
    assert {k for k in res if k.startswith("waic_")} == reading | individual
    assert res["waic_lse"].shape == (CHAINS, K_S + K_N)


def test_reading_is_what_omitting_the_option_is():
    a, calls_a, stats_a = run(waic=True)
    b, calls_b, stats_b = run(waic=True, waic_by="reading")
    assert calls_a == calls_b == [("enable_pointwise",)] and stats_a == stats_b
    assert list(a) == list(b) and all(np.array_equal(a[k], b[k]) for k in a)
    res, calls, _ = run(waic_by="individual")  # without waic the option switches nothing on
    assert calls == [] and not [k for k in res if k.startswith("waic_")]
    assert compare.SUMMARY.options == {"waic": False, "waic_by": "reading"}


def test_an_unknown_unit_is_refused_before_the_device_is_touched():
    m = IndStubModel()
    with pytest.raises(ValueError, match="subject"):
        sampler.sample(m, tune=1, draws=2, waic=True, waic_by="subject")
    assert m.ctx.calls == []


def test_host_sampler_refuses_it():
    m = IndStubModel()
    with pytest.raises(ValueError, match="native"):
        sampler.sample(m, tune=1, draws=2, native=False, waic=True, waic_by="individual")
    assert m.ctx.calls == []


def test_cli_flag(golden_dir):
    from abdpymc_amd import cli

    a = cli.build_parser().parse_args(["--tune", "1", "--draws", "1", "--waic", "--waic_by", "individual"])
    assert a.waic and a.waic_by == "individual"
    assert cli.build_parser().parse_args(["--tune", "1", "--draws", "1", "--waic"]).waic_by is None
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["--tune", "1", "--draws", "1", "--waic", "--waic_by", "subject"])
    with pytest.raises(SystemExit, match="--waic"):  # before a model is built
        cli.main(["--tune", "1", "--draws", "1", "--cores", "1", "--ititers_data", os.path.join(golden_dir, "test_cohort"),
                  "--waic_by", "individual"])
    opts = compare.SUMMARY.cli_options(a, None, 2, 1)
    assert opts == {"waic": True, "waic_by": "individual"}
    assert compare.SUMMARY.cli_options(cli.build_parser().parse_args(["--tune", "1", "--draws", "1"]), None, 2, 1) == {
        "waic": False, "waic_by": "reading"}


def test_report_lines_and_the_npz_writer(tmp_path, monkeypatch):
    from abdpymc_amd import cli

    monkeypatch.setitem(sys.modules, "arviz", None)
    data = SimpleNamespace(coords={"gap": np.arange(G), "ind": np.arange(100, 100 + N)})
    res, _, _ = run(waic=True, waic_by="individual")
    rng = np.random.default_rng(0)
    res["waic_ind_lse"] = rng.standard_normal((CHAINS, N)) - 20.0
    res["waic_ind_lse"][:, 4] = -90.0  # the worst of those with readings (3, with none, is lower still)
    res["waic_ind_lse"][:, 3] = -500.0
    lines = compare.SUMMARY.report(res, data)
    assert len(lines) == 1 and lines[0].startswith("WAIC by individual: elpd_waic ")
    assert f"({int((N_READINGS > 0).sum())} individuals, {CHAINS * DRAWS} draws; 0 with p_waic_j > 0.4; worst: individual 104 elpd " in lines[0]
    assert res["elpd_waic_ind"].shape == res["p_waic_ind"].shape == (N,) and res["elpd_waic_ind"][3] == 0.0
    both, _, _ = run(waic=True, waic_by="both")
    lines = compare.SUMMARY.report(both, data)
    assert [ln.split(":")[0] for ln in lines] == ["WAIC", "WAIC by individual"]
    plain, _, _ = run(waic=True)
    assert [ln.split(":")[0] for ln in compare.SUMMARY.report(plain, data)] == ["WAIC"] and "elpd_waic_ind" not in plain
    out = cli.write_posterior(dict(both), str(tmp_path / "post.npz"), data.coords)
    z = np.load(out)
    assert z["elpd_waic_ind"].shape == (N,) and z["p_waic_ind"].shape == (N,)
    owner = {k: next((s for s in summaries.registry() if s.owns(k)), None) for k in both}
    group = {k: s.group(k) for k, s in owner.items() if s is not None}
    assert {k for k, g in group.items() if g == "constant_data"} >= {"elpd_waic_ind", "p_waic_ind", "elpd_waic_i_it_s_lik"}
    assert all(owner[k] is compare.SUMMARY and group[k] is None
               for k in ("waic_ind_lse", "waic_ind_mean", "waic_ind_m2", "waic_ind_n_readings", "waic_n_draws", "waic_lse"))
    assert compare.SUMMARY.dims["elpd_waic_ind"] == ["ind"] and compare.SUMMARY.dims["p_waic_ind"] == ["ind"]


def test_null_handles_need_no_gpu():
    from abdpymc_amd import _native

    lib = _native.load()
    for call in (lambda: lib.abd_individual_loglik(None, 0, None, None, None),
                 lambda: lib.abd_sampler_enable_individual_loglik(None, 1),
                 lambda: lib.abd_sampler_individual_loglik_stats(None, 0, None, None, None)):
        assert call() == -1
        assert b"NULL" in lib.abd_last_error()
