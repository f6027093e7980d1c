"""
The host plumbing of the per-draw summaries (abdpymc_amd/summaries.py) against a stub context / sampler that records its
calls: what ``sample`` enables and in which order, the host budget's running total at its exact boundaries, the keywords
``sample`` accepts, the host sampler's refusals and the routing of the result keys.  No device, no library.
"""
import sys

import numpy as np
import pytest

from abdpymc_amd import diagnostics, risk, sampler, summaries, timelines
from abdpymc_amd._native import N_THETA, STAT_NAMES

G, N, CHAINS, DRAWS, K_S, K_N = 5, 7, 2, 6, 4, 3
SPEC = risk.spec(0, 4, [1.0, 2.0], [0.5], True, n_gaps=G)
ALL_ON = dict(waic=True, ppc=True, curves=True, sero_thresholds=(1.0, 2.0), diagnostics=True, diag_batch=2, risk=SPEC,
              timelines=True, timeline_ranges=((-3, 7), (-2, 6)))
# the enable calls of ALL_ON at DRAWS draws, in the order they must be made
ENABLE_CALLS = [("enable_pointwise",), ("enable_predictive",), ("enable_curves", 6, (1.0, 2.0)), ("enable_diagnostics", 6, 2),
                ("enable_risk", 6, 0, 4, 1, [1.0, 2.0], [0.5]), ("enable_timelines", 6, (-3.0, 7.0), (-2.0, 6.0))]


class StubSampler:
    n_obs = (K_S, K_N)

    def __init__(self, calls, n):
        self.calls, self.n = calls, n

    def enable_pointwise(self):
        self.calls.append(("enable_pointwise",))

    def enable_predictive(self):
        self.calls.append(("enable_predictive",))

    def enable_curves(self, draws, sero_thresholds):
        self.calls.append(("enable_curves", draws, sero_thresholds))

    def enable_diagnostics(self, planned, batch):
        self.calls.append(("enable_diagnostics", planned, batch))

    def enable_risk(self, draws, spec):
        self.calls.append(("enable_risk", draws, spec["start"], spec["end"], spec["first_only"], list(spec["edges_s"]), list(spec["edges_n"])))

    def enable_timelines(self, planned, range_n, range_s):
        self.calls.append(("enable_timelines", planned, range_n, range_s))

    def run(self, n_iter):
        return np.zeros((self.n, n_iter, N_THETA)), {name: np.zeros((self.n, n_iter)) for name in STAT_NAMES}

    def run_record(self, n_iter, first, thin=1, **arrays):
        for a in arrays.values():
            if a is not None:
                a[:, first:first + -(-n_iter // thin)] = 0
        return self.run(n_iter)

    def means(self, k):
        return np.zeros((G, N)), np.zeros((G, N)), np.zeros((G, N)), DRAWS

    def pointwise_stats(self, k):
        return np.zeros((3, K_S + K_N)), DRAWS

    predictive_stats = pointwise_stats

    def curves(self, k):
        return {"counts": np.zeros((DRAWS, 4, G), np.int64), "n_infections": np.zeros((DRAWS, 8), np.int64),
                "titer_sums": np.zeros((DRAWS, 2, G))}

    def diagnostics(self, k):
        return {"i_counts": np.zeros((4, G, N), np.int64), "ab_n_mu": np.zeros((6, G, N)), "ab_s_mu": np.zeros((6, G, N)),
                "info": np.zeros(4, np.int64)}

    def risk(self, k):
        return np.zeros((DRAWS, 2, 2, G, 8), np.int64)

    def timelines(self, k, hist=False):
        out = {"inf": np.zeros((G, N), np.int64), "cum": np.zeros((G, N), np.int64), "ninf": np.zeros((N, 8), np.int64), "n_draws": DRAWS}
        if hist:
            out["hist_n"], out["hist_s"] = np.zeros((G, N, 64), np.uint16), np.zeros((G, N, 64), np.uint16)
        return out

    def timeline_quantiles(self, q):
        return np.zeros((len(q), G, N)), np.zeros((len(q), G, N))

    def close(self):
        pass


class StubContext:
    n_obs_s, n_obs_n = K_S, K_N

    def __init__(self):
        self.calls = []

    def set_discrete(self, chain, i_raw, waner):
        self.calls.append(("set_discrete", chain))

    def sampler(self, chains, theta0, **kw):
        self.calls.append(("sampler", sorted(kw)))
        return StubSampler(self.calls, len(chains))

    def set_follow_up(self, last_gap):
        self.calls.append(("set_follow_up", last_gap))


class StubModel:
    n_gaps, n_inds, n_chains = G, N, CHAINS

    def __init__(self):
        self.ctx = StubContext()

    def initial_point(self):
        return {"i_raw": np.zeros((G, N)), "ab_s_waner": np.zeros(N)}

    def ravel(self, pt):
        return np.zeros(N_THETA)


def run(model=None, **kw):
    model = model or StubModel()
    res = sampler.sample(model, tune=2, draws=DRAWS, chains=CHAINS, **kw)
    return res, [c for c in model.ctx.calls if c[0].startswith(("enable_", "set_follow_up"))]


def test_enable_calls_are_the_expected_list_in_order():
    res, calls = run(**ALL_ON)
    assert calls == ENABLE_CALLS + [("set_follow_up", None)]
    expect = {"waic_": 5, "ppc_": 5, "curves_": 8, "diag_": 4, "risk_": 4, "tl_": 8}
    assert {p: sum(k.startswith(p) for k in res) for p in expect} == expect
    assert res["risk_table"].shape == (CHAINS, DRAWS, 2, 2, G, 8) and res["tl_q_n"].shape == (3, G, N)


@pytest.mark.parametrize("on, k", [(dict(waic=True), 0), (dict(ppc=True), 1), (dict(curves=True, sero_thresholds=(1.0, 2.0)), 2),
                                   (dict(diagnostics=True, diag_batch=2), 3), (dict(risk=SPEC), 4),
                                   (dict(timelines=True, timeline_ranges=((-3, 7), (-2, 6))), 5)])
def test_one_summary_on_makes_only_its_call(on, k):
    _, calls = run(**on)
    assert calls == [ENABLE_CALLS[k]] + ([("set_follow_up", None)] if k in (2, 4, 5) else [])


def test_no_summary_on_makes_no_call():
    res, calls = run()
    assert calls == []
    assert not [k for k in res if k.startswith(tuple(s.prefix for s in summaries.registry()))]


# host bytes, computed here from the public size functions
RECORD = sampler.record_bytes(CHAINS, DRAWS, G, N, True, True)
DIAG = diagnostics.result_bytes(CHAINS, G, N)
RISK = CHAINS * DRAWS * 4 * G * 8 * 8
TL = timelines.result_bytes(CHAINS, G, N, 3, False)
NOTHING = dict(record_deterministics=False, record_discrete=False)
DIAG_ON, RISK_ON, TL_ON = dict(diagnostics=True), dict(risk=SPEC), dict(timelines=True)
BUDGET_CASES = [  # (options, exact need, what the refusal one byte below names)
    ({}, RECORD, "recording"),
    ({**NOTHING, **DIAG_ON}, DIAG, "the diagnostics of"),
    (DIAG_ON, RECORD + DIAG, "the diagnostics of"),
    ({**NOTHING, **RISK_ON}, RISK, "the risk tables of"),
    ({**DIAG_ON, **RISK_ON}, RECORD + DIAG + RISK, "the risk tables of"),
    ({**NOTHING, **TL_ON}, TL, "the timelines of"),
    ({**NOTHING, **DIAG_ON, **RISK_ON, **TL_ON}, DIAG + RISK + TL, "the timelines of"),
    ({**DIAG_ON, **RISK_ON, **TL_ON}, RECORD + DIAG + RISK + TL, "the timelines of"),
]


@pytest.mark.parametrize("on, need, named", BUDGET_CASES)
def test_budget_boundary(on, need, named):
    assert need > 0
    res, _ = run(budget_bytes=need, **on)
    assert "n_grad_evals" in res
    m = StubModel()
    with pytest.raises(ValueError, match="budget") as e:
        run(m, budget_bytes=need - 1, **on)
    assert named in str(e.value)
    assert m.ctx.calls == []


def test_budget_names_the_first_summary_that_crosses():
    every = {**DIAG_ON, **RISK_ON, **TL_ON}
    for budget, named in ((RECORD - 1, "recording"), (RECORD + DIAG - 1, "the diagnostics of"),
                          (RECORD + DIAG + RISK - 1, "the risk tables of")):
        m = StubModel()
        with pytest.raises(ValueError, match="budget") as e:
            run(m, budget_bytes=budget, **every)
        assert named in str(e.value) and m.ctx.calls == []


def test_uncounted_summaries_do_not_touch_the_budget():
    run(budget_bytes=0, waic=True, ppc=True, curves=True, **NOTHING)


# the keywords of sample() before the summaries were described in one place, with their defaults
SAMPLE_KEYWORDS = dict(chains=1, seed=0, record_deterministics=True, progress=None, device_gibbs=True, native=True, record_discrete=True,
                       chain_offset=0, dense_metric=False, thin=1, budget_bytes=None, log_likelihood=False, waic=False,
                       posterior_predictive=False, ppc=False, curves=False, sero_thresholds=None, diagnostics=False, diag_batch=None,
                       risk=None, timelines=False, timeline_ranges=((-4, 8), (-4, 8)), timeline_q=(0.025, 0.5, 0.975),
                       timelines_hist=False)


def test_every_keyword_of_sample_is_still_accepted():
    m = StubModel()
    res = sampler.sample(m, tune=1, draws=2, **SAMPLE_KEYWORDS)
    assert res["n_grad_evals"].shape == (1,)
    assert not [c for c in m.ctx.calls if c[0].startswith("enable_")]  # the defaults switch nothing on
    for native in (True, False):
        with pytest.raises(TypeError, match="timeline_rnages"):
            sampler.sample(StubModel(), tune=1, draws=2, native=native, timeline_rnages=((0, 1), (0, 1)))
    with pytest.raises(TypeError, match="curvse"):
        sampler.sample_native(StubModel(), 1, 2, curvse=True)


@pytest.mark.parametrize("on", [dict(waic=True), dict(ppc=True), dict(curves=True), dict(diagnostics=True), dict(risk=SPEC),
                                dict(timelines=True)])
def test_host_sampler_refuses_each_summary(on):
    m = StubModel()
    with pytest.raises(ValueError, match="native") as e:
        sampler.sample(m, tune=1, draws=2, native=False, **on)
    assert next(iter(on)) in str(e.value) and m.ctx.calls == []


def test_prefixes_are_distinct_and_every_option_has_one_owner():
    reg = summaries.registry()
    assert [s.name for s in reg] == ["waic", "ppc", "curves", "diagnostics", "risk", "timelines"]
    prefixes = [s.prefix for s in reg]
    assert all(p and not q.startswith(p) for i, p in enumerate(prefixes) for j, q in enumerate(prefixes) if i != j)
    owned = [k for s in reg for k in s.options]
    assert len(owned) == len(set(owned)) and all(s.name in s.options for s in reg)
    assert [s.name for s in reg if s.follow_up] == ["curves", "risk", "timelines"]


def test_write_posterior_npz_keeps_every_key(tmp_path, monkeypatch):
    from abdpymc_amd import cli

    monkeypatch.setitem(sys.modules, "arviz", None)  # the .npz path, whether ArviZ is installed or not
    res, _ = run(log_likelihood=True, posterior_predictive=True, **ALL_ON)
    res.update({"curves_summary_incidence": np.zeros((3, G)), "diag_summary_scalar_names": np.array(["lp"]), "risk_by_bin": np.zeros(3),
                "tl_summary_p_inf": np.zeros((G, N)), "elpd_waic_i_it_s_lik": np.zeros(K_S), "ppc_p_it_n_lik": np.zeros(K_N),
                "observed_data_it_s_lik": np.zeros(K_S)})
    out = cli.write_posterior(dict(res), str(tmp_path / "post.npz"), {"gap": np.arange(G), "ind": np.arange(N)})
    z = np.load(out)
    assert set(z.files) == set(res) | {"coord_gap", "coord_ind"}
    for k, v in res.items():
        assert z[k].dtype == v.dtype and z[k].shape == v.shape
    # where a NetCDF file would keep each key: beside the sample statistics (a draw axis), as constant data, or not at all
    group = {k: next(s for s in summaries.registry() if s.owns(k)).group(k) for k in res if any(s.owns(k) for s in summaries.registry())}
    assert {k for k, g in group.items() if g == "sample_stats"} == {
        "curves_infected", "curves_ever_infected", "curves_seropos_s", "curves_seropos_n", "curves_titer_s", "curves_titer_n",
        "curves_n_infections", "risk_table", "risk_by_bin"}
    assert {k for k, g in group.items() if g is None} == {"waic_lse", "waic_mean", "waic_m2", "waic_n_draws", "waic_n_obs", "ppc_mean",
                                                          "ppc_m2", "ppc_pit", "ppc_n_draws", "ppc_n_obs", "diag_summary_scalar_names"}
    assert not [k for k in group if k.startswith(("log_likelihood_", "posterior_predictive_", "observed_data_", "stat_", "mean_"))]
