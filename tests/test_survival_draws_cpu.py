"""
Per-draw survival fits without a GPU (abdpymc_amd.survival: event_time, sample_draws, draws_summary, --per_draw; include/abd_hip.h:
abd_survival_draws_*): the event-time form of a draw's dataset, the batched driver against ``_chain`` run alone, the
scheduler's invariant, the pooled read-out against NumPy one-liners, and every refusal that needs no device.
"""
import ctypes
import os
import types

import numpy as np
import pytest

from abdpymc_amd import _native, risk, survival
from tests import survival_restatement as R
from tests.survival_draws_cases import datasets as _datasets, host_model as _host_model


# ---- 1. event_time ----

def _binary_draw(rng, G, N):
    i = (rng.random((G, N)) < 0.12).astype(np.int8)
    return i, rng.uniform(-1.0, 6.0, (G, N)), rng.uniform(-1.0, 6.0, (G, N))


def test_event_time_round_trip_on_survival_arrays_of_binary_draws():
    rng = np.random.default_rng(0)
    G, N = 14, 60
    seen = set()
    for k in range(20):
        i, s_mu, n_mu = _binary_draw(rng, G, N)
        last_gap = rng.integers(-1, G, size=N)
        last_gap[:3] = (-1, 0, G - 1)
        start, end = (0, G) if k % 2 else (2, 11)
        arr = risk.survival_arrays(i, s_mu, n_mu, last_gap, start, end)
        T = end - start - 1
        n_risk, event = survival.event_time(arr["infected"], arr["exposure"])
        assert n_risk.dtype == np.int32 and event.dtype == np.int32
        assert ((n_risk >= 0) & (n_risk <= T)).all() and ((event == -1) | (event == n_risk - 1)).all()
        y, e = survival.event_time_arrays(n_risk, event, T)
        # the same data: NaN and exposure-0 cells are both "not at risk" (creation makes y = e = 0 of either)
        y0, e0, _ = R.clean(arr["infected"], arr["exposure"], [])
        y1, e1, _ = R.clean(y, e, [])
        np.testing.assert_array_equal(y0, y1)
        np.testing.assert_array_equal(e0, e1)
        seen |= {"never" if (n_risk == 0).any() else "", "full" if ((n_risk == T) & (event == -1)).any() else "",
                 "first" if (event == 0).any() else "", "last" if (event == T - 1).any() else ""}
    assert {"never", "full", "first", "last"} <= seen  # the draws reach every pattern


def test_event_time_hand_written_cases():
    nan = np.nan
    y = np.array([[nan, nan, nan, nan], [1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, nan], [0, 1, nan, nan], [0, 0, 0, 0]], dtype=float)
    e = np.array([[nan, nan, nan, nan], [1, 0, 0, 0], [1, 1, 1, 1], [1, 1, 1, nan], [1, 1, nan, nan], [1, 1, 1, 1]], dtype=float)
    n_risk, event = survival.event_time(y, e)
    assert n_risk.tolist() == [0, 1, 4, 3, 2, 4]  # never at risk, event at t = 0, event at T - 1, followed without an event, ...
    assert event.tolist() == [-1, 0, 3, -1, 1, -1]
    d = survival.SurvivalDraws(n_risk[None], event[None], np.zeros((1, 4, 6)), np.zeros((1, 4, 6)), [[0, 0]])
    assert d.events().tolist() == [[1.0, 1.0, 0.0, 1.0]]  # Y_t
    yy, ee, xs, xn = d.arrays(0)
    assert xs.shape == (6, 4)
    np.testing.assert_array_equal(np.nan_to_num(yy), np.nan_to_num(y))
    np.testing.assert_array_equal(np.nan_to_num(ee), np.nan_to_num(e))


def test_event_time_refuses_other_forms():
    ok_y, ok_e = np.array([[0.0, 1.0, 0.0]]), np.array([[1.0, 1.0, 0.0]])
    survival.event_time(ok_y, ok_e)
    with pytest.raises(ValueError, match="fractional"):  # the plug-in arrays of posterior means
        survival.event_time(np.array([[0.25, 0.5, 0.0]]), np.array([[1.0, 0.75, 0.25]]) * 0 + np.array([[1.0, 1.0, 0.0]]))
    with pytest.raises(ValueError, match="prefix"):
        survival.event_time(np.array([[0.25, 0.5, 0.0]]), np.array([[1.0, 0.75, 0.25]]))
    with pytest.raises(ValueError, match="prefix"):  # at risk again behind a gap
        survival.event_time(np.zeros((1, 3)), np.array([[1.0, 0.0, 1.0]]))
    with pytest.raises(ValueError, match="last interval at risk"):  # an infection that does not end the follow-up
        survival.event_time(np.array([[1.0, 0.0, 0.0]]), np.array([[1.0, 1.0, 0.0]]))
    with pytest.raises(ValueError, match="last interval at risk"):  # two infections
        survival.event_time(np.array([[1.0, 1.0, 0.0]]), np.array([[1.0, 1.0, 0.0]]))
    with pytest.raises(ValueError, match="individual 1"):
        survival.event_time(np.array([[0.0, 0.0], [0.5, 0.0]]), np.ones((2, 2)))


# ---- 2. sample_draws against _chain ----

def test_sample_draws_is_chain_per_dataset_bit_for_bit():
    M, N, T, c, tune, draws, seed = 3, 40, 5, 2, 30, 20, 7
    d = _datasets(M, N, T)
    model, rs, evaluator, calls = _host_model(d, 2)
    fit = survival.sample_draws(model, tune=tune, draws=draws, chains_per_dataset=c, seed=seed, evaluator=evaluator)
    assert fit["dataset"].tolist() == [0, 0, 1, 1, 2, 2] and fit["a"].shape == (M * c, draws, 2) and fit["lam0"].shape == (M * c, draws, T)
    assert int(fit["n_evaluations"]) == sum(len(v) for v in calls) and int(fit["n_calls"]) == len(calls)
    np.testing.assert_array_equal(fit["source"], d.source)
    q0 = survival._initial_point(model)
    for m in range(M):
        for k in range(c):
            out, stats = survival._chain(rs[m].logp_dlogp, model.dim, tune, draws, np.random.default_rng([seed, m, k]), 0.8, q0)
            row = m * c + k
            got = np.stack([fit[name][row] for name in model.names], axis=-1)
            np.testing.assert_array_equal(got, out)
            for name, v in stats.items():
                np.testing.assert_array_equal(fit["stat_" + name][row], v, err_msg=name)
    assert fit["stat_tree_depth"].max() >= 3  # real trees
    # the keys of ``sample`` and its readers
    line = survival.report_line(fit)
    assert line.startswith("survival: a[S]") and "a[N]" in line
    assert survival.summary(fit)["a"]["mean"].shape == (2,)


def test_every_call_carries_one_point_of_every_chain_in_flight():
    M, c = 10, 2  # 20 chains: four wait for a slot
    d = _datasets(M, 24, 3, seed=1)
    model, rs, evaluator, calls = _host_model(d, 1)
    seen_chain = []

    def recording(datasets, q):
        # a chain is known by its point: the jitter makes every chain's points distinct
        seen_chain.append([row.tobytes() for row in q])
        return evaluator(datasets, q)

    # count the chains not yet finished at every call from the outside: run every chain alone first
    q0 = survival._initial_point(model)
    n_alone = []
    for m in range(M):
        for k in range(c):
            n = [0]

            def fn(q, m=m, n=n):
                n[0] += 1
                return rs[m].logp_dlogp(q)

            survival._chain(fn, model.dim, 12, 6, np.random.default_rng([3, m, k]), 0.8, q0)
            n_alone.append(n[0])
    calls.clear()
    fit = survival.sample_draws(model, tune=12, draws=6, chains_per_dataset=c, seed=3, evaluator=recording)
    assert int(fit["n_evaluations"]) == sum(n_alone)  # nothing evaluated twice, nothing besides
    # replay the schedule: 16 slots, a finished chain's slot goes to the next waiting chain
    left = list(n_alone)
    flight, nxt = list(range(16)), 16
    for datasets, points in zip(calls, seen_chain):
        unfinished = sum(1 for v in left if v > 0)
        assert len(datasets) == min(16, unfinished)
        assert len(set(points)) == len(points)  # no chain twice in a call
        assert sorted(datasets.tolist()) == sorted(j // c for j in flight)
        for j in flight:
            left[j] -= 1
        fin = [j for j in flight if left[j] == 0]
        flight = [j for j in flight if left[j] > 0]
        for _ in fin:
            if nxt < M * c:
                flight.append(nxt)
                nxt += 1
    assert not flight and all(v == 0 for v in left)
    assert max(len(v) for v in calls) == 16 and len(calls) < int(fit["n_evaluations"]) / 2


# ---- 3. draws_summary ----

def test_draws_summary_matches_numpy_one_liners():
    rng = np.random.default_rng(5)
    M, c, n = 4, 2, 50
    a = rng.normal(1.5, 0.3, (M * c, n)) + np.repeat(rng.normal(0, 0.5, M), c)[:, None]
    b = rng.normal(-0.2, 0.6, (M * c, n)) + np.repeat([-1.0, 1.0, -1.0, 0.5], c)[:, None]
    fit = {"a": a, "b": b, "antigens": np.array(["S"]), "dataset": np.repeat(np.arange(M), c)}
    plug = {"a": rng.normal(1.5, 0.2, (2, n)), "b": rng.normal(-1.0, 0.3, (2, n)), "antigens": np.array(["S"])}
    sm = survival.draws_summary(fit, plug_in=plug, prob=0.9)
    assert list(sm) == ["a[S]", "b[S]", "protection[S]@0", "protection[S]@2", "protection[S]@4"]
    prot2 = 1.0 - 1.0 / (1.0 + np.exp(-b * (2.0 - a)))
    for name, x, px in (("a[S]", a, plug["a"]), ("b[S]", b, plug["b"]), ("protection[S]@2", prot2, None)):
        per = x.reshape(M, c * n)
        W, B = per.var(axis=1, ddof=1).mean(), per.mean(axis=1).var(ddof=1)
        r = sm[name]
        assert r["W"] == pytest.approx(W, rel=1e-13) and r["B"] == pytest.approx(B, rel=1e-13)
        assert r["frac_between"] == pytest.approx(B / (B + W), rel=1e-13) and 0.0 <= r["frac_between"] <= 1.0
        tail = (1.0 - 0.9) / 2.0  # prob = 0.9, equal tails
        lo, med, hi = np.quantile(x.reshape(-1), [tail, 0.5, 1.0 - tail])
        assert (r["lower"], r["median"], r["upper"]) == (lo, med, hi)
        np.testing.assert_array_equal(r["dataset_median"], np.median(per, axis=1))
        if px is not None:
            assert r["sd_ratio"] == pytest.approx(x.reshape(-1).std(ddof=1) / px.reshape(-1).std(ddof=1), rel=1e-13)
    assert sm["b[S]"]["n_negative"] == int((np.median(b.reshape(M, -1), axis=1) < 0).sum()) >= 1
    assert sm["b[S]"]["n_positive"] == M - sm["b[S]"]["n_negative"] >= 1
    # identical datasets: nothing lies between them, exactly
    same = {"a": np.tile(a[:c], (M, 1)), "b": np.tile(b[:c], (M, 1)), "antigens": np.array(["S"]), "dataset": np.repeat(np.arange(M), c)}
    for r in survival.draws_summary(same).values():
        assert r["B"] == 0.0 and r["frac_between"] == 0.0 and r["W"] > 0
    # a combined fit has every quantity per antigen
    both = {"a": np.stack([a, a + 1], axis=-1), "b": np.stack([b, -b], axis=-1), "antigens": np.array(["S", "N"]), "dataset": fit["dataset"]}
    sb = survival.draws_summary(both)
    assert len(sb) == 10 and sb["a[S]"]["W"] == sm["a[S]"]["W"] and sb["b[N]"]["n_negative"] == sm["b[S]"]["n_positive"]
    keys = survival.draws_fit_keys(sb)
    assert keys["draws_frac_between"].shape == (10,) and keys["draws_dataset_median"].shape == (10, M)


# ---- 4. refusals through the library, before any device is touched ----

def _good(M=2, N=5, T=4, K=2):
    n_risk = np.array([[0, 1, 4, 3, 2]] * M, dtype=np.int32)
    event = np.array([[-1, 0, 3, -1, 1]] * M, dtype=np.int32)
    xs = [np.full((M, T, N), 1.5) for _ in range(K)]
    for x in xs:
        x[:, 3, 3] = np.nan  # individual 3 is at risk in t < 3: a NaN behind it is no offence
    return n_risk, event, xs


def _refused(n_risk, event, xs, priors=R.PRIORS[2]):
    with pytest.raises(ValueError) as err:
        _native.SurvivalDraws(n_risk, event, xs, priors)
    assert str(err.value) == _native._err(_native.load())
    return str(err.value)


def test_creation_refuses_before_the_device_is_touched_and_names_the_cell():
    lib = _native.load()
    n_risk, event, xs = _good()
    for bad, msg in ((-1, "dataset 1, individual 2: n_risk=-1 outside [0, 4]"), (5, "dataset 1, individual 2: n_risk=5 outside [0, 4]")):
        nr = n_risk.copy()
        nr[1, 2] = bad
        assert _refused(nr, event, xs) == msg
    ev = event.copy()
    ev[1, 3] = 1  # n_risk 3: the event must be 2 or -1
    assert _refused(n_risk, ev, xs) == "dataset 1, individual 3, interval 1: event must be -1 or n_risk - 1 = 2"
    ev = event.copy()
    ev[0, 0] = 0  # never at risk, yet infected
    assert "dataset 0, individual 0, interval 0" in _refused(n_risk, ev, xs)
    ev = event.copy()
    ev[0, 4] = -2
    assert "dataset 0, individual 4, interval -2" in _refused(n_risk, ev, xs)
    for k, v in ((0, np.nan), (1, np.inf)):
        x = [a.copy() for a in xs]
        x[k][1, 2, 3] = v  # individual 3 is at risk in interval 2
        assert _refused(n_risk, event, x) == f"dataset 1, individual 3, interval 2: titer {k} of a cell at risk must be finite"
    # the first offender is named: datasets in order, then individuals
    nr, x = n_risk.copy(), [a.copy() for a in xs]
    nr[1, 0], x[0][0, 0, 4] = 9, np.nan
    assert "dataset 0, individual 4, interval 0" in _refused(nr, event, x)
    # shapes that survival_check_shape refuses, M < 1, K
    assert "n_intervals=512" in _refused(np.zeros((1, 2), np.int32), -np.ones((1, 2), np.int32), [np.zeros((1, 512, 2))], R.PRIORS[1])
    d = _native._SurvivalDrawsDesc()
    h = ctypes.c_void_p()
    buf = np.zeros(64)
    d.n_datasets, d.n_inds, d.n_intervals, d.n_titers, d.device = 0, 5, 4, 1, -1
    d.n_risk = d.event = buf.ctypes.data
    d.titer[0] = buf.ctypes.data
    d.ab_sd, d.lam0_mu_mean, d.lam0_mu_sd, d.lam0_sd_rate, d.lam0_z_sd = R.PRIORS[1]
    for field, value, msg in (("n_datasets", 0, b"n_datasets=0 must be >= 1"), ("n_inds", 0, b"n_inds=0 must be >= 1"),
                              ("n_intervals", 0, b"n_intervals=0 outside"), ("n_titers", 3, b"n_titers=3")):
        d.n_datasets, d.n_inds, d.n_intervals, d.n_titers = 1, 5, 4, 1
        setattr(d, field, value)
        assert lib.abd_survival_draws_create(ctypes.byref(d), ctypes.byref(h)) == -1 and h.value is None
        assert msg in lib.abd_last_error(), lib.abd_last_error()
    # NULL pointers
    d.n_datasets, d.n_inds, d.n_intervals, d.n_titers = 1, 5, 4, 2  # K = 2 without a second titer
    assert lib.abd_survival_draws_create(ctypes.byref(d), ctypes.byref(h)) == -1 and b"NULL array" in lib.abd_last_error()
    d.n_titers = 1
    for field in ("n_risk", "event"):
        keep = getattr(d, field)
        setattr(d, field, None)
        assert lib.abd_survival_draws_create(ctypes.byref(d), ctypes.byref(h)) == -1 and b"NULL array" in lib.abd_last_error()
        setattr(d, field, keep)
    assert lib.abd_survival_draws_create(None, ctypes.byref(h)) == -1 and b"NULL" in lib.abd_last_error()
    assert lib.abd_survival_draws_create(ctypes.byref(d), None) == -1 and b"NULL" in lib.abd_last_error()
    # what survival_check_priors refuses
    for k, name in ((0, "ab_sd"), (2, "lam0_mu_sd"), (3, "lam0_sd_rate"), (4, "lam0_z_sd")):
        for v in (0.0, -1.0, np.inf, np.nan):
            pri = list(R.PRIORS[2])
            pri[k] = v
            assert "must be positive and finite" in _refused(n_risk, event, xs, pri) and name in _native._err(lib)
    pri = list(R.PRIORS[2])
    pri[1] = np.nan
    assert "lam0_mu_mean must be finite" in _refused(n_risk, event, xs, pri)


def test_the_other_calls_refuse_null_and_the_handle_is_its_own_type():
    lib = _native.load()
    buf = np.zeros(64)
    p = buf.ctypes.data
    assert lib.abd_survival_draws_dim(None) == -1
    assert lib.abd_survival_draws_destroy(None) == 0
    for call in (lambda: lib.abd_survival_draws_logp_dlogp(None, 1, p, p, p, p), lambda: lib.abd_survival_draws_loglik_sums(None, 0, p, p)):
        lib.abd_survival_dim(None)
        assert call() == -1
        assert b"NULL" in lib.abd_last_error()
    # WAIC, PPC and replicate calls have nothing to run on
    for name in ("individual_loglik", "waic_accumulate", "waic_stats", "predictive_configure", "predictive_accumulate", "replicate"):
        assert hasattr(_native.Survival, name) and not hasattr(_native.SurvivalDraws, name) and not hasattr(survival.SurvivalDrawsModel, name)
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "abd_hip.h")).read()
    assert "typedef struct abd_survival_draws abd_survival_draws;" in header
    # the binding's own shape checks
    n_risk, event, xs = _good()
    with pytest.raises(ValueError, match="share a shape"):
        _native.SurvivalDraws(n_risk, event[:1], xs, R.PRIORS[2])
    with pytest.raises(ValueError, match=r"\(M, T, N\)"):
        _native.SurvivalDraws(n_risk, event, [xs[0].transpose(0, 2, 1)], R.PRIORS[1])


# ---- 5. posterior_draws and the command line ----

def test_posterior_draws_needs_recorded_draws(tmp_path):
    G, N = 6, 4
    means = {k: np.zeros((2, G, N)) for k in ("mean_i", "mean_ab_s_mu", "mean_ab_n_mu")}
    for src in (means, {"i": np.zeros((G, N)), "ab_s_mu": np.zeros((G, N)), "ab_n_mu": np.zeros((G, N))}):
        with pytest.raises(ValueError, match="--thin"):
            survival.posterior_draws(src)
    rec = {"i": np.zeros((2, 3, G, N), np.int8), "ab_s_mu": np.ones((2, 3, G, N)), "ab_n_mu": np.ones((2, 3, G, N))}
    np.savez(tmp_path / "p.npz", **rec, **means)
    d = survival.posterior_draws(str(tmp_path / "p.npz"))
    assert d["i"].shape == (2, 3, G, N) and d["ab_s_mu"].shape == (2, 3, G, N)
    cohort = types.SimpleNamespace(last_gap=np.array([5, 5, 2, -1]), t0="2020-01")
    sa = survival.SurvivalAnalysis(str(tmp_path / "p.npz"), 0, G, cohort)
    ds = sa.draws(n_datasets=4)
    assert ds.source.tolist() == [[0, 0], [0, 2], [1, 0], [1, 2]]  # spaced evenly over chains x draws
    assert ds.n_risk.tolist() == [[5, 5, 2, 0]] * 4 and (ds.event == -1).all() and ds.s_titer.shape == (4, 5, N)
    assert sa.draws(index=[5, 1]).source.tolist() == [[1, 2], [0, 1]] and sa.draws().n_datasets == 6
    for kw in (dict(n_datasets=0), dict(n_datasets=7), dict(index=[6]), dict(n_datasets=2, index=[0])):
        with pytest.raises(ValueError):
            sa.draws(**kw)
    with pytest.raises(ValueError, match="--thin"):
        survival.SurvivalAnalysis(means, 0, G, cohort).draws()


def test_cli_refuses_what_per_draw_does_not_cover(tmp_path, golden_dir, capsys):
    from abdpymc_amd.data import TiterData

    cohort = os.path.join(golden_dir, "test_cohort")
    data = TiterData.from_disk(cohort)
    post = tmp_path / "means.npz"
    np.savez(post, **{k: np.full((2, data.n_gaps, data.n_inds), 0.01 if k == "mean_i" else 1.0) for k in ("mean_i", "mean_ab_s_mu", "mean_ab_n_mu")})
    base = ["--posterior", str(post), "--ititers_data", cohort, "--start", "2", "--end", "20", "--out", str(tmp_path / "fit.npz"), "--per_draw", "4"]
    for extra, word in ((["--model", "s_groups", "--groups", "g.txt"], "s_groups"), (["--model", "n_periods"], "n_periods"),
                        (["--model", "s", "--waic"], "--waic"), (["--model", "combined", "--ppc"], "--ppc")):
        with pytest.raises(SystemExit) as err:
            survival.main(base + extra)
        assert err.value.code == 2 and word in capsys.readouterr().err  # argparse's error: a message and exit status 2
    with pytest.raises(SystemExit):
        survival.main(base[:-2] + ["--per_draw_chains", "2"])
    assert "--per_draw_chains goes with --per_draw" in capsys.readouterr().err
    with pytest.raises(SystemExit) as err:  # a posterior that holds only means
        survival.main(base + ["--model", "combined"])
    assert "--thin" in str(err.value.code) and str(err.value.code).startswith("survival: ")
    assert not os.path.exists(tmp_path / "fit.npz")
