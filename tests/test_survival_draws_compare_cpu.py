"""
Model comparison of per-draw survival fits without a GPU (abdpymc_amd.survival.waic_draws / loo_draws / compare_draws):
the pooling rules against numbers worked by hand, the host path per dataset against ``survival.waic`` / ``survival.loo`` of that
dataset alone (exact: the same NumPy path), independence of the order of the chains, the refusals, the command line, and the NULL
refusals of the new C calls.
"""
import math
import types

import numpy as np
import pytest

from abdpymc_amd import _native, compare, survival
from tests import survival_pointwise_restatement as RP
from tests.survival_draws_cases import datasets, host_model

# ---- the pooling rules, by hand ----


def _per(elpd, p, se, n_warn=0):
    """a per-dataset WAIC dictionary with the entries pool_draws reads"""
    return dict(elpd_waic=elpd, p_waic=p, se=se, n_warn=n_warn, n_draws=10, elpd_i=np.array([elpd, 0.0]), p_waic_i=np.array([p, 0.0]),
                n_readings_i=np.array([3, 0]))


def test_pooling_of_one_dataset_has_no_between_part():
    w = survival.pool_draws([_per(-10.0, 1.5, 2.0, n_warn=1)], "waic")
    assert (w["elpd"], w["p"], w["W"], w["B"], w["se"], w["frac_between"]) == (-10.0, 1.5, 4.0, 0.0, 2.0, 0.0)
    assert w["n_warn"] == 1 and w["worst"] == (0, 0) and w["n_datasets"] == 1 and w["n_draws"].tolist() == [10]


def test_pooling_of_three_datasets_is_rubins_rule():
    """elpd_m = -10, -12, -14: mean -12, B = 4; se_m = 1, 2, 3: W = 14 / 3; se^2 = 14 / 3 + (4 / 3) 4 = 10; frac_between = (16 / 3) / 10"""
    w = survival.pool_draws([_per(-10.0, 1.0, 1.0), _per(-12.0, 2.0, 2.0, n_warn=2), _per(-14.0, 3.0, 3.0, n_warn=1)], "waic")
    assert w["elpd"] == -12.0 and w["p"] == 2.0 and w["B"] == 4.0 and w["W"] == pytest.approx(14.0 / 3.0, rel=1e-15)
    assert w["se"] == pytest.approx(math.sqrt(10.0), rel=1e-15) and w["frac_between"] == pytest.approx(8.0 / 15.0, rel=1e-15)
    assert w["n_warn"] == 3 and w["worst"] == (2, 0) and w["elpd_m"].tolist() == [-10.0, -12.0, -14.0]
    with pytest.raises(ValueError, match="ic must be"):
        survival.pool_draws([_per(-1.0, 1.0, 1.0)], "dic")
    with pytest.raises(ValueError, match="no datasets"):
        survival.pool_draws([], "waic")


def _recorded(elpd_ind, M_source=None, start=2, end=20):
    """a fit that holds what waic_draws records, of (M, N) elpd_j with p_waic_j = 0.1 and every individual followed"""
    e = np.asarray(elpd_ind, dtype=np.float64)
    M = e.shape[0] if M_source is None else M_source
    return {"draws_elpd_waic_ind": e, "draws_p_waic_ind": np.full(e.shape, 0.1), "draws_waic_n_cells": np.full(e.shape, 4, dtype=np.int64),
            "draws_waic_n_draws": np.full(e.shape[0], 50, dtype=np.int64), "source": np.stack([np.zeros(M, np.int64), np.arange(M)], axis=1),
            "start": np.array(start), "end": np.array(end)}


def test_compare_draws_of_three_datasets_by_hand():
    """A: elpd_m = -3, -4, -4; B: -2.5, -5, -7.  A is ahead pooled (-11/3 against -14.5/3), B is ahead in dataset 0.
    elpd_diff_m = -0.5, 1, 3: mean 3.5/3, var (ddof 1) 37/12.  Paired differences per individual: (0, -0.5), (0, 1), (0, 3):
    dse_m^2 = 2 Var = 0.125, 0.5, 4.5.  dse^2 = 5.125 / 3 + (4 / 3)(37 / 12) = 52.375 / 9."""
    fits = {"B": _recorded([[-1.0, -1.5], [-1.0, -4.0], [-2.0, -5.0]]), "A": _recorded([[-1.0, -2.0], [-1.0, -3.0], [-2.0, -2.0]])}
    t = survival.compare_draws(fits)
    a, b = t["A"], t["B"]
    assert (a["rank"], b["rank"]) == (0, 1) and a["elpd"] == pytest.approx(-11.0 / 3.0) and b["elpd"] == pytest.approx(-14.5 / 3.0)
    assert a["elpd_diff"] == 0.0 and a["dse"] == 0.0 and a["p_ahead"] == 0.0 and a["elpd_waic"] == a["elpd"]
    assert b["elpd_diff_m"].tolist() == [-0.5, 1.0, 3.0] and b["elpd_diff"] == pytest.approx(3.5 / 3.0, rel=1e-15)
    np.testing.assert_allclose(b["dse_m"] ** 2, [0.125, 0.5, 4.5], rtol=1e-15)
    assert b["dse"] == pytest.approx(math.sqrt(52.375) / 3.0, rel=1e-15) and b["p_ahead"] == pytest.approx(1.0 / 3.0)
    assert b["dse_frac_between"] == pytest.approx((37.0 / 9.0) / (52.375 / 9.0), rel=1e-15)
    # se of A: se_m^2 = 2 Var_j(elpd_j) = 0.5, 2, 0: W = 2.5 / 3; B = var(-3, -4, -4) = 1 / 3
    assert a["se"] == pytest.approx(math.sqrt(2.5 / 3.0 + (4.0 / 3.0) / 3.0), rel=1e-15)
    assert a["frac_between"] == pytest.approx((4.0 / 9.0) / (2.5 / 3.0 + 4.0 / 9.0), rel=1e-15)
    lines = survival.draws_compare_lines(t)
    assert lines[0].split()[:4] == ["A", "rank", "0", "elpd_waic"] and lines[1].split()[0] == "B" and "p_ahead 0.33" in lines[1] and "frac_between" in lines[1]


def test_compare_draws_of_one_dataset_is_compare_by_individual():
    """M = 1: no between part, and elpd_diff / dse / se are compare.compare(..., by="individual")'s of that dataset."""
    rng = np.random.default_rng(0)
    fits = {name: _recorded(rng.normal(-2.0, 1.0, (1, 30)) - shift) for name, shift in (("near", 0.0), ("far", 0.5), ("mid", 0.2))}
    t = survival.compare_draws(fits)
    plug = compare.compare({name: survival.draws_ic_of_fit(f)["datasets"][0] for name, f in fits.items()}, by="individual")
    for name in fits:
        assert t[name]["rank"] == plug[name]["rank"] and t[name]["frac_between"] == 0.0 and t[name]["dse_frac_between"] == 0.0
        for key in ("elpd_diff", "dse", "se"):
            assert t[name][key] == plug[name][key], (name, key)
        assert t[name]["elpd"] == plug[name]["elpd_waic"] and t[name]["p"] == plug[name]["p_waic"]


# ---- the host path per dataset: the same NumPy path as survival.waic / survival.loo of that dataset ----


def _case(M=3, N=9, T=6, K=2, chains_per_dataset=2, draws=30):
    d = datasets(M, N, T)
    model, rs, _, _ = host_model(d, K)
    model.n_risk, model.start, model.end = d.n_risk, 2, 2 + T + 1
    rng = np.random.default_rng(1)
    q = np.zeros(model.dim)
    q[:K], q[K:2 * K], q[2 * K] = 1.5, -1.0, -3.0
    pts = q + 0.1 * rng.normal(size=(M * chains_per_dataset, draws, model.dim))
    fit = {name: pts[:, :, k].copy() for k, name in enumerate(model.names)}
    fit["dataset"] = np.repeat(np.arange(M), chains_per_dataset)
    fit["source"] = d.source

    def pointwise(ds, Q):
        return np.stack([RP.pointwise(rs[int(m)], row) for m, row in zip(ds, Q)])

    return d, model, rs, fit, pointwise


def _one_dataset(model, d, fit, m):
    """what survival.waic / survival.loo take of dataset m alone: the model's view and the chains of that dataset"""
    rows = np.asarray(fit["dataset"]) == m
    return types.SimpleNamespace(names=model.names, n_cells=d.n_risk[m].astype(np.int64)), {name: fit[name][rows] for name in model.names}


@pytest.mark.parametrize("M", (1, 3))
def test_host_path_equals_waic_and_loo_of_every_dataset_alone(M):
    d, model, rs, fit, pointwise = _case(M=M)
    w, lo = survival.waic_draws(model, fit, pointwise=pointwise), survival.loo_draws(model, fit, pointwise=pointwise)
    assert w["n_datasets"] == M == lo["n_datasets"] and w["n_draws"].tolist() == [60] * M
    assert all(k in fit for k in survival.DRAWS_WAIC_FIT_KEYS + survival.DRAWS_LOO_FIT_KEYS) and (int(fit["start"]), int(fit["end"])) == (2, 9)
    for m in range(M):
        m1, f1 = _one_dataset(model, d, fit, m)
        w1 = survival.waic(m1, f1, pointwise=RP.pointwise_matrix(rs[m]))
        lo1 = survival.loo(m1, f1, pointwise=RP.pointwise_matrix(rs[m]))
        for key in ("elpd_waic", "p_waic", "se", "n_warn", "n_draws", "n_individuals"):
            assert w["datasets"][m][key] == w1[key], (m, key)
        np.testing.assert_array_equal(w["datasets"][m]["elpd_i"], w1["elpd_i"])
        np.testing.assert_array_equal(fit["draws_elpd_waic_ind"][m], f1["elpd_waic_ind"])
        np.testing.assert_array_equal(fit["draws_p_waic_ind"][m], f1["p_waic_ind"])
        np.testing.assert_array_equal(fit["draws_waic_n_cells"][m], d.n_risk[m])
        for key in ("elpd_loo", "p_loo", "se", "n_bad", "n_warn", "worst", "n_draws"):
            assert lo["datasets"][m][key] == lo1[key], (m, key)
        np.testing.assert_array_equal(fit["draws_pareto_k_ind"][m], f1["pareto_k_ind"])
        np.testing.assert_array_equal(fit["draws_elpd_loo_ind"][m], f1["elpd_loo_ind"])
        assert w1["elpd_i"][d.n_risk[m] == 0].tolist() == [0.0] * int((d.n_risk[m] == 0).sum()) and (d.n_risk[m] == 0).any()
    # the pooled values are the rule applied to those
    e = np.array([v["elpd_waic"] for v in w["datasets"]])
    s = np.array([v["se"] for v in w["datasets"]])
    B = float(np.var(e, ddof=1)) if M > 1 else 0.0
    assert w["elpd"] == float(e.mean()) and w["B"] == B and w["se"] == float(np.sqrt(np.mean(s ** 2) + (1 + 1 / M) * B))
    if M == 1:
        assert w["se"] == w["datasets"][0]["se"] and w["frac_between"] == 0.0
    # and they come back from the recorded keys
    for ic, got in (("waic", w), ("loo", lo)):
        again = survival.draws_ic_of_fit(fit, ic)
        for key in ("elpd", "p", "se", "W", "B", "frac_between", "n_warn", "worst"):
            assert again[key] == got[key], (ic, key)
    assert survival.draws_ic_line(w).startswith("survival per-draw WAIC: elpd_waic ") and "frac_between" in survival.draws_ic_line(w)
    assert survival.draws_ic_line(lo).startswith("survival per-draw PSIS-LOO: elpd_loo ") and "pareto_k > 0.7" in survival.draws_ic_line(lo)


def test_result_does_not_depend_on_the_order_of_the_chains_of_different_datasets():
    d, model, rs, fit, pointwise = _case(M=3)
    ref = dict(fit)
    w, lo = survival.waic_draws(model, ref, pointwise=pointwise), survival.loo_draws(model, ref, pointwise=pointwise)
    perm = np.array([4, 0, 2, 5, 1, 3])  # datasets 2, 0, 1, 2, 0, 1: every dataset's two chains keep their order
    assert np.asarray(fit["dataset"])[perm].tolist() == [2, 0, 1, 2, 0, 1]
    mixed = {k: (np.asarray(v)[perm] if k in model.names or k == "dataset" else v) for k, v in fit.items()}
    w2, lo2 = survival.waic_draws(model, mixed, pointwise=pointwise), survival.loo_draws(model, mixed, pointwise=pointwise)
    for a, b in ((w, w2), (lo, lo2)):
        for key in ("elpd", "p", "se", "frac_between", "worst"):
            assert a[key] == b[key], key
        np.testing.assert_array_equal(a["elpd_m"], b["elpd_m"])
    for key in survival.DRAWS_WAIC_FIT_KEYS + survival.DRAWS_LOO_FIT_KEYS:  # what is recorded is by dataset, not by chain
        np.testing.assert_array_equal(mixed[key], ref[key], err_msg=key)
    # a fit that leaves a dataset out, or is no fit of sample_draws, is refused
    with pytest.raises(ValueError, match=r"no chain on the datasets \[1\]"):
        survival.waic_draws(model, {k: (np.asarray(v)[[0, 1, 4, 5]] if k in model.names or k == "dataset" else v) for k, v in fit.items()}, pointwise=pointwise)
    with pytest.raises(ValueError, match="outside"):
        survival.loo_draws(model, dict(fit, dataset=np.array([0, 0, 1, 1, 2, 3])), pointwise=pointwise)


# ---- refusals of compare_draws ----


def test_compare_draws_names_the_odd_ones_out():
    rng = np.random.default_rng(2)
    base = {name: _recorded(rng.normal(-2.0, 1.0, (3, 12))) for name in ("s", "n", "combined")}
    assert sorted(v["rank"] for v in survival.compare_draws(base).values()) == [0, 1, 2]
    other_source = dict(base["n"], source=base["n"]["source"] + 1)
    with pytest.raises(ValueError, match="n differs from the others in source"):
        survival.compare_draws(dict(base, n=other_source))
    fewer = _recorded(rng.normal(-2.0, 1.0, (2, 12)))
    with pytest.raises(ValueError, match="n differs from the others in source, the number of datasets"):
        survival.compare_draws(dict(base, n=fewer))
    with pytest.raises(ValueError, match=r"s differs from the others in start / end"):
        survival.compare_draws(dict(base, s=dict(base["s"], start=np.array(3))))
    with pytest.raises(ValueError, match="combined differs from the others in the number of individuals"):
        survival.compare_draws(dict(base, combined=_recorded(rng.normal(-2.0, 1.0, (3, 11)))))
    unfollowed = dict(base["s"], draws_waic_n_cells=np.where(np.arange(12) == 5, 0, 4)[None, :].repeat(3, axis=0))
    with pytest.raises(ValueError, match="s differs from the others in which individuals are followed"):
        survival.compare_draws(dict(base, s=unfollowed))
    with pytest.raises(ValueError, match=r"n: no per-draw WAIC in the fit .*draws_p_waic_ind.* missing"):
        survival.compare_draws(dict(base, n={k: v for k, v in base["n"].items() if k != "draws_p_waic_ind"}))
    plug_in = {"elpd_waic_ind": np.zeros(12), "p_waic_ind": np.zeros(12), "waic_n_cells": np.full(12, 4), "waic_n_draws": np.array(50)}
    with pytest.raises(ValueError, match="plug: no per-draw WAIC in the fit"):
        survival.compare_draws(dict(base, plug=plug_in))
    with pytest.raises(ValueError, match="s: no per-draw PSIS-LOO in the fit"):
        survival.compare_draws(base, ic="loo")
    with pytest.raises(ValueError, match="n: no source"):
        survival.compare_draws(dict(base, n={k: v for k, v in base["n"].items() if k != "source"}))
    with pytest.raises(ValueError, match="ic must be"):
        survival.compare_draws(base, ic="dic")


# ---- the command line ----


def test_cli_flag_refusals_and_compare_of_written_per_draw_fits(tmp_path, capsys):
    fit_args = ["--posterior", "p.npz", "--ititers_data", "d", "--start", "2", "--end", "20", "--out", "o.npz", "--model", "s"]
    with pytest.raises(SystemExit) as err:
        survival.main(fit_args + ["--per_draw_ic", "waic"])
    assert err.value.code == 2 and "--per_draw_ic goes with --per_draw" in capsys.readouterr().err
    for extra, words in ((["--waic"], ("--per_draw does not go with --waic / --ppc", "--per_draw_ic waic")),
                         (["--ppc"], ("--per_draw does not go with --waic / --ppc", "predictive checks of a per-draw fit are not built")),
                         (["--loo"], ("--per_draw does not go with --loo", "--per_draw_ic loo"))):
        with pytest.raises(SystemExit) as err:
            survival.main(fit_args + ["--per_draw", "2"] + extra)
        msg = capsys.readouterr().err
        assert err.value.code == 2 and all(w in msg for w in words), msg
    # fits of the host path, written, compared without a GPU
    d, model, rs, fit, pointwise = _case(M=3)
    sa = types.SimpleNamespace(start=2, end=9, intervals=np.arange(6), t0="", infected=np.zeros((9, 6)))
    fits, paths = {}, []
    for name, shift in (("near", 0.0), ("far", 1.0)):
        f = dict(fit)
        f[model.names[0]] = fit[model.names[0]] + shift  # another a_S: another model, as far as the comparison goes
        survival.waic_draws(model, f, pointwise=pointwise)
        survival.loo_draws(model, f, pointwise=pointwise)
        fits[name] = f
        paths.append(survival.write(f, str(tmp_path / f"{name}.npz"), sa))
        with np.load(paths[-1]) as stored:
            assert all(k in stored.files for k in survival.DRAWS_WAIC_FIT_KEYS + survival.DRAWS_LOO_FIT_KEYS + ("start", "end", "source"))
    for ic in ("waic", "loo"):
        capsys.readouterr()
        assert survival.main(["--compare"] + paths + ["--ic", ic]) == 0
        rows = capsys.readouterr().out.strip().split("\n")
        table = survival.compare_draws(fits, ic=ic)
        assert rows == survival.draws_compare_lines(table) and len(rows) == 2 and "(3 datasets)" in rows[0]
        assert float(rows[1].split("elpd_diff ")[1].split()[0]) == float(f"{[v for v in table.values() if v['rank'] == 1][0]['elpd_diff']:.3f}")
    # some files with the per-draw entries and some without: an error that says which
    plug = {"elpd_waic_ind": np.zeros(9), "p_waic_ind": np.zeros(9), "waic_n_cells": np.full(9, 4), "waic_n_draws": np.array(50)}
    paths.append(survival.write(plug, str(tmp_path / "plug.npz"), sa))
    with pytest.raises(SystemExit) as err:
        survival.main(["--compare"] + paths)
    msg = str(err.value.code)
    assert msg.startswith("survival: ") and "near, far hold the per-draw entries" in msg and "plug does not" in msg


# ---- the C calls ----


def test_new_symbols_refuse_null_before_the_device_is_touched():
    lib = _native.load()
    buf, i32, i64 = np.zeros(8), np.zeros(8, np.int32), np.zeros(8, np.int64)
    p, pi, pl = buf.ctypes.data, i32.ctypes.data, i64.ctypes.data
    for call in (lambda: lib.abd_survival_draws_individual_loglik(None, 1, pi, p, p), lambda: lib.abd_survival_draws_waic_reset(None),
                 lambda: lib.abd_survival_draws_waic_accumulate(None, 1, pi, p), lambda: lib.abd_survival_draws_waic_stats(None, p, p, p, pl, pi),
                 lambda: lib.abd_survival_draws_loo_reserve(None, 8), lambda: lib.abd_survival_draws_loo_reset(None),
                 lambda: lib.abd_survival_draws_loo_accumulate(None, 1, pi, p), lambda: lib.abd_survival_draws_loo_stats(None, p, p, p, pi, pl)):
        lib.abd_survival_draws_dim(None)
        assert call() == -1
        assert b"NULL" in lib.abd_last_error()
    header = open(_native.__file__.replace("abdpymc_amd/_native.py", "include/abd_hip.h")).read()
    for name in ("individual_loglik", "waic_reset", "waic_accumulate", "waic_stats", "loo_reserve", "loo_reset", "loo_accumulate", "loo_stats"):
        assert "abd_survival_draws_" + name in _native.SYMBOLS and f"int abd_survival_draws_{name}(" in header
    assert _native.SurvivalDraws.LOO_MAX_DRAWS == 16384
    for cls in (_native.SurvivalDraws, _native.SurvivalDrawsGroups, _native.SurvivalDrawsPeriods):  # one set of calls serves all three
        assert all(hasattr(cls, "draws_" + m) for m in ("individual_loglik", "waic_reset", "waic_accumulate", "waic_stats", "loo_reserve", "loo_reset",
                                                        "loo_accumulate", "loo_stats"))
    for cls in (survival.SurvivalDrawsModel, survival.SurvivalDrawsGroupsModel, survival.SurvivalDrawsPeriodsModel):  # named as the C calls are
        assert all(hasattr(cls, "draws_" + m) for m in ("individual_loglik", "waic_accumulate", "waic_stats", "loo_accumulate", "loo_stats"))
