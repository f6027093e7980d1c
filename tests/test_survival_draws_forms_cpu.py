"""
Per-draw fits of the survival models by group and by period without a GPU (include/abd_hip.h: abd_survival_draws_create_groups /
_periods; abdpymc_amd.survival: sample_draws, draws_summary, protection): the ABI, every refusal that needs no device,
the batched driver on a host model of each form against ``_chain`` run alone, and the pooled read-out of fits with labels against
NumPy one-liners.
"""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from abdpymc_amd import _native, survival
from tests import survival_groups_restatement as RG
from tests import survival_periods_restatement as RPD
from tests.survival_draws_cases import datasets as _datasets

FORMS = ("groups", "periods")


# ---- 1. the ABI ----

def test_the_header_declares_the_two_creators_and_the_binding_has_them():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "abd_hip.h")).read()
    for form in FORMS:
        name = f"abd_survival_draws_create_{form}"
        assert re.search(rf"int {name}\(const abd_survival_draws_{form}_desc\* desc, abd_survival_draws\*\* out\);", header)
        assert f"}} abd_survival_draws_{form}_desc;" in header
        res, args = _native.SYMBOLS[name]
        assert res is ctypes.c_int and len(args) == 2
        assert hasattr(_native.load(), name)
    # the descriptors of the binding have the header's fields, in its order
    for form, desc, label in (("groups", _native._SurvivalDrawsGroupsDesc, "group"), ("periods", _native._SurvivalDrawsPeriodsDesc, "period")):
        body = header[header.index("typedef struct {", header.index(f"abd_survival_draws_loglik_sums(")):]
        body = body[:body.index(f"}} abd_survival_draws_{form}_desc;")]
        body = body[body.rindex("typedef struct {"):]
        fields = re.findall(r"^  [\w* ]*?(\w+);", body, re.M)  # a declaration per line, ahead of its comment
        assert fields == [f for f, _ in desc._fields_]
        assert fields[:5] == ["n_datasets", "n_inds", "n_intervals", "n_" + form, "device"] and fields[5:9] == ["n_risk", "event", "titer", label]
        assert len(fields) == 17  # ... and the eight priors
    for cls in (_native.SurvivalDrawsGroups, _native.SurvivalDrawsPeriods):
        assert issubclass(cls, _native.SurvivalDraws) and not hasattr(cls, "individual_loglik")


# ---- 2. refusals through the library, before any device is touched ----

def _good(M=2, N=5, T=4):
    n_risk = np.array([[0, 1, 4, 3, 2]] * M, dtype=np.int32)
    event = np.array([[-1, 0, 3, -1, 1]] * M, dtype=np.int32)
    x = np.full((M, T, N), 1.5)
    x[:, 3, 3] = np.nan  # individual 3 is at risk in t < 3: a NaN behind it is no offence
    return n_risk, event, x


LABELS = {"groups": np.array([0, 1, 1, 0, 2], dtype=np.int32), "periods": np.array([0, 0, 1, 2], dtype=np.int32)}
PRIORS = {"groups": RG.PRIORS, "periods": RPD.PRIORS}
MAKE = {"groups": _native.SurvivalDrawsGroups, "periods": _native.SurvivalDrawsPeriods}


def _refused(form, n_risk, event, x, labels=None, n_labels=3, priors=None):
    with pytest.raises(ValueError) as err:  # ABD_ERR_ARG
        MAKE[form](n_risk, event, x, LABELS[form] if labels is None else labels, n_labels, PRIORS[form] if priors is None else priors)
    assert str(err.value) == _native._err(_native.load())
    return str(err.value)


@pytest.mark.parametrize("form", FORMS)
def test_creation_refuses_before_the_device_is_touched_and_names_the_cell(form):
    lib = _native.load()
    n_risk, event, x = _good()
    # what abd_survival_draws_create refuses of a dataset
    for bad, msg in ((-1, "dataset 1, individual 2: n_risk=-1 outside [0, 4]"), (5, "dataset 1, individual 2: n_risk=5 outside [0, 4]")):
        nr = n_risk.copy()
        nr[1, 2] = bad
        assert _refused(form, nr, event, x) == msg
    ev = event.copy()
    ev[1, 3] = 1  # n_risk 3: the event must be 2 or -1
    assert _refused(form, n_risk, ev, x) == "dataset 1, individual 3, interval 1: event must be -1 or n_risk - 1 = 2"
    ev = event.copy()
    ev[0, 0] = 0  # never at risk, yet infected
    assert "dataset 0, individual 0, interval 0" in _refused(form, n_risk, ev, x)
    for v in (np.nan, np.inf):
        xx = x.copy()
        xx[1, 2, 3] = v  # individual 3 is at risk in interval 2
        assert _refused(form, n_risk, event, xx) == "dataset 1, individual 3, interval 2: titer 0 of a cell at risk must be finite"
    # the first offender is named: datasets in order, then individuals
    nr, xx = n_risk.copy(), x.copy()
    nr[1, 0], xx[0, 0, 4] = 9, np.nan
    assert "dataset 0, individual 4, interval 0" in _refused(form, nr, event, xx)
    # the labels and their count
    lab = LABELS[form].copy()
    if form == "groups":
        for bad in (-1, 3):
            lab[3] = bad
            assert _refused(form, n_risk, event, x, lab) == f"individual 3: group {bad} outside [0, 3)"
        for Gr in (0, -1, _native.SURVIVAL_MAX_GROUPS + 1):
            assert _refused(form, n_risk, event, x, n_labels=Gr) == f"n_groups={Gr} outside [1, {_native.SURVIVAL_MAX_GROUPS}]"
    else:
        for bad in (-1, 3):
            lab[2] = bad
            assert _refused(form, n_risk, event, x, lab) == f"interval 2: period {bad} outside [0, 3)"
        for P in (0, 5):
            assert _refused(form, n_risk, event, x, n_labels=P) == f"n_periods={P} outside [1, 4]"
    # a label is refused ahead of a dataset
    nr = n_risk.copy()
    nr[0, 0] = 9
    lab = LABELS[form].copy()
    lab[1] = 7
    assert "outside [0, 3)" in _refused(form, nr, event, x, lab)
    # shapes that survival_check_shape refuses, and M < 1, through the descriptor
    assert "n_intervals=512" in _refused(form, np.zeros((1, 2), np.int32), -np.ones((1, 2), np.int32), np.zeros((1, 512, 2)),
                                         np.zeros(2 if form == "groups" else 512, np.int32), 1)
    d = (_native._SurvivalDrawsGroupsDesc if form == "groups" else _native._SurvivalDrawsPeriodsDesc)()
    create = getattr(lib, f"abd_survival_draws_create_{form}")
    count, label = ("n_groups", "group") if form == "groups" else ("n_periods", "period")
    h = ctypes.c_void_p()
    buf = np.zeros(64)
    d.device = -1
    d.n_risk = d.event = d.titer = buf.ctypes.data
    setattr(d, label, buf.ctypes.data)
    (d.lam0_mu_mean, d.lam0_mu_sd, d.lam0_sd_rate, d.lam0_z_sd, d.a_mu_sd, d.a_sd_rate, d.a_z_sd, d.b_sd) = PRIORS[form]
    for field, value, msg in (("n_datasets", 0, b"n_datasets=0 must be >= 1"), ("n_inds", 0, b"n_inds=0 must be >= 1"),
                              ("n_intervals", 0, b"n_intervals=0 outside")):
        d.n_datasets, d.n_inds, d.n_intervals = 1, 5, 4
        setattr(d, count, 2)
        setattr(d, field, value)
        assert create(ctypes.byref(d), ctypes.byref(h)) == -1 and h.value is None
        assert msg in lib.abd_last_error(), lib.abd_last_error()
    # NULL pointers
    d.n_datasets, d.n_inds, d.n_intervals = 1, 5, 4
    for field in ("n_risk", "event", "titer", label):
        keep = getattr(d, field)
        setattr(d, field, None)
        assert create(ctypes.byref(d), ctypes.byref(h)) == -1 and b"NULL array" in lib.abd_last_error()
        setattr(d, field, keep)
    assert create(None, ctypes.byref(h)) == -1 and b"NULL" in lib.abd_last_error()
    assert create(ctypes.byref(d), None) == -1 and b"NULL" in lib.abd_last_error()
    # what the form's prior check refuses
    names = ("lam0_mu_mean", "lam0_mu_sd", "lam0_sd_rate", "lam0_z_sd", "a_mu_sd", "a_sd_rate", "a_z_sd", "b_sd")
    for k in range(1, 8):
        for v in (0.0, -1.0, np.inf, np.nan):
            pri = list(PRIORS[form])
            pri[k] = v
            assert "must be positive and finite" in _refused(form, n_risk, event, x, priors=pri) and names[k] in _native._err(lib)
    pri = list(PRIORS[form])
    pri[0] = np.nan
    assert "lam0_mu_mean must be finite" in _refused(form, n_risk, event, x, priors=pri)
    # the binding's own shape checks
    with pytest.raises(ValueError, match="share a shape"):
        MAKE[form](n_risk, event[:1], x, LABELS[form], 3, PRIORS[form])
    with pytest.raises(ValueError, match=r"\(M, T, N\)"):
        MAKE[form](n_risk, event, x.transpose(0, 2, 1), LABELS[form], 3, PRIORS[form])
    with pytest.raises(ValueError, match=f"{label} must have shape"):
        MAKE[form](n_risk, event, x, LABELS[form][:-1], 3, PRIORS[form])


def test_the_defaults_of_the_two_forms_differ_in_lam0_mu_mean():
    assert survival.PRIORS_GROUPS[0] == 0.0 and survival.PRIORS_PERIODS[0] == -3.0 and survival.PRIORS_GROUPS[1:] == survival.PRIORS_PERIODS[1:]
    assert survival.PRIORS_GROUPS == RG.PRIORS and survival.PRIORS_PERIODS == RPD.PRIORS
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "abd_hip.h")).read()
    assert "the eight priors of abd_survival_groups_desc, with its defaults: 0, 0.5" in header
    assert "the eight priors of abd_survival_periods_desc, with its defaults: -3, 0.5" in header


# ---- 3. sample_draws against _chain, on a host model of each form ----

def _host_model(form, d):
    """what sample_draws asks of a model with labels, and a restatement of the form per dataset behind ``evaluator``"""
    N, T = d.n_inds, d.n_int
    rs = []
    if form == "groups":
        group = np.arange(N) % 3
        for m in range(d.n_datasets):
            y, e, xs, _ = d.arrays(m)
            rs.append(RG.GroupsRestatement(y, e, xs, group, 3))
        extra = dict(groups=np.array(["a", "b", "c"]), group_name="arm", Gr=3)
        n_labels, priors = 3, RG.PRIORS
    else:
        period = np.array([0, 0, 1, 1, 1])
        for m in range(d.n_datasets):
            y, e, xs, _ = d.arrays(m)
            rs.append(RPD.PeriodsRestatement(y, e, xs, period, 2))
        extra = dict(periods=np.array([2021, 2022]), period_name="year", period_index=period.astype(np.int32), P=2)
        n_labels, priors = 2, RPD.PRIORS
    model = types.SimpleNamespace(dim=rs[0].dim, K=1, n_datasets=d.n_datasets, names=survival.names_groups(T, n_labels), priors=priors,
                                  source=d.source, antigens=("S",), constrain=lambda q: survival.constrain_groups(q, T, n_labels),
                                  initial_point=lambda: survival.initial_point_groups(T, n_labels, priors), **extra)
    calls = []

    def evaluator(datasets, q):
        calls.append(np.array(datasets))
        out = [rs[int(m)].logp_dlogp(row) for m, row in zip(datasets, q)]
        return np.array([o[0] for o in out]), np.stack([o[1] for o in out])

    return model, rs, evaluator, calls


@pytest.mark.parametrize("form", FORMS)
def test_sample_draws_is_chain_per_dataset_bit_for_bit_and_records_the_labels(form):
    M, N, T, c, tune, draws, seed = 3, 40, 5, 2, 30, 20, 7
    d = _datasets(M, N, T)
    model, rs, evaluator, calls = _host_model(form, d)
    fit = survival.sample_draws(model, tune=tune, draws=draws, chains_per_dataset=c, seed=seed, evaluator=evaluator)
    n_labels = 3 if form == "groups" else 2
    assert fit["dataset"].tolist() == [0, 0, 1, 1, 2, 2] and fit["a"].shape == (M * c, draws, n_labels) and fit["b"].shape == (M * c, draws)
    assert fit["lam0"].shape == (M * c, draws, T) and int(fit["n_evaluations"]) == sum(len(v) for v in calls) and int(fit["n_calls"]) == len(calls)
    q0 = survival._initial_point(model)
    assert q0[0] == (0.0 if form == "groups" else -3.0)  # the form's own initial point, not the ungrouped one
    for m in range(M):
        for k in range(c):
            out, stats = survival._chain(rs[m].logp_dlogp, model.dim, tune, draws, np.random.default_rng([seed, m, k]), 0.8, q0)
            row = m * c + k
            np.testing.assert_array_equal(np.stack([fit[name][row] for name in model.names], axis=-1), out)
            for name, v in stats.items():
                np.testing.assert_array_equal(fit["stat_" + name][row], v, err_msg=name)
    assert fit["stat_tree_depth"].max() >= 3  # real trees
    # the label keys of ``sample``, and its readers
    if form == "groups":
        assert fit["groups"].tolist() == ["a", "b", "c"] and str(fit["group_name"]) == "arm" and "periods" not in fit
        assert survival.report_line(fit).startswith("survival: a[S, arm a]")
        p = survival.protection(fit, np.array([0.0, 2.0]), group="b")
    else:
        assert fit["periods"].tolist() == [2021, 2022] and str(fit["period_name"]) == "year" and "groups" not in fit
        assert fit["period_index"].tolist() == [0, 0, 1, 1, 1] and fit["period_index"].dtype == np.int32
        assert survival.report_line(fit).startswith("survival: a[S, year 2021]")
        p = survival.protection(fit, np.array([0.0, 2.0]), period=2022)
        np.testing.assert_array_equal(p["median"], survival.protection(fit, np.array([0.0, 2.0]), interval=3)["median"])
    a, b = fit["a"][..., 1].reshape(-1, 1), fit["b"].reshape(-1, 1)
    np.testing.assert_array_equal(p["mean"], (1.0 - 1.0 / (1.0 + np.exp(-b * (np.array([0.0, 2.0])[None] - a)))).mean(axis=0))
    assert survival.summary(fit)["a"]["mean"].shape == (n_labels,)
    # ``sample`` records the same keys through the same block
    one = survival.sample(model, tune=5, draws=3, chains=1, seed=0, evaluator=rs[0].logp_dlogp)
    for k in ("groups", "group_name", "periods", "period_name", "period_index"):
        assert (k in one) == (k in fit)
        if k in fit:
            np.testing.assert_array_equal(one[k], fit[k])


# ---- 4. draws_summary ----

def _hand_made(rng, M, c, n, n_labels):
    shift = np.repeat(rng.normal(0, 0.5, (M, n_labels)), c, axis=0)[:, None, :]
    a = rng.normal(1.5, 0.3, (M * c, n, n_labels)) + shift + 0.4 * np.arange(n_labels)
    b = rng.normal(-0.8, 0.3, (M * c, n)) + np.repeat([-0.3, 0.2, 0.0, 0.1][:M], c)[:, None]
    return a, b


ROW_KEYS = ["median", "lower", "upper", "sd", "W", "B", "frac_between", "dataset_median", "n_negative", "n_positive"]


@pytest.mark.parametrize("form", FORMS)
def test_draws_summary_of_a_fit_with_labels_matches_numpy_one_liners(form):
    rng = np.random.default_rng(11)
    M, c, n = 4, 2, 50
    labels = ["ctl", "vax", "zzz"] if form == "groups" else [0, 1, 2]
    a, b = _hand_made(rng, M, c, n, 3)
    fit = {"a": a, "b": b, "antigens": np.array(["N"]), "dataset": np.repeat(np.arange(M), c)}
    if form == "groups":
        fit.update(groups=np.array(labels), group_name=np.array("arm"))
    else:
        fit.update(periods=np.array(labels), period_name=np.array("era"), period_index=np.array([0, 0, 1, 2], dtype=np.int32))
    sm = survival.draws_summary(fit, prob=0.9)
    contrasts = [f"a[N|{labels[1]}] - a[N|{labels[0]}]", f"a[N|{labels[2]}] - a[N|{labels[0]}]"]
    assert list(sm) == [f"a[N|{v}]" for v in labels] + ["b[N]"] + [f"protection[N|{v}]@{x}" for v in labels for x in (0, 2, 4)] + contrasts
    prot = 1.0 - 1.0 / (1.0 + np.exp(-b * (2.0 - a[..., 2])))
    checks = [(f"a[N|{labels[1]}]", a[..., 1]), ("b[N]", b), (f"protection[N|{labels[2]}]@2", prot), (contrasts[0], a[..., 1] - a[..., 0]),
              (contrasts[1], a[..., 2] - a[..., 0])]
    for name, x in checks:
        per = x.reshape(M, c * n)
        W, B = per.var(axis=1, ddof=1).mean(), per.mean(axis=1).var(ddof=1)
        r = sm[name]
        assert list(r) == ROW_KEYS + (["p_positive"] if name in contrasts else [])
        assert r["W"] == pytest.approx(W, rel=1e-13) and r["B"] == pytest.approx(B, rel=1e-13)
        assert r["frac_between"] == pytest.approx(B / (B + W), rel=1e-13) and 0.0 < r["frac_between"] < 1.0
        tail = (1.0 - 0.9) / 2.0  # prob = 0.9, equal tails
        lo, med, hi = np.quantile(x.reshape(-1), [tail, 0.5, 1.0 - tail])
        assert (r["lower"], r["median"], r["upper"]) == (lo, med, hi)
        assert r["sd"] == pytest.approx(x.reshape(-1).std(ddof=1), rel=1e-13)
        np.testing.assert_array_equal(r["dataset_median"], np.median(per, axis=1))
        if name in contrasts:
            assert r["p_positive"] == (x > 0).sum() / x.size and 0.0 < r["p_positive"] <= 1.0
    # a plug-in fit of the same form gives sd_ratio for every row, the contrasts included
    plug = dict(fit, a=a[:2], b=b[:2])
    del plug["dataset"]
    sp = survival.draws_summary(fit, plug_in=plug)
    for name, x in checks:
        assert sp[name]["sd_ratio"] == pytest.approx(sm[name]["sd"] / _plug_sd(name, plug, labels), rel=1e-12)
    with pytest.raises(ValueError, match="plug-in fit has no"):
        survival.draws_summary(fit, plug_in={"a": a[:2, :, 0], "b": b[:2], "antigens": np.array(["N"])})
    # one label: no contrast; nine: none either (2 to 8)
    for k in (1, 9):
        ak, bk = _hand_made(rng, M, c, n, k)
        key = "groups" if form == "groups" else "periods"
        many = {"a": ak, "b": bk, "antigens": np.array(["S"]), "dataset": fit["dataset"], key: np.arange(k)}
        assert list(survival.draws_summary(many)) == [f"a[S|{v}]" for v in range(k)] + ["b[S]"] + [f"protection[S|{v}]@{x}" for v in range(k) for x in (0, 2, 4)]
    ak, bk = _hand_made(rng, M, c, n, 8)
    assert len(survival.draws_summary({"a": ak, "b": bk, "antigens": np.array(["S"]), "dataset": fit["dataset"], key: np.arange(8)})) == 8 + 1 + 24 + 7
    # labels that do not fit a
    with pytest.raises(ValueError, match="labels"):
        survival.draws_summary(dict(fit, a=a[..., :2]))


def _plug_sd(name, plug, labels):
    a, b = plug["a"], plug["b"]
    if " - " in name:
        k = [f"a[N|{v}]" for v in labels].index(name.split(" - ")[0])
        x = a[..., k] - a[..., 0]
    elif name.startswith("a["):
        x = a[..., [f"a[N|{v}]" for v in labels].index(name)]
    elif name.startswith("b["):
        x = b
    else:
        x = 1.0 - 1.0 / (1.0 + np.exp(-b * (2.0 - a[..., 2])))
    return x.reshape(-1).std(ddof=1)


def test_draws_summary_of_fits_without_labels_is_what_it_was():
    """An ungrouped K = 1 fit and a K = 2 fit: the keys listed explicitly, every value against the formula, no ``p_positive``."""
    rng = np.random.default_rng(5)
    M, c, n = 4, 2, 50
    a = rng.normal(1.5, 0.3, (M * c, n)) + np.repeat(rng.normal(0, 0.5, M), c)[:, None]
    b = rng.normal(-0.2, 0.6, (M * c, n)) + np.repeat([-1.0, 1.0, -1.0, 0.5], c)[:, None]
    ds = np.repeat(np.arange(M), c)
    one = survival.draws_summary({"a": a, "b": b, "antigens": np.array(["S"]), "dataset": ds})
    assert list(one) == ["a[S]", "b[S]", "protection[S]@0", "protection[S]@2", "protection[S]@4"]
    both = survival.draws_summary({"a": np.stack([a, a + 1], axis=-1), "b": np.stack([b, -b], axis=-1), "antigens": np.array(["S", "N"]), "dataset": ds})
    assert list(both) == ["a[S]", "b[S]", "protection[S]@0", "protection[S]@2", "protection[S]@4",
                          "a[N]", "b[N]", "protection[N]@0", "protection[N]@2", "protection[N]@4"]
    values = {"a[S]": a, "b[S]": b, "a[N]": a + 1, "b[N]": -b}
    for ag, (ak, bk) in (("S", (a, b)), ("N", (a + 1, -b))):
        for x in (0.0, 2.0, 4.0):
            values[f"protection[{ag}]@{x:g}"] = 1.0 - 1.0 / (1.0 + np.exp(-bk * (x - ak)))
    for sm in (one, both):
        for name, r in sm.items():
            x = values[name]
            per = x.reshape(M, c * n)
            assert list(r) == ROW_KEYS
            assert r["W"] == float(np.mean([np.var(v, ddof=1) for v in per])) and r["B"] == float(np.var([v.mean() for v in per], ddof=1))
            assert r["frac_between"] == r["B"] / (r["B"] + r["W"]) and r["sd"] == float(np.std(x.reshape(-1), ddof=1))
            tail = (1.0 - 0.95) / 2.0  # the default prob, equal tails
            assert (r["lower"], r["median"], r["upper"]) == tuple(np.quantile(x.reshape(-1), [tail, 0.5, 1.0 - tail]))
            np.testing.assert_array_equal(r["dataset_median"], np.median(per, axis=1))
            assert (r["n_negative"], r["n_positive"]) == (int((np.median(per, axis=1) < 0).sum()), int((np.median(per, axis=1) > 0).sum()))
    for name in one:
        for k in ROW_KEYS:
            np.testing.assert_array_equal(one[name][k], both[name][k])


# ---- 5. the command line still refuses, and says where the fits are ----

def test_the_cli_refusal_names_the_python_entry_points(capsys):
    for model_name, method in (("s_groups", "model_alone_groups_draws"), ("n_periods", "model_alone_periods_draws")):
        with pytest.raises(SystemExit) as err:
            survival.main(["--posterior", "p.npz", "--ititers_data", "d", "--start", "2", "--end", "20", "--out", "f.npz", "--per_draw", "4",
                           "--model", model_name] + (["--groups", "g.txt"] if model_name == "s_groups" else []))
        msg = capsys.readouterr().err
        assert err.value.code == 2 and model_name in msg and method in msg and "sample_draws" in msg
    for form in FORMS:
        assert callable(getattr(survival.SurvivalAnalysis, f"model_alone_{form}_draws"))
        assert hasattr(getattr(survival, f"SurvivalDraws{form.capitalize()}Model"), "initial_point")
