"""
The survival model by period on the CPU (``SurvivalAnalysis.model_alone_periods``): the committed 40-digit fixture
regenerated, the case table, the NumPy restatement against central differences and against the fixture (``E_NP_PERIODS``, and the
per-individual log-likelihood within the pointwise table's figures), the P = 1 identity with the grouped restatement, the sampler
through ``evaluator=``, a simulated cohort whose two eras differ, ``periods_from_splits``, ``protection(period=)`` /
``(interval=)``, ``report_line``, the refusals of ``abd_survival_create_periods`` (no GPU) and the CLI's argument errors.
"""
import ctypes
import math
import os
import types

import numpy as np
import pytest

from abdpymc_amd import _native, survival
from tests import survival_groups_restatement as RG
from tests import survival_periods_restatement as R
from tests import survival_pointwise_restatement as RP

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def fixture():
    return R.load_fixture(GOLDEN)


def test_fixture_is_the_40_digit_statement(fixture):
    import mpmath  # noqa: F401  (no skip: this test is what ties the committed file to mp_evaluate_periods)

    # the third is a pointwise shape: its ll and ll_S are tied to the statement too
    for key, N, T, P, name in (("N1_T1_P1_eta_800", 1, 1, 1, "eta_800"), ("N200_T2_P2_a_spread", 200, 2, 2, "a_spread"),
                               ("N67_T30_P3_b_minus_50", 67, 30, 3, "b_minus_50")):
        y, e, x, period = R.make_case(N, T, P)
        r = R.mp_evaluate_periods(y, e, x, period, P, R.make_point(name, T, P), pointwise=(N, T, P) in R.SHAPES_POINTWISE)
        assert ("ll" in r) == (N == 67) and len([k for k in fixture if k.startswith(key + "/")]) == len(r)
        for what, v in r.items():
            np.testing.assert_array_equal(np.asarray(v), fixture[f"{key}/{what}"])
    assert os.path.getsize(os.path.join(GOLDEN, R.FIXTURE)) < 1 << 20


def test_case_table_is_what_the_kernel_can_get_wrong(fixture):
    assert R.SHAPES == [(1, 1, 1), (67, 30, 3), (130, 65, 65), (200, 2, 2), (67, 511, 4), (1000, 199, 5), (2100, 129, 4)]
    assert len(list(R.cases())) == 7 * 9 and R.POINTS == RG.POINTS and "a_spread" in R.POINTS
    lengths = {s: np.bincount(R.make_periods(*s), minlength=s[2]) for s in R.SHAPES}
    assert list(lengths[(67, 30, 3)]) == [12, 1, 17]                   # unequal, one of a single interval
    assert (lengths[(130, 65, 65)] == 1).all() and (65 + 63) // 64 == 2  # monthly; two finalize workgroups for S_t and for W0_t
    assert (np.diff(R.make_periods(67, 511, 4)) < 0).any()            # not monotone
    assert lengths[(1000, 199, 5)][3] == 0                             # a period without intervals
    # the plan of the launches from N and T alone: only the last shape has ranges of more than one interval, and its last range
    # holds one
    for N, T, P in R.SHAPES[:-1]:
        assert R.plan(N, T)[1] == 1
    ntile, seg_len, nseg = R.plan(2100, 129)
    assert (ntile, seg_len, nseg) == (33, 2, 65) and -(-4096 // 33) == 125 < 129 and 129 - (nseg - 1) * seg_len == 1
    for key, N, T, P, name in R.cases():
        assert fixture[f"{key}/sums"].shape == (2 * T + 2,) and fixture[f"{key}/grad"].shape == (T + P + 5,)
        assert (f"{key}/ll" in fixture) == ((N, T, P) in R.SHAPES_POINTWISE)
    assert survival.PRIORS_PERIODS == R.PRIORS and R.PRIORS[0] == -3.0 and R.PRIORS[1:] == RG.PRIORS[1:]


@pytest.mark.parametrize("shape", [(7, 5, 3), (70, 9, 9), (3, 4, 1)])
def test_restatement_gradient_against_central_differences(shape):
    """The restatement with the package's priors and the package's mapping of labels to indices; the gradient's layout is the one
    ``names_groups`` and ``constrain_groups`` describe."""
    N, T, P = shape
    y, e, (x,) = R.make_data(N, T, 1)
    labels, period = survival.period_indices(np.array(["w", "x", "y", "z"])[(np.arange(T) * 2) % P] if P < T else 10 * np.arange(T), T)
    assert len(labels) == P
    rs = R.PeriodsRestatement(y, e, x, period, P, priors=survival.PRIORS_PERIODS)
    q = R.make_point("typical", T, P)
    lp, g = rs.logp_dlogp(q)
    assert np.isfinite(lp) and g.shape == (rs.dim,) and rs.dim == T + P + 5 == len(survival.names_groups(T, P))
    np.testing.assert_array_equal(survival.constrain_groups(q, T, P)["a"][period], rs.a_t(q))
    h = 1e-5
    num = np.array([(rs.logp(q + h * d) - rs.logp(q - h * d)) / (2 * h) for d in np.eye(rs.dim)])
    # truncation h^2 f''' / 6 ~ 1e-10 relative, rounding u |logp| / h ~ 1e-16 * 1e3 / 1e-5 = 1e-8
    assert np.abs(num - g).max() <= 1e-6 * max(1.0, np.abs(g).max())


def test_one_period_is_the_grouped_model_with_one_group():
    """With the package's priors of the model by period on both sides (the grouped model's own differ in lam0_mu_mean)."""
    for N, T in ((67, 30), (3, 4)):
        y, e, (x,) = R.make_data(N, T, 1)
        rs = R.PeriodsRestatement(y, e, x, survival.period_indices(np.full(T, "all"), T)[1], 1, priors=survival.PRIORS_PERIODS)
        rg = RG.GroupsRestatement(y, e, x, np.zeros(N, dtype=int), 1, priors=survival.PRIORS_PERIODS)
        for name in R.POINTS:
            q = R.make_point(name, T, 1)
            (lp, g), (lp_g, g_g) = rs.logp_dlogp(q), rg.logp_dlogp(q)
            sp, sg = rs.sums(q), rg.sums(q)
            np.testing.assert_array_equal(sp[:T + 2], sg[:T + 2])
            assert lp == lp_g  # logp does not read W0: the same operations on the same numbers
            # W0 = sum_t W0_t against the sum over all cells at once: two pairwise sums of the same N T terms w, each within
            # (log2(N T) + 2) u sum |w| <= 20 u sum |w|; the gradient takes W0 times b, a_sd b, a_sd _a_z b and a
            m, s_, z, a_mu, a_sl, az, b = rs.split(q)
            a_sd, a0 = math.exp(a_sl), float(survival.constrain_groups(q, T, 1)["a"][0])
            with np.errstate(over="ignore", under="ignore"):
                eta = b * (rs.x - a0)
                w = (rs.y - R._invlogit(m + math.exp(s_) * z)[None, :] * rs.e * R._invlogit(eta)) * R._invlogit(-eta)
            factor = max(abs(b), a_sd * abs(b), a_sd * abs(az[0] * b), abs(a0))
            assert np.abs(g - g_g).max() <= 40 * R.U * np.abs(w).sum() * factor + 4 * R.U * np.abs(g_g).max(), name


def test_restatement_against_the_40_digit_reference(fixture):
    """The worst error of the float64 restatement over the whole case table, per class of point, in units of u S_k:
    E_NP_PERIODS of the restatement file."""
    worst = {name: (0.0, None) for name in R.POINTS}
    handles = {}
    for key, N, T, P, name in R.cases():
        if (N, T, P) not in handles:
            handles[(N, T, P)] = R.model_of(N, T, P)[0]
        rs = handles[(N, T, P)]
        q = R.make_point(name, T, P)
        sums = rs.sums(q)
        lp, g = rs.logp_dlogp(q)
        assert np.isfinite(sums).all() and np.isfinite(lp) and np.isfinite(g).all(), key
        for got, what in ((sums, "sums"), (np.array([lp]), "logp"), (g, "grad")):
            ref, S = np.atleast_1d(fixture[f"{key}/{what}"]), np.atleast_1d(fixture[f"{key}/{what}_S"])
            err = np.abs(got - ref)
            assert (err[S == 0] == 0).all(), (key, what)
            e_ = float((err[S > 0] / S[S > 0] / R.U).max()) if (S > 0).any() else 0.0
            if e_ > worst[name][0]:
                worst[name] = (e_, (key, what))
    for name, (e_, where) in worst.items():
        print(f"E_np_periods[{name}] = {e_:.2f} u S at {where}")
    for name, (e_, where) in worst.items():
        assert e_ <= R.E_NP_PERIODS[name], (name, e_, where)
        assert R.c_device(name) == 4.0 * R.E_NP_PERIODS[name]


def test_pointwise_restatement_against_the_40_digit_reference(fixture):
    """The per-individual log-likelihood of the float64 restatement stays within E_NP of the pointwise table, class by class:
    the device's budget for this model is that table's."""
    worst = {name: 0.0 for name in R.POINTS}
    for N, T, P in R.SHAPES_POINTWISE:
        rs = R.model_of(N, T, P)[0]
        for name in R.POINTS:
            key = f"N{N}_T{T}_P{P}_{name}"
            ref, S = fixture[f"{key}/ll"], fixture[f"{key}/ll_S"]
            got = rs.pointwise(R.make_point(name, T, P))
            assert (got[S == 0] == 0).all() and (S == 0).any()  # an individual without follow-up: exactly 0
            worst[name] = max(worst[name], float((np.abs(got - ref)[S > 0] / S[S > 0] / R.U).max()))
            # sum_j ll_j is the data part of logp: the 40-digit numbers agree to the rounding of the stored float64
            data = fixture[f"{key}/logp"] - _priors_logp(R.make_point(name, T, P), T, P)
            assert abs(ref.sum() - data) <= 8 * R.U * (S.sum() + fixture[f"{key}/logp_S"]), key
    for name, e_ in worst.items():
        print(f"E_np_periods_pointwise[{name}] = {e_:.2f} u S_j (pointwise table: {RP.E_NP[name]})")
    for name, e_ in worst.items():
        assert e_ <= RP.E_NP[name], (name, e_)
        assert R.c_device_pointwise(name) == 4.0 * RP.E_NP[name]


def _priors_logp(q, T, P):
    """the prior part of logp in float64 (the closed forms of the restatement with every data sum 0)"""
    mu_mean, mu_sd, sd_rate, z_sd, a_mu_sd, a_sd_rate, a_z_sd, b_sd = R.PRIORS
    m, s, z, a_mu, a_sl, az, b = q[0], q[1], q[2:2 + T], q[T + 2], q[T + 3], q[T + 4:T + 4 + P], q[T + 4 + P]

    def normal(v, mean, sd_):
        return math.fsum(-0.5 * ((np.atleast_1d(v) - mean) / sd_) ** 2 - math.log(sd_) - 0.9189385332046727)

    return math.fsum([normal(m, mu_mean, mu_sd), normal(z, 0.0, z_sd), math.log(sd_rate), -sd_rate * math.exp(s), s, normal(a_mu, 0.0, a_mu_sd),
                      normal(az, 0.0, a_z_sd), math.log(a_sd_rate), -a_sd_rate * math.exp(a_sl), a_sl, normal(b, 0.0, b_sd)])


# Data from the model itself with two eras whose midpoints differ.  The seed is chosen so that the assertion of
# test_logp_prefers_the_true_order_of_the_eras holds for the restatement (every seed from 0 to 9 did: the difference of logp was
# between 154 and 257 nats, 179.2 at this seed); the evaluation is deterministic.
SIM = dict(N=400, T=8, seed=1, a=(0.5, 2.5), b=2.0)


def simulate(N, T, seed, a, b):
    rng = np.random.default_rng(seed)
    period = (np.arange(T) >= T // 2).astype(np.int64)
    x = rng.uniform(0.0, 4.0, size=(N, T))
    lam0 = rng.uniform(0.15, 0.3, size=T)
    e = rng.uniform(0.3, 1.0, size=(N, T))
    y = rng.poisson(e * lam0[None, :] / (1.0 + np.exp(-b * (x - np.asarray(a)[period][None, :])))).astype(np.float64)
    return y, e, x, period, lam0


def _true_point(T, lam0, a, b, a_sl=0.0):
    """the unconstrained point of the simulation's truth: sd = 1, a_mu = mean(a), a_sd = e^a_sl"""
    a_mu = float(np.mean(a))
    return np.concatenate([[0.0, 0.0], np.log(lam0 / (1.0 - lam0)), [a_mu, a_sl], (np.asarray(a) - a_mu) / math.exp(a_sl), [b]])


def test_logp_prefers_the_true_order_of_the_eras():
    y, e, x, period, lam0 = simulate(**SIM)
    labels, index = survival.period_indices(np.where(period == 0, "delta", "omicron"), SIM["T"])  # as a user would label the eras
    assert list(labels) == ["delta", "omicron"] and index.tolist() == period.tolist()
    rs = R.PeriodsRestatement(y, e, x, index, 2, priors=survival.PRIORS_PERIODS)
    q = _true_point(SIM["T"], lam0, SIM["a"], SIM["b"])
    swapped = q.copy()
    swapped[SIM["T"] + 4:SIM["T"] + 6] = q[SIM["T"] + 4:SIM["T"] + 6][::-1]  # the priors see the same values: only the data part moves
    lp, lp_swapped = rs.logp(q), rs.logp(swapped)
    print("logp at the truth", lp, "with the two midpoints swapped", lp_swapped)
    assert lp > lp_swapped
    np.testing.assert_allclose(survival.constrain_groups(q, SIM["T"], 2)["a"], SIM["a"], rtol=1e-15)


def _fake_model(rs, labels, name="era"):
    T, P = rs.T, rs.P
    return types.SimpleNamespace(dim=rs.dim, K=1, names=survival.names_groups(T, P), antigens=("S",), periods=np.asarray(labels),
                                 period_name=name, period_index=rs.period.astype(np.int32),
                                 constrain=lambda q: survival.constrain_groups(q, T, P),
                                 initial_point=lambda: survival.initial_point_groups(T, P, survival.PRIORS_PERIODS))


@pytest.fixture(scope="module")
def simulated_fit():
    y, e, x, period, _ = simulate(**SIM)
    rs = R.PeriodsRestatement(y, e, x, period, 2)
    return survival.sample(_fake_model(rs, ["delta", "omicron"]), tune=60, draws=40, chains=2, seed=0, evaluator=rs.logp_dlogp)


def test_sample_gives_names_shapes_and_constrain(simulated_fit):
    res, T = simulated_fit, SIM["T"]
    assert res["a"].shape == (2, 40, 2) and res["b"].shape == (2, 40) and res["lam0"].shape == (2, 40, T)
    assert res["a_mu"].shape == (2, 40) and (res["a_sd"] > 0).all() and res["_a_z_1"].shape == (2, 40)
    assert list(res["periods"]) == ["delta", "omicron"] and str(res["period_name"]) == "era"
    assert res["period_index"].tolist() == [0] * 4 + [1] * 4 and "groups" not in res
    q = np.stack([res[n] for n in survival.names_groups(T, 2)], axis=-1)
    np.testing.assert_array_equal(survival.constrain_groups(q, T, 2)["a"], res["a"])
    np.testing.assert_array_equal(res["a"], res["a_mu"][..., None] + res["a_sd"][..., None] * np.stack([res["_a_z_0"], res["_a_z_1"]], -1))
    sm = survival.summary(res)
    assert sm["a"]["rhat"].shape == (2,) and sm["lam0"]["ess"].shape == (T,)
    q0 = survival.initial_point_groups(T, 2, survival.PRIORS_PERIODS)
    assert q0[0] == -3.0 and q0[1] == -math.log(2.0) and q0[T + 3] == -math.log(2.0) and np.count_nonzero(q0) == 3


def test_protection_and_report_line_of_a_fit_by_period(simulated_fit):
    res = simulated_fit
    x = np.array([0.0, 2.0, 4.0])
    p = survival.protection(res, x, period="omicron")
    a, b = res["a"][..., 1].reshape(-1, 1), res["b"].reshape(-1, 1)
    np.testing.assert_allclose(p["mean"], (1.0 - 1.0 / (1.0 + np.exp(-b * (x[None] - a)))).mean(axis=0), rtol=1e-14)
    assert ((p["lower"] <= p["median"]) & (p["median"] <= p["upper"])).all() and ((p["mean"] >= 0) & (p["mean"] <= 1)).all()
    for t in range(SIM["T"]):  # interval= reads the a of the period the interval belongs to
        want = survival.protection(res, x, period="delta" if t < 4 else "omicron")
        got = survival.protection(res, x, interval=t)
        for k in want:
            np.testing.assert_array_equal(got[k], want[k])
    for kw in ({}, {"period": "alpha"}, {"interval": 8}, {"interval": -1}, {"interval": 1.5}, {"period": "delta", "interval": 0}, {"group": "delta"}):
        with pytest.raises(ValueError):
            survival.protection(res, x, **kw)
    for kw in ({"period": "delta"}, {"interval": 0}):
        with pytest.raises(ValueError):
            survival.protection({"a": res["a"][..., 0], "b": res["b"]}, x, **kw)  # with a fit that has no periods
    line = survival.report_line(res)
    assert line.startswith("survival: a[S, era delta] ") and "a[S, era omicron] " in line and "\n" not in line
    assert line.count("protection at titer 0 / 2 / 4") == 2 and line.count("b[S] ") == 1 and "max R-hat of a, b " in line
    two = dict(res, a=res["a"].copy())
    two["a"][1, :, 1] += 9.0  # one chain elsewhere in one period's midpoint
    assert "THE CHAINS DISAGREE" in survival.report_line(two)


def test_waic_and_compare_read_a_fit_by_period(simulated_fit):
    y, e, x, period, _ = simulate(**SIM)
    rs = R.PeriodsRestatement(y, e, x, period, 2)
    model = _fake_model(rs, ["delta", "omicron"])
    model.n_cells = survival.followed_cells(y, e)
    fit = dict(simulated_fit)
    w = survival.waic(model, fit, pointwise=rs.pointwise_matrix())
    assert np.isfinite(w["elpd_waic"]) and w["elpd_i"].shape == (SIM["N"],) and w["n_draws"] == 80
    one = R.PeriodsRestatement(y, e, x, np.zeros(SIM["T"], dtype=int), 1)
    m1 = _fake_model(one, ["all"])
    m1.n_cells = model.n_cells
    fit1 = survival.sample(m1, tune=60, draws=40, chains=2, seed=0, evaluator=one.logp_dlogp)
    survival.waic(m1, fit1, pointwise=one.pointwise_matrix())
    table = survival.compare({"S": fit1, "S by era": fit})
    print(survival.compare_lines(table))
    assert table["S by era"]["rank"] == 0 and table["S"]["elpd_diff"] > 0  # the cohort was simulated with two eras


def test_periods_are_mapped_by_sorted_unique_and_from_splits():
    labels, idx = survival.period_indices(np.array(["omicron", "delta", "omicron", "pre"]), 4)
    assert list(labels) == ["delta", "omicron", "pre"] and list(idx) == [1, 0, 1, 2] and idx.dtype == np.int32
    for bad in (np.zeros(3), np.zeros((4, 1))):
        with pytest.raises(ValueError):
            survival.period_indices(bad, 4)
    sa = types.SimpleNamespace(start=3, intervals=np.arange(10))  # intervals cover the gaps 4 .. 13
    splits = survival.SurvivalAnalysis.periods_from_splits
    assert splits(sa, (6, 12)).tolist() == [0, 0, 1, 1, 1, 1, 1, 1, 2, 2]
    assert splits(sa, (4,)).tolist() == [1] * 10 and splits(sa, (14,)).tolist() == [0] * 10 and splits(sa, ()).tolist() == [0] * 10
    assert splits(sa, (12, 6)).tolist() == splits(sa, (6, 12)).tolist()
    assert hasattr(survival.SurvivalAnalysis, "model_alone_periods") and hasattr(_native, "SurvivalPeriods")


def _desc(y, e, x, labels, P, **over):
    d = _native._SurvivalPeriodsDesc()
    keep = [np.ascontiguousarray(v, dtype=np.float64) for v in (y, e, x)] + [np.ascontiguousarray(labels, dtype=np.int32)]
    d.n_inds, d.n_intervals, d.n_periods, d.device = keep[0].shape[0], keep[0].shape[1], P, 0
    d.infected, d.exposure, d.titer, d.period = (k.ctypes.data for k in keep)
    (d.lam0_mu_mean, d.lam0_mu_sd, d.lam0_sd_rate, d.lam0_z_sd, d.a_mu_sd, d.a_sd_rate, d.a_z_sd, d.b_sd) = R.PRIORS
    for k, v in over.items():
        setattr(d, k, v)
    return d, keep


def test_create_periods_refuses_bad_arguments_without_a_gpu():
    lib = _native.load()
    out = ctypes.c_void_p()

    def refused(d, word):
        assert lib.abd_survival_create_periods(ctypes.byref(d[0]), ctypes.byref(out)) == -1
        assert word in lib.abd_last_error().decode(), lib.abd_last_error()
        assert not out.value

    assert lib.abd_survival_create_periods(None, ctypes.byref(out)) == -1 and b"NULL" in lib.abd_last_error()
    y, e = np.array([[0.25, 0.0, 0.5], [0.0, 0.0, 0.1]]), np.array([[1.0, 0.75, 0.75], [1.0, 1.0, 1.0]])
    x = np.array([[1.0, 2.0, 3.0], [0.5, 0.5, 0.5]])
    ok = [0, 1, 0]
    assert lib.abd_survival_create_periods(ctypes.byref(_desc(y, e, x, ok, 2)[0]), None) == -1
    refused(_desc(y, e, x, ok, 2, period=None), "NULL")
    refused(_desc(y, e, x, ok, 2, titer=None), "NULL")
    refused(_desc(y, e, x, ok, 2, infected=None), "NULL")
    refused(_desc(y, e, x, [0, 2, 0], 2), "period 2")            # a label outside [0, P)
    refused(_desc(y, e, x, [0, 0, -1], 2), "period -1")
    refused(_desc(y, e, x, [0, 0, 0], 0), "n_periods")
    refused(_desc(y, e, x, [0, 1, 2], 4), "n_periods")            # more periods than intervals
    refused(_desc(y, e, x, ok, 2, n_intervals=0), "n_intervals")
    refused(_desc(y, e, x, ok, 2, n_intervals=_native.MAX_GAPS), "n_intervals")
    refused(_desc(y, e, x, ok, 2, n_inds=0), "n_inds")
    refused(_desc(y, e, x, ok, 2, a_sd_rate=0.0), "positive")
    refused(_desc(y, e, x, ok, 2, b_sd=np.inf), "positive")
    refused(_desc(y, e, x, ok, 2, lam0_mu_mean=np.nan), "finite")
    # the cell rule of the other models
    refused(_desc(np.array([[0.25, -0.1, 0.5], [0, 0, 0]]), e, x, ok, 2), "negative")
    refused(_desc(np.array([[0.25, 0.1, 0.5], [0, 0, 0]]), np.array([[1.0, 0.0, 0.75], [1, 1, 1]]), x, ok, 2), "exposure 0")
    refused(_desc(y, e, np.array([[1.0, np.inf, 3.0], [0, 0, 0]]), ok, 2), "titer")
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "abd_hip.h")).read()
    assert "abd_survival_create_periods(const abd_survival_periods_desc* desc, abd_survival** out);" in header
    with pytest.raises(ValueError):  # the binding's own shape check, before the library is asked
        _native.SurvivalPeriods(y, e, x, [0, 1], 2, R.PRIORS)


def test_cli_argument_errors(tmp_path, capsys):
    from abdpymc_amd.data import TiterData

    cohort = os.path.join(GOLDEN, "test_cohort")
    data = TiterData.from_disk(cohort)
    G, N = data.n_gaps, data.n_inds
    rng = np.random.default_rng(0)
    post = tmp_path / "posterior.npz"
    np.savez(post, mean_i=rng.random((G, N)) * 0.02, mean_ab_s_mu=rng.normal(size=(G, N)), mean_ab_n_mu=rng.normal(size=(G, N)))
    base = ["--posterior", str(post), "--ititers_data", cohort, "--start", "2", "--end", "20", "--out", str(tmp_path / "fit.npz")]
    T = 20 - 2 - 1
    short = tmp_path / "periods.txt"
    short.write_text("\n".join(str(t % 2) for t in range(T - 1)) + "\n")
    with pytest.raises(SystemExit) as ei:
        survival.main(base + ["--model", "s_periods", "--periods", str(short)])
    assert f"{T - 1} labels for {T} intervals" in str(ei.value)
    for extra, word in ((["--model", "n_periods", "--periods", "splits"], "--split_delta"),
                        (["--model", "s_periods", "--split_delta"], "--periods splits"),
                        (["--model", "s", "--split_omicron"], "--periods splits"),
                        (["--model", "s", "--periods", "splits"], "s_periods"),
                        (["--model", "s_groups", "--period_name", "era"], "s_periods")):
        with pytest.raises(SystemExit) as ei:
            survival.main(base + extra)
        assert ei.value.code == 2 and word in capsys.readouterr().err
    good = tmp_path / "seasons.txt"
    good.write_text("\n".join("winter" if t % 12 < 3 else "rest" for t in range(T)) + "\n")
    assert sorted(set(survival.read_periods(str(good), T))) == ["rest", "winter"]
