"""
The survival model by group on the CPU (``SurvivalAnalysis.model_alone_groups``): the committed 40-digit fixture
regenerated, the NumPy restatement against central differences and against the fixture (``E_NP_GROUPS``), the sampler on data
simulated from the model through ``evaluator=``, the label mapping, the refusals of ``abd_survival_create_groups`` (no GPU),
``protection(group=)``, ``report_line`` and the CLI's exit on a label file of the wrong length.
"""
import ctypes
import math
import os
import types

import numpy as np
import pytest

from abdpymc_amd import _native, survival
from tests import survival_groups_restatement as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def fixture():
    return R.load_fixture(GOLDEN)


def test_fixture_is_the_40_digit_statement(fixture):
    import mpmath  # noqa: F401  (no skip: this test is what ties the committed file to mp_evaluate_groups)

    for key, N, T, Gr, name in (("N1_T1_G1_eta_800", 1, 1, 1, "eta_800"), ("N200_T2_G70_a_spread", 200, 2, 70, "a_spread")):
        y, e, x, group = R.make_case(N, T, Gr)
        r = R.mp_evaluate_groups(y, e, x, group, Gr, R.make_point(name, T, Gr))
        for what, v in r.items():
            np.testing.assert_array_equal(np.asarray(v), fixture[f"{key}/{what}"])


def test_case_table_is_what_the_kernel_can_get_wrong():
    assert len(list(R.cases())) == 6 * 9
    sizes = {(N, T, Gr): np.bincount(R.make_groups(N, T, Gr), minlength=Gr) for N, T, Gr in R.SHAPES}
    assert sorted(sizes[(67, 30, 3)]) == [1, 2, 64]
    assert list(sizes[(1000, 199, 5)]) == [700, 129, 128, 42, 1]
    assert sizes[(130, 65, 4)][1] == 0 and (sizes[(200, 2, 70)] <= 3).all()
    y, e, x, group = R.make_case(130, 65, 4)
    assert np.isnan(y[group == 3]).all() and (group == 3).sum() == 13  # a group without any follow-up
    for (N, T, Gr), n in sizes.items():
        if Gr > 1:
            assert (np.diff(R.make_groups(N, T, Gr)) < 0).any()  # interleaved, not pre-sorted
    for name in R.POINTS:
        q = R.make_point(name, 30, 3)
        a = survival.constrain_groups(q, 30, 3)["a"]
        if name == "eta_800":
            assert (a == 2.5).all()
        elif name == "a_spread":
            assert q[33] == 3.0
        else:
            assert (np.abs(a - 1.5) < 2.0).all()


def test_restatement_gradient_against_central_differences():
    y, e, x, group = R.make_case(67, 30, 3)
    rs = R.GroupsRestatement(y, e, x, group, 3)
    q = R.make_point("typical", 30, 3)
    lp, g = rs.logp_dlogp(q)
    assert np.isfinite(lp) and g.shape == (rs.dim,) and rs.dim == 30 + 3 + 5
    h = 1e-5
    num = np.array([(rs.logp(q + h * d) - rs.logp(q - h * d)) / (2 * h) for d in np.eye(rs.dim)])
    # truncation h^2 f''' / 6 ~ 1e-10 relative, rounding u |logp| / h ~ 1e-16 * 1e3 / 1e-5 = 1e-8
    assert np.abs(num - g).max() <= 1e-6 * max(1.0, np.abs(g).max())


def test_restatement_against_the_40_digit_reference(fixture):
    """The worst error of the float64 restatement over the whole case table, per class of point, in units of u S_k:
    E_NP_GROUPS of the restatement file."""
    worst = {name: (0.0, None) for name in R.POINTS}
    handles = {}
    for key, N, T, Gr, name in R.cases():
        if (N, T, Gr) not in handles:
            y, e, x, group = R.make_case(N, T, Gr)
            handles[(N, T, Gr)] = R.GroupsRestatement(y, e, x, group, Gr)
        rs = handles[(N, T, Gr)]
        q = R.make_point(name, T, Gr)
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
        print(f"E_np_groups[{name}] = {e_:.2f} u S at {where}")
    for name, (e_, where) in worst.items():
        assert e_ <= R.E_NP_GROUPS[name], (name, e_, where)
        assert R.c_device(name) == 4.0 * R.E_NP_GROUPS[name]


# The data seed and the lengths chosen on the CPU so that the assertions hold with room.  What the test runs -- 2 chains of 200 + 200,
# sampler seed 0 -- gives 95 % intervals a_0 [0.36, 1.50], a_1 [1.19, 2.28], a_2 [2.25, 3.34] around the truth (0.5, 1.5, 2.5), a
# median of a_2 - a_0 of 1.81 and split R-hat of a_g below 1.01; while choosing, 2 chains of 250 + 250 with sampler seeds 0, 1, 2
# and 4 chains of 300 + 300 gave lower ends of a_0 of 0.30 .. 0.40 and medians of the difference of 1.80 .. 1.83.  The hazard
# rises with the titer (b = 2 > 0) for the reason given in tests/test_survival_cpu.py.
SIM = dict(N=600, T=6, seed=3, a=(0.5, 1.5, 2.5), b=2.0)


def simulate(N, T, seed, a, b):
    """Data from the model itself, the groups interleaved."""
    rng = np.random.default_rng(seed)
    group = np.arange(N) % len(a)
    x = rng.uniform(0.0, 4.0, size=(N, T))
    lam0 = rng.uniform(0.15, 0.3, size=T)
    e = rng.uniform(0.3, 1.0, size=(N, T))
    y = rng.poisson(e * lam0[None, :] / (1.0 + np.exp(-b * (x - np.asarray(a)[group][:, None])))).astype(np.float64)
    return y, e, x, group


def _fake_model(rs, labels):
    T, Gr = rs.T, rs.Gr
    return types.SimpleNamespace(dim=rs.dim, K=1, names=survival.names_groups(T, Gr), antigens=("S",), groups=np.asarray(labels),
                                 group_name="arm", constrain=lambda q: survival.constrain_groups(q, T, Gr),
                                 initial_point=lambda: survival.initial_point_groups(T, Gr))


@pytest.fixture(scope="module")
def simulated_fit():
    y, e, x, group = simulate(**SIM)
    rs = R.GroupsRestatement(y, e, x, group, 3)
    return survival.sample(_fake_model(rs, ["p", "q", "r"]), tune=200, draws=200, chains=2, seed=0, evaluator=rs.logp_dlogp)


def test_sampler_recovers_simulated_group_midpoints(simulated_fit):
    res = simulated_fit
    T = SIM["T"]
    assert res["a"].shape == (2, 200, 3) and res["b"].shape == (2, 200) and res["lam0"].shape == (2, 200, T)
    assert res["a_mu"].shape == (2, 200) and (res["a_sd"] > 0).all() and res["_a_z_2"].shape == (2, 200)
    assert list(res["groups"]) == ["p", "q", "r"] and str(res["group_name"]) == "arm"
    diff = np.median(res["a"][..., 2] - res["a"][..., 0])
    print("median of a_2 - a_0", diff)
    assert diff > 0
    for k, truth in enumerate(SIM["a"]):
        lo, hi = np.quantile(res["a"][..., k], [0.025, 0.975])
        print(f"a_{k}: 95 % interval {lo:.3f} to {hi:.3f}, truth {truth}")
        assert lo < truth < hi
    sm = survival.summary(res)
    assert sm["a"]["rhat"].shape == (3,) and sm["a"]["mean"].shape == (3,) and sm["lam0"]["ess"].shape == (T,)
    print("rhat a", sm["a"]["rhat"], "b", sm["b"]["rhat"])


def test_protection_and_report_line_of_a_grouped_fit(simulated_fit):
    res = simulated_fit
    x = np.array([0.0, 2.0, 4.0])
    p = survival.protection(res, x, group="r")
    a, b = res["a"][..., 2].reshape(-1, 1), res["b"].reshape(-1, 1)
    np.testing.assert_allclose(p["mean"], (1.0 - 1.0 / (1.0 + np.exp(-b * (x[None] - a)))).mean(axis=0), rtol=1e-14)
    assert ((p["lower"] <= p["median"]) & (p["median"] <= p["upper"])).all()
    # the group with the lowest midpoint is the least protected at a titer between the midpoints
    assert survival.protection(res, np.array([1.5]), group="p")["median"][0] < survival.protection(res, np.array([1.5]), group="r")["median"][0]
    for bad in (None, "nobody"):
        with pytest.raises(ValueError):
            survival.protection(res, x, group=bad)
    with pytest.raises(ValueError):
        survival.protection({"a": res["a"][..., 0], "b": res["b"]}, x, group="r")  # group= with an ungrouped fit
    line = survival.report_line(res)
    assert line.startswith("survival: a[S, arm p] ") and "\n" not in line
    assert line.count("protection at titer 0 / 2 / 4") == 3 and line.count("b[S] ") == 1 and "max R-hat of a, b " in line
    for label in ("p", "q", "r"):
        assert f"a[S, arm {label}] " in line
    two = dict(res, a=res["a"].copy())
    two["a"][1, :, 1] += 9.0  # one chain elsewhere in one group's midpoint
    assert "THE CHAINS DISAGREE" in survival.report_line(two) and "DISAGREE" not in line


def test_labels_are_mapped_by_sorted_unique():
    labels, idx = survival.group_indices(np.array(["b", "a", "c", "a"]), 4)
    assert list(labels) == ["a", "b", "c"] and list(idx) == [1, 0, 2, 0] and idx.dtype == np.int32
    labels, idx = survival.group_indices([30, 10, 10, 20], 4)
    assert list(labels) == [10, 20, 30] and list(idx) == [2, 0, 0, 1]
    for bad in (np.zeros(3), np.zeros((4, 1))):
        with pytest.raises(ValueError):
            survival.group_indices(bad, 4)
    q0 = survival.initial_point_groups(6, 3)
    assert q0[0] == 0.0 and q0[1] == -math.log(2.0) and q0[6 + 3] == -math.log(2.0) and np.count_nonzero(q0) == 2 and q0.shape == (14,)
    assert survival.names_groups(2, 2) == ("_lam0_raw_mu", "_lam0_raw_sd_log__", "__lam0_raw_z_0", "__lam0_raw_z_1", "a_mu",
                                           "a_sd_log__", "_a_z_0", "_a_z_1", "b")
    assert survival.PRIORS_GROUPS == R.PRIORS
    assert hasattr(survival.SurvivalAnalysis, "model_alone_groups")


def _desc(y, e, x, labels, Gr, **over):
    d = _native._SurvivalGroupsDesc()
    keep = [np.ascontiguousarray(v, dtype=np.float64) for v in (y, e, x)] + [np.ascontiguousarray(labels, dtype=np.int32)]
    d.n_inds, d.n_intervals, d.n_groups, d.device = keep[0].shape[0], keep[0].shape[1], Gr, 0
    d.infected, d.exposure, d.titer, d.group = (k.ctypes.data for k in keep)
    (d.lam0_mu_mean, d.lam0_mu_sd, d.lam0_sd_rate, d.lam0_z_sd, d.a_mu_sd, d.a_sd_rate, d.a_z_sd, d.b_sd) = R.PRIORS
    for k, v in over.items():
        setattr(d, k, v)
    return d, keep


def test_create_groups_refuses_bad_arguments_without_a_gpu():
    lib = _native.load()
    out = ctypes.c_void_p()

    def refused(d, word):
        assert lib.abd_survival_create_groups(ctypes.byref(d[0]), ctypes.byref(out)) == -1
        assert word in lib.abd_last_error().decode(), lib.abd_last_error()
        assert not out.value

    assert lib.abd_survival_create_groups(None, ctypes.byref(out)) == -1 and b"NULL" in lib.abd_last_error()
    y, e = np.array([[0.25, 0.0, 0.5], [0.0, 0.0, 0.1]]), np.array([[1.0, 0.75, 0.75], [1.0, 1.0, 1.0]])
    x = np.array([[1.0, 2.0, 3.0], [0.5, 0.5, 0.5]])
    assert lib.abd_survival_create_groups(ctypes.byref(_desc(y, e, x, [0, 1], 2)[0]), None) == -1
    refused(_desc(y, e, x, [0, 1], 2, group=None), "NULL")
    refused(_desc(y, e, x, [0, 1], 2, titer=None), "NULL")
    refused(_desc(y, e, x, [0, 2], 2), "group 2")            # a label outside [0, Gr)
    refused(_desc(y, e, x, [-1, 0], 2), "group -1")
    refused(_desc(y, e, x, [0, 0], 0), "n_groups")
    refused(_desc(y, e, x, [0, 0], _native.SURVIVAL_MAX_GROUPS + 1), "n_groups")
    refused(_desc(y, e, x, [0, 1], 2, n_intervals=0), "n_intervals")
    refused(_desc(y, e, x, [0, 1], 2, n_intervals=_native.MAX_GAPS), "n_intervals")
    refused(_desc(y, e, x, [0, 1], 2, n_inds=0), "n_inds")
    refused(_desc(y, e, x, [0, 1], 2, a_sd_rate=0.0), "positive")
    refused(_desc(y, e, x, [0, 1], 2, b_sd=np.inf), "positive")
    refused(_desc(y, e, x, [0, 1], 2, lam0_mu_mean=np.nan), "finite")
    # the cell rule of the ungrouped models
    refused(_desc(np.array([[0.25, -0.1, 0.5], [0, 0, 0]]), e, x, [0, 1], 2), "negative")
    refused(_desc(np.array([[0.25, 0.1, 0.5], [0, 0, 0]]), np.array([[1.0, 0.0, 0.75], [1, 1, 1]]), x, [0, 1], 2), "exposure 0")
    refused(_desc(y, e, np.array([[1.0, np.inf, 3.0], [0, 0, 0]]), [0, 1], 2), "titer")
    assert _native.SURVIVAL_MAX_GROUPS == 256
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "abd_hip.h")).read()
    assert "#define ABD_SURVIVAL_MAX_GROUPS 256" in header


def test_cli_exits_on_a_label_file_of_the_wrong_length(tmp_path):
    from abdpymc_amd.data import TiterData

    cohort = os.path.join(GOLDEN, "test_cohort")
    data = TiterData.from_disk(cohort)
    G, N = data.n_gaps, data.n_inds
    rng = np.random.default_rng(0)
    post = tmp_path / "posterior.npz"
    np.savez(post, mean_i=rng.random((G, N)) * 0.02, mean_ab_s_mu=rng.normal(size=(G, N)), mean_ab_n_mu=rng.normal(size=(G, N)))
    base = ["--posterior", str(post), "--ititers_data", cohort, "--start", "2", "--end", "20", "--out", str(tmp_path / "fit.npz")]
    short = tmp_path / "groups.txt"
    short.write_text("\n".join(str(j % 2) for j in range(N - 1)) + "\n")
    with pytest.raises(SystemExit) as ei:
        survival.main(base + ["--model", "s_groups", "--groups", str(short)])
    assert f"{N - 1} labels for {N} individuals" in str(ei.value)
    np.save(tmp_path / "groups.npy", np.arange(N + 2) % 3)
    with pytest.raises(SystemExit) as ei:
        survival.main(base + ["--model", "n_groups", "--groups", str(tmp_path / "groups.npy")])
    assert f"{N + 2} labels for {N} individuals" in str(ei.value)
    with pytest.raises(SystemExit) as ei:
        survival.main(base + ["--model", "s_groups"])
    assert "--groups" in str(ei.value)
    # what the reader makes of a file of the right length: numbers where every line is one, else the words
    good = tmp_path / "arms.txt"
    good.write_text("\n".join("vaccinated" if j % 3 else "not" for j in range(N)) + "\n")
    assert sorted(set(survival.read_groups(str(good), N))) == ["not", "vaccinated"]
    short.write_text("\n".join(str(j % 2) for j in range(N)) + "\n")
    assert survival.read_groups(str(short), N).dtype.kind == "i"
