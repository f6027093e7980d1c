"""
The posterior predictive checks of the survival models on the CPU: the committed fixture regenerated, the NumPy
restatement against its 40-digit tables (``E_NP``), no boundary cell in any replicate case, the terms header
``abd_survival_predictive_terms.hpp`` through its stand-alone harness (plain and under the sanitizers), the refusals of the new
symbols without a GPU, ``survival.predictive(replicate=)`` on host models, and the argument rules of ``default_edges`` and of the
command line.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from abdpymc_amd import _native, survival
from tests import survival_predictive_restatement as R
from tests.test_survival_pointwise_cpu import SIM, HostModel, simulate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def fixture():
    return R.load_fixture(GOLDEN)


@pytest.fixture(scope="module")
def models():
    return {shape: R.model_of(shape) for shape in R.SHAPES}


# ---- 1. the restatement and the fixture ----


def test_fixture_is_the_40_digit_statement_and_the_restatements_replicates(fixture):
    import mpmath  # noqa: F401  (no skip: this test is what ties the committed file to mp_expected)
    from tests.golden.make_survival_predictive_fixtures import replicate_case

    for shape, name in ((("k", 65, 3, 2), "eta_800"), (("groups", 130, 65, 4), "a_spread")):
        rs, _, variables, edges = R.model_of(shape)
        E, S = R.mp_expected(rs, R.point_of(shape, name), variables, edges)
        np.testing.assert_array_equal(E, fixture[f"{R.tag(shape)}_{name}/E"])
        np.testing.assert_array_equal(S, E)  # every addend is non-negative
    for shape, seed, draw0 in R.REPLICATE_CASES[1::3]:
        r, boundary = replicate_case(shape, seed, draw0)
        np.testing.assert_array_equal(r, fixture[f"{R.tag(shape)}_rep/r"])
    assert len(fixture) == len(list(R.cases())) + 2 * len(R.REPLICATE_CASES)
    assert os.path.getsize(os.path.join(GOLDEN, R.FIXTURE)) < 1 << 20


def test_restatement_against_the_40_digit_reference(fixture, models):
    """The worst error of the float64 restatement over the case table, per class of point, in units of u E: E_NP of the restatement
    file (each measured figure rounded up by a tenth and to the next integer); a bin without followed cells is exactly 0."""
    worst = {name: (0.0, None) for name in R.E_NP}
    for key, shape, name in R.cases():
        rs, _, variables, edges = models[shape]
        got, Ej = R.expected(rs, R.point_of(shape, name), variables, edges)
        ref = fixture[key + "/E"]
        assert got.shape == ref.shape == (len(variables), 8) and np.isfinite(got).all(), key
        assert (got[ref == 0] == 0).all(), key
        cells = R.constants(rs, variables, edges)[2]
        assert (ref[cells[:len(variables)] == 0] == 0).all(), key
        assert abs(Ej.sum() - got[0].sum()) <= 1e-12 * got[0].sum() + 0.0
        m = ref > 0
        e_ = float((np.abs(got - ref)[m] / ref[m] / R.U).max()) if m.any() else 0.0
        if e_ > worst[name][0]:
            worst[name] = (e_, key)
    for name, (e_, where) in worst.items():
        print(f"E_np_predictive[{name}] = {e_:.2f} u E at {where}")
    for name, (e_, where) in worst.items():
        assert e_ <= R.E_NP[name], (name, e_, where)
        assert R.E_NP[name] == max(1.0, math.ceil(1.1 * R.MEASURED_E_NP[name])) and R.c_device(name) == 4.0 * R.E_NP[name]
    # the empty last bin of the second variable, and the classes' shapes, are in the table
    assert (R.constants(*[models[("k", 130, 65, 2)][i] for i in (0, 2, 3)])[2][1, 3:] == 0).all()
    assert R.STREAM not in (0x40000000, 0x40000001, 0x40000010, 0x40000011)


# ---- 2. boundary cells ----


def test_no_replicate_case_has_a_boundary_cell(fixture, models):
    """Only where u lies within 2^-36 of a cumulative value the inversion examined can two correctly working exponentials disagree on
    k: the seeds of the replicate cases leave no such cell (expected share about 1e-11 per cell), so the device owes the fixture's
    replicates exactly."""
    total = 0
    for shape, seed, draw0 in R.REPLICATE_CASES:
        rs = models[shape][0]
        for d, name in enumerate(R.REPLICATE_POINTS):
            assert name in ("typical", "b_plus_50", "b_minus_50")
            r, boundary = R.replicates(rs, R.point_of(shape, name), seed, draw0 + d)
            total += boundary
            np.testing.assert_array_equal(r, fixture[f"{R.tag(shape)}_rep/r"][d])
            assert (r[rs.e == 0] == 0).all()
        assert int(fixture[f"{R.tag(shape)}_rep/boundary"]) == 0
    assert total == 0
    # the flag itself: a uniform placed on a cumulative value is a boundary cell, one placed 2^-30 away is not
    c0 = math.exp(-0.5)
    assert R.poisson_inverse(0.5, c0)[1] and R.poisson_inverse(0.5, c0 * 1.5)[1] and not R.poisson_inverse(0.5, c0 + 2.0 ** -30)[1]
    assert R.poisson_inverse(0.0, 1.0 - 2.0 ** -53)[0] == 0  # mu = 0 needs no guard


# ---- 3. the native harness ----

HARNESS_SRC = os.path.join(ROOT, "tests", "native", "survival_predictive_harness.cpp")
INCLUDES = ["-I", os.path.join(ROOT, "tests", "native", "fake_hip"), "-I", os.path.join(ROOT, "abdpymc_amd", "csrc")]


@pytest.fixture(scope="module", params=["plain", "sanitizers"])
def harness(request, tmp_path_factory):
    """the stand-alone program, built plain and with -fsanitize=address,undefined; either way it runs as a child process"""
    out = tmp_path_factory.mktemp("survival_predictive") / f"harness_{request.param}"
    flags = ["-O2"] if request.param == "plain" else ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.check_call(["g++", "-std=c++17", *flags, "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", *INCLUDES, HARNESS_SRC, "-o", str(out)])
    return str(out)


def grouped_slots(group, Gr):
    """the column of every individual in the grouped layout: sorted by group, every group padded to whole tiles"""
    slot, base = np.empty(len(group), dtype=np.int64), 0
    for g in range(Gr):
        members = np.flatnonzero(group == g)
        slot[members] = base + np.arange(len(members))
        base += (len(members) + 63) // 64 * 64
    return slot, max(base, 64)


def run_harness(harness, tmp_path, rs, variables, edges, seed, draw, mu, slot=None, ld=None, grid=None):
    N, T = rs.y.shape
    ld = (N + 63) // 64 * 64 if ld is None else ld
    col = np.arange(N) if slot is None else slot
    y, e = np.zeros((T, ld)), np.zeros((T, ld))
    y[:, col], e[:, col] = rs.y.T, rs.e.T
    ed = np.zeros((len(variables), 7))
    for v, x in enumerate(edges):
        ed[v, :len(x)] = x
    grid = (np.empty(0), np.empty(0)) if grid is None else grid
    head = [N, T, ld, len(variables), len(edges[0]), len(edges[-1]), seed, draw, int(slot is not None), len(grid[0])]
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array(head, dtype=np.uint64).tobytes() + y.tobytes() + e.tobytes() + np.ascontiguousarray(mu, dtype=np.float64).tobytes()
                + np.ascontiguousarray(np.stack(variables), dtype=np.float64).tobytes() + ed.tobytes()
                + (b"" if slot is None else np.asarray(slot, dtype=np.int64).tobytes()) + grid[0].tobytes() + grid[1].tobytes())
    r = subprocess.run([harness, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    out = np.fromfile(tmp_path / "out.bin")
    if out[0] != 0:
        return out[0]
    nv, n = len(variables), N * T
    sizes = [nv * n, n, n, 16, 16, 16, N, ld, len(grid[0])]
    assert out.size == 1 + sum(sizes)
    parts = np.split(out[1:], np.cumsum(sizes)[:-1])
    return dict(bins=parts[0].reshape(nv, N, T), u=parts[1].reshape(N, T), r=parts[2].reshape(N, T), observed=parts[3].reshape(2, 8),
                person_time=parts[4].reshape(2, 8), n_cells=parts[5].reshape(2, 8), observed_ind=parts[6], slot_j=parts[7], grid_k=parts[8])


def test_host_terms_equal_the_restatement(harness, models, tmp_path):
    """Bins, uniforms and replicates of the replicate cases exactly; the constants within one rounding of math.fsum; slot_j is the
    inverse of the grouped layout, so the uniforms are keyed by the caller's index."""
    rng = np.random.default_rng(5)
    grid = (np.concatenate([[0.0, 4.0], rng.uniform(0.0, 4.0, 2000)]), np.concatenate([[1.0 - 2.0 ** -53, 1.0 - 2.0 ** -53], rng.random(2000)]))
    grid_k, grid_near = R.poisson_inverse(*grid)
    assert grid_k.max() >= 10 and grid_k[0] == 0
    for shape, seed, draw0 in R.REPLICATE_CASES:
        rs, made, variables, edges = models[shape]
        slot, ld = grouped_slots(rs.group, rs.Gr) if shape[0] == "groups" else (None, None)
        for d, name in enumerate(R.REPLICATE_POINTS[:2]):
            mu = R.mu_of(rs, R.point_of(shape, name))
            got = run_harness(harness, tmp_path, rs, variables, edges, seed, draw0 + d, mu, slot, ld, grid)
            bins = R.bins_of(rs, variables, edges)
            np.testing.assert_array_equal(got["bins"], np.where(bins < 0, 0, bins))
            np.testing.assert_array_equal(got["u"], R.uniform(seed, *rs.y.shape, draw0 + d))
            np.testing.assert_array_equal(got["r"], R.replicates(rs, R.point_of(shape, name), seed, draw0 + d)[0])
            np.testing.assert_array_equal(got["grid_k"][~grid_near], grid_k[~grid_near])
            O, PT, cells, O_j = R.constants(rs, variables, edges)
            np.testing.assert_array_equal(got["n_cells"][:len(variables)], cells)
            for a, b in ((got["observed"][:len(variables)], O), (got["person_time"][:len(variables)], PT), (got["observed_ind"], O_j)):
                assert (np.abs(a - b) <= 2 * R.U * np.abs(b)).all()
            want = np.full(got["slot_j"].shape, -1.0)
            want[np.arange(rs.N) if slot is None else slot] = np.arange(rs.N)
            np.testing.assert_array_equal(got["slot_j"], want)
    assert (got["observed"][len(variables):] == 0).all()


def test_host_terms_refuse_what_configuration_refuses(harness, models, tmp_path):
    rs, made, variables, edges = models[("k", 65, 3, 2)]
    mu = R.mu_of(rs, R.point_of(("k", 65, 3, 2), "typical"))
    j, t = np.argwhere(rs.e > 0)[7]
    bad = [v.copy() for v in variables]
    bad[1][j, t] = np.inf
    assert run_harness(harness, tmp_path, rs, bad, edges, 0, 0, mu) == 1.0 + j  # a non-finite titer in a followed cell
    ok = [np.where(rs.e > 0, v, np.nan) for v in variables]
    assert isinstance(run_harness(harness, tmp_path, rs, ok, edges, 0, 0, mu), dict)  # NaN where nothing is followed is fine
    for wrong in ((1.0, 1.0), (2.0, 1.0), (0.0, np.nan), (0.0, np.inf)):
        assert run_harness(harness, tmp_path, rs, variables, [edges[0], wrong], 0, 0, mu) == -1.0
    import copy
    big = copy.copy(rs)
    big.e = rs.e.copy()
    big.e[j, t] = 4.5
    assert run_harness(harness, tmp_path, big, variables, edges, 0, 0, mu) == 1.0 + j  # exposure above 4


def test_new_symbols_refuse_null_without_a_gpu():
    lib = _native.load()
    buf, n = np.zeros(64), ctypes.c_int64()
    for call in (lambda: lib.abd_survival_predictive_configure(None, 1, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, 0),
                 lambda: lib.abd_survival_predictive_reset(None),
                 lambda: lib.abd_survival_predictive_accumulate(None, 1, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data),
                 lambda: lib.abd_survival_predictive_stats(None, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, ctypes.byref(n)),
                 lambda: lib.abd_survival_predictive_observed(None, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data),
                 lambda: lib.abd_survival_replicate(None, 1, buf.ctypes.data, 0, buf.ctypes.data)):
        lib.abd_survival_dim(None)
        assert call() == -1
        assert b"NULL" in lib.abd_last_error()
    for cls in (_native.Survival, _native.SurvivalGroups, _native.SurvivalPeriods):
        for name in ("predictive_configure", "predictive_reset", "predictive_accumulate", "predictive_stats", "predictive_observed", "replicate"):
            assert callable(getattr(cls, name)) and callable(getattr(survival.SurvivalModel, name))


# ---- 4. survival.predictive on host models ----

PPC_EDGES = {"S": [2.0]}  # the lower and the upper half of the S titers (uniform on [0, 4])
PPC_SEED = 11


class HostPredictiveModel(HostModel):
    """tests/test_survival_pointwise_cpu.py's host model with what ``survival.predictive(replicate=)`` asks for besides"""

    def __init__(self, infected, exposure, titers, antigens):
        super().__init__(infected, exposure, titers, antigens)
        self.infected, self.exposure, self.followed = infected, exposure, survival.followed_mask(infected, exposure)
        self.replicate_host = R.replicate_callable(self.rs, PPC_SEED)


def fit_and_check(make, use_device):
    """the fits of the S and of the N model on SIM's data, each checked by the S titer in two bins"""
    y, e, x_s, x_n = simulate(**SIM)
    out = {}
    for ag, x in (("S", x_s), ("N", x_n)):
        m = make(y, e, [x], (ag,))
        try:
            fit = survival.sample(m, tune=150, draws=150, chains=2, seed=0, evaluator=None if use_device else m.logp_dlogp)
            out[ag] = (m, fit, survival.predictive(m, fit, {"S": x_s}, edges=PPC_EDGES, seed=PPC_SEED, replicate=None if use_device else m.replicate_host))
        finally:
            if use_device:
                m.close()
    return out


def check_statements(checked):
    """The S model binned by S: no bin flagged and every ratio's interval covers 1.  The N model binned by S: the highest S bin is
    flagged.  SIM's data come from b = 2 > 0: the hazard RISES with the S titer, so the N model, blind to it, expects too few
    infections in the upper half -- the small tail there is p_high = P(R >= O) -- and too many in the lower half, where p_low is
    small; both bins are flagged."""
    s, n = checked["S"][2]["variables"]["S"], checked["N"][2]["variables"]["S"]
    for name, v in (("S", s), ("N", n)):
        print(name, "p_low", v["p_low"], "p_high", v["p_high"], "ratio", v["ratio_lower"], v["ratio_upper"], "O", v["observed"], "E", v["expected_median"])
    assert len(s["flagged"]) == 0 and (s["ratio_lower"] <= 1).all() and (s["ratio_upper"] >= 1).all()
    assert np.minimum(s["p_low"], s["p_high"]).min() > 0.1
    assert list(n["flagged"]) == [0, 1]
    assert n["p_high"][1] < 0.005 and n["p_low"][0] < 0.005 and n["p_low"][1] > 0.99 and n["p_high"][0] > 0.99


@pytest.fixture(scope="module")
def checked():
    return fit_and_check(HostPredictiveModel, use_device=False)


def test_summary_is_plain_numpy_on_the_replicate_matrix(checked):
    m, fit, p = checked["S"]
    y, e, x_s, x_n = simulate(**SIM)
    q = survival.fit_points(m, fit)
    mu, r = m.replicate_host(q, 0)
    assert mu.shape == r.shape == (300, 300, 6) and p["n_draws"] == 300
    v = p["variables"]["S"]
    lo, hi = x_s < 2.0, x_s >= 2.0
    np.testing.assert_array_equal(v["observed"], [y[lo].sum(), y[hi].sum()])
    np.testing.assert_allclose(v["person_time"], [e[lo].sum(), e[hi].sum()], rtol=1e-13)
    np.testing.assert_array_equal(v["n_cells"], [lo.sum(), hi.sum()])
    R_ = np.stack([r[:, lo].sum(axis=1), r[:, hi].sum(axis=1)], axis=1)
    E_ = np.stack([mu[:, lo].sum(axis=1), mu[:, hi].sum(axis=1)], axis=1)
    np.testing.assert_array_equal(v["replicate"], R_)
    np.testing.assert_allclose(v["expected"], E_, rtol=1e-13)
    np.testing.assert_array_equal(v["p_low"], (R_ <= v["observed"]).mean(axis=0))
    np.testing.assert_array_equal(v["p_high"], (R_ >= v["observed"]).mean(axis=0))
    np.testing.assert_allclose(v["expected_median"], np.median(E_, axis=0), rtol=1e-13)
    np.testing.assert_allclose(v["ratio_lower"], np.quantile(v["observed"] / E_, 0.025, axis=0), rtol=1e-12)
    np.testing.assert_allclose(v["ratio_upper"], np.quantile(v["observed"] / E_, 0.975, axis=0), rtol=1e-12)
    np.testing.assert_allclose(p["expected_i"], mu.sum(axis=2).mean(axis=0), rtol=1e-12)
    np.testing.assert_array_equal(p["p_infected_i"], (r.sum(axis=2) >= 1).mean(axis=0))
    np.testing.assert_array_equal(p["replicate_mean_i"], r.sum(axis=2).sum(axis=0) / 300)
    np.testing.assert_array_equal(p["observed_i"], y.sum(axis=1))
    # what predictive records in the fit, and the line
    assert all(k in fit for k in survival.PPC_FIT_KEYS) and list(fit["ppc_variables"]) == ["S"] and int(fit["ppc_n_draws"]) == 300
    assert fit["ppc_expected"].shape == (300, 1, 8) and np.isnan(fit["ppc_expected"][:, :, 2:]).all() and int(fit["ppc_seed"]) == PPC_SEED
    np.testing.assert_array_equal(fit["ppc_replicate"][:, 0, :2], R_)
    line = survival.predictive_line(p)
    assert line.startswith("survival PPC by S: observed/expected per bin ") and "0 of 2 bins flagged (300 draws)" in line and "\n" not in line


def test_replicate_counts_match_their_expectation():
    """One point repeated 4 000 times: a bin's mean replicate count is within 5 standard errors sqrt(E / n) of its E."""
    y, e, x_s, x_n = simulate(**SIM)
    m = HostPredictiveModel(y, e, [x_s], ("S",))
    q = np.concatenate([[1.5, 2.0, -1.4, math.log(0.3)], np.zeros(6)])
    n = 4000
    mu = R.mu_of(m.rs, q)
    u = np.stack([R.uniform(PPC_SEED, 300, 6, d) for d in range(n)])
    r = R.poisson_inverse(mu[None], u)[0]
    for sel in (x_s < 2.0, x_s >= 2.0):
        E = mu[sel].sum()
        mean = r[:, sel].sum(axis=1).mean()
        print("E", E, "mean replicate", mean, "se", math.sqrt(E / n))
        assert abs(mean - E) <= 5 * math.sqrt(E / n)


def test_s_model_fits_and_n_model_misses_the_s_titer(checked):
    """Observed on the host path (2 chains of 150 + 150, sampler seed 0, replicate seed 11, S bins [< 2, >= 2]): S model p_low 0.31 /
    0.85 and p_high 0.73 / 0.17 with ratio intervals 0.73-1.16 and 0.96-1.32; N model p_low 0.000 / 1.000, p_high 1.000 / 0.000."""
    check_statements(checked)


# ---- 5. argument rules ----


def test_default_edges_are_populated_octiles():
    rng = np.random.default_rng(0)
    x, m = rng.uniform(0, 4, (50, 7)), rng.random((50, 7)) < 0.8
    x[~m] = np.nan
    ed = survival.default_edges(x, m)
    assert ed.shape == (7,) and (np.diff(ed) > 0).all()
    counts = np.bincount(R.bin_of(x[m], ed), minlength=8)
    assert (counts > 0).all() and counts.max() - counts.min() <= 2
    few = survival.default_edges(np.array([[0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 2.0, 2.0]]), np.ones((1, 8), bool))  # repeated titers: fewer edges
    np.testing.assert_array_equal(few, [1.0, 2.0])
    assert (np.bincount(R.bin_of([0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 2.0, 2.0], few)) > 0).all()
    assert survival.default_edges(np.ones((2, 2)), np.ones((2, 2), bool)).size == 0  # one value: one bin
    for bad, msg in (((np.ones((2, 2)), np.zeros((2, 2), bool)), "no followed cell"), ((np.full((2, 2), np.inf), np.ones((2, 2), bool)), "finite"),
                     ((np.ones((2, 2)), np.ones((2, 3), bool)), "share a shape")):
        with pytest.raises(ValueError, match=msg):
            survival.default_edges(*bad)
    for bad, msg in (([1.0] * 2, "strictly ascending"), (list(range(8)), "at most 7"), ([0.0, np.nan], "finite")):
        with pytest.raises(ValueError, match=msg):
            survival.check_edges(bad)


def test_predictive_refuses_wrong_arguments(checked):
    m, fit, p = checked["S"]
    y, e, x_s, x_n = simulate(**SIM)
    for by, edges, msg in (({}, None, "one or two"), ({"a": x_s, "b": x_s, "c": x_s}, None, "one or two"), ({"S": x_s}, {"N": [1.0]}, "not binning variables"),
                           ({"S": x_s}, {"S": [2.0, 1.0]}, "strictly ascending")):
        with pytest.raises(ValueError, match=msg):
            survival.predictive(m, dict(fit), by, edges=edges, replicate=m.replicate_host)
    both = survival.predictive(m, dict(fit), {"S": x_s, "N": x_n}, seed=PPC_SEED, replicate=m.replicate_host)  # default edges, two variables
    assert [len(v["observed"]) for v in both["variables"].values()] == [8, 8] and (both["variables"]["N"]["n_cells"] > 0).all()
    np.testing.assert_array_equal(both["variables"]["S"]["replicate"].sum(axis=1), both["variables"]["N"]["replicate"].sum(axis=1))


@pytest.fixture()
def cli(tmp_path, monkeypatch):
    from abdpymc_amd.data import TiterData

    cohort = os.path.join(GOLDEN, "test_cohort")
    data = TiterData.from_disk(cohort)
    rng = np.random.default_rng(0)
    post = tmp_path / "posterior.npz"
    np.savez(post, mean_i=rng.random((data.n_gaps, data.n_inds)) * 0.02, mean_ab_s_mu=rng.normal(size=(data.n_gaps, data.n_inds)),
             mean_ab_n_mu=rng.normal(size=(data.n_gaps, data.n_inds)))
    real = survival.predictive
    monkeypatch.setattr(survival.SurvivalAnalysis, "model_alone",
                        lambda sa, ag: sa._windowed(HostPredictiveModel(sa.infected, sa.exposure, [sa.s_titer if ag == "S" else sa.n_titer], (ag,))))
    monkeypatch.setattr(survival, "predictive", lambda model, fit, by, **kw: real(model, fit, by, **dict(kw, replicate=model.replicate_host)))
    return lambda out, *more: survival.main(["--posterior", str(post), "--ititers_data", cohort, "--start", "2", "--end", "20", "--model", "s",
                                             "--out", str(out), "--tune", "30", "--draws", "30", "--chains", "2", *more])


def test_ppc_flag_adds_one_line_per_variable_after_the_waic_line(cli, tmp_path, capsys):
    assert cli(tmp_path / "plain.npz", "--waic") == 0
    plain = capsys.readouterr().out.splitlines()
    assert cli(tmp_path / "checked.npz", "--waic", "--ppc", "--ppc_edges_n", "0,0.5", "--ppc_seed", "4") == 0
    lines = capsys.readouterr().out.splitlines()
    assert len(plain) == 2 and len(lines) == 4 and lines[:2] == plain and lines[1].startswith("survival WAIC: ")
    assert lines[2].startswith("survival PPC by S: ") and lines[3].startswith("survival PPC by N: ") and "(60 draws)" in lines[3]
    assert "of 3 bins flagged" in lines[3]
    with np.load(tmp_path / "plain.npz") as f:
        assert not set(survival.PPC_FIT_KEYS) & set(f.files)
    with np.load(tmp_path / "checked.npz") as f:
        assert set(survival.PPC_FIT_KEYS) <= set(f.files) and list(f["ppc_variables"]) == ["S", "N"] and int(f["ppc_seed"]) == 4
        assert f["ppc_expected"].shape == (60, 2, 8) and f["ppc_replicate"].shape == (60, 2, 8) and int(f["ppc_n_bins"][1]) == 3
        np.testing.assert_array_equal(f["ppc_edges"][1, :2], [0.0, 0.5])
        assert f["ppc_expected_ind"].shape == f["ppc_observed_ind"].shape == f["elpd_waic_ind"].shape
    for bad in (["--ppc_edges_s", "1,2"], ["--ppc", "--ppc_edges_s", "2,1"], ["--ppc", "--ppc_edges_n", "a"], ["--ppc_seed", "3"]):
        with pytest.raises(SystemExit):
            cli(tmp_path / "bad.npz", *bad)
