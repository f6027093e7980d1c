"""
PSIS-LOO by individual of the survival models, without a GPU: ``compare.psis_loo_from_matrix`` against the two
restatements of tests/survival_loo_restatement.py, the known tail shapes, the edges, the refusals of the new symbols and the
plumbing of ``survival.loo`` / ``loo_of_fit`` / ``compare(ic="loo")`` and the command line.

The bound on a value, relative to max(1, |value|), against the 40-digit restatement: max(64 g, S 2^-53), g the fp64 restatement's
own worst gap to the 40-digit values over these matrices (tests/golden/NOTICE_survival_loo.md): a different order of an S-term sum
alone may move a value by S u.
"""
import ctypes
import types

import numpy as np
import pytest

from tests import survival_loo_restatement as R
from abdpymc_amd import _native, compare, survival

# the fp64 restatement's own worst gap to the 40-digit values (python tests/survival_loo_restatement.py), per quantity
G = dict(elpd=7.4e-14, k=5.0e-15, lppd=3.2e-15)


def bound(what, S):
    return max(64.0 * G[what], S * 2.0 ** -53)


def check_against_40_digits(got, name):
    """``got`` = (elpd, k, lppd, n_tail) of the case's matrix against its 40-digit values: prints every figure, then asserts."""
    ll, ref = R.case(name)
    S = ll.shape[0]
    np.testing.assert_array_equal(np.asarray(got[3]), ref[3])
    for i, what in enumerate(("elpd", "k", "lppd")):
        gap = R.rel_gap(got[i], ref[i])  # asserts the inf / NaN pattern
        print(f"case {name}: {what} gap {gap:.3g} bound {bound(what, S):.3g}")
        assert gap <= bound(what, S), (name, what, gap)


@pytest.mark.parametrize("name", R.CASES)
def test_restatement_is_within_its_recorded_gap(name):
    ll, ref = R.case(name)
    got = R.matrix_of(R.psis_column, ll, R.UNFOLLOWED)
    np.testing.assert_array_equal(got[3], ref[3])
    for i, what in enumerate(("elpd", "k", "lppd")):
        assert R.rel_gap(got[i], ref[i]) <= G[what], (name, what)


@pytest.mark.parametrize("name", R.CASES)
def test_host_path_against_the_restatements(name):
    ll, _ = R.case(name)
    got = compare.psis_loo_from_matrix(ll)
    fp64 = R.matrix_of(R.psis_column, ll, R.UNFOLLOWED)
    np.testing.assert_array_equal(got[3], fp64[3])  # the tail is decided by exact operations
    np.testing.assert_array_equal(np.isposinf(got[1]), np.isposinf(fp64[1]))
    np.testing.assert_array_equal(np.isnan(got[1]), np.isnan(fp64[1]))
    check_against_40_digits(got, name)


@pytest.mark.parametrize("k0", (0.3, 0.7))
def test_known_tail_shape(k0):
    ll = R.known_k(k0)
    assert ll.shape == (4000, 64)
    med = float(np.median(R.matrix_of(R.psis_column, ll)[1]))
    print(f"k0 {k0}: the restatement's median k {med:.4f}")
    assert abs(med - k0) <= 0.1  # a condition on the restatement first
    got = float(np.median(compare.psis_loo_from_matrix(ll)[1]))
    print(f"k0 {k0}: the host path's median k {got:.4f}")
    assert abs(got - k0) <= 0.1


def test_edges():
    lse = compare._logsumexp
    # S = 24: M = 4, so n_tail <= 4, k = +inf and the weights are the raw x
    ll, _ = R.case(24)
    elpd, k, lppd, n_tail = compare.psis_loo_from_matrix(ll)
    assert R.tail_len(24) == 4 and (n_tail[:5] <= 4).all() and np.isposinf(k[:5]).all()
    for j in range(5):
        x = -ll[:, j] - (-ll[:, j]).max()
        assert elpd[j] == lse(ll[:, j] + (x - lse(x)))
        assert lppd[j] == lse(ll[:, j]) - np.log(24)
    # S = 25: M = 5, the smallest tail that is fitted
    ll, _ = R.case(25)
    elpd, k, lppd, n_tail = compare.psis_loo_from_matrix(ll)
    assert R.tail_len(25) == 5 and (n_tail[:4] == 5).all() and np.isfinite(k[:4]).all()
    # every row four times: ties at the cut-off fall out of the tail
    ll, _ = R.case("ties")
    assert ll.shape[0] == 404 and all((ll[:101] == ll[101 * r:101 * (r + 1)]).all() for r in range(4))
    n_tail = compare.psis_loo_from_matrix(ll)[3]
    assert R.tail_len(404) == 61 and (n_tail[:4] == 60).all()
    # a spread above 750: exp underflows and the cut is clipped at log(DBL_MIN)
    for name in R.CASES:
        ll, _ = R.case(name)
        S, col = ll.shape[0], ll[:, 4]
        x = -col - (-col).max()
        assert x.min() < -750 and np.sort(x)[S - R.tail_len(S) - 1] < np.log(R.DBL_MIN) and np.exp(x.min()) == 0.0
        assert compare.psis_loo_from_matrix(ll)[3][4] == (x > np.log(R.DBL_MIN)).sum() < R.tail_len(S)
    # an unfollowed individual
    ll, _ = R.case(257)
    for cells in (None, np.array([3, 3, 3, 3, 3, 0])):
        elpd, k, lppd, n_tail = compare.psis_loo_from_matrix(ll, cells)
        assert elpd[5] == 0.0 and lppd[5] == 0.0 and np.isnan(k[5]) and n_tail[5] == 0
    w = compare.loo_from_individual(elpd, k, lppd, np.array([3, 3, 3, 3, 3, 0]), 257)
    assert w["n_individuals"] == 5 and w["elpd_loo"] == elpd[:5].sum() and w["se"] == np.sqrt(5 * np.var(elpd[:5]))
    assert w["p_loo"] == (lppd[:5] - elpd[:5]).sum()
    assert w["n_bad"] == (k[:5] > 0.7).sum() and w["n_warn"] == (k[:5] > min(1 - 1 / np.log10(257), 0.7)).sum() >= w["n_bad"]
    assert w["worst"] == int(np.argmax(k[:5]))


def test_new_symbols_refuse_before_the_device_is_touched():
    """Argument errors need no GPU."""
    lib = _native.load()
    buf, n, i32 = np.zeros(8), ctypes.c_int64(), np.zeros(8, np.int32)
    p = buf.ctypes.data
    for call in (lambda: lib.abd_survival_loo_reserve(None, 8), lambda: lib.abd_survival_loo_reset(None),
                 lambda: lib.abd_survival_loo_accumulate(None, 1, p), lambda: lib.abd_survival_loo_append_rows(None, 1, p),
                 lambda: lib.abd_survival_loo_rows(None, 0, 1, p),
                 lambda: lib.abd_survival_loo_stats(None, p, p, p, i32.ctypes.data, ctypes.byref(n), i32.ctypes.data)):
        lib.abd_survival_dim(None)
        assert call() == -1
        assert b"NULL" in lib.abd_last_error()
    header = open(_native.__file__.replace("abdpymc_amd/_native.py", "include/abd_hip.h")).read()
    for name in ("reserve", "reset", "accumulate", "append_rows", "rows", "stats"):
        assert "abd_survival_loo_" + name in _native.SYMBOLS and f"int abd_survival_loo_{name}(" in header
    assert "#define ABD_SURVIVAL_LOO_MAX_DRAWS 16384" in header and _native.Survival.LOO_MAX_DRAWS == 16384


# ---- plumbing ----


class HostModel:
    """What ``survival.loo`` / ``waic`` ask of a model with ``pointwise=``: two parameters, N individuals, one of them unfollowed."""

    names = ("a", "b")

    def __init__(self, shift, N=40, seed=5):
        rng = np.random.default_rng(seed)
        self.u = rng.normal(size=N)
        self.n_cells = np.full(N, 4, dtype=np.int64)
        self.n_cells[7] = 0
        self.shift, self.start, self.end = shift, 2, 20

    def pointwise(self, q):
        ll = -0.5 * (self.u[None, :] - q[:, :1] - self.shift) ** 2 * np.exp(q[:, 1:2])
        ll[:, 7] = 0.0
        return ll


def make_fit(seed=0, chains=2, draws=60):
    rng = np.random.default_rng(seed)
    return {"a": rng.normal(0.0, 0.3, (chains, draws)), "b": rng.normal(0.0, 0.2, (chains, draws))}


def test_loo_records_its_keys_and_round_trips_through_write(tmp_path):
    m, fit = HostModel(0.0), make_fit()
    w = survival.loo(m, fit, pointwise=m.pointwise)
    assert survival.LOO_FIT_KEYS == ("elpd_loo_ind", "pareto_k_ind", "lppd_ind", "loo_n_cells", "loo_n_draws")
    assert all(k in fit for k in survival.LOO_FIT_KEYS) and int(fit["start"]) == 2 and int(fit["end"]) == 20
    q = survival.fit_points(m, fit)
    assert q.shape == (120, 2) and (q[60 + 3] == [fit["a"][1, 3], fit["b"][1, 3]]).all()  # chain after chain
    elpd, k, lppd, _ = compare.psis_loo_from_matrix(m.pointwise(q), m.n_cells)
    np.testing.assert_array_equal(fit["elpd_loo_ind"], elpd)
    np.testing.assert_array_equal(fit["pareto_k_ind"], k)
    assert w["n_draws"] == 120 and w["n_individuals"] == 39 and np.isnan(w["pareto_k"][7]) and w["elpd_i"][7] == 0.0
    assert w["elpd_loo"] == elpd.sum() and w["p_loo"] == (lppd - elpd).sum() and w["p_loo"] > 0
    sa = types.SimpleNamespace(start=2, end=20, intervals=np.arange(18), t0="2020-01", infected=np.zeros((40, 18)))
    path = survival.write(fit, str(tmp_path / "fit.npz"), sa)
    with np.load(path) as f:
        stored = {key: f[key] for key in f.files}
    again = survival.loo_of_fit(stored)
    for key in ("elpd_loo", "p_loo", "se", "n_bad", "n_warn", "n_draws", "n_individuals", "worst"):
        assert again[key] == w[key], key
    np.testing.assert_array_equal(again["pareto_k"], w["pareto_k"])
    line = survival.loo_line(w)
    assert line.startswith("survival PSIS-LOO: elpd_loo ") and " p_loo " in line and " se " in line and "pareto_k > 0.7" in line
    assert ("warning" in line) == (w["n_bad"] > 0)
    bad = dict(w, n_bad=1, worst=3, pareto_k=np.where(np.arange(40) == 3, 0.93, w["pareto_k"]))
    assert "warning" in survival.loo_line(bad) and "individual 3 pareto_k 0.93" in survival.loo_line(bad)
    with pytest.raises(ValueError, match="no PSIS-LOO in the fit"):
        survival.loo_of_fit(make_fit())


def test_compare_ranks_by_loo_and_is_unchanged_for_waic(tmp_path, capsys):
    models = {"near": HostModel(0.0), "far": HostModel(1.5)}
    fits = {}
    for name, m in models.items():
        fits[name] = make_fit()
        survival.waic(m, fits[name], pointwise=m.pointwise)
        survival.loo(m, fits[name], pointwise=m.pointwise)
    table = survival.compare(fits, ic="loo")
    assert table["near"]["rank"] == 0 and table["far"]["rank"] == 1 and table["near"]["elpd_diff"] == 0.0
    w = {name: survival.loo_of_fit(f) for name, f in fits.items()}
    assert table["far"]["elpd_loo"] == w["far"]["elpd_loo"] and table["far"]["p_loo"] == w["far"]["p_loo"]
    assert table["far"]["elpd_diff"] == w["near"]["elpd_loo"] - w["far"]["elpd_loo"] > 0
    has = models["near"].n_cells > 0
    assert table["far"]["dse"] == float(np.sqrt(39 * np.var((w["near"]["elpd_i"] - w["far"]["elpd_i"])[has])))
    assert "elpd_waic" not in table["far"]
    # without ic: what it returned before
    today = compare.compare({name: survival.waic_of_fit(f) for name, f in fits.items()}, by="individual")
    assert survival.compare(fits) == today == survival.compare(fits, ic="waic")
    assert survival.compare_lines(today)[0].split()[2:4] == ["0", "elpd_waic"]
    with pytest.raises(ValueError, match="ic must be"):
        survival.compare(fits, ic="dic")
    with pytest.raises(ValueError, match="far: no PSIS-LOO"):
        survival.compare({"near": fits["near"], "far": {k: v for k, v in fits["far"].items() if k not in survival.LOO_FIT_KEYS}}, ic="loo")
    # the command line: --compare FIT... --ic loo needs neither a cohort nor a GPU
    sa = types.SimpleNamespace(start=2, end=20, intervals=np.arange(18), t0="", infected=np.zeros((40, 18)))
    paths = [survival.write(fits[name], str(tmp_path / f"{name}.npz"), sa) for name in ("far", "near")]
    capsys.readouterr()
    assert survival.main(["--compare"] + paths + ["--ic", "loo"]) == 0
    rows = capsys.readouterr().out.strip().split("\n")
    assert len(rows) == 2 and rows[0].split()[:4] == ["near", "rank", "0", "elpd_loo"] and rows[1].split()[0] == "far"
    assert survival.main(["--compare"] + paths) == 0
    assert capsys.readouterr().out.strip().split("\n") == survival.compare_lines(today)
    fit_args = ["--posterior", "p.npz", "--ititers_data", "d", "--start", "2", "--end", "20", "--out", "o.npz", "--model", "s"]
    with pytest.raises(SystemExit):
        survival.main(fit_args + ["--per_draw", "2", "--loo"])
    assert "--per_draw does not go with --loo" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        survival.main(fit_args + ["--ic", "loo"])
    assert "--ic goes with --compare" in capsys.readouterr().err
