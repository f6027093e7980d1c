"""
The per-individual log-likelihood of the survival models and the comparison of fitted models on the CPU: the
committed 40-digit fixture regenerated, the NumPy restatement against it (``E_NP``), the 40-digit ll_j against the 40-digit data
log-likelihood written the other way round, the host header ``abd_survival_pointwise_terms.hpp`` through its stand-alone harness,
the refusals of the four new symbols (no GPU), ``survival.waic(pointwise=)`` / ``survival.compare`` and the command line's
``--waic`` / ``--compare`` on host models.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from abdpymc_amd import _native, compare, survival
from tests import survival_pointwise_restatement as P
from tests import survival_restatement as R1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def fixture():
    return P.load_fixture(GOLDEN)


@pytest.fixture(scope="module")
def models():
    """the restatement object of every shape of the table, made once"""
    out = {}
    for key, N, T, K, Gr, name in P.cases():
        if (N, T, K, Gr) not in out:
            out[(N, T, K, Gr)] = P.model_of(N, T, K, Gr)[0]
    return out


def test_fixture_is_the_40_digit_statement(fixture):
    import mpmath  # noqa: F401  (no skip: this test is what ties the committed file to mp_pointwise)

    for key, N, T, K, Gr, name in (("N1_T1_K1_eta_800", 1, 1, 1, None, "eta_800"), ("N67_T30_G3_a_spread", 67, 30, None, 3, "a_spread")):
        rs, _ = P.model_of(N, T, K, Gr)
        r = P.mp_pointwise(rs, P.point_of(name, T, K, Gr))
        for what, v in r.items():
            np.testing.assert_array_equal(np.asarray(v), fixture[f"{key}/{what}"])


def test_case_table_is_what_the_kernel_can_get_wrong(fixture, models):
    assert len(list(P.cases())) == 4 * 2 * 8 + 2 * 9 and len(fixture) == 2 * len(list(P.cases()))
    for (N, T, K, Gr), rs in models.items():
        C, cells = P.constants(rs)
        np.testing.assert_array_equal(cells, survival.followed_cells(*P.model_of(N, T, K, Gr)[1][1:3]))
        if N > 64:  # every multi-tile shape has an individual without a followed cell: its ll_j and S_j are exactly 0
            assert (cells == 0).any() and (C[cells == 0] == 0).all()
            key = f"N{N}_T{T}_" + (f"K{K}" if Gr is None else f"G{Gr}") + "_typical"
            assert (fixture[key + "/ll_S"][cells == 0] == 0).all() and (fixture[key + "/ll"][cells == 0] == 0).all()
            assert (fixture[key + "/ll_S"][cells > 0] > 0).all()
    assert (P.constants(models[(130, 65, None, 4)])[1][models[(130, 65, None, 4)].group == 3] == 0).all()


def test_restatement_against_the_40_digit_reference(fixture, models):
    """The worst error of the float64 restatement over the case table, per class of point, in units of u S_j: E_NP of the
    restatement file; an individual with S_j = 0 gets exactly 0."""
    worst = {name: (0.0, None) for name in P.POINTS_GROUPS}
    for key, N, T, K, Gr, name in P.cases():
        got = P.pointwise(models[(N, T, K, Gr)], P.point_of(name, T, K, Gr))
        ref, S = fixture[key + "/ll"], fixture[key + "/ll_S"]
        assert got.shape == (N,) and np.isfinite(got).all(), key
        assert (got[S == 0] == 0).all(), key
        e_ = float((np.abs(got - ref)[S > 0] / S[S > 0] / P.U).max())
        if e_ > worst[name][0]:
            worst[name] = (e_, key)
    for name, (e_, where) in worst.items():
        print(f"E_np_pointwise[{name}] = {e_:.2f} u S at {where}")
    for name, (e_, where) in worst.items():
        assert e_ <= P.E_NP[name], (name, e_, where)
        assert P.c_device(name) == 4.0 * P.E_NP[name]


@pytest.mark.parametrize("N,T,K,Gr,name", [(67, 30, 2, None, "typical"), (67, 30, 1, None, "r_minus_800"), (67, 30, None, 3, "a_spread"),
                                           (130, 65, None, 4, "b_plus_50")])
def test_individuals_add_up_to_the_data_loglik_at_40_digits(models, N, T, K, Gr, name):
    import mpmath as mp

    rs = models[(N, T, K, Gr)]
    q = P.point_of(name, T, K, Gr)
    total = mp.fsum(P.mp_pointwise(rs, q, raw=True)["ll"])
    whole = P.mp_data_loglik(rs, q)
    assert abs(total - whole) <= mp.mpf("1e-30") * abs(whole), (total, whole)
    # and the float64 restatement's sum is that number to float64's accuracy of a sum of N terms
    assert abs(P.pointwise(rs, q).sum() - float(whole)) <= 1e-12 * abs(float(whole))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = tmp_path_factory.mktemp("survival_pointwise") / "survival_pointwise_harness"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "abdpymc_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "survival_pointwise_harness.cpp"), "-o", str(out)])
    return str(out)


@pytest.mark.parametrize("N,T,K,Gr,name,n_draw", [(67, 30, 1, None, "typical", 0), (130, 65, 2, None, "r_minus_800", 3),
                                                  (130, 65, None, 4, "a_spread", 4000), (1, 1, 1, None, "sd_e10", 1)])
def test_host_terms_equal_the_restatement(harness, models, tmp_path, N, T, K, Gr, name, n_draw):
    rs = models[(N, T, K, Gr)]
    q = P.point_of(name, T, K, Gr)
    ld = (N + 63) // 64 * 64
    y, e = np.zeros((T, ld)), np.zeros((T, ld))  # the planes as creation lays them out: cleaned, padded with unfollowed cells
    y[:, :N], e[:, :N] = rs.y.T, rs.e.T
    K = K or 1
    n_ab = 2 * K if Gr is None else Gr + 1
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([T, ld, K, Gr or 0, n_draw], dtype=np.int64).tobytes() + y.tobytes() + e.tobytes() + q.tobytes())
    subprocess.check_call([harness, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    out = np.fromfile(tmp_path / "out.bin")
    assert out.shape == (2 * ld + 2 * T + n_ab + 1,)
    C, cells, row = out[:ld], out[ld:2 * ld], out[2 * ld:]
    C_ref, cells_ref = P.constants(rs)
    np.testing.assert_array_equal(cells[:N], cells_ref)
    assert (cells[N:] == 0).all() and (C[N:] == 0).all() and (C[:N][cells_ref == 0] == 0).all()
    # a compensated sum against fsum of the same terms; the terms themselves come from two libraries: log and the product within a
    # few u of the term, and lgamma(y + 1) for y + 1 in [1, 2] -- where lgamma passes through 0 -- within a few u of 1, not of its
    # own small value, in Python's math.lgamma (a Lanczos sum of size 1): 4 u per term for each
    sabs = np.array([sum(abs(yy * math.log(ee)) + abs(math.lgamma(yy + 1.0)) for yy, ee in zip(yr, er) if yy > 0) for yr, er in zip(rs.y, rs.e)])
    assert (np.abs(C[:N] - C_ref) <= 4 * P.U * (sabs + (rs.y > 0).sum(axis=1))).all()
    ref = P.parameter_row(rs, q, n_draw)
    # lambda, log lambda: two libraries' exp and log1p (each within 1 ulp), one addition and one division each: a few u
    np.testing.assert_allclose(row[:2 * T], ref[:2 * T], rtol=1e-15, atol=0)
    if Gr is None:
        np.testing.assert_array_equal(row[2 * T:2 * T + n_ab], ref[2 * T:2 * T + n_ab])  # a, b as given
    else:  # a_g = a_mu + a_sd z_g may cancel to the size of u (|a_mu| + a_sd |z_g|)
        m, s, z, a_mu, a_sl, az, b = rs.split(q)
        np.testing.assert_allclose(row[2 * T:2 * T + Gr], ref[2 * T:2 * T + Gr], rtol=0, atol=4 * P.U * (abs(a_mu) + np.exp(a_sl) * np.abs(az).max()))
        assert row[2 * T + Gr] == b
    assert row[-1] == (1.0 / n_draw if n_draw else 0.0)  # the host's division, exactly


def test_new_symbols_refuse_null_without_a_gpu():
    lib = _native.load()
    buf = np.zeros(8)
    n, cells = ctypes.c_int64(), np.zeros(8, np.int32)
    for call in (lambda: lib.abd_survival_individual_loglik(None, 1, buf.ctypes.data, buf.ctypes.data),
                 lambda: lib.abd_survival_waic_reset(None),
                 lambda: lib.abd_survival_waic_accumulate(None, 1, buf.ctypes.data),
                 lambda: lib.abd_survival_waic_stats(None, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, ctypes.byref(n), cells.ctypes.data)):
        lib.abd_survival_dim(None)
        assert call() == -1
        assert b"NULL" in lib.abd_last_error()
    for name in ("abd_survival_individual_loglik", "abd_survival_waic_reset", "abd_survival_waic_accumulate", "abd_survival_waic_stats"):
        assert name in _native.SYMBOLS


# ---- survival.waic / survival.compare on host models ----


def _names(K, T, antigens):
    ab = [f"{v}_{ag}" for v in "ab" for ag in antigens] if K > 1 else ["a", "b"]
    return tuple(ab + ["_lam0_raw_mu", "_lam0_raw_sd_log__"] + [f"__lam0_raw_z_{t}" for t in range(T)])


class HostModel:
    """What ``survival.sample`` / ``waic`` / ``main`` ask of a model, on the NumPy restatement."""

    def __init__(self, infected, exposure, titers, antigens, start=None, end=None):
        self.rs = R1.Restatement(infected, exposure, titers)
        self.K, self.dim, self.T, self.antigens = self.rs.K, self.rs.dim, self.rs.T, tuple(antigens)
        self.priors = survival.PRIORS[self.K]
        self.names = _names(self.K, self.T, self.antigens)
        self.n_cells = survival.followed_cells(infected, exposure)
        self.logp_dlogp = self.rs.logp_dlogp
        self.pointwise = P.pointwise_matrix(self.rs)
        self.rows = []
        if start is not None:
            self.start, self.end = start, end

    def waic_reset(self):
        self.rows = []

    def waic_accumulate(self, q):
        self.rows.append(self.pointwise(q))

    def waic_stats(self):
        return compare.stats_from_matrix(np.concatenate(self.rows)), self.n_cells

    def close(self):
        pass


# Data from an S-only model: the hazard depends on the S titer alone (a = 1.5, b = 2; tests/test_survival_cpu.py says why b > 0),
# the N titer is independent noise.  The data seed and the lengths were chosen on the CPU so that the margin below holds with room:
# what the test runs -- 2 chains of 150 + 150, sampler seed 0 -- ranks S first, combined second (elpd_diff 1.8, dse 2.5: the N
# slope earns nothing) and N last; S against N alone: elpd_diff 28.9, dse 6.3, that is 4.6 dse; data seeds 1, 2, 4 gave 5.4, 3.9
# and 5.8 dse.
SIM = dict(N=300, T=6, seed=3, a=1.5, b=2.0)


def simulate(N, T, seed, a, b):
    rng = np.random.default_rng(seed)
    x_s, x_n = rng.uniform(0.0, 4.0, size=(N, T)), rng.uniform(0.0, 4.0, size=(N, T))
    lam0 = rng.uniform(0.15, 0.3, size=T)
    e = rng.uniform(0.3, 1.0, size=(N, T))
    y = rng.poisson(e * lam0[None, :] / (1.0 + np.exp(-b * (x_s - a)))).astype(np.float64)
    return y, e, x_s, x_n


def variants(y, e, x_s, x_n, make):
    return {"S": make(y, e, [x_s], ("S",)), "N": make(y, e, [x_n], ("N",)), "combined": make(y, e, [x_s, x_n], ("S", "N"))}


def fit_and_score(models, use_device):
    fits, w = {}, {}
    for name, m in models.items():
        fits[name] = survival.sample(m, tune=150, draws=150, chains=2, seed=0, evaluator=None if use_device else m.logp_dlogp)
        w[name] = survival.waic(m, fits[name], pointwise=None if use_device else m.pointwise)
    return fits, w


@pytest.fixture(scope="module")
def simulated():
    models = variants(*simulate(**SIM), make=lambda y, e, xs, ag: HostModel(y, e, xs, ag, start=0, end=SIM["T"] + 1))
    return (models,) + fit_and_score(models, use_device=False)


def test_waic_is_waic_from_matrix_by_individual(simulated):
    models, fits, w = simulated
    m, fit = models["combined"], fits["combined"]
    q = survival.fit_points(m, fit)
    assert q.shape == (300, m.dim)
    np.testing.assert_array_equal(q[150 + 7], [fit[name][1, 7] for name in m.names])  # chain after chain
    y, e, x_s, x_n = simulate(**SIM)
    e[5] = np.nan  # an individual without follow-up
    hm = HostModel(y, e, [x_s, x_n], ("S", "N"))
    ll = hm.pointwise(q)
    assert ll.shape == (300, 300) and (ll[:, 5] == 0).all() and hm.n_cells[5] == 0 and (np.delete(hm.n_cells, 5) == 6).all()
    got = survival.waic(hm, dict(fit), pointwise=hm.pointwise)
    followed = np.flatnonzero(hm.n_cells > 0)
    ref = compare.waic_from_matrix(ll[:, followed], groups=followed, n_groups=300)
    for k in ("elpd_waic", "p_waic", "se", "n_warn", "n_draws", "n_individuals"):
        assert got[k] == ref[k], k
    np.testing.assert_array_equal(got["elpd_i"], ref["elpd_i"])
    np.testing.assert_array_equal(got["p_waic_i"], ref["p_waic_i"])
    assert got["elpd_i"][5] == 0.0 and got["p_waic_i"][5] == 0.0 and got["n_individuals"] == 299 and got["n_draws"] == 300
    # the device's place taken by the model's own accumulate / stats: the same plumbing, the same numbers
    via = survival.waic(hm, dict(fit))
    np.testing.assert_array_equal(via["elpd_i"], got["elpd_i"])
    # what waic records in the fit is what waic_of_fit reads again
    rec = dict(fit)
    survival.waic(m, rec, pointwise=m.pointwise)
    assert all(k in rec for k in survival.WAIC_FIT_KEYS) and int(rec["start"]) == 0 and int(rec["end"]) == 7
    again = survival.waic_of_fit(rec)
    for k in ("elpd_waic", "p_waic", "se", "n_warn", "n_draws", "n_individuals"):
        assert again[k] == w["combined"][k], k


def test_s_model_ranks_above_n_model_on_s_only_data(simulated):
    models, fits, w = simulated
    table = survival.compare(fits)
    for name, row in table.items():
        print(name, {k: round(float(v), 3) for k, v in row.items()})
    assert sorted(v["rank"] for v in table.values()) == [0, 1, 2]
    assert table["N"]["rank"] == 2 and table["S"]["rank"] < table["N"]["rank"]
    gap = table["N"]["elpd_waic"] - table["S"]["elpd_waic"]
    pair = compare.compare({"S": w["S"], "N": w["N"]}, by="individual")
    assert pair["S"]["rank"] == 0 and pair["N"]["elpd_diff"] == -gap
    print("S over N: elpd_diff", pair["N"]["elpd_diff"], "dse", pair["N"]["dse"])
    assert pair["N"]["elpd_diff"] > 2.0 * pair["N"]["dse"] > 0.0
    for v in table.values():
        assert v["elpd_diff"] >= 0 and np.isfinite(list(v.values())).all()


def test_compare_refuses_another_window_and_names_it(simulated):
    models, fits, w = simulated
    odd = dict(fits["N"], end=np.array(9))
    with pytest.raises(ValueError) as ei:
        survival.compare({"S": fits["S"], "late": odd, "combined": fits["combined"]})
    assert "late differs" in str(ei.value) and "start / end" in str(ei.value) and "end 9" in str(ei.value) and "S differs" not in str(ei.value)
    fewer = dict(fits["N"], waic_n_cells=np.where(np.arange(300) == 3, 0, fits["N"]["waic_n_cells"]))
    with pytest.raises(ValueError) as ei:
        survival.compare({"S": fits["S"], "combined": fits["combined"], "other": fewer})
    assert "other differs" in str(ei.value) and "followed" in str(ei.value)
    short = {k: (v[:-1] if k in ("elpd_waic_ind", "p_waic_ind", "waic_n_cells") else v) for k, v in fits["N"].items()}
    with pytest.raises(ValueError) as ei:
        survival.compare({"S": fits["S"], "combined": fits["combined"], "short": short})
    assert "short differs" in str(ei.value) and "number of individuals" in str(ei.value)
    with pytest.raises(ValueError) as ei:
        survival.compare({"S": fits["S"], "bare": {k: v for k, v in fits["N"].items() if k != "p_waic_ind"}})
    assert "bare" in str(ei.value) and "p_waic_ind" in str(ei.value)


# ---- the command line, the device's place taken by host models ----


@pytest.fixture()
def cli(tmp_path, monkeypatch):
    from abdpymc_amd.data import TiterData

    cohort = os.path.join(GOLDEN, "test_cohort")
    data = TiterData.from_disk(cohort)
    G, N = data.n_gaps, data.n_inds
    rng = np.random.default_rng(0)
    post = tmp_path / "posterior.npz"
    np.savez(post, mean_i=rng.random((G, N)) * 0.02, mean_ab_s_mu=rng.normal(size=(G, N)), mean_ab_n_mu=rng.normal(size=(G, N)))
    SA = survival.SurvivalAnalysis
    monkeypatch.setattr(SA, "model_alone", lambda sa, ag: sa._windowed(HostModel(sa.infected, sa.exposure, [sa.s_titer if ag == "S" else sa.n_titer], (ag,))))
    monkeypatch.setattr(SA, "model_combined", lambda sa: sa._windowed(HostModel(sa.infected, sa.exposure, [sa.s_titer, sa.n_titer], ("S", "N"))))
    return lambda which, out, *more: survival.main(["--posterior", str(post), "--ititers_data", cohort, "--start", "2", "--end", "20", "--model", which,
                                                    "--out", str(out), "--tune", "30", "--draws", "30", "--chains", "2", *more])


def test_waic_flag_adds_exactly_one_stdout_line(cli, tmp_path, capsys):
    assert cli("s", tmp_path / "plain.npz") == 0
    plain = capsys.readouterr().out.splitlines()
    assert cli("s", tmp_path / "scored.npz", "--waic") == 0
    scored = capsys.readouterr().out.splitlines()
    assert len(plain) == 1 and len(scored) == 2 and scored[0] == plain[0]
    assert scored[1].startswith("survival WAIC: elpd_waic ") and " p_waic " in scored[1] and " se " in scored[1]
    assert "individuals, 60 draws; " in scored[1] and scored[1].endswith(" with p_waic_j > 0.4)")
    with np.load(tmp_path / "plain.npz") as f:
        assert not set(survival.WAIC_FIT_KEYS + ("start", "end")) & set(f.files)
    with np.load(tmp_path / "scored.npz") as f:
        N = f["elpd_waic_ind"].shape[0]
        assert f["p_waic_ind"].shape == (N,) and f["waic_n_cells"].shape == (N,) and int(f["waic_n_draws"]) == 60
        assert int(f["start"]) == 2 and int(f["end"]) == 20 and (f["elpd_waic_ind"][f["waic_n_cells"] == 0] == 0).all()
        assert f"({int((f['waic_n_cells'] > 0).sum())} individuals, " in scored[1]


def test_compare_flag_prints_one_row_per_fit(cli, tmp_path, capsys):
    for which in ("s", "n", "combined"):
        assert cli(which, tmp_path / f"fit_{which}.npz", "--waic") == 0
    capsys.readouterr()
    assert survival.main(["--compare"] + [str(tmp_path / f"fit_{w}.npz") for w in ("s", "n", "combined")]) == 0
    cap = capsys.readouterr()
    rows = cap.out.splitlines()
    assert len(rows) == 3 and sorted(r.split()[0] for r in rows) == ["fit_combined", "fit_n", "fit_s"]
    for k, r in enumerate(rows):
        assert f" rank {k} " in r
        for word in ("elpd_waic", "p_waic", "se", "elpd_diff", "dse"):
            assert f" {word} " in r
    assert " elpd_diff 0.000 " in rows[0]
    assert cli("s", tmp_path / "fit_plain.npz") == 0  # a fit written without --waic is refused by name
    with pytest.raises(SystemExit) as ei:
        survival.main(["--compare", str(tmp_path / "fit_s.npz"), str(tmp_path / "fit_plain.npz")])
    assert "fit_plain" in str(ei.value)
    with pytest.raises(SystemExit):
        survival.main(["--model", "s"])  # without --compare the fit's arguments are required as before
