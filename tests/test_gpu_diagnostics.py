"""
The per-cell convergence accumulators of the native sampler (abd_sampler_enable_diagnostics / abd_sampler_diagnostics;
sample(diagnostics=True); the CLI's --diagnostics) against diagnostics.from_draws of the draws the same run recorded, by the
gates derived in tests/test_diagnostics_cpu.py with the recorded titers as the reference; what the accumulators must not
depend on, as byte equality; the errors; the teardown.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest

from abdpymc_amd import diagnostics as dg
from abdpymc_amd import synthetic
from abdpymc_amd._native import AbdError
from abdpymc_amd.data import TiterData
from tests.test_diagnostics_cpu import EPS, m2_gate, mean_gate
from tests.test_gpu_pointwise import _same_trajectories

pytestmark = pytest.mark.gpu
TUNE, DRAWS, BATCH = 6, 21, 3  # H = 10, B = 3: a trailing draw in each half, the odd last draw ignored


def _dense_model(N, G, n_chains, seed=11):
    from abdpymc_amd.model import AbdModel

    sc = synthetic.make_cohort(N, G, seed=seed)
    d = SimpleNamespace(n_gaps=sc.n_gaps, n_inds=sc.n_inds, vacs=sc.vacs, pcrpos=sc.pcrpos,
                        coords={"gap": np.arange(sc.n_gaps), "ind": np.arange(sc.n_inds)},
                        s=SimpleNamespace(obs=sc.s_obs), n=SimpleNamespace(obs=sc.n_obs))
    return AbdModel(d, n_chains=n_chains)


def _model(which, golden_dir, n_chains):
    from abdpymc_amd.model import model

    if which == "test":  # observation lists
        return model(TiterData.from_disk(os.path.join(golden_dir, "test_cohort")), n_chains=n_chains)
    return _dense_model(100, 70, n_chains)


def delta(xmax, n):
    """What a titer of the accumulators may differ by from the recorded one (the Deterministics tests' per-titer gate) plus
    Welford rounding over n values."""
    return 1e-12 * xmax + 1e-13 + 4 * n * EPS * xmax


def check_against_draws(res, L):
    """every diag_* key of res against from_draws of the i / ab_n_mu / ab_s_mu the same run recorded (unthinned)"""
    D = res["i"].shape[1]
    H, B = D // 2, D // 2 // L
    want_i = dg.from_draws(res["i"], L)
    np.testing.assert_array_equal(res["diag_i_counts"], want_i["counts"])
    assert res["diag_i_counts"].dtype == np.int64 and res["diag_info"].dtype == np.int64
    np.testing.assert_array_equal(res["diag_info"], want_i["info"])
    assert res["diag_info"][0].tolist() == [H, H, 2 * B, L]
    for var in ("ab_n_mu", "ab_s_mu"):
        x = res[var][:, :2 * H]
        got, ref = res[f"diag_{var}"], dg.from_draws(res[var], L)["moments"]
        assert got.shape == ref.shape
        xmax = np.abs(x).max()
        d = delta(xmax, H)
        for h in (0, 1):
            err_mean, err_m2 = np.abs(got[:, 2 * h] - ref[:, 2 * h]), np.abs(got[:, 2 * h + 1] - ref[:, 2 * h + 1])
            gate_m2 = m2_gate(H, ref[:, 2 * h + 1], xmax, d)
            print(f"{var} half {h}: mean error {err_mean.max():.3e} (gate {d:.3e}), M2 error {err_m2.max():.3e} (gate at that cell "
                  f"{gate_m2.ravel()[err_m2.argmax()]:.3e})")
            assert (err_mean <= d).all(), (var, h)
            assert (err_m2 <= gate_m2).all(), (var, h)
        if B:
            chains = x.shape[0]
            bm = np.concatenate([x[:, h * H:h * H + B * L].reshape((chains, B, L) + x.shape[2:]).mean(axis=2) for h in (0, 1)], axis=1)
            bmax = np.abs(bm).max()
            db = delta(bmax, 2 * B)
            err_mean, err_m2 = np.abs(got[:, 4] - ref[:, 4]), np.abs(got[:, 5] - ref[:, 5])
            print(f"{var} batch means: mean error {err_mean.max():.3e} (gate {db:.3e}), M2 error {err_m2.max():.3e}")
            assert (err_mean <= db).all(), var
            assert (err_m2 <= m2_gate(2 * B, ref[:, 5], bmax, db)).all(), var
        # something happened in these cells: the test is not about zeros
        assert (got[:, 1] > 0).any() and np.isfinite(got).all()


def _same_diag(a, b):
    for k in dg.RESULT_KEYS:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
        assert a[k].tobytes() == b[k].tobytes(), k


_runs = {}


def run(golden_dir, which, chains, **kw):
    """sample(...) of the main case, computed once per variant and left alone"""
    from abdpymc_amd.sampler import sample

    key = (which, chains, tuple(sorted(kw.items())))
    if key not in _runs:
        m = _model(which, golden_dir, chains)
        launch = kw.pop("launch_config", None)
        if launch:
            m.ctx.set_launch_config(*launch)
        _runs[key] = sample(m, tune=TUNE, draws=DRAWS, chains=chains, seed=7, **kw)
        m.close()
    return _runs[key]


@pytest.mark.parametrize("chains", [2, 5])  # units of 1 and of 2 chains
@pytest.mark.parametrize("which", ["dense", "test"])
def test_accumulators_equal_from_draws_of_the_recorded_draws(golden_dir, which, chains):
    res = run(golden_dir, which, chains, diagnostics=True, diag_batch=BATCH)
    G, N = res["i"].shape[2:]
    assert res["diag_i_counts"].shape == (chains, 4, G, N) and res["diag_ab_n_mu"].shape == (chains, 6, G, N)
    assert res["diag_ab_s_mu"].shape == (chains, 6, G, N) and res["diag_info"].shape == (chains, 4)
    assert res["diag_info"].tolist() == [[10, 10, 6, 3]] * chains
    check_against_draws(res, BATCH)
    sm = dg.summary(res)
    assert sm["i"]["rhat"].shape == (G, N) and sm["i"]["n_constant"] + np.isfinite(sm["i"]["rhat"]).sum() + np.isinf(sm["i"]["rhat"]).sum() == G * N
    assert set(sm["scalars"]) >= {"lp"} and len(sm["scalars"]) == 18


@pytest.mark.parametrize("N,G", [(1, 63), (3, 64), (67, 65), (5, 130), (9, 300)])  # one wave; a full word; past it and more than
def test_shapes_of_the_walker_and_the_transpose_tile(N, G):                          # two tiles; three words; the 8-word form
    from abdpymc_amd.sampler import sample

    m = _dense_model(N, G, 2, seed=3)
    assert m.ctx.is_dense
    res = sample(m, tune=2, draws=8, chains=2, seed=5, diagnostics=True, diag_batch=2)
    m.close()
    assert res["diag_info"].tolist() == [[4, 4, 4, 2]] * 2
    check_against_draws(res, 2)


def test_thin_same_seed_and_plain_run(golden_dir):
    base = run(golden_dir, "dense", 2, diagnostics=True, diag_batch=BATCH)
    thinned = run(golden_dir, "dense", 2, diagnostics=True, diag_batch=BATCH, thin=3)
    assert thinned["i"].shape[1] == 7
    _same_diag(thinned, base)
    from abdpymc_amd.sampler import sample

    m = _model("dense", golden_dir, 2)
    again = sample(m, tune=TUNE, draws=DRAWS, chains=2, seed=7, diagnostics=True, diag_batch=BATCH)
    plain = sample(m, tune=TUNE, draws=DRAWS, chains=2, seed=7)
    m.close()
    _same_diag(again, base)
    assert not any(k.startswith("diag_") for k in plain)
    _same_trajectories(base, plain, keys=("i_raw", "ab_s_waner", "i", "ab_s_mu", "ab_n_mu"))
    # the default batch length: floor(sqrt(H))
    assert dg.default_batch(DRAWS) == 3


@pytest.mark.parametrize("which", ["dense", "test"])
def test_launch_configuration_changes_nothing(golden_dir, which):
    base = run(golden_dir, which, 2, diagnostics=True, diag_batch=BATCH)
    other = run(golden_dir, which, 2, diagnostics=True, diag_batch=BATCH, launch_config=(3, 1))
    _same_diag(other, base)


def _sampler(m, chains, tune, **kw):
    pt = m.initial_point()
    q0 = np.tile(m.ravel(pt), (chains, 1))
    for c in range(chains):
        m.ctx.set_discrete(c, pt["i_raw"].astype(np.int8), pt["ab_s_waner"].astype(np.int8))
    return m.ctx.sampler(list(range(chains)), q0, tune=tune, seed=1, **kw)


@pytest.mark.parametrize("which", ["dense", "test"])
def test_cutting_the_run_into_calls_changes_nothing(golden_dir, which):
    """tune 5, 22 draws, L = 3 (H = 11): the cut after iteration 9 falls behind draw 3, inside the batch of draws 3 .. 5, and the
    half boundary (draw 11 = iteration 16) inside the second call"""
    m = _model(which, golden_dir, 2)
    whole = _sampler(m, 2, 5, diagnostics=(22, 3))
    whole.run(27)
    a = [whole.diagnostics(k) for k in range(2)]
    whole.close()
    cut = _sampler(m, 2, 5, diagnostics=(22, 3))
    cut.run(9)
    assert cut.diagnostics(0)["info"].tolist() == [4, 0, 1, 3]  # readable between the calls
    cut.run(18)
    b = [cut.diagnostics(k) for k in range(2)]
    cut.close()
    m.close()
    for x, y in zip(a, b):
        assert x["info"].tolist() == [11, 11, 6, 3]
        for k in x:
            assert x[k].tobytes() == y[k].tobytes(), k
        assert x["i_counts"][:2].sum() > 0


def test_errors(golden_dir):
    m = _dense_model(100, 70, 2)
    smp = _sampler(m, 2, TUNE, diagnostics=(9, 2))
    smp.run(TUNE + 4)
    before = [smp.diagnostics(k) for k in range(2)]
    assert before[0]["info"].tolist() == [4, 0, 2, 2]
    with pytest.raises(AbdError, match="planned"):
        smp.run(6)  # draws 4 .. 9 pass the planned 9: refused before anything is launched
    for k in range(2):
        now = smp.diagnostics(k)
        for key in now:
            assert now[key].tobytes() == before[k][key].tobytes(), key
    smp.run(5)  # ... and the run goes on to its planned end
    assert smp.diagnostics(1)["info"].tolist() == [4, 4, 4, 2]
    # enabling after the first run is a state error
    assert smp._lib.abd_sampler_enable_diagnostics(smp._h, 20, 2) == -3
    smp.close()
    # without the option there is nothing to read
    smp = _sampler(m, 2, 0)
    with pytest.raises(AbdError, match="not enabled"):
        smp.diagnostics(0)
    # argument errors; 0 releases
    assert smp._lib.abd_sampler_enable_diagnostics(smp._h, 1, 1) == -1
    assert smp._lib.abd_sampler_enable_diagnostics(smp._h, 8, 0) == -1
    assert smp._lib.abd_sampler_enable_diagnostics(smp._h, -1, 1) == -1
    assert smp._lib.abd_sampler_enable_diagnostics(smp._h, 8, 2) == 0
    assert smp.diagnostics(0)["info"].tolist() == [0, 0, 0, 2] and not smp.diagnostics(0)["ab_n_mu"].any()
    assert smp._lib.abd_sampler_enable_diagnostics(smp._h, 0, 0) == 0
    with pytest.raises(AbdError, match="not enabled"):
        smp.diagnostics(0)
    smp.close()
    with pytest.raises(ValueError):
        _sampler(m, 2, 0, diagnostics=(-1, 1))
    from abdpymc_amd.sampler import sample

    with pytest.raises(ValueError, match="native"):
        sample(m, tune=1, draws=4, chains=1, native=False, diagnostics=True)
    with pytest.raises(ValueError, match="draws >= 2"):
        sample(m, tune=1, draws=1, chains=1, diagnostics=True)
    with pytest.raises(ValueError, match="budget"):
        sample(m, tune=1, draws=4, chains=2, diagnostics=True, record_deterministics=False, record_discrete=False,
               budget_bytes=dg.result_bytes(2, 70, 100) - 1)
    m.close()


@pytest.mark.parametrize("kind", ["dense", "test"])
def test_teardown_with_the_buffers_live(golden_dir, kind):
    """create / enable / destroy without running; destroy with the buffers live after a run; the context closed first; enabled,
    dropped and enabled again"""
    from abdpymc_amd._native import _check

    m = _model(kind, golden_dir, 2)
    for _ in range(3):
        smp = _sampler(m, 2, 2, diagnostics=(6, 1))
        smp.close()
    smp = _sampler(m, 2, 2)
    for planned in (6, 0, 6):
        _check(smp._lib, smp._lib.abd_sampler_enable_diagnostics(smp._h, planned, 1))
    smp.run(8)
    first = smp.diagnostics(1)
    smp.close()
    smp.close()
    smp = _sampler(m, 2, 2, diagnostics=(6, 1))
    smp.run(8)
    again = smp.diagnostics(1)
    for k in first:
        assert first[k].tobytes() == again[k].tobytes(), k
    m.ctx.close()  # the context while its sampler holds the buffers: Context.close closes the sampler first
    assert not smp._h.value
    smp.close()
    m.close()


def test_cli_writes_the_diagnostics(tmp_path, golden_dir, capsys):
    from abdpymc_amd import cli

    out = tmp_path / "post.npz"
    d = os.path.join(golden_dir, "test_cohort")
    rc = cli.main(["--tune", "6", "--draws", "8", "--cores", "1", "--ititers_data", d, "--diagnostics", "--diag_batch", "2", "--thin", "2",
                   "--netcdf", str(out)])
    assert rc == 0
    line = [ln for ln in capsys.readouterr().err.splitlines() if ln.startswith("diagnostics:")]
    assert len(line) == 1 and "max R-hat" in line[0] and "min ESS" in line[0] and "worst scalar" in line[0]
    for var in ("i ", "ab_n_mu ", "ab_s_mu "):
        assert var + "max R-hat" in line[0]
    z = np.load(out)
    td = TiterData.from_disk(d)
    G, N = td.n_gaps, td.n_inds
    assert z["diag_i_counts"].shape == (2, 4, G, N) and z["diag_ab_n_mu"].shape == (2, 6, G, N) and z["diag_ab_s_mu"].shape == (2, 6, G, N)
    assert z["diag_info"].tolist() == [[4, 4, 4, 2]] * 2
    assert z["i"].shape[1] == 4  # (the record is thinned, the accumulators are not)
    res = {k: z[k] for k in z.files if not k.startswith("diag_summary_")}
    arrays = dg.summary_arrays(dg.summary(res, td.last_gap))
    assert arrays.keys() == {k for k in z.files if k.startswith("diag_summary_")}
    for k, v in arrays.items():
        np.testing.assert_array_equal(z[k], v, err_msg=k)
