"""
The infection-risk-by-titer table of every draw inside the native sampler (abd_sampler_enable_risk / abd_sampler_risk;
sample(risk=spec); the CLI's --risk): row d of chain c against risk.from_deterministics of the draw a plain run of the same
seed recorded, exactly, with edges that no recorded titer comes within delta of (tests/test_gpu_risk.py).
"""
import ctypes
import os

import numpy as np
import pytest

from abdpymc_amd import risk
from abdpymc_amd._native import AbdError, _risk_spec
from abdpymc_amd.data import TiterData
from tests.test_gpu_curves_sampler import _model
from tests.test_gpu_pointwise import _same_trajectories
from tests.test_gpu_risk import pick_edges

pytestmark = pytest.mark.gpu
TUNE, DRAWS = 6, 10


@pytest.mark.parametrize("chains", [2, 5])  # units of 1 and of 2 chains
@pytest.mark.parametrize("which", ["dense", "test"])
def test_every_draw_has_its_table(golden_dir, which, chains):
    from abdpymc_amd.sampler import sample

    m = _model(which, golden_dir, chains)
    G, N = m.n_gaps, m.n_inds
    assert m.ctx.is_dense == (which == "dense")
    kw = dict(tune=TUNE, draws=DRAWS, chains=chains, seed=7)
    plain = sample(m, **kw)
    assert not any(k.startswith("risk_") for k in plain)
    # edges from the plain run's recorded titers: no recorded titer of any draw within delta of one (pick_edges asserts it)
    sp = risk.spec(1, G - 1, pick_edges(plain["ab_s_mu"]), pick_edges(plain["ab_n_mu"], 5), 1, n_gaps=G)
    res = sample(m, risk=sp, **kw)
    # documented keys and shapes
    assert res["risk_table"].shape == (chains, DRAWS, 2, 2, G, 8) and res["risk_table"].dtype == np.int64
    assert res["risk_edges_s"].shape == (chains, 7) and res["risk_edges_n"].shape == (chains, 7)
    np.testing.assert_array_equal(res["risk_edges_n"][-1][:5], sp["edges_n"])
    assert np.isnan(res["risk_edges_n"][:, 5:]).all()
    np.testing.assert_array_equal(res["risk_window"], np.tile([1, G - 1, 1], (chains, 1)))
    # nothing the chains draw changes
    _same_trajectories(res, plain, keys=("i_raw", "ab_s_waner", "i", "ab_s_mu", "ab_n_mu"))
    # row d of chain c is the table of the recorded draw, under the follow-up of the model's data
    last = getattr(m.data, "last_gap", None)
    assert (last is not None) == (which == "test")
    ref = risk.from_deterministics(res["i"], res["ab_s_mu"], res["ab_n_mu"], last, sp)
    np.testing.assert_array_equal(res["risk_table"], ref)
    assert ref[:, :, :, 0].any() and (ref[:, :, 0, 1].sum(axis=(-1, -2)) <= N).all()
    # thinning the record does not thin the tables; all infections instead of the first
    sp_all = dict(sp, first_only=0)
    thinned = sample(m, risk=sp_all, thin=3, **kw)
    assert thinned["i"].shape[1] == 4
    np.testing.assert_array_equal(thinned["risk_table"], risk.from_deterministics(res["i"], res["ab_s_mu"], res["ab_n_mu"], last, sp_all))
    again = sample(m, risk=sp, thin=3, **kw)
    for k in risk.RESULT_KEYS:
        np.testing.assert_array_equal(again[k], res[k])
        assert again[k].tobytes() == res[k].tobytes()
    sm = risk.summary(res)
    assert sm["n_draws"] == chains * DRAWS and np.isfinite(sm["s"]["person_gaps"]["median"]).all()
    # beside the curves: both on, both unchanged
    both = sample(m, risk=sp, curves=True, **kw)
    np.testing.assert_array_equal(both["risk_table"], res["risk_table"])
    assert both["curves_infected"].shape == (chains, DRAWS, G)
    with pytest.raises(ValueError, match="budget"):
        sample(m, risk=sp, budget_bytes=chains * DRAWS * 32 * G * 8 - 1, record_deterministics=False, record_discrete=False, **kw)
    with pytest.raises(ValueError, match="native"):
        sample(m, risk=sp, native=False, **kw)
    with pytest.raises(ValueError):
        sample(m, risk=dict(sp, end=G + 1), **kw)
    m.close()


def test_capacity_is_checked_before_anything_runs(golden_dir):
    m = _model("dense", golden_dir, 2)
    G = m.n_gaps
    pt = m.initial_point()
    q0 = np.tile(m.ravel(pt), (2, 1))
    for c in range(2):
        m.ctx.set_discrete(c, pt["i_raw"].astype(np.int8), pt["ab_s_waner"].astype(np.int8))
    sp = risk.spec(0, G, [1.0, 2.0], [0.5], 1)
    smp = m.ctx.sampler([0, 1], q0, tune=TUNE, seed=1, risk=9, risk_spec=sp)
    smp.run(TUNE)
    assert smp.risk(0).shape == (0, 2, 2, G, 8)
    with pytest.raises(AbdError, match="capacity"):
        smp.run(DRAWS)  # 10 draws into 9 rows: refused before anything is launched
    for c in range(2):
        assert smp.risk(c).shape[0] == 0
    smp.run(9)
    got = smp.risk(1)
    assert got.shape == (9, 2, 2, G, 8) and got.dtype == np.int64
    assert (got[:, :, 0, 1:].sum(axis=-1) <= m.n_inds).all() and got[:, 0, 0, 1].sum(axis=-1).tolist() == [m.n_inds] * 9
    with pytest.raises(AbdError):
        smp.run(1)
    # a range beyond the draws is an argument error; enabling after the first run a state error
    assert smp._lib.abd_sampler_risk(smp._h, 0, 5, 5, None, None) == -1
    assert smp._lib.abd_sampler_risk(smp._h, 2, 0, 1, None, None) == -1
    c_sp = _risk_spec(sp)
    assert smp._lib.abd_sampler_enable_risk(smp._h, 20, ctypes.byref(c_sp)) == -3
    smp.close()
    # without the option there is nothing to read; capacity 0 releases the buffers again
    smp = m.ctx.sampler([0, 1], q0, tune=0, seed=1)
    with pytest.raises(AbdError, match="not enabled"):
        smp.risk(0)
    assert smp._lib.abd_sampler_enable_risk(smp._h, 4, ctypes.byref(c_sp)) == 0
    assert smp.risk(0).shape[0] == 0
    assert smp._lib.abd_sampler_enable_risk(smp._h, 0, None) == 0
    with pytest.raises(AbdError, match="not enabled"):
        smp.risk(0)
    # a spec the ABI refuses, a negative capacity
    bad = _risk_spec(dict(sp, end=G + 1))
    assert smp._lib.abd_sampler_enable_risk(smp._h, 4, ctypes.byref(bad)) == -1
    assert smp._lib.abd_sampler_enable_risk(smp._h, 4, None) == -1
    assert smp._lib.abd_sampler_enable_risk(smp._h, -1, ctypes.byref(c_sp)) == -1
    with pytest.raises(ValueError):
        m.ctx.sampler([0, 1], q0, tune=0, seed=1, risk=-1, risk_spec=sp)
    with pytest.raises(ValueError):
        m.ctx.sampler([0, 1], q0, tune=0, seed=1, risk=3)
    smp.close()
    m.close()


def test_cli_writes_the_risk_tables(tmp_path, golden_dir, capsys):
    from abdpymc_amd import cli

    out = tmp_path / "post.npz"
    d = os.path.join(golden_dir, "test_cohort")
    td = TiterData.from_disk(d)
    G = td.n_gaps
    rc = cli.main(["--tune", "6", "--draws", "5", "--cores", "1", "--ititers_data", d, "--risk", "--risk_edges_s", "0.5,1.5,2.5",
                   "--risk_edges_n=0.25,1.0", "--risk_start", "1", "--thin", "2", "--netcdf", str(out)])
    assert rc == 0
    line = [ln for ln in capsys.readouterr().err.splitlines() if ln.startswith("risk:")]
    assert len(line) == 1 and line[0].count("S ") >= 1 and "N " in line[0]
    z = np.load(out)
    want = {"risk_by_bin": (2, 5, 2, 2, 8), "risk_rate_ratio": (2, 5, 2, 8), "risk_table_sum": (2, 2, 2, G, 8),
            "risk_edges_s": (2, 7), "risk_edges_n": (2, 7), "risk_window": (2, 3)}
    want.update({f"risk_summary_{a}_{q}": (4, 8) for a in ("s", "n") for q in risk.QUANTITIES})
    assert {k for k in z.files if k.startswith("risk_")} == set(want)  # (the full per-draw table is not written)
    for k, shape in want.items():
        assert z[k].shape == shape, k
    assert z["i"].shape[1] == 3  # (the record is thinned, the tables are not)
    np.testing.assert_array_equal(z["risk_window"], [[1, G, 1]] * 2)
    np.testing.assert_array_equal(z["risk_edges_s"][0][:3], [0.5, 1.5, 2.5])
    np.testing.assert_array_equal(z["risk_by_bin"].sum(axis=1), z["risk_table_sum"].sum(axis=-2))
    assert not z["risk_by_bin"][:, :, 0, :, 4:].any() and not z["risk_by_bin"][:, :, 1, :, 3:].any()
    np.testing.assert_array_equal(z["risk_summary_s_person_gaps"][1], np.median(z["risk_by_bin"][:, :, 0, 0].reshape(10, 8), axis=0))
    # the flags are checked before anything is built
    with pytest.raises(SystemExit, match="risk"):
        cli.main(["--tune", "1", "--draws", "1", "--ititers_data", d, "--risk", "--risk_edges_s", "2,1"])
    with pytest.raises(SystemExit, match="risk"):
        cli.main(["--tune", "1", "--draws", "1", "--ititers_data", d, "--risk", "--risk_start", str(G - 1)])
