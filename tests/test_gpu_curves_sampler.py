"""
The epidemic curves of every draw inside the native sampler (abd_sampler_enable_curves / abd_sampler_curves; sample(curves=True);
the CLI's --curves): row d of chain c against curves.from_deterministics of the draw the same run recorded, by the criteria of
tests/test_gpu_curves.py with the recorded titers as the reference.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest

from abdpymc_amd import curves, synthetic
from abdpymc_amd._native import AbdError
from abdpymc_amd.data import TiterData
from tests.test_gpu_curves import check_against
from tests.test_gpu_pointwise import _same_trajectories

pytestmark = pytest.mark.gpu
TUNE, DRAWS = 6, 10


def _model(which, golden_dir, n_chains):
    from abdpymc_amd.model import AbdModel, model

    if which == "test":  # observation lists; the follow-up is the data's
        return model(TiterData.from_disk(os.path.join(golden_dir, "test_cohort")), n_chains=n_chains)
    sc = synthetic.make_cohort(100, 70, seed=11)  # dense; no last_gap: everyone to the last gap
    d = SimpleNamespace(n_gaps=sc.n_gaps, n_inds=sc.n_inds, vacs=sc.vacs, pcrpos=sc.pcrpos,
                        coords={"gap": np.arange(sc.n_gaps), "ind": np.arange(sc.n_inds)},
                        s=SimpleNamespace(obs=sc.s_obs), n=SimpleNamespace(obs=sc.n_obs))
    return AbdModel(d, n_chains=n_chains)


@pytest.mark.parametrize("chains", [2, 5])  # units of 1 and of 2 chains
@pytest.mark.parametrize("which", ["dense", "test"])
def test_every_draw_has_its_row(golden_dir, which, chains):
    from abdpymc_amd.sampler import sample

    m = _model(which, golden_dir, chains)
    G, N = m.n_gaps, m.n_inds
    assert m.ctx.is_dense == (which == "dense")
    kw = dict(tune=TUNE, draws=DRAWS, chains=chains, seed=7)
    plain = sample(m, **kw)
    assert not any(k.startswith("curves_") for k in plain)
    thr = (float(np.median(plain["ab_s_mu"])), float(np.median(plain["ab_n_mu"])))
    res = sample(m, curves=True, sero_thresholds=thr, **kw)
    # documented keys and shapes
    for k in curves.RESULT_KEYS:
        want = {"curves_n_infections": (chains, DRAWS, 8), "curves_n_followed": (chains, G)}.get(k, (chains, DRAWS, G))
        assert res[k].shape == want, k
    last = getattr(m.data, "last_gap", None)
    assert (last is not None) == (which == "test")
    np.testing.assert_array_equal(res["curves_n_followed"][0], curves.n_followed(np.full(N, G - 1) if last is None else last, G))
    # nothing the chains draw changes
    _same_trajectories(res, plain, keys=("i_raw", "ab_s_waner", "i", "ab_s_mu", "ab_n_mu"))
    # row d of chain c is the curves of the recorded draw
    for c in range(chains):
        for d in range(DRAWS):
            dev = {"counts": np.stack([res[f"curves_{n}"][c, d] for n in curves.COUNT_NAMES]),
                   "n_infections": res["curves_n_infections"][c, d],
                   "titer_sums": np.stack([res["curves_titer_s"][c, d], res["curves_titer_n"][c, d]])}
            check_against(dev, res["i"][c, d], res["ab_s_mu"][c, d], res["ab_n_mu"][c, d], last, *thr)
    # thinning the record does not thin the curves
    thinned = sample(m, curves=True, sero_thresholds=thr, thin=3, **kw)
    assert thinned["i"].shape[1] == 4
    for k in curves.RESULT_KEYS:
        np.testing.assert_array_equal(thinned[k], res[k])
        assert thinned[k].tobytes() == res[k].tobytes()
    sm = curves.summary(res)
    assert sm["n_draws"] == chains * DRAWS and np.isfinite(sm["attack_rate"]["median"][sm["n_followed"] > 0]).all()
    m.close()


def test_capacity_is_checked_before_anything_runs(golden_dir):
    m = _model("dense", golden_dir, 2)
    pt = m.initial_point()
    q0 = np.tile(m.ravel(pt), (2, 1))
    for c in range(2):
        m.ctx.set_discrete(c, pt["i_raw"].astype(np.int8), pt["ab_s_waner"].astype(np.int8))
    smp = m.ctx.sampler([0, 1], q0, tune=TUNE, seed=1, curves=9)
    smp.run(TUNE)
    assert smp.curves(0)["counts"].shape == (0, 4, m.n_gaps)
    with pytest.raises(AbdError, match="capacity"):
        smp.run(DRAWS)  # 10 draws into 9 rows: refused before anything is launched
    for c in range(2):
        assert smp.curves(c)["counts"].shape[0] == 0
    smp.run(9)
    got = smp.curves(1)
    assert got["counts"].shape == (9, 4, m.n_gaps) and got["n_infections"].shape == (9, 8) and got["titer_sums"].shape == (9, 2, m.n_gaps)
    assert (got["n_infections"].sum(axis=1) == m.n_inds).all()
    with pytest.raises(AbdError):
        smp.run(1)
    # a range beyond the draws is an argument error; enabling after the first run a state error
    assert smp._lib.abd_sampler_curves(smp._h, 0, 5, 5, None, None, None, None) == -1
    assert smp._lib.abd_sampler_enable_curves(smp._h, 20, 0.0, 0.0) != 0
    smp.close()
    # without the option there is nothing to read
    smp = m.ctx.sampler([0, 1], q0, tune=0, seed=1)
    with pytest.raises(AbdError, match="not enabled"):
        smp.curves(0)
    with pytest.raises(ValueError):
        m.ctx.sampler([0, 1], q0, tune=0, seed=1, curves=-1)
    smp.close()
    m.close()


def test_cli_writes_the_curves(tmp_path, golden_dir, capsys):
    from abdpymc_amd import cli

    out = tmp_path / "post.npz"
    d = os.path.join(golden_dir, "test_cohort")
    rc = cli.main(["--tune", "6", "--draws", "5", "--cores", "1", "--ititers_data", d, "--curves", "--sero_threshold_s", "2.0",
                   "--sero_threshold_n", "1.0", "--thin", "2", "--netcdf", str(out)])
    assert rc == 0
    line = [ln for ln in capsys.readouterr().err.splitlines() if ln.startswith("curves:")]
    assert line and "cumulative attack rate" in line[0] and "peak monthly incidence" in line[0]
    z = np.load(out)
    td = TiterData.from_disk(d)
    G = td.n_gaps
    for k in curves.RESULT_KEYS:
        want = {"curves_n_infections": (2, 5, 8), "curves_n_followed": (2, G)}.get(k, (2, 5, G))
        assert z[k].shape == want, k
    assert z["i"].shape[1] == 3  # (the record is thinned, the curves are not)
    np.testing.assert_array_equal(z["curves_n_followed"][0], curves.n_followed(td.last_gap, G))
    assert z["curves_summary_attack_rate"].shape == (3, G)
    sm = curves.summary({k: z[k] for k in curves.RESULT_KEYS})
    np.testing.assert_array_equal(z["curves_summary_attack_rate"][1], sm["attack_rate"]["median"])
