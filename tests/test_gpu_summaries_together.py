"""
Every per-draw summary of the native sampler switched on in ONE run -- the curves, the risk tables, the convergence accumulators,
the timelines with their histograms, WAIC and PPC, beside the recorded Deterministics -- against four runs with one summary each:
a summary's arrays do not depend on what else is on, byte for byte, and nothing the chains draw does.  The summaries share the
sampler's per-draw launch sequence and address their chain's part of every buffer by the same accessors (abd_sampler.hpp), which
only a run with several of them on can get wrong.  Conditions only: nothing here is a tolerance.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest

from abdpymc_amd import risk, synthetic
from abdpymc_amd.data import TiterData

pytestmark = pytest.mark.gpu
CHAINS, TUNE, DRAWS = 3, 3, 8  # units of one and of two chains
PREFIXES = {"curves": "curves_", "risk": "risk_", "diagnostics": "diag_", "timelines": "tl_"}


def _model(which, golden_dir):
    from abdpymc_amd.model import AbdModel, model

    if which == "test":  # observation lists; the follow-up is the data's
        return model(TiterData.from_disk(os.path.join(golden_dir, "test_cohort")), n_chains=CHAINS)
    # dense: two slabs of 64 + 3 individuals, a second word of one gap, more than one workgroup of waves; a follow-up with
    # never-followed individuals, ends inside either word and at the last gap
    N, G = 67, 65
    sc = synthetic.make_cohort(N, G, seed=11)
    last = np.full(N, G - 1, dtype=np.int32)
    last[::5] = -1
    last[1::5] = np.arange(len(last[1::5])) * 4 % (G - 1)  # 0, 4, ..., 52
    last[2::5] = 63
    assert {-1, 0, 63, G - 1} <= set(last.tolist()) and last[64:].tolist() == [G - 1, -1, 52]
    d = SimpleNamespace(n_gaps=sc.n_gaps, n_inds=sc.n_inds, vacs=sc.vacs, pcrpos=sc.pcrpos, last_gap=last,
                        coords={"gap": np.arange(sc.n_gaps), "ind": np.arange(sc.n_inds)},
                        s=SimpleNamespace(obs=sc.s_obs), n=SimpleNamespace(obs=sc.n_obs))
    return AbdModel(d, n_chains=CHAINS)


@pytest.mark.parametrize("which", ["dense", "test"])
def test_a_summary_does_not_depend_on_the_others(golden_dir, which):
    from abdpymc_amd.model import THETA_NAMES
    from abdpymc_amd.sampler import sample

    m = _model(which, golden_dir)
    G = m.n_gaps
    assert m.ctx.is_dense == (which == "dense")
    sp = risk.spec(0, G, 0.5 * np.arange(1, 8), 0.25 * np.arange(1, 8), 1)  # seven edges per antigen, the whole window
    options = {"curves": dict(curves=True, sero_thresholds=(1.0, 0.5)), "risk": dict(risk=sp), "diagnostics": dict(diagnostics=True),
               "timelines": dict(timelines=True, timelines_hist=True)}
    kw = dict(tune=TUNE, draws=DRAWS, chains=CHAINS, seed=7)
    joint = sample(m, waic=True, ppc=True, **{k: v for o in options.values() for k, v in o.items()}, **kw)
    recorded = tuple(THETA_NAMES) + ("i", "ab_n_mu", "ab_s_mu")
    assert joint["i"].shape == (CHAINS, DRAWS, G, m.n_inds)
    for name, opt in options.items():
        single = sample(m, **opt, **kw)
        keys = sorted(k for k in joint if k.startswith(PREFIXES[name]))
        assert keys and keys == sorted(k for k in single if k.startswith(PREFIXES[name])), name
        for other, prefix in PREFIXES.items():
            assert other == name or not any(k.startswith(prefix) for k in single), (name, other)
        for k in keys:
            assert joint[k].dtype == single[k].dtype and joint[k].shape == single[k].shape, k
            assert joint[k].tobytes() == single[k].tobytes(), k
        for k in recorded:
            assert joint[k].tobytes() == single[k].tobytes(), (name, k)
    # the tables hold something
    for k in ("curves_infected", "curves_titer_s", "curves_n_infections", "risk_table", "diag_i_counts", "diag_ab_n_mu", "diag_ab_s_mu",
              "tl_inf", "tl_cum", "tl_ninf", "tl_hist_n", "tl_hist_s", "waic_mean", "ppc_mean"):
        assert np.asarray(joint[k]).any(), k
    assert (joint["tl_hist_n"].sum(axis=-1) == DRAWS).all() and (joint["diag_info"][:, :2] == DRAWS // 2).all()
    m.close()
