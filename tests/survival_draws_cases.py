"""
The datasets and the host model of the per-draw survival tests (tests/test_survival_draws_cpu.py, tests/test_gpu_survival_draws.py).
TEST INFRASTRUCTURE ONLY: the package never imports it.
"""
import types

import numpy as np

from abdpymc_amd import survival
from tests import survival_restatement as R


def datasets(M, N, T, seed=0):
    """M event-time datasets with every pattern: never at risk, event at 0, event at T - 1, followed throughout, random ones."""
    rng = np.random.default_rng([seed, M, N, T])
    n_risk = rng.integers(0, T + 1, size=(M, N)).astype(np.int32)
    has = rng.random((M, N)) < 0.4
    n = min(N, 4)
    n_risk[:, :n] = np.array([T, 1, 0, T])[None, :n]  # event at T - 1, event at 0, never at risk, followed without an event
    has[:, :n] = np.array([True, True, False, False])[None, :n]
    event = np.where(has & (n_risk > 0), n_risk - 1, -1).astype(np.int32)
    xs, xn = rng.uniform(-1.0, 6.0, (M, T, N)), rng.uniform(-1.0, 6.0, (M, T, N))
    off = np.arange(T)[None, :, None] >= n_risk[:, None, :]
    xs[off & (rng.random((M, T, N)) < 0.5)] = np.nan  # a titer of a cell not at risk may be anything: it reaches no sum
    xn[off & (rng.random((M, T, N)) < 0.5)] = np.inf
    return survival.SurvivalDraws(n_risk, event, xs, xn, np.stack([np.zeros(M, np.int64), np.arange(M)], axis=1))


def host_model(d, K):
    """what sample_draws asks of a model, and a Restatement per dataset behind ``evaluator``"""
    rs = []
    for m in range(d.n_datasets):
        y, e, xs, xn = d.arrays(m)
        rs.append(R.Restatement(y, e, [xs, xn][:K]))
    names = tuple([f"{v}_{ag}" for v in "ab" for ag in "SN"] if K == 2 else ["a", "b"]) + ("_lam0_raw_mu", "_lam0_raw_sd_log__") \
        + tuple(f"__lam0_raw_z_{t}" for t in range(d.n_int))
    model = types.SimpleNamespace(dim=rs[0].dim, K=K, n_datasets=d.n_datasets, names=names, priors=R.PRIORS[K], source=d.source)
    calls = []

    def evaluator(datasets, q):
        calls.append(np.array(datasets))
        out = [rs[int(m)].logp_dlogp(row) for m, row in zip(datasets, q)]
        return np.array([o[0] for o in out]), np.stack([o[1] for o in out])

    return model, rs, evaluator, calls
