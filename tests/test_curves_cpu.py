"""
Epidemic curves without a GPU (abdpymc_amd.curves): the definition on a hand-written example, the summary's quantiles, the
merges, TiterData.last_gap against the table, and the C ABI's declarations.
"""
import os

import numpy as np
import pytest

from abdpymc_amd import curves
from abdpymc_amd.data import TiterData
from tests.test_abi_symbols import header_functions


def test_from_deterministics_by_hand():
    # gaps x individuals; individual 0 is infected twice, 1 is never followed, 2 and 3 leave early (3 before its second infection)
    i = np.array([[1, 0, 0, 1, 0],
                  [0, 0, 1, 1, 0],
                  [1, 0, 0, 0, 1]], dtype=np.int8)
    last = np.array([2, -1, 1, 0, 2])
    mu_s = np.arange(15, dtype=float).reshape(3, 5)
    mu_n = mu_s / 2
    r = curves.from_deterministics(i, mu_s, mu_n, last, thr_s=6.0, thr_n=1.0)
    np.testing.assert_array_equal(curves.n_followed(last, 3), [4, 3, 2])
    np.testing.assert_array_equal(r["counts"], [[2, 1, 2],    # infected
                                                [2, 2, 2],    # ever infected
                                                [0, 2, 2],    # S titer >= 6 among the followed
                                                [3, 3, 2]])   # N titer >= 1
    np.testing.assert_array_equal(r["n_infections"], [0, 3, 1, 0, 0, 0, 0, 0])
    np.testing.assert_array_equal(r["titer_sums"], [[9.0, 21.0, 24.0], [4.5, 10.5, 12.0]])
    assert r["counts"].dtype == np.int64 and r["n_infections"].dtype == np.int64
    # defaults: everyone to the last gap, thresholds off
    d = curves.from_deterministics(i, mu_s, mu_n)
    np.testing.assert_array_equal(d["counts"], [[2, 2, 2], [2, 3, 4], [0, 0, 0], [0, 0, 0]])
    np.testing.assert_array_equal(d["n_infections"], [1, 2, 2, 0, 0, 0, 0, 0])
    np.testing.assert_array_equal(d["titer_sums"][0], mu_s.sum(axis=1))
    # leading axes are kept
    b = curves.from_deterministics(np.stack([i, i]), np.stack([mu_s, mu_s]), np.stack([mu_n, mu_n]), last, 6.0, 1.0)
    assert b["counts"].shape == (2, 4, 3) and b["n_infections"].shape == (2, 8) and b["titer_sums"].shape == (2, 2, 3)
    np.testing.assert_array_equal(b["counts"][1], r["counts"])
    for bad in ([2, -2, 1, 0, 2], [2, 3, 1, 0, 2]):
        with pytest.raises(ValueError):
            curves.from_deterministics(i, mu_s, mu_n, np.array(bad))


def test_seven_or_more_bin():
    G = 12
    i = np.zeros((G, 4), dtype=np.int8)
    i[:6, 0] = 1      # 6
    i[:7, 1] = 1      # 7
    i[:, 2] = 1       # 12 ...
    i[:, 3] = 1       # ... of which 3 while followed
    z = np.zeros((G, 4))
    r = curves.from_deterministics(i, z, z, np.array([G - 1, G - 1, G - 1, 2]))
    np.testing.assert_array_equal(r["n_infections"], [0, 0, 0, 1, 0, 0, 1, 2])


def _result(rng, chains, draws, G, N):
    i = (rng.random((chains, draws, G, N)) < 0.1).astype(np.int8)
    mu_s, mu_n = rng.normal(3, 1, i.shape), rng.normal(1, 1, i.shape)
    last = rng.integers(-1, G, N)
    r = curves.from_deterministics(i, mu_s, mu_n, last, 3.0, 1.0)
    return (i, mu_s, mu_n, last), curves.as_result(r["counts"], r["n_infections"], r["titer_sums"], curves.n_followed(last, G))


def test_summary_quantiles():
    rng = np.random.default_rng(0)
    G = 6
    inf = rng.integers(0, 50, (3, 40, G))
    nf = np.array([50, 50, 40, 40, 10, 0])
    res = {k: np.zeros((3, 40, G)) for k in curves.RESULT_KEYS}
    res["curves_infected"] = inf
    res["curves_ever_infected"] = np.cumsum(inf, axis=-1)
    res["curves_titer_s"] = rng.normal(100, 10, (3, 40, G))
    res["curves_n_infections"] = np.tile(np.array([5, 3, 2, 0, 0, 0, 0, 0]), (3, 40, 1))
    res["curves_n_followed"] = np.tile(nf, (3, 1))
    sm = curves.summary(res, prob=0.9)
    pooled = inf.reshape(-1, G)[:, :5] / nf[:5]
    # (the levels (1 -+ prob) / 2 are a rounding away from 0.05 / 0.95: the quantiles agree to rounding, not bit for bit)
    close = lambda a, b: np.testing.assert_allclose(a, b, rtol=1e-12, atol=0)  # noqa: E731
    close(sm["incidence"]["median"][:5], np.quantile(pooled, 0.5, axis=0))
    close(sm["incidence"]["lower"][:5], np.quantile(pooled, 0.05, axis=0))
    close(sm["incidence"]["upper"][:5], np.quantile(pooled, 0.95, axis=0))
    ts = res["curves_titer_s"].reshape(-1, G)[:, :5] / nf[:5]
    close(sm["mean_titer_s"]["upper"][:5], np.quantile(ts, 0.95, axis=0))
    ar = res["curves_ever_infected"].reshape(-1, G)[:, :5] / nf[:5]
    close(sm["attack_rate"]["median"][:5], np.quantile(ar, 0.5, axis=0))
    close(sm["first_incidence"]["median"][:5], np.quantile(np.diff(ar, axis=1, prepend=0.0), 0.5, axis=0))
    for k in ("incidence", "attack_rate", "seroprev_s", "mean_titer_n"):  # nobody is followed at the last gap
        assert all(np.isnan(sm[k][q][5]) for q in ("lower", "median", "upper"))
    np.testing.assert_allclose(sm["n_infections"], [0.5, 0.3, 0.2, 0, 0, 0, 0, 0], rtol=1e-13)  # (a mean of 120 equal shares)
    assert sm["n_draws"] == 120 and sm["prob"] == 0.9
    np.testing.assert_array_equal(sm["n_followed"], nf)
    with pytest.raises(ValueError):
        curves.summary({"curves_infected": inf})
    flat = curves.summary_arrays(sm)
    assert flat["curves_summary_incidence"].shape == (3, G) and flat["curves_summary_n_infections"].shape == (8,)


def test_merges():
    rng = np.random.default_rng(1)
    G, N = 9, 37
    (i, mu_s, mu_n, last), whole = _result(rng, 2, 5, G, N)
    cut = 15
    parts = []
    for sl in (slice(0, cut), slice(cut, N)):
        r = curves.from_deterministics(i[..., sl], mu_s[..., sl], mu_n[..., sl], last[sl], 3.0, 1.0)
        parts.append(curves.as_result(r["counts"], r["n_infections"], r["titer_sums"], curves.n_followed(last[sl], G)))
    merged = curves.merge_individual_shards(parts)
    for k in curves.RESULT_KEYS:
        if "titer" not in k:
            np.testing.assert_array_equal(merged[k], whole[k])
    followed = np.arange(G)[:, None] <= last[None, :]
    for k, mu in (("curves_titer_s", mu_s), ("curves_titer_n", mu_n)):
        bound = N * 2.0 ** -52 * np.where(followed, np.abs(mu), 0.0).sum(axis=-1)
        assert (np.abs(merged[k] - whole[k]) <= bound).all()
    both = curves.merge_chains([whole, whole])
    assert both["curves_infected"].shape == (4, 5, G) and both["curves_n_followed"].shape == (4, G)
    np.testing.assert_array_equal(both["curves_n_infections"][2:], whole["curves_n_infections"])
    # pooled twice: the same quantiles
    np.testing.assert_array_equal(curves.summary(both)["attack_rate"]["median"], curves.summary(whole)["attack_rate"]["median"])


def test_last_gap_of_the_golden_cohort(golden_dir):
    import pandas as pd

    d = os.path.join(golden_dir, "test_cohort")
    td = TiterData.from_disk(d)
    df = pd.read_csv(os.path.join(d, "df.csv"), index_col=0)
    df = df[df["measurement"].isin(["10222020-S", "40588-V08B"])]
    want = np.full(td.n_inds, -1, dtype=np.int64)
    for j, g in df.groupby("individual_i")["elapsed_months"].max().items():
        want[int(j)] = int(g)
    np.testing.assert_array_equal(td.last_gap, want)
    assert td.last_gap.shape == (td.n_inds,) and td.last_gap.max() == td.n_gaps - 1
    np.testing.assert_array_equal(curves.n_followed(td.last_gap, td.n_gaps)[0], (want >= 0).sum())
    # an individual without readings is never followed
    td2 = TiterData.from_arrays(4, 3, ([1, 3], [0, 2], [0.0, 0.0], [1.0, 1.0]), ([2], [0], [0.0], [1.0]), np.zeros((3, 4)),
                                np.zeros((3, 4)))
    np.testing.assert_array_equal(td2.last_gap, [2, -1, 3])


def test_header_declares_the_curves():
    names = header_functions()
    for name in ("abd_set_follow_up", "abd_curves", "abd_sampler_enable_curves", "abd_sampler_curves"):
        assert name in names


def test_sampler_without_the_native_path_refuses_curves():
    from types import SimpleNamespace

    from abdpymc_amd.sampler import sample

    m = SimpleNamespace(n_chains=1, ctx=SimpleNamespace())
    with pytest.raises(ValueError, match="curves"):
        sample(m, tune=1, draws=1, native=False, curves=True)
