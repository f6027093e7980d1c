"""
Per-draw fits of the survival models by group and by period on the device (abd_survival_draws_create_groups / _periods;
abdpymc_amd.survival.model_alone_groups_draws / model_alone_periods_draws): the two ensemble kernels are bit for bit the
plug-in kernel of their form on every dataset, a point's bits do not depend on the launch, the batched driver is ``_chain`` per
dataset, and both fits end to end on the golden cohort.

No tolerance appears here: every parity check is bit equality against the plug-in kernels, which tests/test_gpu_survival_groups*.py
and tests/test_gpu_survival_periods*.py tie to the 40-digit fixtures.
"""
import os

import numpy as np
import pytest

from abdpymc_amd import _native, survival
from abdpymc_amd.data import TiterData
from tests import survival_groups_restatement as RG
from tests import survival_periods_restatement as RPD

pytestmark = pytest.mark.gpu


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _points(T, n_labels):
    """RG.POINTS with two seeds: 18 points, so that a call is one launch of 16 and one of 2"""
    return np.stack([RG.make_point(name, T, n_labels, seed=s) for s in (0, 1) for name in RG.POINTS])


def _dataset_vector(n, M):
    return ((np.arange(n) * 5 + 2) % M).astype(np.int32)  # M = 3: 2, 1, 0, 2, ...: not monotone, every dataset more than once


def _slots(group, Gr):
    """(column of every individual, tile count) of the grouped layout: sorted by group (stable), every group padded to whole tiles"""
    tiles = (np.bincount(group, minlength=Gr) + 63) // 64
    nxt = np.concatenate([[0], np.cumsum(tiles)[:-1]]) * 64
    slot = np.empty(len(group), dtype=np.int64)
    for j, g in enumerate(group):
        slot[j] = nxt[g]
        nxt[g] += 1
    return slot, int(tiles.sum())


def _datasets(M, N, T, slot, never=(), seed=0):
    """M event-time datasets as tests/survival_draws_cases.datasets makes them -- never at risk, event at 0, event at T - 1,
    followed throughout, random ones, NaN / inf titers behind n_risk -- and, for N >= 130, one whole tile of the device layout
    (``slot``: the column of every individual) whose individuals are never at risk, so that a wave skips its entire range: of the
    tiles that hold none of the four patterned individuals, the one with the most individuals.  ``never``: individuals that are
    never at risk besides."""
    rng = np.random.default_rng([seed, M, N, T])
    n_risk = rng.integers(0, T + 1, size=(M, N)).astype(np.int32)
    has = rng.random((M, N)) < 0.4
    n = min(N, 4)
    n_risk[:, :n] = np.array([T, 1, 0, T])[None, :n]  # event at T - 1, event at 0, never at risk, followed without an event
    has[:, :n] = np.array([True, True, False, False])[None, :n]
    tile = np.asarray(slot) // 64
    skipped = None
    if N >= 130:
        free = [t for t in np.unique(tile) if not (tile[:n] == t).any()]
        skipped = max(free, key=lambda t: ((tile == t).sum(), -t))
        n_risk[:, tile == skipped] = 0
    n_risk[:, np.asarray(never, dtype=np.int64)] = 0
    event = np.where(has & (n_risk > 0), n_risk - 1, -1).astype(np.int32)
    xs, xn = rng.uniform(-1.0, 6.0, (M, T, N)), rng.uniform(-1.0, 6.0, (M, T, N))
    off = np.arange(T)[None, :, None] >= n_risk[:, None, :]
    xs[off & (rng.random((M, T, N)) < 0.5)] = np.nan  # a titer of a cell not at risk may be anything: it reaches no sum
    xs[off & (rng.random((M, T, N)) < 0.2)] = np.inf
    d = survival.SurvivalDraws(n_risk, event, xs, xn, np.stack([np.zeros(M, np.int64), np.arange(M)], axis=1))
    if N >= 130:
        assert (d.n_risk[:, tile == skipped] == 0).all() and (tile == skipped).any()
    assert N < 4 or ((d.n_risk == 0).any() and (d.event == 0).any() and (d.event == T - 1).any() and ((d.n_risk == T) & (d.event == -1)).any())
    return d


class _Groups:
    """the grouped form of one case: labels, datasets, the ensemble handle and the plug-in handle of a dataset"""

    def __init__(self, N, T, Gr, M):
        self.T, self.n_labels, self.M = T, Gr, M
        self.group = RG.make_groups(N, T, Gr).astype(np.int32)
        slot, self.ntile = _slots(self.group, Gr)
        never = np.flatnonzero(self.group == 3) if (N, Gr) == (130, 4) else ()  # a group without follow-up, as RG.make_case has it
        self.d = _datasets(M, N, T, slot, never)
        self.dim = T + Gr + 5
        self.n_sums = T + 2 + Gr

    def ensemble(self):
        return _native.SurvivalDrawsGroups(self.d.n_risk, self.d.event, self.d.s_titer, self.group, self.n_labels, RG.PRIORS)

    def plug_in(self, m):
        y, e, xs, _ = self.d.arrays(m)
        return _native.SurvivalGroups(y, e, xs, self.group, self.n_labels, RG.PRIORS)


class _Periods:
    def __init__(self, N, T, P, M):
        self.T, self.n_labels, self.M = T, P, M
        self.period = RPD.make_periods(N, T, P).astype(np.int32)
        self.ntile = (N + 63) // 64
        self.d = _datasets(M, N, T, np.arange(N))
        self.dim = T + P + 5
        self.n_sums = 2 * T + 2

    def ensemble(self):
        return _native.SurvivalDrawsPeriods(self.d.n_risk, self.d.event, self.d.s_titer, self.period, self.n_labels, RPD.PRIORS)

    def plug_in(self, m):
        y, e, xs, _ = self.d.arrays(m)
        return _native.SurvivalPeriods(y, e, xs, self.period, self.n_labels, RPD.PRIORS)


def _assert_bit_equal_on_every_dataset(case):
    T, M = case.T, case.M
    pts = _points(T, case.n_labels)
    ds = _dataset_vector(len(pts), M)
    h = case.ensemble()
    try:
        assert h.dim == case.dim and h.n_sums == case.n_sums
        lp, g = h.logp_dlogp(ds, pts)
        assert np.isfinite(lp).all() and np.isfinite(g).all()
        sums = np.stack([h.loglik_sums(int(m), q) for m, q in zip(ds, pts)])
        assert sums.shape == (len(pts), case.n_sums)
        for m in range(M):
            p = case.plug_in(m)
            try:
                assert p.dim == h.dim
                rows = np.flatnonzero(ds == m)
                lp_m, g_m = p.logp_dlogp(pts[rows])
                np.testing.assert_array_equal(_bits(lp[rows]), _bits(lp_m))
                np.testing.assert_array_equal(_bits(g[rows]), _bits(g_m))
                for r in rows:
                    np.testing.assert_array_equal(_bits(sums[r]), _bits(p.loglik_sums(pts[r])))
            finally:
                p.close()
        if M > 1:  # the datasets differ: the index is read
            other, _ = h.logp_dlogp((ds + 1) % M, pts)
            assert (other != lp).any()
    finally:
        h.close()


# (130, 65, 4, 3): an empty group, a group without follow-up, partial tiles; (200, 2, 70, 2): almost every tile is mostly padding;
# (520, 511, 2, 3): ten tiles, seg_len = 2
@pytest.mark.parametrize("N,T,Gr,M", [(1, 1, 1, 1), (130, 65, 4, 3), (200, 2, 70, 2), (520, 511, 2, 3)])
def test_groups_bit_equal_to_the_plug_in_kernel_on_every_dataset(N, T, Gr, M):
    """logp, gradient and loglik_sums of 18 points, each on its own dataset, equal BITWISE what a handle of
    abd_survival_create_groups made of that dataset's (infected, exposure, titer) and the same labels returns."""
    case = _Groups(N, T, Gr, M)
    if (N, T) == (520, 511):
        assert RPD.plan(case.ntile * 64, T)[1] >= 2  # the padded tile count plans ranges of two intervals
    _assert_bit_equal_on_every_dataset(case)


# (130, 65, 65, 3): monthly, two finalize blocks per plane; (2100, 129, 4, 2): 33 tiles, seg_len = 2; (1000, 199, 5, 2): a period
# without intervals
@pytest.mark.parametrize("N,T,P,M", [(1, 1, 1, 1), (67, 30, 3, 3), (130, 65, 65, 3), (2100, 129, 4, 2), (1000, 199, 5, 2)])
def test_periods_bit_equal_to_the_plug_in_kernel_on_every_dataset(N, T, P, M):
    """The same against a handle of abd_survival_create_periods: S_t, L, W_x and every W0_t."""
    case = _Periods(N, T, P, M)
    if (N, T) == (2100, 129):
        assert RPD.plan(N, T)[1] >= 2
    if (T, P) == (199, 5):
        assert 3 not in case.period
    _assert_bit_equal_on_every_dataset(case)


@pytest.mark.parametrize("form,shape", [(_Groups, (130, 65, 4, 3)), (_Periods, (130, 65, 65, 3))], ids=["groups", "periods"])
def test_bits_do_not_depend_on_the_launch_or_the_row(form, shape):
    case = form(*shape)
    M = case.M
    pts = _points(case.T, case.n_labels)[:16]
    ds = _dataset_vector(16, M)
    h = case.ensemble()
    try:
        lp, g = h.logp_dlogp(ds, pts)
        lp2, g2 = h.logp_dlogp(ds, pts)
        np.testing.assert_array_equal(_bits(lp), _bits(lp2))
        np.testing.assert_array_equal(_bits(g), _bits(g2))
        for row in (0, 5, 15):
            one_lp, one_g = h.logp_dlogp(int(ds[row]), pts[row])  # alone
            assert one_lp == lp[row]
            np.testing.assert_array_equal(one_g, g[row])
            for at in (0, 7, 15):  # as any row of a 16-point launch among other datasets
                m_lp, m_g = h.logp_dlogp(np.roll(ds, at - row), np.roll(pts, at - row, axis=0))
                assert m_lp[at] == lp[row]
                np.testing.assert_array_equal(m_g[at], g[row])
        both_lp, both_g = h.logp_dlogp(np.concatenate([ds, ds[:3]]), np.concatenate([pts, pts[:3]]))  # 19 points: two launches
        np.testing.assert_array_equal(both_lp, np.concatenate([lp, lp[:3]]))
        np.testing.assert_array_equal(both_g, np.concatenate([g, g[:3]]))
        np.testing.assert_array_equal(h.loglik_sums(1, pts[3]), h.loglik_sums(1, pts[3]))
        # a dataset index outside [0, M) is refused, and nothing is evaluated
        for bad in (-1, M):
            with pytest.raises(ValueError, match=rf"point 2: dataset {bad} outside \[0, {M}\)"):
                h.logp_dlogp(np.array([0, 1, bad], dtype=np.int32), pts[:3])
            with pytest.raises(ValueError, match="outside"):
                h.loglik_sums(bad, pts[0])
    finally:
        h.close()


@pytest.mark.parametrize("form", ["groups", "periods"])
def test_driver_on_the_device_is_chain_per_dataset(form):
    M, N, T, tune, draws, seed = 4, 300, 6, 40, 20, 2
    if form == "groups":
        group = np.arange(N) % 3
        d = _datasets(M, N, T, _slots(group, 3)[0])
        model = survival.SurvivalDrawsGroupsModel(d, d.s_titer, "S", np.array(["a", "b", "c"])[group], "arm")
        keys = {"groups": ["a", "b", "c"], "group_name": "arm"}
    else:
        d = _datasets(M, N, T, np.arange(N))
        model = survival.SurvivalDrawsPeriodsModel(d, d.s_titer, "S", [10, 10, 10, 20, 20, 20], "era")
        keys = {"periods": [10, 20], "period_name": "era", "period_index": [0, 0, 0, 1, 1, 1]}
    try:
        assert model.K == 1 and model.n_datasets == M and model.dim == T + (3 if form == "groups" else 2) + 5 == len(model.names)
        calls = []

        def recording(ds, q):
            calls.append(len(ds))
            return model.logp_dlogp(ds, q)

        fit = survival.sample_draws(model, tune=tune, draws=draws, chains_per_dataset=1, seed=seed, evaluator=recording)
        assert int(fit["n_evaluations"]) == sum(calls) and len(calls) < int(fit["n_evaluations"]) / 2
        q0 = survival._initial_point(model)
        np.testing.assert_array_equal(q0, model.initial_point())
        for m in range(M):
            out, stats = survival._chain(lambda q: model.logp_dlogp(m, q), model.dim, tune, draws, np.random.default_rng([seed, m, 0]), 0.8, q0)
            np.testing.assert_array_equal(np.stack([fit[name][m] for name in model.names], axis=-1), out)
            for name, v in stats.items():
                np.testing.assert_array_equal(fit["stat_" + name][m], v, err_msg=name)
        for k, v in keys.items():
            assert np.asarray(fit[k]).tolist() == v, k
        assert fit["a"].shape == (M, draws, len(keys[form])) and fit["b"].shape == (M, draws)
    finally:
        model.close()


def test_per_draw_fits_by_era_and_by_group_of_the_golden_cohort_end_to_end(golden_dir):
    from abdpymc_amd.model import model
    from abdpymc_amd.sampler import sample

    data = TiterData.from_disk(os.path.join(golden_dir, "test_cohort"))
    m = model(data, n_chains=2)
    res = sample(m, tune=20, draws=20, chains=2, seed=1, record_deterministics=True, record_discrete=False)
    m.close()
    sa = survival.SurvivalAnalysis(res, 0, data.n_gaps, data)
    d = sa.draws(n_datasets=4)
    T = sa.n_int
    eras = sa.periods_from_splits(data.calculate_splits(delta=True, omicron=True))
    halves = np.where(np.arange(data.n_inds) % 2 == 0, "even", "odd")
    made = {"era": (lambda: sa.model_alone_periods_draws("S", d, eras, "era"), [0, 1, 2], "periods"),
            "half": (lambda: sa.model_alone_groups_draws("S", halves, d, "half"), ["even", "odd"], "groups")}
    for name, (make, labels, key) in made.items():
        sm = make()
        try:
            assert sm.dim == T + len(labels) + 5 == len(sm.names) and sm.n_datasets == 4 and (sm.start, sm.end) == (0, data.n_gaps)
            fit = survival.sample_draws(sm, tune=60, draws=40, seed=0)
        finally:
            sm.close()
        assert fit["a"].shape == (4, 40, len(labels)) and fit["b"].shape == (4, 40) and fit["lam0"].shape == (4, 40, T)
        assert fit[key].tolist() == labels and fit["dataset"].tolist() == [0, 1, 2, 3] and fit["source"].shape == (4, 2)
        for k, v in fit.items():
            if k not in ("antigens", "groups", "group_name", "periods", "period_name"):
                assert np.isfinite(v).all(), (name, k)
        p = survival.protection(fit, np.linspace(-2.0, 6.0, 9), **({"period": 1} if key == "periods" else {"group": "odd"}))
        for k in ("mean", "median", "lower", "upper"):
            assert ((p[k] >= 0) & (p[k] <= 1)).all(), (name, k)
        assert survival.report_line(fit).startswith(f"survival: a[S, {name} {labels[0]}]")
        summ = survival.draws_summary(fit)
        contrasts = [f"a[S|{v}] - a[S|{labels[0]}]" for v in labels[1:]]
        assert list(summ) == [f"a[S|{v}]" for v in labels] + ["b[S]"] + [f"protection[S|{v}]@{x}" for v in labels for x in (0, 2, 4)] + contrasts
        for qname, row in summ.items():
            assert all(np.isfinite(row[k]) for k in ("median", "lower", "upper", "sd", "W", "B", "frac_between")), qname
            assert 0.0 <= row["frac_between"] <= 1.0 and row["dataset_median"].shape == (4,) and np.isfinite(row["dataset_median"]).all(), qname
            assert row["lower"] <= row["median"] <= row["upper"], qname
            assert ("p_positive" in row) == (qname in contrasts)
        for qname in contrasts:
            assert 0.0 <= summ[qname]["p_positive"] <= 1.0
