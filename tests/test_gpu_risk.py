"""
The infection-risk-by-titer table of one draw (abd_risk) against risk.from_deterministics of the frozen oracle's Deterministics
-- never the device's own -- over the shape table of tests/test_gpu_curves.py.  The table holds integers only, so every
comparison is exact, under one condition on the test's own inputs: the bin edges are midpoints between neighbouring distinct
oracle titers near the septiles, and no oracle titer lies within delta = 1e-9 max(1, max |mu|) of an edge (the per-titer gate of
the seropositive counts in tests/test_gpu_curves.py), so the device's titer and the oracle's fall on the same side of every edge.
"""
import ctypes

import numpy as np
import pytest

from abdpymc_amd import risk
from abdpymc_amd._native import _RiskSpec, _risk_spec
from oracle import abd_oracle as O
from tests.test_gpu_curves import SHAPES, _dense, _random_follow_up, _state
from tests.test_gpu_pointwise import _ctx

pytestmark = pytest.mark.gpu


def pick_edges(mu, n_edges=7):
    """Up to ``n_edges`` ascending edges for the titers ``mu``: for each septile the midpoint of the nearest pair of neighbouring
    distinct values that lie more than 4 delta apart (searching upwards first, then downwards), every pair used once."""
    vals = np.unique(np.asarray(mu, dtype=np.float64).ravel())
    delta = 1e-9 * max(1.0, np.abs(vals).max())
    wide = np.flatnonzero(np.diff(vals) > 4 * delta)  # pair k is (vals[k], vals[k + 1])
    taken = []
    for q in range(1, n_edges + 1):
        at = np.searchsorted(vals, np.quantile(mu, q / (n_edges + 1)))
        free = np.setdiff1d(wide, taken)
        if not free.size:
            break
        up = free[free >= min(at, vals.size - 2)]
        taken.append(int(up[0] if up.size else free[-1]))
    edges = np.array(sorted(0.5 * (vals[k] + vals[k + 1]) for k in taken))
    assert_clear_of(mu, edges)
    return edges


def assert_clear_of(mu, edges):
    """no titer within delta of an edge: the one condition under which the table is compared exactly"""
    mu = np.asarray(mu, dtype=np.float64)
    delta = 1e-9 * max(1.0, np.abs(mu).max())
    for e in edges:
        assert np.abs(mu - e).min() > delta, (e, np.abs(mu - e).min(), delta)
    assert (np.diff(edges) > 0).all()


def windows_of(G):
    ws = [(0, G), (G // 3, G - 2) if G >= 8 else (0, G - 1)]
    if G > 64:
        ws.append((62, min(67, G)))  # across a word boundary: gaps 63 and 64 are at risk (end <= G cuts it short at 65 gaps)
    return ws


def _same(a, b):
    np.testing.assert_array_equal(a, b)
    assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_risk_against_the_oracle(golden_dir, shape):
    coh, splits, ignore = SHAPES[shape](golden_dir)
    G, N = coh.n_gaps, coh.n_inds
    ctx = _ctx(coh, splits, ignore)
    for seed, density in ((1, 2.0 / G), (2, 0.3)):
        theta, i_raw, w = _state(coh, seed, density)
        ctx.set_discrete(0, i_raw, w)
        i, mu_n, mu_s = O.deterministics(theta, i_raw, w, coh, splits, ignore)
        edges_s, edges_n = pick_edges(mu_s), pick_edges(mu_n)
        for last in (None, _random_follow_up(G, N, seed)):
            ctx.set_follow_up(last)
            lg = np.full(N, G - 1) if last is None else last
            for first_only in (1, 0):
                for start, end in windows_of(G):
                    sp = risk.spec(start, end, edges_s, edges_n, first_only, n_gaps=G)
                    dev = ctx.risk(0, theta, sp)
                    ref = risk.from_deterministics(i, mu_s, mu_n, last, sp)
                    assert dev.dtype == np.int64 and dev.shape == (2, 2, G, 8)
                    np.testing.assert_array_equal(dev, ref)
                    # derived, exact: the antigens differ in the bin only; at most one event per individual
                    np.testing.assert_array_equal(dev[0].sum(axis=-1), dev[1].sum(axis=-1))
                    inside = (np.arange(G)[:, None] > start) & (np.arange(G)[:, None] < end) & (np.arange(G)[:, None] <= lg[None, :])
                    if first_only:
                        assert dev[0, 1].sum() == ((i != 0) & inside).any(axis=0).sum() <= N
                    else:
                        np.testing.assert_array_equal(dev[0, 1].sum(axis=-1), ((i != 0) & inside).sum(axis=1))
                        np.testing.assert_array_equal(dev[0, 0].sum(axis=-1), inside.sum(axis=1))
                    if (start, end) == (0, G):
                        by_bin = ref[0].sum(axis=-2)  # S: (at risk, events) x bin
                        if first_only and density < 0.3 and N > 1 and last is None:
                            # the test bins something (a single individual has one event at most and cannot show this)
                            assert (by_bin[0] > 0).sum() >= 4 and (by_bin[1] > 0).sum() >= 2, by_bin
                        if not first_only and density == 0.3 and N > 1 and last is None:
                            assert (by_bin[1][by_bin[0] > 0] > 0).all(), by_bin
                        if not first_only and last is None:
                            cur = ctx.curves(0, theta)["counts"][0]
                            np.testing.assert_array_equal(dev[0, 1].sum(axis=-1)[1:], cur[1:])
                            assert (dev[0, 0].sum(axis=-1)[1:] == N).all() and not dev[:, :, 0].any()
                        # the same bits again, also under another launch configuration
                        _same(ctx.risk(0, theta, sp), dev)
                        ctx.set_launch_config(blocks=3, chains_per_wave=1)
                        _same(ctx.risk(0, theta, sp), dev)
                        ctx.set_launch_config(blocks=10 ** 6, chains_per_wave=0)


def test_fewer_edges_leave_the_upper_bins_empty():
    coh = _dense(70, 100)
    theta, i_raw, w = _state(coh, 2, 0.3)
    i, mu_n, mu_s = O.deterministics(theta, i_raw, w, coh)
    ctx = _ctx(coh)
    ctx.set_discrete(0, i_raw, w)
    es, en = pick_edges(mu_s, 3), pick_edges(mu_n, 1)
    for sp in (risk.spec(0, 70, es, en, 0), risk.spec(5, 60, (), (), 1)):  # (every cell at risk: the top quarter is populated)
        dev = ctx.risk(0, theta, sp)
        np.testing.assert_array_equal(dev, risk.from_deterministics(i, mu_s, mu_n, None, sp))
        assert not dev[0, :, :, sp["edges_s"].size + 1:].any() and not dev[1, :, :, sp["edges_n"].size + 1:].any()
        assert dev[0, 0, :, sp["edges_s"].size].any() and dev[1, 0, :, sp["edges_n"].size].any()


def test_dense_and_lists_agree_bit_for_bit(monkeypatch):
    coh = _dense(65, 130)
    theta, i_raw, w = _state(coh, 3, 0.05)
    last = _random_follow_up(65, 130, 3)
    sp = risk.spec(1, 65, [1.0, 2.0, 3.0], [0.5, 1.0], 1)

    def run():
        ctx = _ctx(coh)
        ctx.set_discrete(0, i_raw, w)
        ctx.set_follow_up(last)
        return ctx.is_dense, ctx.risk(0, theta, sp)

    dense, a = run()
    monkeypatch.setenv("ABD_FORCE_SPARSE", "1")
    lists, b = run()
    assert dense and not lists and a[:, 1].any()
    _same(a, b)


def test_refusals_and_non_finite_theta():
    coh = _dense(64, 70)
    theta, i_raw, w = _state(coh, 5, 0.05)
    ctx = _ctx(coh)
    ctx.set_discrete(0, i_raw, w)
    ctx.set_follow_up(_random_follow_up(64, 70, 5))
    good = dict(start=0, end=64, first_only=1, edges_s=[1.0, 2.0], edges_n=[0.5])
    ok = ctx.risk(0, theta, good)
    assert ok[:, 1].any()
    table = np.empty((2, 2, 64, 8), np.int64)
    t = np.ascontiguousarray(theta, dtype=np.float64)

    def raw(sp, th=t, out=table, chain=0):
        return ctx._lib.abd_risk(ctx._h, chain, th.ctypes.data if th is not None else None,
                                 ctypes.byref(sp) if sp is not None else None, out.ctypes.data if out is not None else None)

    assert raw(_risk_spec(good)) == 0
    for change in (dict(start=-1), dict(end=65), dict(start=63), dict(start=10, end=11), dict(first_only=2), dict(first_only=-1),
                   dict(edges_s=[1.0, 1.0]), dict(edges_n=[2.0, 1.0]), dict(edges_s=[np.nan]), dict(edges_n=[np.inf]),
                   dict(edges_s=[1.0, 2.0, -np.inf])):
        bad = dict(good, **change)
        with pytest.raises(ValueError):
            ctx.risk(0, theta, bad)
        assert raw(_risk_spec(bad)) == -1, change
    for field, value in (("n_edges_s", 8), ("n_edges_s", -1), ("n_edges_n", 8), ("n_edges_n", -1)):
        sp = _risk_spec(good)
        setattr(sp, field, value)
        assert raw(sp) == -1, field
    assert isinstance(_risk_spec(good), _RiskSpec)
    with pytest.raises(ValueError):
        ctx.risk(0, theta, dict(good, edges_s=np.arange(8.0)))  # (does not fit the ABI's struct)
    assert raw(None) == -1 and raw(_risk_spec(good), th=None) == -1 and raw(_risk_spec(good), out=None) == -1
    assert raw(_risk_spec(good), chain=1) == -1  # the context has one chain slot
    with pytest.raises(ValueError):
        ctx.risk(0, theta[:-1], good)
    # the extreme windows are fine
    assert ctx.risk(0, theta, dict(good, start=62, end=64))[:, 0, 63].any()
    # a refused call leaves nothing behind: the same bits as before
    _same(ctx.risk(0, theta, good), ok)
    # non-finite theta: every comparison fails, everything lands in bin 0; the totals do not change; no error
    nan = ctx.risk(0, np.full(17, np.nan), good)
    assert not nan[..., 1:].any()
    np.testing.assert_array_equal(nan[..., 0], ok.sum(axis=-1))
