"""
The epidemic curves of one draw (abd_curves, abd_set_follow_up) against curves.from_deterministics of the frozen oracle's
Deterministics -- never the device's own.  Every bound below is derived, none is measured:
  counts of infections      exact
  seropositive counts       between the oracle's counts at thr + delta and thr - delta, delta = 1e-9 max(1, max |mu|)
  titer sums, per gap       sum_j (1e-12 |mu_j| + 1e-13)  -- the per-titer gate of the Deterministics tests --
                            + 2 N 2^-52 sum_j |mu_j|      -- N additions on either side
"""
import os
import re

import numpy as np
import pytest

from abdpymc_amd import curves, synthetic
from abdpymc_amd.data import TiterData
from oracle import abd_oracle as O
from tests.helpers import oracle_cohort_from_synth, random_sparse_cohort
from tests.test_data_loader import default_cohort
from tests.test_gpu_pointwise import _cohort_of, _ctx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _slab():
    src = open(os.path.join(ROOT, "abdpymc_amd", "csrc", "abd_curves.hpp")).read()
    return int(re.search(r"#define\s+ABD_CURVES_SLAB\s+(\d+)", src).group(1))


def _dense(G, N):
    return oracle_cohort_from_synth(synthetic.make_cohort(N, G, seed=G + N))


SHAPES = {
    "test": lambda gd: (_cohort_of(TiterData.from_disk(os.path.join(gd, "test_cohort"))), None, False),
    "test_splits": lambda gd: (_cohort_of(TiterData.from_disk(os.path.join(gd, "test_cohort"))), (14, 20), False),
    "test_ignore_pcrpos": lambda gd: (_cohort_of(TiterData.from_disk(os.path.join(gd, "test_cohort"))), None, True),
    "default": lambda gd: (_cohort_of(default_cohort(gd)), None, False),
    "dense_70x100": lambda gd: (_dense(70, 100), None, False),
    "dense_64x130": lambda gd: (_dense(64, 130), None, False),
    "dense_65x130": lambda gd: (_dense(65, 130), None, False),
    "dense_200x50": lambda gd: (_dense(200, 50), None, False),
    "sparse_300": lambda gd: (random_sparse_cohort(60, 300, 900, 700, seed=4), None, False),   # the 8-word form
    "one_individual": lambda gd: (random_sparse_cohort(1, 31, 12, 9, seed=2), None, False),
    "slabs": lambda gd: (random_sparse_cohort(2 * _slab() + 22, 40, 900, 700, seed=6), None, False),  # ragged last slab
}


def _state(coh, seed, density):
    rng = np.random.default_rng(seed)
    i_raw = (rng.random((coh.n_gaps, coh.n_inds)) < density).astype(np.int8)
    w = (rng.random(coh.n_inds) < 0.5).astype(np.int8)
    theta = synthetic.theta_init(coh.n_gaps) + 0.3 * rng.standard_normal(17)
    return theta, i_raw, w


def _random_follow_up(G, N, seed):
    """includes -1 and G - 1 (as far as N allows)"""
    last = np.random.default_rng(seed).integers(-1, G, N)
    last[0] = G - 1
    if N > 1:
        last[-1] = -1
    return last


def check_against(dev, i, mu_s, mu_n, last, thr_s, thr_n):
    """device curves against the curves of reference Deterministics (G, N), by the module's criteria"""
    G, N = i.shape
    ref = curves.from_deterministics(i, mu_s, mu_n, last, thr_s, thr_n)
    np.testing.assert_array_equal(dev["counts"][:2], ref["counts"][:2])
    np.testing.assert_array_equal(dev["n_infections"], ref["n_infections"])
    last = np.full(N, G - 1) if last is None else last
    assert ref["n_infections"].sum() == (last >= 0).sum()
    followed = np.arange(G)[:, None] <= last[None, :]
    for row, mu, thr in ((0, mu_s, thr_s), (1, mu_n, thr_n)):
        delta = 1e-9 * max(1.0, np.abs(mu).max())
        lo = ((mu >= thr + delta) & followed).sum(axis=1)
        hi = ((mu >= thr - delta) & followed).sum(axis=1)
        got = dev["counts"][2 + row]
        assert (lo <= got).all() and (got <= hi).all(), (row, lo, got, hi)
        a = np.where(followed, np.abs(mu), 0.0)
        bound = (1e-12 * a + 1e-13 * followed).sum(axis=1) + 2 * N * 2.0 ** -52 * a.sum(axis=1)
        err = np.abs(dev["titer_sums"][row] - ref["titer_sums"][row])
        assert (err <= bound).all(), (row, err.max(), bound.min())
    return ref


def _same(a, b):
    for k in ("counts", "n_infections", "titer_sums"):
        np.testing.assert_array_equal(a[k], b[k])  # (no NaNs here: equal values are equal bits but for the sign of zero ...)
        assert a[k].tobytes() == b[k].tobytes()    # ... and that too


@pytest.mark.parametrize("shape", list(SHAPES))
def test_curves_against_the_oracle(golden_dir, shape):
    coh, splits, ignore = SHAPES[shape](golden_dir)
    G, N = coh.n_gaps, coh.n_inds
    if shape == "slabs":
        assert N > 2 * _slab() and N % _slab() != 0
    ctx = _ctx(coh, splits, ignore)
    for seed, density in ((1, 2.0 / G), (2, 0.3)):  # few infections; many (the bins up to "7 or more")
        theta, i_raw, w = _state(coh, seed, density)
        ctx.set_discrete(0, i_raw, w)
        i, mu_n, mu_s = O.deterministics(theta, i_raw, w, coh, splits, ignore)
        thr_s, thr_n = float(np.median(mu_s)), float(np.median(mu_n))
        for last in (None, _random_follow_up(G, N, seed)):
            ctx.set_follow_up(last)
            dev = ctx.curves(0, theta, thr_s, thr_n)
            ref = check_against(dev, i, mu_s, mu_n, last, thr_s, thr_n)
            if last is None and density == 0.3:
                # both sides of the thresholds are populated (with few infections more than half of the N titers may tie at
                # the never-infected baseline, which then is the median: every cell is at or above it)
                assert 0 < ref["counts"][2].sum() < G * N and 0 < ref["counts"][3].sum() < G * N
            # thresholds off
            off = ctx.curves(0, theta)
            assert not off["counts"][2:].any()
            np.testing.assert_array_equal(off["counts"][:2], dev["counts"][:2])
            # the same bits again, also under another launch configuration
            _same(ctx.curves(0, theta, thr_s, thr_n), dev)
            ctx.set_launch_config(blocks=3, chains_per_wave=1)
            _same(ctx.curves(0, theta, thr_s, thr_n), dev)
            ctx.set_launch_config(blocks=10 ** 6, chains_per_wave=0)


def test_many_infections_reach_the_last_bin(golden_dir):
    coh = _dense(70, 100)
    theta, i_raw, w = _state(coh, 2, 0.3)
    i, _, _ = O.deterministics(theta, i_raw, w, coh)
    ctx = _ctx(coh)
    ctx.set_discrete(0, i_raw, w)
    got = ctx.curves(0, theta)["n_infections"]
    assert got[7] == (i.sum(axis=0) >= 7).sum() > 0


def test_dense_and_lists_agree_bit_for_bit(monkeypatch):
    coh = _dense(65, 130)
    theta, i_raw, w = _state(coh, 3, 0.05)
    last = _random_follow_up(65, 130, 3)

    def run():
        ctx = _ctx(coh)
        ctx.set_discrete(0, i_raw, w)
        ctx.set_follow_up(last)
        return ctx.is_dense, ctx.curves(0, theta, 2.0, 1.0)

    dense, a = run()
    monkeypatch.setenv("ABD_FORCE_SPARSE", "1")
    lists, b = run()
    assert dense and not lists
    _same(a, b)


def test_follow_up_arguments_and_non_finite_theta():
    import ctypes

    coh = _dense(64, 70)
    theta, i_raw, w = _state(coh, 5, 0.05)
    ctx = _ctx(coh)
    ctx.set_discrete(0, i_raw, w)
    good = np.full(70, 10)
    for bad in (-2, 64):
        lg = good.copy()
        lg[7] = bad
        with pytest.raises(ValueError):
            ctx.set_follow_up(lg)
        lg32 = np.ascontiguousarray(lg, dtype=np.int32)  # ... and the library's own check
        assert ctx._lib.abd_set_follow_up(ctx._h, ctypes.c_void_p(lg32.ctypes.data)) == -1
    with pytest.raises(ValueError):
        ctx.set_follow_up(good[:-1])
    with pytest.raises(ValueError):
        ctx.set_follow_up(good.astype(float))
    # a refused follow-up leaves the one before it in place
    ctx.set_follow_up(good)
    ok = ctx.curves(0, theta, 2.0, 1.0)
    with pytest.raises(ValueError):
        ctx.set_follow_up(np.full(70, 64))
    _same(ctx.curves(0, theta, 2.0, 1.0), ok)
    assert (ok["counts"][:, 11:] == 0).all() and (ok["titer_sums"][:, 11:] == 0).all()
    with pytest.raises(ValueError):
        ctx.curves(1, theta)  # the context has one chain slot
    # non-finite theta: non-finite sums, comparisons false, no error
    nan = ctx.curves(0, np.full(17, np.nan), 2.0, 1.0)
    assert np.isnan(nan["titer_sums"][:, :11]).all() and not nan["counts"][2:].any()
    np.testing.assert_array_equal(nan["counts"][:2], ok["counts"][:2])
    np.testing.assert_array_equal(nan["n_infections"], ok["n_infections"])
