"""
The plane form of the dense gap loop (abd_dense.hpp: dense_walk_planes; ABD_DENSE_PLANES, default 1) against the legacy form
(ABD_DENSE_PLANES=0) in two contexts of one process: the same bits from every launch form, for discrete states that put the
first exposure where the bookkeeping can go wrong; both against the oracle at the other tests' 1e-6; and no writer of a slot's
discrete state leaves a stale plane behind.

Shapes: with a grid that is a multiple of the CU count these planes are cut into ranges of one to a few rows, so every gap is
some range's start (the start state is hit at every g0); through logp_dlogp_many with K = 64 the fused launch's ranges run
across the end of one lane group into the next.
"""
import os

import numpy as np
import pytest

from abdpymc_amd import synthetic
from oracle import abd_oracle as O

from tests.helpers import random_sparse_cohort

pytestmark = pytest.mark.gpu

SHAPES = [(1, 2), (65, 33), (130, 65), (200, 257)]
K_MANY = 64


class _env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update({k: str(v) for k, v in self.kv.items()})

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _cohort(n_inds, n_gaps, kind):
    """'full': vaccinations and PCR positives; 'bare': neither (a lane is exposed by the chain's infections alone);
    'distinct': every log dilution another value, so the cohort has no split panels (one-chain launches read the pair panels)"""
    sc = synthetic.make_cohort(n_inds, n_gaps, seed=n_inds + n_gaps)
    if kind == "bare":
        sc.vacs = np.zeros_like(sc.vacs)
        sc.pcrpos = np.zeros_like(sc.pcrpos)
    if kind == "distinct":
        k = np.arange(sc.x_s.size)
        sc.x_s = sc.x_s + 1e-4 * k / k.size
        sc.x_n = sc.x_n + 1e-4 * (k[::-1]) / k.size
    return sc


def _context(sc, n_chains, planes=1, storage="f64"):
    from abdpymc_amd._native import Context

    with _env(ABD_DENSE_PLANES=planes):
        ctx = Context(sc.n_gaps, sc.n_inds, sc.s_obs, sc.n_obs, sc.vacs, sc.pcrpos, n_chains=n_chains, storage=storage)
    assert ctx.is_dense
    return ctx


def _states(n_inds, n_gaps):
    """(name, i_raw (G, N), waner (N,)): all zeros, all ones, one infection at gap 0 / 31 / 32 / G - 1, random"""
    G, N = n_gaps, n_inds
    rng = np.random.default_rng(G * 7 + N)
    w = (rng.random(N) < 0.5).astype(np.int8)
    out = [("zeros", np.zeros((G, N), np.int8), w), ("ones", np.ones((G, N), np.int8), 1 - w)]
    for g in sorted({0, 31, 32, G - 1}):
        if g < G:
            i = np.zeros((G, N), np.int8)
            i[g, :: 2 if N > 1 else 1] = 1  # every other individual: the others are never exposed by an infection
            out.append((f"one@{g}", i, w))
    out.append(("random", *synthetic.make_chain_state(N, G, 3)))
    dense = (rng.random((G, N)) < 0.2).astype(np.int8)
    out.append(("random-dense", dense, w))
    return out


def _thetas(n_gaps, n, salt=0):
    return np.stack([synthetic.make_thetas(n_gaps, 1, 13 * salt + c)[0] for c in range(n)])


def _load(ctx, states):
    for s, (_, i_raw, w) in enumerate(states):
        ctx.set_discrete(s, i_raw, w)


def _all_forms(ctx, n_states, n_gaps):
    """every state through launches of 1, 2, 3 and 4 chains (synchronous), and through the fused launches of a K = 64 call of
    four chains and of one"""
    out = []
    for n in (1, 2, 3, 4):
        for start in range(n_states):
            chains = [(start + k) % n_states for k in range(n)]
            if len(set(chains)) < n:
                continue
            out.append(ctx.logp_dlogp_batch(chains, _thetas(n_gaps, n, salt=start)))
    for n, starts in ((4, range(0, n_states, 3)), (1, (0, n_states - 1))):
        for start in starts:
            chains = [(start + k) % n_states for k in range(n)]
            th = np.stack([_thetas(n_gaps, n, salt=k) for k in range(K_MANY)])
            out.append(ctx.logp_dlogp_many(chains, th))
    assert ctx.wait_fallbacks == 0
    return out


def _assert_same(a, b):
    assert len(a) == len(b)
    for (lp1, g1), (lp0, g0) in zip(a, b):
        assert np.all(np.isfinite(lp1))
        np.testing.assert_array_equal(lp1, lp0)
        np.testing.assert_array_equal(g1, g0)


# ---- 1. plane form == legacy form, bit for bit ----


@pytest.mark.parametrize("n_inds,n_gaps", SHAPES)
@pytest.mark.parametrize("kind,storage", [("full", "f64"), ("bare", "f64"), ("full", "f32"), ("bare", "f32")])
def test_plane_form_equals_legacy_form(n_inds, n_gaps, kind, storage):
    sc = _cohort(n_inds, n_gaps, kind)
    states = _states(n_inds, n_gaps)
    res = []
    for planes in (1, 0):
        ctx = _context(sc, len(states), planes, storage)
        _load(ctx, states)
        res.append(_all_forms(ctx, len(states), n_gaps))
        ctx.close()
    _assert_same(*res)


@pytest.mark.parametrize("storage", ["f64", "f32"])
def test_pair_panels_in_one_chain_launches(storage):
    """a cohort without split panels: launches of one and three chains walk the pair panels one chain per workgroup"""
    n_inds, n_gaps = 130, 65
    sc = _cohort(n_inds, n_gaps, "distinct")
    states = _states(n_inds, n_gaps)
    res = []
    for planes in (1, 0):
        ctx = _context(sc, len(states), planes, storage)
        _load(ctx, states)
        res.append(_all_forms(ctx, len(states), n_gaps))
        ctx.close()
    _assert_same(*res)


@pytest.mark.parametrize("unit", [1, 2, 4])
@pytest.mark.parametrize("kind,storage", [("full", "f64"), ("distinct", "f32")])
def test_sampler_trains_draw_the_same(unit, kind, storage):
    """a short seeded run of the native sampler without the sweep, units of 1, 2 and 4 chains: the train kernels (which keep
    the legacy form, abd_dense.hpp: dense_plane_form) fed by evaluations of either form must draw the same"""
    n_inds, n_gaps = 130, 65
    sc = _cohort(n_inds, n_gaps, kind)
    q0 = np.stack([synthetic.theta_init(n_gaps) + 0.01 * c for c in range(4)])
    draws = []
    for planes in (1, 0):
        ctx = _context(sc, 4, planes, storage)
        for c in range(4):
            ctx.set_discrete(c, *synthetic.make_chain_state(n_inds, n_gaps, c))
        with _env(ABD_SAMPLER_UNIT=unit):
            smp = ctx.sampler([0, 1, 2, 3], q0, tune=6, seed=5, max_treedepth=4, gibbs=False)
        theta, stats = smp.run(8)
        draws.append((theta, stats["lp"], stats["n_steps"]))
        smp.close()
        ctx.close()
    assert np.all(np.isfinite(draws[0][0]))
    assert draws[0][2].sum() > 8 * 4  # (leapfrogs were taken)
    for a, b in zip(*draws):
        np.testing.assert_array_equal(a, b)


# ---- 2. against the oracle ----


@pytest.mark.parametrize("n_inds,n_gaps", SHAPES)
def test_against_the_oracle(n_inds, n_gaps):
    sc = _cohort(n_inds, n_gaps, "full")
    coh = O.Cohort(sc.n_gaps, sc.n_inds, sc.vacs, sc.pcrpos, O.AntigenObs(*sc.s_obs), O.AntigenObs(*sc.n_obs))
    states = [s for s in _states(n_inds, n_gaps) if s[0] in ("zeros", "one@0", "random", "random-dense")]
    ctx = _context(sc, len(states))
    _load(ctx, states)
    th = _thetas(n_gaps, len(states))
    chains = list(range(len(states)))
    lp4, g4 = ctx.logp_dlogp_batch(chains, th)                       # four chains per workgroup
    lp1 = [ctx.logp_dlogp_batch([c], th[c:c + 1]) for c in chains]  # one chain, split panels
    ctx.close()
    for c, (name, i_raw, w) in enumerate(states):
        lp_ref, g_ref = O.logp_dlogp(th[c], i_raw, w, coh, ())
        scale = np.maximum(np.abs(g_ref), 1e-6 * np.abs(g_ref).max())
        for lp, g in ((lp4[c], g4[c]), (lp1[c][0][0], lp1[c][1][0])):
            print(f"{n_inds} x {n_gaps} {name}: logp {abs(lp - lp_ref) / abs(lp_ref):.2e}, dlogp {(np.abs(g - g_ref) / scale).max():.2e}")
            assert abs(lp - lp_ref) <= 1e-6 * abs(lp_ref)
            assert (np.abs(g - g_ref) / scale).max() <= 1e-6


# ---- 3. no writer leaves a stale plane ----


def _fresh_eval(sc, ctx, chain, theta, storage="f64"):
    """the evaluation of a fresh context given the slot's discrete state as read back"""
    i_raw, w = ctx.get_discrete(chain)
    fresh = _context(sc, 1, 1, storage)
    fresh.set_discrete(0, i_raw, w)
    out = fresh.logp_dlogp(0, theta)
    fresh.close()
    return out


def _assert_current(sc, ctx, chain, theta):
    lp, g = ctx.logp_dlogp(chain, theta)
    lp_ref, g_ref = _fresh_eval(sc, ctx, chain, theta)
    assert np.isfinite(lp)
    assert lp == lp_ref
    np.testing.assert_array_equal(g, g_ref)
    return lp


@pytest.mark.parametrize("n_inds,n_gaps", [(130, 65), (200, 257)])
def test_no_writer_leaves_a_stale_plane(n_inds, n_gaps):
    sc = _cohort(n_inds, n_gaps, "full")
    ctx = _context(sc, 2)
    theta = synthetic.theta_init(n_gaps)
    thetas = np.stack([theta, theta])
    for c in range(2):
        ctx.set_discrete(c, *synthetic.make_chain_state(n_inds, n_gaps, c))
    seen = {_assert_current(sc, ctx, 0, theta)}
    # set_discrete over an evaluated slot
    ctx.set_discrete(0, *synthetic.make_chain_state(n_inds, n_gaps, 7))
    seen.add(_assert_current(sc, ctx, 0, theta))
    # flip_discrete: an infection in the last lane group's last individual, one in the first, a waner flip
    for flat in ((n_gaps - 1) * n_inds + n_inds - 1, 0, 33 % n_gaps * n_inds + 64, n_gaps * n_inds + 3):
        ctx.flip_discrete(0, flat)
        seen.add(_assert_current(sc, ctx, 0, theta))
    # one sweep of the dense family (both slots in one launch)
    acc, prop = ctx.gibbs_sweep([0, 1], thetas, seed=11, sweep=0)
    assert acc.sum() > 0
    for c in range(2):
        seen.add(_assert_current(sc, ctx, c, theta))
    # five compound sampler iterations
    smp = ctx.sampler([0, 1], thetas, tune=3, seed=2, max_treedepth=3)
    smp.run(5)
    smp.close()
    for c in range(2):
        seen.add(_assert_current(sc, ctx, c, theta))
    # the slot reused for another chain's state
    i1, w1 = ctx.get_discrete(1)
    ctx.set_discrete(0, i1, w1)
    assert _assert_current(sc, ctx, 0, theta) == ctx.logp_dlogp(1, theta)[0]
    assert len(seen) >= 6  # (the writers did change the state)
    ctx.close()


def test_list_family_sweep_on_an_observation_list_cohort():
    """a cohort kept as observation lists has no planes: its sweep and evaluations are untouched"""
    from abdpymc_amd._native import Context

    coh = random_sparse_cohort(70, 26, 300, 280, seed=4)
    obs = lambda a: (a.idx_gap, a.idx_ind, a.log_dilution, a.od)
    mk = lambda: Context(coh.n_gaps, coh.n_inds, obs(coh.s), obs(coh.n), coh.vacs, coh.pcrpos, n_chains=1)
    ctx = mk()
    assert not ctx.is_dense
    theta = synthetic.theta_init(coh.n_gaps)
    ctx.set_discrete(0, *synthetic.make_chain_state(coh.n_inds, coh.n_gaps, 0))
    lp0, _ = ctx.logp_dlogp(0, theta)
    acc, _ = ctx.gibbs_sweep([0], theta[None], seed=3, sweep=0)
    assert acc.sum() > 0
    lp, g = ctx.logp_dlogp(0, theta)
    fresh = mk()
    fresh.set_discrete(0, *ctx.get_discrete(0))
    lp_ref, g_ref = fresh.logp_dlogp(0, theta)
    assert lp != lp0 and lp == lp_ref
    np.testing.assert_array_equal(g, g_ref)
    fresh.close()
    ctx.close()
