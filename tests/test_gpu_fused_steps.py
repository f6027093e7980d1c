"""
abd_logp_dlogp_many on dense cohorts puts consecutive steps of a call into one launch (abd_fuse_plan.hpp: up to four, at most
16 rows, S from (K, n, pipes) alone).  Every step of such a call against the synchronous evaluation of that step's thetas
(abd_logp_dlogp_batch: another launch shape), at the tolerances the launch shapes are held to among themselves: 1e-12
relative on logp, 1e-9 of the largest gradient entry on dlogp.
"""
import ctypes as C

import numpy as np
import pytest

from abdpymc_amd import synthetic

pytestmark = pytest.mark.gpu

S_MAX = 4  # abd_fuse_plan.hpp: kFuseMaxSteps
LP_RTOL, G_RTOL = 1e-12, 1e-9


def _context(n_inds, n_gaps, n_chains, storage="f64", seed=5):
    from abdpymc_amd._native import Context

    sc = synthetic.make_cohort(n_inds, n_gaps, seed=seed)
    ctx = Context(n_gaps, n_inds, sc.s_obs, sc.n_obs, sc.vacs, sc.pcrpos, n_chains=n_chains, storage=storage)
    assert ctx.is_dense
    for c in range(n_chains):
        ctx.set_discrete(c, *synthetic.make_chain_state(n_inds, n_gaps, c))
    return ctx


def _thetas(n_gaps, K, n):
    return np.stack([np.stack([synthetic.make_thetas(n_gaps, 1, 11 * k + c)[0] for c in range(n)]) for k in range(K)])


def _k_fused(ctx):
    """fused launches on every pipe, a remainder of three steps, and the call's last launch shaped for an empty chip"""
    return 4 * S_MAX * ctx.n_pipes + 3


def _assert_steps_match_batch(ctx, chains, th, lp, g=None, steps=None):
    worst_lp = worst_g = 0.0
    for k in range(th.shape[0]) if steps is None else steps:
        lp_ref, g_ref = ctx.logp_dlogp_batch(chains, th[k])
        worst_lp = max(worst_lp, float((np.abs(lp[k] - lp_ref) / np.abs(lp_ref)).max()))
        if g is not None:
            worst_g = max(worst_g, float((np.abs(g[k] - g_ref).max(axis=1) / np.abs(g_ref).max(axis=1)).max()))
    print(f"n={len(chains)} K={th.shape[0]}: worst logp {worst_lp:.3e} (relative), dlogp {worst_g:.3e} (of the largest entry)")
    assert worst_lp <= LP_RTOL
    assert worst_g <= G_RTOL


@pytest.fixture(scope="module")
def ctx17():
    """1000 x 60 (BASELINE config 2's shape), 17 chain slots: the rows of a range never bind, so a launch of S steps really
    has 1 / S of the ranges per grid row"""
    ctx = _context(1000, 60, 17)
    yield ctx
    ctx.close()


def test_four_chains_fused_with_remainder_and_step_count(ctx17):
    K = _k_fused(ctx17)
    th = _thetas(60, K, 4)
    ctx17.kernel_timing(2)
    ctx17.kernel_time(reset=True)
    lp, g = ctx17.logp_dlogp_many([0, 1, 2, 3], th)
    ms, count = ctx17.kernel_time(reset=True)
    ctx17.kernel_timing(0)
    assert count == K  # window mode counts steps, not launches
    assert ms > 0.0
    _assert_steps_match_batch(ctx17, [0, 1, 2, 3], th, lp, g)
    assert ctx17.wait_fallbacks == 0


# n = 2: two chains and two ranges per workgroup; 1: split panels, four ranges per workgroup; 5: one chain per workgroup,
# three steps at most; 16: a step fills the launch; 17: two launches per step, never fused; 3: twelve grid rows
@pytest.mark.parametrize("n", [2, 1, 5, 16, 17, 3])
def test_other_chain_counts(ctx17, n):
    K = _k_fused(ctx17)
    chains = list(range(n))
    th = _thetas(60, K, n)
    lp, g = ctx17.logp_dlogp_many(chains, th)
    _assert_steps_match_batch(ctx17, chains, th, lp, g)
    assert ctx17.wait_fallbacks == 0


def test_chains_in_another_order_and_a_short_call(ctx17):
    """the launch's rows follow the caller's chain order; a call too short to fuse"""
    chains = [6, 2, 9, 4]
    for K in (_k_fused(ctx17), 5, 1):
        th = _thetas(60, K, 4)
        lp, g = ctx17.logp_dlogp_many(chains, th)
        _assert_steps_match_batch(ctx17, chains, th, lp, g)


def test_identical_calls_identical_bits_and_new_discrete_state_is_seen(ctx17):
    K = _k_fused(ctx17)
    th = _thetas(60, K, 4)
    lp1, g1 = ctx17.logp_dlogp_many([0, 1, 2, 3], th)
    lp2, g2 = ctx17.logp_dlogp_many([0, 1, 2, 3], th)
    np.testing.assert_array_equal(lp1, lp2)
    np.testing.assert_array_equal(g1, g2)
    ctx17.set_discrete(1, *synthetic.make_chain_state(1000, 60, 101))
    try:
        lp3, g3 = ctx17.logp_dlogp_many([0, 1, 2, 3], th)
        np.testing.assert_array_equal(lp3[:, [0, 2, 3]], lp1[:, [0, 2, 3]])
        assert np.all(lp3[:, 1] != lp1[:, 1])
        _assert_steps_match_batch(ctx17, [0, 1, 2, 3], th, lp3, g3)
    finally:
        ctx17.set_discrete(1, *synthetic.make_chain_state(1000, 60, 1))


def test_logp_only(ctx17):
    """grad = NULL through the C ABI: the kernels' logp-only form"""
    K = _k_fused(ctx17)
    chains = np.arange(4, dtype=np.int32)
    th = np.ascontiguousarray(_thetas(60, K, 4))
    lp = np.full((K, 4), np.nan)
    dp = C.POINTER(C.c_double)
    rc = ctx17._lib.abd_logp_dlogp_many(ctx17._h, K, 4, chains.ctypes.data_as(C.POINTER(C.c_int32)), th.ctypes.data_as(dp),
                                        lp.ctypes.data_as(dp), None)
    assert rc == 0
    _assert_steps_match_batch(ctx17, list(chains), th, lp)


def test_f32_storage():
    ctx = _context(1000, 60, 4, storage="f32")
    K = _k_fused(ctx)
    th = _thetas(60, K, 4)
    lp, g = ctx.logp_dlogp_many([0, 1, 2, 3], th)
    _assert_steps_match_batch(ctx, [0, 1, 2, 3], th, lp, g)
    ctx.close()


def test_ring_window_ends_inside_a_group():
    """more steps than result slots; with 5 chains the groups are of three steps and 1024 is no multiple of three"""
    ctx = _context(400, 30, 5, seed=3)
    K = ctx.n_result_slots + 37
    for n in (2, 5):
        chains = list(range(n))
        th = _thetas(30, K, n)
        lp, g = ctx.logp_dlogp_many(chains, th)
        _assert_steps_match_batch(ctx, chains, th, lp, g)
    assert ctx.wait_fallbacks == 0
    ctx.close()


@pytest.mark.parametrize("n_inds,n_gaps", [(64, 2), (65, 3)])
def test_cohorts_of_one_and_two_lane_groups(n_inds, n_gaps):
    """ranges shorter than a column and fewer workgroups than rows to sum: the sums of a launch go out as their own launch"""
    ctx = _context(n_inds, n_gaps, 4, seed=n_inds)
    K = _k_fused(ctx)
    for n in (4, 1):
        chains = list(range(n))
        th = _thetas(n_gaps, K, n)
        lp, g = ctx.logp_dlogp_many(chains, th)
        _assert_steps_match_batch(ctx, chains, th, lp, g)
    assert ctx.wait_fallbacks == 0
    ctx.close()
