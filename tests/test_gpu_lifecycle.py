"""
Life cycle of what the library owns on the device (abd_owned.hpp: every buffer, pinned block, stream and event is a member
handle of the context, its slots and pipes, the sampler and its train units): create / use / close over and over, close in
either order and twice, a sampler that fails half-built, accumulators enabled and dropped again, staging that grows.  Nothing
here is about arithmetic, so the cohorts are tiny: a dense one (two lane groups, one word) and one of observation lists, 2
chains, and the three run loops of the native sampler -- dense trains, list trains, plain units (dense_metric).
"""
import numpy as np
import pytest

from abdpymc_amd import synthetic
from tests.helpers import random_sparse_cohort

pytestmark = pytest.mark.gpu
N_INDS, N_GAPS, CHAINS = 70, 20, 2
FLAVOURS = [("dense", False), ("lists", False), ("lists", True)]  # (cohort, dense_metric): dense trains, list trains, plain units
THETA0 = np.array([synthetic.make_thetas(N_GAPS, 1, c)[0] for c in range(CHAINS)])


def make_ctx(kind):
    from abdpymc_amd._native import Context

    if kind == "dense":
        sc = synthetic.make_cohort(N_INDS, N_GAPS)
        ctx = Context(sc.n_gaps, sc.n_inds, sc.s_obs, sc.n_obs, sc.vacs, sc.pcrpos, n_chains=CHAINS)
    else:
        coh = random_sparse_cohort(N_INDS, N_GAPS, 300, 300)
        ctx = Context(coh.n_gaps, coh.n_inds, (coh.s.idx_gap, coh.s.idx_ind, coh.s.log_dilution, coh.s.od),
                      (coh.n.idx_gap, coh.n.idx_ind, coh.n.log_dilution, coh.n.od), coh.vacs, coh.pcrpos, n_chains=CHAINS)
    assert ctx.is_dense == (kind == "dense")
    for c in range(CHAINS):
        ctx.set_discrete(c, *synthetic.make_chain_state(N_INDS, N_GAPS, c))
    return ctx


def make_sampler(ctx, dense_metric=False, pointwise=True, predictive=True, theta0=THETA0):
    return ctx.sampler(list(range(CHAINS)), theta0, tune=2, seed=11, dense_metric=dense_metric, pointwise=pointwise,
                       predictive=predictive)


def run3(ctx, smp):
    """3 iterations with everything recorded that has staging of its own -> every array the run returns but the host's clock"""
    G, N, cap = ctx.n_gaps, ctx.n_inds, 3
    rec = dict(i_raw=np.zeros((CHAINS, cap, G, N), np.int8), ab_n_mu=np.zeros((CHAINS, cap, G, N)),
               ll_s=np.zeros((CHAINS, cap, ctx.n_obs_s)), ll_n=np.zeros((CHAINS, cap, ctx.n_obs_n)),
               yrep_s=np.zeros((CHAINS, cap, ctx.n_obs_s)), yrep_n=np.zeros((CHAINS, cap, ctx.n_obs_n)))
    theta, stats = smp.run_record(3, 0, **rec)
    out = dict(rec, theta=theta, **{"stat_" + k: v for k, v in stats.items() if k != "t_done"})  # (t_done: the host's clock)
    for k in range(CHAINS):
        out[f"pw{k}"], out[f"pp{k}"] = smp.pointwise_stats(k)[0], smp.predictive_stats(k)[0]
    return out


def one_round(kind, dense_metric=False):
    ctx = make_ctx(kind)
    lp, g = ctx.logp_dlogp_batch(list(range(CHAINS)), THETA0)
    smp = make_sampler(ctx, dense_metric)
    out = dict(run3(ctx, smp), lp=lp, g=g)
    smp.close()
    ctx.close()
    return out


def assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


_fresh = {}


def fresh(kind, dense_metric=False):
    """what a fresh context and sampler return, computed once per flavour and left alone"""
    if (kind, dense_metric) not in _fresh:
        _fresh[kind, dense_metric] = one_round(kind, dense_metric)
    return _fresh[kind, dense_metric]


@pytest.mark.parametrize("kind", ["dense", "lists"])
def test_eight_rounds_of_create_use_close(kind):
    first = fresh(kind)
    assert np.all(np.isfinite(first["lp"])) and np.all(np.isfinite(first["stat_lp"]))
    for _ in range(6):
        one_round(kind)
    assert_same(one_round(kind), first)


@pytest.mark.parametrize("kind,dense_metric", FLAVOURS)
def test_close_in_either_order_and_twice(kind, dense_metric):
    ctx = make_ctx(kind)
    smp = make_sampler(ctx, dense_metric)
    assert_same(dict(run3(ctx, smp)), {k: v for k, v in fresh(kind, dense_metric).items() if k not in ("lp", "g")})
    smp.close()  # the sampler first
    ctx.close()
    smp.close()  # and again: nothing to do, no error
    ctx.close()

    ctx = make_ctx(kind)
    smp = make_sampler(ctx, dense_metric)
    smp.run(3)
    ctx.close()  # the context while its sampler is open: Context.close closes it first
    assert not smp._h.value
    smp.close()
    ctx.close()


@pytest.mark.parametrize("kind,dense_metric", FLAVOURS)
def test_sampler_that_fails_half_built_leaves_the_context_whole(kind, dense_metric):
    ctx = make_ctx(kind)
    bad = THETA0.copy()
    bad[1, 13] = 800.0  # sigma = e^800: logp is not finite -- found after the train units and side streams were made
    with pytest.raises(ValueError):
        make_sampler(ctx, dense_metric, theta0=bad)
    lp, g = ctx.logp_dlogp_batch(list(range(CHAINS)), THETA0)
    smp = make_sampler(ctx, dense_metric)
    assert_same(dict(run3(ctx, smp), lp=lp, g=g), fresh(kind, dense_metric))
    ctx.close()


@pytest.mark.parametrize("kind", ["dense", "lists"])
def test_accumulators_enabled_dropped_and_enabled_again(kind):
    from abdpymc_amd._native import _check

    ctx = make_ctx(kind)
    smp = make_sampler(ctx, pointwise=False, predictive=False)
    for fn in (ctx._lib.abd_sampler_enable_pointwise, ctx._lib.abd_sampler_enable_predictive):
        for on in (1, 0, 1):
            _check(ctx._lib, fn(smp._h, on))
    smp.run(3)
    once = fresh(kind)
    for k in range(CHAINS):
        np.testing.assert_array_equal(smp.pointwise_stats(k)[0], once[f"pw{k}"])
        np.testing.assert_array_equal(smp.predictive_stats(k)[0], once[f"pp{k}"])
    ctx.close()


@pytest.mark.parametrize("kind", ["dense", "lists"])
def test_reading_staging_grows_and_is_reused(kind):
    ctx = make_ctx(kind)
    first = ctx.pointwise_loglik(0, THETA0[0])  # one row of staging
    rep = ctx.posterior_predictive(0, THETA0[0], seed=3, mean=True)  # two rows: the staging grows
    third = ctx.pointwise_loglik(0, THETA0[0])  # one row of the larger staging
    assert all(np.all(np.isfinite(a)) for a in first + rep)
    for a, b in zip(first, third):
        np.testing.assert_array_equal(a, b)
    ctx.close()
