"""
tests/compound_replay.py has teeth (no GPU).

A "recorded run" is made from the C restatement alone, by a loop of its own: 3 chains in slots 0, 1, 2 with chain_offset 5, 12
iterations, the points a random walk around `theta_init`; on a dense 67 x 33 cohort and on a sparse one of 29 x 31.  The replay
passes on it, unthinned and with thin = 5, and fails -- each defect on its own, at the check that should see it -- on a run
whose maker sweeps at the point of the iteration before, numbers its sweeps one off, ignores chain_offset, uses the seed
unshifted or records one draw late, and on a run with one flipped cell, one flipped waner or one count off by one.
"""
import functools

import numpy as np
import pytest

from abdpymc_amd import synthetic
from oracle import c_oracle
from tests import compound_replay as R
from tests.helpers import oracle_cohort_from_synth, random_sparse_cohort

C, N_ITER, OFFSET, SEED = 3, 12, 5, 2**33 + 7
SLOTS = (0, 1, 2)


@functools.lru_cache(maxsize=None)
def _make(kind):
    if kind == "dense":
        coh, splits = oracle_cohort_from_synth(synthetic.make_cohort(67, 33, seed=3)), (11, 22)
    else:
        coh, splits = random_sparse_cohort(29, 31, 420, 380, seed=78), (10, 21)
    co = c_oracle.COracle(coh, splits)
    G, N = coh.n_gaps, coh.n_inds
    rng = np.random.default_rng(17)
    i0 = (rng.random((C, G, N)) < 2.0 / G).astype(np.int8)
    w0 = (rng.random((C, N)) < 0.5).astype(np.int8)
    start = synthetic.theta_init(G) + 0.1 * rng.standard_normal((C, 17))
    theta = start[:, None, :] + np.cumsum(0.1 * rng.standard_normal((C, N_ITER, 17)), axis=1)
    return co, theta, start, i0, w0


def make_run(kind, thin, defect=None):
    """the run a sampler with `defect` would return: (recorded, stats, final); its lp is always the logp of the iteration's point
    at the state it left behind, as a consistent but wrong sampler's would be"""
    co, theta, start, i0, w0 = _make(kind)
    n_rec = (N_ITER + thin - 1) // thin
    rec = dict(i_raw=np.full((C, n_rec) + i0.shape[1:], -1, np.int8), ab_s_waner=np.full((C, n_rec) + w0.shape[1:], -1, np.int8))
    stats = {k: np.zeros((C, N_ITER)) for k in ("gibbs_accepted", "gibbs_proposed", "lp")}
    final = []
    for c in range(C):
        i_raw, w = i0[c], w0[c]
        for t in range(N_ITER):
            before = (i_raw, w)
            at = (theta[c, t - 1] if t else start[c]) if defect == "theta of the iteration before" else theta[c, t]
            i_raw, w, acc, prop = co.gibbs_sweep(
                at, i_raw, w,
                chain=SLOTS[c] + (0 if defect == "chain_offset ignored" else OFFSET),
                seed=SEED & R.MASK64 if defect == "seed unshifted" else ((SEED << 20) ^ 0x5EED) % 2**64,
                sweep=t + (1 if defect == "sweep number one off" else 0), nthreads=2)
            stats["gibbs_accepted"][c, t], stats["gibbs_proposed"][c, t] = acc, prop
            stats["lp"][c, t] = co.logp_dlogp(theta[c, t], i_raw, w)[0]
            if t % thin == 0:
                rec["i_raw"][c, t // thin], rec["ab_s_waner"][c, t // thin] = before if defect == "recorded one draw late" else (i_raw, w)
        final.append((i_raw, w))
    return rec, stats, final


def _replay(kind, thin, rec, stats, final):
    co, theta, _, i0, w0 = _make(kind)
    return R.replay(co, theta, i0, w0, SLOTS, OFFSET, SEED, 0, rec, thin, stats, final=final, nthreads=2)


@pytest.mark.parametrize("kind", ["dense", "sparse"])
@pytest.mark.parametrize("thin", [1, 5])
def test_the_replay_passes_on_a_run_of_the_restatement(kind, thin):
    rec, stats, final = make_run(kind, thin)
    out = _replay(kind, thin, rec, stats, final)
    assert out.sweeps == C * N_ITER and np.all(out.accepted > 0) and np.all(out.recorded == (N_ITER + thin - 1) // thin)
    assert np.all(out.recorded_changed == out.recorded_pairs) and out.worst_lp == 0.0
    assert np.array_equal(out.proposed, stats["gibbs_proposed"].sum(axis=1))
    # ... and in two calls, the second one starting from what the first left
    a, b = 7, N_ITER - 7
    if thin == 1:
        co, theta, _, i0, w0 = _make(kind)
        cut = lambda d, lo, hi: {k: v[:, lo:hi] for k, v in d.items()}
        first = R.replay(co, theta[:, :a], i0, w0, SLOTS, OFFSET, SEED, 0, cut(rec, 0, a), 1, cut(stats, 0, a), nthreads=2)
        both = R.replay(co, theta[:, a:], slots=SLOTS, chain_offset=OFFSET, seed=SEED, first_iteration=a, recorded=cut(rec, a, a + b),
                        stats=cut(stats, a, a + b), start=first, final=final, nthreads=2)
        assert both.sweeps == C * N_ITER and np.array_equal(both.accepted, out.accepted)


@pytest.mark.parametrize("kind", ["dense", "sparse"])
@pytest.mark.parametrize("defect", ["theta of the iteration before", "sweep number one off", "chain_offset ignored", "seed unshifted",
                                    "recorded one draw late"])
def test_a_defective_sampler_is_caught_at_its_first_iteration(kind, defect):
    for thin in (1, 5):
        with pytest.raises(R.ReplayMismatch) as e:
            _replay(kind, thin, *make_run(kind, thin, defect))
        assert e.value.kind == "state" and e.value.chain == 0 and e.value.iteration == 0, str(e.value)
        assert "first differing individual" in str(e.value) and "cells of i_raw" in str(e.value)
        # a late record has the right counts; every other defect proposes other dims
        assert ("the counts agree" in str(e.value)) == (defect == "recorded one draw late"), str(e.value)


@pytest.mark.parametrize("kind", ["dense", "sparse"])
def test_one_flipped_cell_of_one_recorded_i_raw(kind):
    rec, stats, final = make_run(kind, 1)
    G, N = rec["i_raw"].shape[2:]
    rec["i_raw"][1, 8, G - 1, N - 2] ^= 1
    with pytest.raises(R.ReplayMismatch) as e:
        _replay(kind, 1, rec, stats, final)
    assert (e.value.kind, e.value.chain, e.value.iteration) == ("state", 1, 8)
    assert f"1 cells of i_raw and 0 of ab_s_waner differ from the reference, first differing individual {N - 2}" in str(e.value)


@pytest.mark.parametrize("kind", ["dense", "sparse"])
def test_one_flipped_waner(kind):
    rec, stats, final = make_run(kind, 5)
    rec["ab_s_waner"][2, 2, 4] ^= 1
    with pytest.raises(R.ReplayMismatch) as e:
        _replay(kind, 5, rec, stats, final)
    assert (e.value.kind, e.value.chain, e.value.iteration) == ("state", 2, 10)
    assert "0 cells of i_raw and 1 of ab_s_waner" in str(e.value) and "individual 4" in str(e.value)


@pytest.mark.parametrize("kind", ["dense", "sparse"])
def test_a_count_off_by_one_at_an_unrecorded_iteration(kind):
    rec, stats, final = make_run(kind, 5)
    stats["gibbs_accepted"][1, 7] += 1
    with pytest.raises(R.ReplayMismatch) as e:
        _replay(kind, 5, rec, stats, final)
    assert (e.value.kind, e.value.chain, e.value.iteration) == ("counts", 1, 7) and "not recorded" in str(e.value)


@pytest.mark.parametrize("kind", ["dense", "sparse"])
def test_the_other_checks_fail_on_their_own_too(kind):
    """lp beyond its gate, a wrong constrained i, a wrong state after the call"""
    co, theta, _, i0, w0 = _make(kind)
    rec, stats, final = make_run(kind, 1)
    pcr_gn = co.pcr.T
    rec["i"] = np.stack([[R.O.constrain_infections(rec["i_raw"][c, r], pcr_gn, tuple(co.splits)) for r in range(N_ITER)] for c in range(C)])
    assert _replay(kind, 1, rec, stats, final).worst_lp == 0.0
    lp = stats["lp"][0, 3]
    stats["lp"][0, 3] = lp * (1 + 0.5e-9)
    assert 0.4e-9 < _replay(kind, 1, rec, stats, final).worst_lp < 0.6e-9  # within the gate
    stats["lp"][0, 3] = lp * (1 + 2e-9)
    with pytest.raises(R.ReplayMismatch) as e:
        _replay(kind, 1, rec, stats, final)
    assert (e.value.kind, e.value.chain, e.value.iteration) == ("lp", 0, 3)
    stats["lp"][0, 3] = lp
    rec["i"][2, 11, 5, 6] ^= 1
    with pytest.raises(R.ReplayMismatch) as e:
        _replay(kind, 1, rec, stats, final)
    assert (e.value.kind, e.value.chain, e.value.iteration) == ("i", 2, 11)
    rec["i"][2, 11, 5, 6] ^= 1
    final[1] = (final[1][0], final[1][1] ^ 1)
    with pytest.raises(R.ReplayMismatch) as e:
        _replay(kind, 1, rec, stats, final)
    assert (e.value.kind, e.value.chain) == ("final", 1)
