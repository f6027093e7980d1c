"""
The perm sums of the dense kernel (gradient entries 1, perm_n, and 5, perm_s) as differences of the H sums (abd_planes.hpp:
abd_hc_open / abd_hc_close; abd_dense.hpp) and the S boost by selects, on hand-made discrete states that put the first exposure
where the difference can go wrong: nobody exposed, everybody infected at gap 0, first infection at the last gap, vaccination only,
infection and vaccination in one gap, and a random state.

Shapes: N = 130 is three lane groups, the last with 2 lanes; G = 7 and G = 33 are odd and G = 33 crosses one 32-gap word.  Calls of
1, 2 and 4 chains cover the three forms of the kernel (a one-chain launch reads the split panels); the full grid of a synchronous
call starts many ranges inside an individual's gaps, and the fused launches of a K = 64 call have ranges that run from one lane
group into the next.  Everything against the oracle at test_gpu_parity.py's RTOL and scaling.
"""
import dataclasses

import numpy as np
import pytest

from abdpymc_amd import synthetic
from oracle import abd_oracle as O

pytestmark = pytest.mark.gpu

RTOL = 1e-6  # (test_gpu_parity.py)
N_INDS = 130
K_MANY = 64
K_CHECK = (0, 37, K_MANY - 1)  # steps of a K = 64 call that are compared with a synchronous call at the same point


def _cohort(n_gaps, kind):
    """'bare': no vaccinations, no PCR positives (a lane is exposed by the chain's infections alone); 'vacs': every other
    individual vaccinated once, in gap 2, no PCR positives; 'full': the synthetic cohort as it is"""
    sc = synthetic.make_cohort(N_INDS, n_gaps, seed=N_INDS + n_gaps)
    if kind in ("bare", "vacs"):
        sc = dataclasses.replace(sc, vacs=np.zeros_like(sc.vacs), pcrpos=np.zeros_like(sc.pcrpos))
    if kind == "vacs":
        sc.vacs[::2, 2] = 1
    return sc


def _states(n_gaps, kind):
    """four (name, i_raw (G, N), waner (N,)) for the four slots of a context"""
    G, N = n_gaps, N_INDS
    rng = np.random.default_rng(G)
    w = (rng.random(N) < 0.5).astype(np.int8)
    z = np.zeros((G, N), np.int8)
    if kind == "bare":
        at0, last, mixed = z.copy(), z.copy(), z.copy()
        at0[0, :] = 1
        last[G - 1, :] = 1
        mixed[0, 0::3] = 1      # a third at gap 0, a third at the last gap, a third never
        mixed[G - 1, 1::3] = 1
        return [("nobody", z, w), ("all@0", at0, w), ("first@last", last, 1 - w), ("thirds", mixed, w)]
    if kind == "vacs":
        same, later, before = z.copy(), z.copy(), z.copy()
        same[2, :] = 1           # the vaccinated: infection and dose in one gap; the others: infection alone
        later[G - 1, 0::4] = 1   # half of the vaccinated: dose first, first infection at the last gap
        before[0, :] = 1         # infection before the dose
        return [("vaccination only", z, w), ("infection and dose in one gap", same, w), ("dose, then infection", later, 1 - w),
                ("infection, then dose", before, w)]
    return [("random %d" % c, *synthetic.make_chain_state(N, G, c)) for c in range(4)]


def _thetas(n_gaps, salt):
    return np.stack([synthetic.make_thetas(n_gaps, 1, 13 * salt + c)[0] for c in range(4)])


def _context(sc, storage):
    from abdpymc_amd._native import Context

    ctx = Context(sc.n_gaps, sc.n_inds, sc.s_obs, sc.n_obs, sc.vacs, sc.pcrpos, n_chains=4, storage=storage)
    assert ctx.is_dense
    return ctx


def _oracle_cohort(sc, storage):
    r = (lambda a: a.astype(np.float32).astype(np.float64)) if storage == "f32" else (lambda a: a)
    return O.Cohort(sc.n_gaps, sc.n_inds, sc.vacs, sc.pcrpos, O.AntigenObs(sc.idx_gap, sc.idx_ind, r(sc.x_s), r(sc.y_s)),
                    O.AntigenObs(sc.idx_gap, sc.idx_ind, r(sc.x_n), r(sc.y_n)))


def _assert_close(lp, g, lp_ref, g_ref, what):
    scale = np.maximum(np.abs(g_ref), 1e-6 * np.abs(g_ref).max())
    err = np.abs(g - g_ref) / scale
    print(f"{what}: logp {abs(lp - lp_ref) / abs(lp_ref):.2e}, dlogp {err.max():.2e}, perm_n {err[1]:.2e}, perm_s {err[5]:.2e}")
    assert abs(lp - lp_ref) <= RTOL * abs(lp_ref), (what, lp, lp_ref)
    assert err.max() <= RTOL, (what, err, g, g_ref)


def _evaluate(ctx, n_gaps):
    """every slot through calls of 1, 2 and 4 chains: -> {n: (lp [len(K_CHECK)][4], g [len(K_CHECK)][4][17])} of the synchronous
    calls; the K = 64 calls are checked against them on the way"""
    th = np.stack([_thetas(n_gaps, k) for k in range(K_MANY)])  # [K][4][17]
    out = {}
    for n in (1, 2, 4):
        lp_b, g_b = np.empty((len(K_CHECK), 4)), np.empty((len(K_CHECK), 4, 17))
        for start in range(0, 4, n):
            chains = list(range(start, start + n))
            lp_m, g_m = ctx.logp_dlogp_many(chains, th[:, start:start + n])
            assert np.all(np.isfinite(lp_m)) and np.all(np.isfinite(g_m))
            for q, k in enumerate(K_CHECK):
                lp, g = ctx.logp_dlogp_batch(chains, th[k, start:start + n])
                lp_b[q, start:start + n], g_b[q, start:start + n] = lp, g
                # launch shapes differ: equal to rounding (test_gpu_parity.py asks 1e-12 of launch shapes)
                np.testing.assert_allclose(lp_m[k], lp, rtol=1e-12)
                gs = np.abs(g).max(axis=1, keepdims=True)
                assert (np.abs(g_m[k] - g) / gs).max() <= 1e-12, (n, start, k)
        out[n] = (lp_b, g_b)
    assert ctx.wait_fallbacks == 0
    return th, out


@pytest.mark.parametrize("storage", ["f64", "f32"])
@pytest.mark.parametrize("kind", ["bare", "vacs", "full"])
@pytest.mark.parametrize("n_gaps", [7, 33])
def test_hand_made_states_against_the_oracle(n_gaps, kind, storage):
    sc = _cohort(n_gaps, kind)
    coh = _oracle_cohort(sc, storage)
    states = _states(n_gaps, kind)
    ctx = _context(sc, storage)
    for s, (_, i_raw, w) in enumerate(states):
        ctx.set_discrete(s, i_raw, w)
    th, res = _evaluate(ctx, n_gaps)
    ctx.close()
    for s, (name, i_raw, w) in enumerate(states):
        lp_ref, g_ref = O.logp_dlogp(th[0, s], i_raw, w, coh, ())  # (once per state: step 0 of every call form)
        for n in (1, 2, 4):
            _assert_close(res[n][0][0, s], res[n][1][0, s], lp_ref, g_ref, f"G={n_gaps} {storage} {name}, {n} per call")


@pytest.mark.parametrize("storage", ["f64", "f32"])
@pytest.mark.parametrize("n_gaps", [7, 33])
def test_nobody_exposed_perm_entries_do_not_see_the_data(n_gaps, storage):
    """nobody exposed on a cohort without vaccinations or PCR positives: the data term of d/dperm_n and d/dperm_s is exactly zero,
    so two contexts that differ only in their OD values give the same bits there -- a stale HC - H would not"""
    sc = _cohort(n_gaps, "bare")
    rng = np.random.default_rng(n_gaps)
    sc2 = dataclasses.replace(sc, y_s=sc.y_s + 0.3 * rng.random(sc.y_s.size), y_n=sc.y_n * 0.5 + 0.1)
    states = _states(n_gaps, "bare")
    assert states[0][0] == "nobody"
    res = []
    for cohort in (sc, sc2):
        ctx = _context(cohort, storage)
        # slot 0: nobody exposed; the others: exposed states beside it, whose sums must not leak into slot 0's
        for s, (_, i_raw, w) in enumerate(states):
            ctx.set_discrete(s, i_raw, w)
        res.append(_evaluate(ctx, n_gaps)[1])
        ctx.close()
    for n in (1, 2, 4):
        (lp_a, g_a), (lp_b, g_b) = res[0][n], res[1][n]
        assert not np.array_equal(lp_a[:, 0], lp_b[:, 0])  # (the data did change)
        assert not np.array_equal(g_a[:, 0, 11], g_b[:, 0, 11])  # (d/db_n)
        np.testing.assert_array_equal(g_a[:, 0, 1], g_b[:, 0, 1])
        np.testing.assert_array_equal(g_a[:, 0, 5], g_b[:, 0, 5])
        assert not np.array_equal(g_a[:, 1, 1], g_b[:, 1, 1])  # everybody infected at gap 0: the entry does see the data
