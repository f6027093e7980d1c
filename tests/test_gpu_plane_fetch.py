"""
The scalar side of the plane form of the dense gap loop (abd_dense.hpp: dense_walk_planes; abd_planes.hpp:
abd_plane_first_pair, abd_row_off_next), on the device: the loop fetches the lane masks of the pair after the one it walks
from a running pointer -- at a row's end out of the row's one pair of padding, and the last lane group's row ends the buffer --
and refills its row buffers from a running offset that is clamped at the piece's last row.  The smallest shapes where that can
go wrong: N = 70 (two lane groups, 6 lanes in the last one), rows of 1 to 7 gaps (every piece is in reach of the row's end,
odd and even lengths) and of 65, fp64 and fp32 storage.  The plane form (ABD_DENSE_PLANES=1) against the legacy form (=0),
which reads no planes and works its rows out from the gap index: a synchronous call, single enqueued steps and a 64-step
logp_dlogp_many (four-step launches), bit for bit.  (tests/test_plane_fetch.py steps the same index functions over every
piece of every row length on the CPU.)
"""
import os

import numpy as np
import pytest

from abdpymc_amd import synthetic

pytestmark = pytest.mark.gpu

N_INDS = 70
GAPS = [1, 2, 3, 4, 5, 7, 65]
K_MANY = 64
N_CHAINS = 4


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


def _context(sc, planes, storage):
    from abdpymc_amd._native import Context

    with _env(ABD_DENSE_PLANES=planes):
        ctx = Context(sc.n_gaps, sc.n_inds, sc.s_obs, sc.n_obs, sc.vacs, sc.pcrpos, n_chains=N_CHAINS, storage=storage)
    assert ctx.is_dense
    return ctx


def _states(n_gaps):
    """four discrete states: random, none exposed, everyone in every gap, one infection in the row's last gap (lanes of both
    lane groups, the last individual among them)"""
    G, N = n_gaps, N_INDS
    w = (np.arange(N) % 3 == 0).astype(np.int8)
    last = np.zeros((G, N), np.int8)
    last[G - 1, ::3] = 1
    last[G - 1, N - 1] = 1
    return [synthetic.make_chain_state(N, G, 3), (np.zeros((G, N), np.int8), w), (np.ones((G, N), np.int8), 1 - w), (last, w)]


def _thetas(n_gaps, salt):
    return np.stack([synthetic.make_thetas(n_gaps, 1, 13 * salt + c)[0] for c in range(N_CHAINS)])


def _all_forms(ctx, n_gaps):
    chains = np.arange(N_CHAINS)
    out = [ctx.logp_dlogp_batch(chains, _thetas(n_gaps, 0))]                       # a synchronous call, four chains
    out += [ctx.logp_dlogp_batch([c], _thetas(n_gaps, 1)[c:c + 1]) for c in chains]  # ... and of one chain each
    for k in range(5):                                                             # single enqueued steps
        ctx.enqueue(k, chains, _thetas(n_gaps, 2 + k))
    ctx.enqueue(5, [2], _thetas(n_gaps, 7)[2:3])
    ctx.wait()
    out.append(ctx.fetch_many(np.arange(5), N_CHAINS))
    out.append(ctx.fetch(5, 1))
    th = np.stack([_thetas(n_gaps, 10 + k) for k in range(K_MANY)])
    out.append(ctx.logp_dlogp_many(chains, th))                                    # four-step launches
    out.append(ctx.logp_dlogp_many([1], th[:, 1:2]))
    assert ctx.wait_fallbacks == 0
    return out


@pytest.mark.parametrize("storage", ["f64", "f32"])
@pytest.mark.parametrize("n_gaps", GAPS)
def test_plane_form_equals_legacy_form_at_the_rows_end(n_gaps, storage):
    if n_gaps == 1:
        # the model has no one-gap cohort (Beta(1, n_gaps - 1) prior on p): the library refuses it before any plane exists,
        # whichever form is asked for; the one-gap row is walked on the CPU (tests/test_plane_fetch.py)
        sc = synthetic.make_cohort(N_INDS, 1, seed=N_INDS + 1)
        for planes in (1, 0):
            with pytest.raises(ValueError, match="n_gaps must be >= 2"):
                _context(sc, planes, storage)
        return
    sc = synthetic.make_cohort(N_INDS, n_gaps, seed=N_INDS + n_gaps)
    states = _states(n_gaps)
    res = []
    for planes in (1, 0):
        ctx = _context(sc, planes, storage)
        for s, (i_raw, w) in enumerate(states):
            ctx.set_discrete(s, i_raw, w)
        res.append(_all_forms(ctx, n_gaps))
        ctx.close()
    assert len(res[0]) == len(res[1])
    for (lp1, g1), (lp0, g0) in zip(*res):
        assert np.all(np.isfinite(lp1)) and np.all(np.isfinite(g1))
        np.testing.assert_array_equal(lp1, lp0)
        np.testing.assert_array_equal(g1, g0)
