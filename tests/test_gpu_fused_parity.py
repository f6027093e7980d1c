"""
Fused stream-ordered launches against the 40-digit reference: abd_logp_dlogp_many with enough steps puts up to four consecutive
steps into one dense launch (abd_fuse_plan.hpp) -- step s, chain j is kernel row s n + j, a launch in rotation gets
pipe_blocks / S workgroups per grid row, its partial rows are summed by the next launch on its pipe or by abd_finalize_kernel.
The other tests of that form compare the device with the device (tests/test_gpu_fused_steps.py, test_gpu_hc_sum.py) or one form
of the gap loop with the other (test_gpu_exposure_planes.py, test_gpu_plane_fetch.py): an error in the row mapping, the range
split or the sums repeats on both sides.  Here every output of every row of every step is held to

    |got_k - ref_k| <= C u S_k        (tests/test_gpu_tail_parity.py: the same gate, the same collector, C = R.C_BUDGET)

with every output finite and nothing masked, and every call first PROVES that it fused: the launches are read back from the result
slots (tests/fused_launches.py) and must be the plan of abd_fuse_plan.hpp for (K, n, ctx.n_pipes), K = 16 pipes + 3.

Layer A: the tail table (tests/golden/tail_parity.npz) through fused launches, every row of a launch at another case, so that a
mix-up between the steps or chains of a launch lands on another reference.  Layer B: the smallest cohorts at which a launch of S
steps gets fewer ranges per grid row than a single step (tests/golden/fused_parity.npz; 1376 plane rows in three and in six 64-gap
words) -- asserted from the CU count and the context's pipes before the call.  The budget of layer B is R.C_BUDGET unchanged: the
float64 oracle stays within E_ORACLE on its sets (tests/test_fused_reference_cpu.py: 3.3 u S_k measured).

Measured on an MI355X (256 CUs, 4 pipes), worst ratio per family in u S_k against C = 1536: see DESIGN.md section 6.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from tests import fused_launches as F
from tests import mp_reference as R
from tests.golden import make_fused_fixtures as M
from tests.golden.make_tail_fixtures import case_check
from tests.test_gpu_tail_parity import Worst, _context, cases

pytestmark = pytest.mark.gpu

_FX = R.load_fixture(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"), M.FIXTURE)


def _case_of(k, s, n, n_cases):
    """step k, chain s evaluates case (k n + s) mod n_cases; where n_cases divides n that would give a chain the same case in every
    step (a mix-up between steps would pass), so the steps are shifted by one case each"""
    return (k * n + s + (k if n % n_cases == 0 else 0)) % n_cases


def _many(ctx, chains, th, grad=True):
    """logp_dlogp_many; grad = False: the logp-only form, grad NULL through the C ABI"""
    if grad:
        return ctx.logp_dlogp_many(chains, th)
    ch, th = np.ascontiguousarray(chains, dtype=np.int32), np.ascontiguousarray(th)
    lp = np.full(th.shape[:2], np.nan)
    dp = C.POINTER(C.c_double)
    rc = ctx._lib.abd_logp_dlogp_many(ctx._h, th.shape[0], ch.size, ch.ctypes.data_as(C.POINTER(C.c_int32)), th.ctypes.data_as(dp), lp.ctypes.data_as(dp), None)
    assert rc == 0
    return lp, None


def _check_call(worst, ctx, chains, pick, S, what, grad=True):
    """one call: pick[k][s] = (label, theta, ref (18,), S (18,)) of step k, chain s; the plan first, then every row"""
    K, n = len(pick), len(chains)
    lp, g = _many(ctx, chains, np.array([[p[1] for p in step] for step in pick]), grad)
    plan = F.assert_fused(ctx, K, n, S, lp, g)
    for k in range(K):
        for s in range(n):
            label, _, ref, Sk = pick[k][s]
            if grad:
                worst.check(f"{what} step {k} chain {s}: {label}", lp[k, s], g[k, s], ref, Sk)
            else:
                worst.check(f"{what} step {k} chain {s}: {label}", lp[k, s], [], ref[17:], Sk[17:])
    return plan


# ---- layer A: the tail table through fused launches ----


def _layer_a(name, n, S, storage="f64", grad=True):
    cs = cases(name, storage)
    rows = [r for r in cs.rows if r[4] is cs.rows[0][4] and r[2].tobytes() == cs.rows[0][2].tobytes()]
    assert len(rows) == (25 if name == "65x33" else 5)
    ones = [r for r in cs.rows if r[0] == "ones b=-8"]
    worst = Worst(f"fused launches, layer A, {name} {storage}, {n} chains{'' if grad else ', logp only'}")
    ctx = _context(rows[0][4], n_chains=n + 1, storage=storage)
    assert ctx.is_dense
    for slot in range(n):
        ctx.set_discrete(slot, rows[0][2], rows[0][3])
    K = F.k_fused(ctx)
    item = lambda r: (r[0], r[1], cs.get("ref", r[5]), cs.get("S", r[5]))  # noqa: E731
    # every case of the table is evaluated: one call, or (one pipe, one chain: K = 19) a second one that starts where it ended
    for start in range(0, len(rows), K * n):
        pick = [[item(rows[(start + _case_of(k, s, n, len(rows))) % len(rows)]) for s in range(n)] for k in range(K)]
        plan = _check_call(worst, ctx, list(range(n)), pick, S, f"table from {start}", grad)
    if ones:
        # the extra chain slot holds the all-ones state and takes the call's last place: "ones b=-8" in every step, beside the
        # other chains' cycling cases (alone where n = 1)
        assert ones[0][4] is rows[0][4]
        ctx.set_discrete(n, ones[0][2], ones[0][3])
        pick = [step[:n - 1] + [item(ones[0])] for step in pick]
        assert _check_call(worst, ctx, list(range(n - 1)) + [n], pick, S, "with ones", grad) == plan
    print(f"\nplan of K = {K}, n = {n}, {ctx.n_pipes} pipes: {len(plan) - 1} launches of {S} steps and one of {plan[-1][1]}")
    assert ctx.wait_fallbacks == 0
    ctx.close()
    worst.done()


# 1 and 3: one chain per workgroup, split panels; 2 and 4: two and four chains per workgroup; 5: three steps; 8: two grid rows
# of four chains per step, two steps
_S_OF = {1: 4, 2: 4, 3: 4, 4: 4, 5: 3, 8: 2}


@pytest.mark.parametrize("storage", ["f64", "f32"])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 8])
def test_tail_table_65x33(n, storage):
    """the full table on 65 x 33 (two lane groups, one lane in the second); f32: panels held in float32, against the reference on
    the rounded panels"""
    _layer_a("65x33", n, _S_OF[n], storage)


@pytest.mark.parametrize("n", [1, 4, 5])
def test_two_words_7x65(n):
    """two 64-gap words.  n = 5: a launch has 15 rows and the cap of 65 / 16 = 4 workgroups, fewer than rows to sum: the pending sum
    goes out as abd_finalize_kernel, not inside the next launch"""
    _layer_a("7x65", n, _S_OF[n])


@pytest.mark.parametrize("n", [1, 4])
def test_pair_panels(n):
    """every log dilution another value: no split panels, the one-chain launches read the pair panels"""
    _layer_a("65x33 distinct", n, 4)


@pytest.mark.parametrize("planes", ["1", "0"])
@pytest.mark.parametrize("name,n", [("65x33", 4), ("7x65", 1)])
def test_plane_form_and_legacy_form(name, n, planes, monkeypatch):
    monkeypatch.setenv("ABD_DENSE_PLANES", planes)
    _layer_a(name, n, 4)


@pytest.mark.parametrize("n", [1, 4])
def test_one_pipe(n, monkeypatch):
    """ABD_PIPES=1: a fused launch takes the whole-chip grid and is joined instead of rotated; K = 19 >= 16 gives S = 4"""
    monkeypatch.setenv("ABD_PIPES", "1")
    ctx = _context(cases("65x33").rows[0][4])
    assert ctx.n_pipes == 1 and F.k_fused(ctx) == 19
    ctx.close()
    _layer_a("65x33", n, 4)


def test_logp_only_two_words():
    """the kernels' logp-only form at more than one word: output 17 alone"""
    _layer_a("7x65", 4, 4, grad=False)


# ---- layer B: the smallest cohorts at which a fused launch gets its own range partition ----


@functools.lru_cache(maxsize=None)
def _layer_b_inputs(name, storage):
    """(cohort, [(i_raw, waner)], [(case name, theta)]), checked against the stored checksums"""
    coh, states, table = M.cohort(name), M.states(name), M.set_cases(name)
    ref_coh = R.rounded_to_f32(coh) if storage == "f32" else coh
    for c, (cname, theta) in enumerate(table):
        assert _FX[f"{name}.names"][c] == cname and theta.tobytes() == _FX[f"{name}.{storage}.theta"][c].tobytes()
        for z, (i_raw, w) in enumerate(states):
            np.testing.assert_array_equal(case_check(i_raw, w, ref_coh), _FX[f"{name}.{storage}.check"][c, z])
    return coh, states, table


_LAYER_B = [(name, n, "f64") for name in M.SHAPES for n in (1, 2, 4, 5, 6, 8)] + [("449x172", 4, "f32")]


@pytest.mark.parametrize("name,n,storage", _LAYER_B, ids=[f"{a}-{n}-{st}" for a, n, st in _LAYER_B])
def test_own_range_partition(name, n, storage):
    """193 x 344 (six words: the 8-word kernel forms) and 449 x 172 (three words), 1376 plane rows each: the cap on the grid is 344,
    172 and 86 workgroups for four, two and one chain per workgroup, so with pipe_blocks = 256 a launch of 2, 3 or 4 steps has fewer
    ranges per row than the same step alone.  Steps cycle through the fixture's cases, chain slots alternate between its two states.
    (The CU count comes from torch: the first case of a process pays its import and device query, some ten seconds, once.)"""
    coh, states, table = _layer_b_inputs(name, storage)
    N, G, _ = M.SHAPES[name]
    worst = Worst(f"fused launches, layer B, {name} {storage}, {n} chains")
    ctx = _context(coh, n_chains=n + 1, storage=storage)  # (a spare chain slot: tests/fused_launches.py, observed_plan)
    try:
        assert ctx.is_dense
        K = F.k_fused(ctx)
        S = F.fuse_steps(K, n, ctx.n_pipes)
        assert S == min(4, 16 // n)
        fused, single = F.fused_smaller_than_single_or_skip(ctx, N, G, n, S, may_skip=n in (5, 6))
        for slot in range(n):
            ctx.set_discrete(slot, *states[slot % 2])
        pick = []
        for k in range(K):
            cs = [_case_of(k, s, n, len(table)) for s in range(n)]
            pick.append([(f"{table[c][0]} state {s % 2}", table[c][1], _FX[f"{name}.{storage}.ref"][c, s % 2], _FX[f"{name}.{storage}.S"][c, s % 2])
                         for s, c in enumerate(cs)])
        plan = _check_call(worst, ctx, list(range(n)), pick, S, "call")
        print(f"\nplan of K = {K}, n = {n}, {ctx.n_pipes} pipes: {len(plan) - 1} launches of {S} steps and one of {plan[-1][1]}; "
              f"{fused} workgroups per grid row against {single} of a single step")
        assert ctx.wait_fallbacks == 0
    finally:
        ctx.close()
    worst.done()
