"""
The references of tests/test_gpu_fused_parity.py's layer B (tests/golden/fused_parity.npz, written by
tests/golden/make_fused_fixtures.py), without a GPU:

* the inputs rebuild to the stored checksums;
* the float64 oracle's own error on these sets, in units of u S_k, stays at or below E_ORACLE -- the condition under which the
  device budget C = 32 E_ORACLE of tests/mp_reference.py holds for them unchanged (it was made from the oracle's worst error on
  the sets of tail_parity.npz, the largest of 2 145 readings per antigen; these have 66 392 and 77 228);
* one evaluation of the file is what the generator computes today, bit for bit (needs mpmath: 25 s of it; the whole file is 18
  evaluations, seven and a half minutes of one core).
"""
import os
import warnings

import numpy as np
import pytest

from oracle import abd_oracle as O
from tests import mp_reference as R
from tests.golden import make_fused_fixtures as M
from tests.golden.make_tail_fixtures import case_check

# (set, storage, case, state) -> the outputs O.logp_dlogp returns NaN for: e * s = inf * 0 in lik() where exp(b (a - x)) overflows,
# which the S titers of state 0 reach at b = +40 on cohorts this long (tests/test_tail_reference_cpu.py pins the same for b=+300)
_S_SIDE = [5, 6, 10, 14]
ORACLE_NOT_FINITE = {("193x344", "f64", "b=+40 perm=e^2.5", 0): _S_SIDE, ("449x172", "f64", "b=+40 perm=e^2.5", 0): _S_SIDE,
                     ("449x172", "f32", "b=+40 perm=e^2.5", 0): _S_SIDE}


@pytest.fixture(scope="module")
def fx(golden_dir):
    return R.load_fixture(golden_dir, M.FIXTURE)


def _all_evaluations():
    for name, (_, _, f32) in M.SHAPES.items():
        base, states, cases = M.cohort(name), M.states(name), M.set_cases(name)
        for st in ("f64", "f32") if f32 else ("f64",):
            coh = R.rounded_to_f32(base) if st == "f32" else base
            for c, (cname, theta) in enumerate(cases):
                for z, (i_raw, w) in enumerate(states):
                    yield name, st, c, z, cname, theta, i_raw, w, coh


def test_the_file_holds_the_parts_and_nothing_else(fx):
    keys = {f"{name}.names" for name in M.SHAPES} | {f"{name}.{st}.{k}" for name, st, _, _ in M.parts() for k in ("theta", "ref", "S", "check")}
    assert set(fx) == keys
    assert len(M.parts()) == 18 and os.path.getsize(os.path.join(os.path.dirname(M.__file__), M.FIXTURE)) < 16384


def test_the_rebuilt_inputs_are_the_ones_the_references_were_made_on(fx):
    for name, st, c, z, cname, theta, i_raw, w, coh in _all_evaluations():
        assert fx[f"{name}.names"][c] == cname
        assert theta.tobytes() == fx[f"{name}.{st}.theta"][c].tobytes(), (name, cname)
        np.testing.assert_array_equal(case_check(i_raw, w, coh), fx[f"{name}.{st}.check"][c, z], err_msg=f"{name} {st} {cname} state {z}")
    for name in M.SHAPES:  # the two states differ, and each shape has the plane rows the layer is about
        (i0, w0), (i1, w1) = M.states(name)
        assert i0.tobytes() != i1.tobytes() and w0.tobytes() != w1.tobytes()
        N, G, _ = M.SHAPES[name]
        assert -(-N // 64) * G == 1376


def test_the_oracle_stays_within_e_oracle_on_these_sets(fx):
    worst, where, not_finite = 0.0, None, {}
    for name, st, c, z, cname, theta, i_raw, w, coh in _all_evaluations():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            lp, g = O.logp_dlogp(theta, i_raw, w, coh)
        got, ref, S = np.append(g, lp), fx[f"{name}.{st}.ref"][c, z], fx[f"{name}.{st}.S"][c, z]
        assert np.isfinite(ref).all() and np.isfinite(S).all() and (S > 0).all(), (name, cname)
        bad = np.flatnonzero(~np.isfinite(got)).tolist()
        if bad:
            not_finite[(name, st, cname, z)] = bad
        ok = np.isfinite(got)
        ratio = np.abs(got[ok] - ref[ok]) / (R.U * S[ok])
        if ratio.max() > worst:
            worst, where = float(ratio.max()), (name, st, cname, z, int(np.flatnonzero(ok)[ratio.argmax()]))
    print(f"\nE_oracle measured on the fused-parity sets: {worst:.1f} u S_k at {where}; E_ORACLE = {R.E_ORACLE}, C = {R.C_BUDGET}")
    assert worst <= R.E_ORACLE
    assert not_finite == ORACLE_NOT_FINITE


def test_the_restated_launch_rules_at_256_cus():
    """tests/fused_launches.py at the numbers of an MI355X: the steps per launch the GPU tests name, and on both shapes every chain
    count's fused grid below its single-step grid with 4 and 3 pipes (with 2, pipe_blocks is 512 and the cap decides both grids
    at n = 1, 5 and 6: the GPU test may skip the last two and fails on the first)"""
    from tests import fused_launches as F

    assert [F.fuse_steps(67, n, 4) for n in (1, 2, 3, 4, 5, 6, 8, 16, 17)] == [4, 4, 4, 4, 3, 2, 2, 1, 1]
    assert F.fuse_steps(8, 4, 4) == 1 and F.fuse_steps(19, 4, 1) == 4 and F.fuse_steps(15, 4, 1) == 3
    assert F.fuse_plan(19, 1, 1, 1024) == [(0, 4), (4, 4), (8, 4), (12, 4), (16, 3)]
    assert F.fuse_plan(7, 5, 1, 4) == [(0, 1), (1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (6, 1)]
    assert F.fuse_plan(14, 8, 1, 5)[:4] == [(0, 2), (2, 2), (4, 1), (5, 2)]
    grids = {}
    for name, (N, G, _) in M.SHAPES.items():
        for pipes in (4, 3, 2):
            for n in (1, 2, 4, 5, 6, 8):
                cpw, S = F.pick_cpw(n), F.fuse_steps(16 * pipes + 3, n, pipes)
                grids[(name, pipes, n)] = (F.dense_blocks(256, pipes, N, G, cpw, S * n // cpw, S), F.dense_blocks(256, pipes, N, G, cpw, n // cpw, 1))
        assert [grids[(name, 4, n)] for n in (1, 2, 4, 5, 6, 8)] == [(64, 86), (64, 172), (64, 256), (85, 86), (128, 172), (128, 256)]
    assert all(f < s for (_, pipes, _), (f, s) in grids.items() if pipes > 2)
    assert sorted(n for (name, pipes, n), (f, s) in grids.items() if not f < s and name == "193x344") == [1, 5, 6]
    # a launch outside the rotation -- the call's last, and every launch of a one-pipe context -- takes the grid of an empty chip
    assert F.dense_blocks(256, 4, 65, 33, 4, 4, 4, shared=False) == F.dense_blocks(256, 1, 65, 33, 4, 4, 4) == 16


def test_one_evaluation_is_what_the_generator_computes(fx):
    pytest.importorskip("mpmath")
    part = ("193x344", "f64", M.CASES.index("rho -800/-800"), 1)
    assert part in M.parts()
    (name, st, c, z), ref, S, check = M.generate_part(part)
    for k, v in (("ref", ref), ("S", S), ("check", check)):
        assert v.tobytes() == fx[f"{name}.{st}.{k}"][c, z].tobytes(), k  # bit for bit, the signs of zeros included
