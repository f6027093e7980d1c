"""abd_survival_groups_terms.hpp on the CPU: the host half of a grouped survival evaluation -- lambda_t, a_g, b for the kernel, and
logp and the gradient from the device sums -- against the NumPy restatement given the same sums; an empty group's gradient
entry; and the layout of the individuals by group."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import survival_groups_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("survival_groups") / "libsurvival_groups_harness.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror", "-I",
                           os.path.join(ROOT, "abdpymc_amd", "csrc"), os.path.join(ROOT, "tests", "native", "survival_groups_harness.cpp"),
                           "-o", str(out)])
    lib = C.CDLL(str(out))
    lib.survival_groups_terms.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_double] + [C.c_void_p] * 4
    lib.survival_groups_layout.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 4
    return lib


def _terms(lib, rs, q, sums):
    T, Gr = rs.T, rs.Gr
    pri = np.array(R.PRIORS)
    par, g, lp = np.empty(T + Gr + 1), np.empty(rs.dim), C.c_double()
    D = lib.survival_groups_terms(T, Gr, pri.ctypes.data, q.ctypes.data, rs.Y.ctypes.data, rs.C, sums.ctypes.data, par.ctypes.data,
                                  C.addressof(lp), g.ctypes.data)
    assert D == rs.dim == T + Gr + 5
    return par, lp.value, g


@pytest.mark.parametrize("name", R.POINTS)
def test_host_terms_equal_the_restatement(lib, name):
    N, T, Gr = 130, 65, 4  # with an empty group and a group without follow-up
    y, e, x, group = R.make_case(N, T, Gr)
    rs = R.GroupsRestatement(y, e, x, group, Gr)
    q = R.make_point(name, T, Gr)
    sums = rs.sums(q)
    lp_ref, g_ref = rs.combine(q, sums)
    par, lp, g = _terms(lib, rs, q, sums)
    m, s, z, a_mu, a_sl, az, b = rs.split(q)
    # two libraries' exp (each within 1 ulp), one addition and one division each: a few u
    np.testing.assert_allclose(par[:T], R._invlogit(m + np.exp(s) * z), rtol=1e-15, atol=0)
    # a_g = a_mu + a_sd z_g: one exp, one product, one sum; the sum may cancel to the size of u (|a_mu| + a_sd |z_g|)
    np.testing.assert_allclose(par[T:T + Gr], a_mu + np.exp(a_sl) * az, rtol=0, atol=4 * R.U * (abs(a_mu) + np.exp(a_sl) * np.abs(az).max()))
    assert par[T + Gr] == b
    assert np.isfinite(lp) and np.isfinite(g).all()
    # the same closed form in another order of additions: a few roundings of the largest addend
    assert abs(lp - lp_ref) <= 1e-13 * max(1.0, abs(lp_ref), np.abs(sums).max())
    np.testing.assert_allclose(g, g_ref, rtol=1e-12, atol=1e-13 * max(1.0, np.abs(g_ref).max()))


def test_an_empty_groups_gradient_is_its_priors(lib):
    N, T, Gr = 130, 65, 4
    y, e, x, group = R.make_case(N, T, Gr)
    rs = R.GroupsRestatement(y, e, x, group, Gr)
    for name in ("typical", "a_spread", "b_plus_50"):
        q = R.make_point(name, T, Gr)
        sums = rs.sums(q)
        assert sums[T + 2 + 1] == 0.0 and sums[T + 2 + 3] == 0.0  # W0 of the empty group and of the group without follow-up
        _, _, g = _terms(lib, rs, q, sums)
        for k in (1, 3):
            assert g[T + 4 + k] == -q[T + 4 + k] / R.PRIORS[6] ** 2  # exactly -z_g / a_z_sd^2


def test_layout_sorts_by_group_and_pads_to_whole_tiles(lib):
    for N, T, Gr in R.SHAPES:
        group = R.make_groups(N, T, Gr).astype(np.int32)
        slot = np.empty(N, dtype=np.int32)
        tile_group = np.full((N + 63) // 64 + Gr, -1, dtype=np.int32)
        group_tile = np.empty(Gr + 1, dtype=np.int32)
        ntile = lib.survival_groups_layout(N, Gr, group.ctypes.data, slot.ctypes.data, tile_group.ctypes.data, group_tile.ctypes.data)
        sizes = np.bincount(group, minlength=Gr)
        assert ntile == ((sizes + 63) // 64).sum() and ntile <= len(tile_group)
        np.testing.assert_array_equal(np.diff(group_tile), (sizes + 63) // 64)  # an empty group has no tile
        assert group_tile[0] == 0 and group_tile[Gr] == ntile and (tile_group[ntile:] == -1).all()
        np.testing.assert_array_equal(tile_group[:ntile], np.repeat(np.arange(Gr), (sizes + 63) // 64))
        assert len(set(slot.tolist())) == N and slot.min() >= 0 and slot.max() < ntile * 64
        np.testing.assert_array_equal(tile_group[slot // 64], group)  # every individual sits in a tile of its group
        for g in range(Gr):
            mine = slot[group == g]
            np.testing.assert_array_equal(mine, group_tile[g] * 64 + np.arange(len(mine)))  # stable, packed from the group's first column
