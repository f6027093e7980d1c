"""abd_survival_terms.hpp on the CPU: the host half of a survival evaluation -- lambda_t, a, b for the kernel, and logp and the
gradient from the device sums -- against the NumPy restatement given the same sums; the rule for one cell at creation; and the
planes, Y_t and C that creation makes of the caller's arrays, in the ungrouped and in the grouped layout."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from tests import survival_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("survival") / "libsurvival_harness.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror", "-I",
                           os.path.join(ROOT, "abdpymc_amd", "csrc"), os.path.join(ROOT, "tests", "native", "survival_harness.cpp"),
                           "-o", str(out)])
    lib = C.CDLL(str(out))
    lib.survival_terms.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_double] + [C.c_void_p] * 4
    lib.survival_cell.argtypes = [C.c_int, C.c_void_p, C.c_char_p, C.c_int]
    lib.survival_planes.argtypes = [C.c_int] * 3 + [C.c_void_p] * 5 + [C.c_int] * 2 + [C.c_void_p] * 5 + [C.c_char_p, C.c_int]
    return lib


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("name", R.POINTS)
def test_host_terms_equal_the_restatement(lib, K, name):
    N, T = 67, 30
    rs = R.Restatement(*R.make_data(N, T, K))
    q = R.make_point(name, T, K)
    sums = rs.sums(q)
    lp_ref, g_ref = rs.combine(q, sums)
    pri = np.array(R.PRIORS[K])
    par, g, lp = np.empty(T + 2 * K), np.empty(rs.dim), C.c_double()
    D = lib.survival_terms(K, T, pri.ctypes.data, q.ctypes.data, rs.Y.ctypes.data, rs.C, sums.ctypes.data, par.ctypes.data,
                           C.addressof(lp), g.ctypes.data)
    assert D == rs.dim
    a, b, m, s, z = rs.split(q)
    # two libraries' exp (each within 1 ulp), one addition and one division each: a few u
    np.testing.assert_allclose(par[:T], R._invlogit(m + np.exp(s) * z), rtol=1e-15, atol=0)
    np.testing.assert_array_equal(par[T:], q[:2 * K])
    assert np.isfinite(lp.value) and np.isfinite(g).all()
    # the same closed form in another order of additions: a few roundings of the largest addend
    assert abs(lp.value - lp_ref) <= 1e-13 * max(1.0, abs(lp_ref), np.abs(sums).max())
    np.testing.assert_allclose(g, g_ref, rtol=1e-12, atol=1e-13 * max(1.0, np.abs(g_ref).max()))


def test_cell_rule(lib):
    def cell(K, *v):
        c = np.array(v, dtype=np.float64)
        msg = C.create_string_buffer(128)
        rc = lib.survival_cell(K, c.ctypes.data, msg, 128)
        return rc, c, msg.value.decode()

    nan, inf = np.nan, np.inf
    assert cell(1, 0.25, 0.5, 3.0)[:1] == (0,) and list(cell(1, 0.25, 0.5, 3.0)[1]) == [0.25, 0.5, 3.0]
    for v in ((nan, 0.5, 3.0), (0.25, nan, 3.0), (nan, nan, nan), (0.0, 0.0, inf)):  # no follow-up: y = e = x = 0
        rc, c, _ = cell(1, *v)
        assert rc == 0 and list(c) == [0.0, 0.0, 0.0]
    assert list(cell(2, nan, 1.0, 2.0, nan)[1]) == [0.0, 0.0, 0.0, 0.0]
    assert cell(1, 0.0, 0.5, 3.0)[0] == 0 and cell(1, 0.0, 0.5, 3.0)[1][2] == 3.0  # followed, no infection: the titer stays
    for v, word in (((-0.1, 0.5, 3.0), "negative"), ((0.1, -0.5, 3.0), "negative"), ((0.1, 0.0, 3.0), "exposure 0"),
                    ((0.1, 0.5, nan), "titer"), ((0.0, 0.5, inf), "titer"), ((inf, 0.5, 3.0), "finite"), ((0.1, inf, 3.0), "finite")):
        rc, _, msg = cell(1, *v)
        assert rc == 1 and word in msg, (v, msg)
    assert cell(2, 0.1, 0.5, 3.0, -inf)[0] == 1


def _pack(lib, y, e, xs, ld, group=None, Gr=0):
    """(ld, planes (4, T, ld) = y, e, x0, x1 (NaN where the library wrote nothing), Y, C, slot), or (0, (j, t), message)."""
    N, T = y.shape
    y, e = np.ascontiguousarray(y), np.ascontiguousarray(e)
    xs = [np.ascontiguousarray(x) for x in xs]
    planes, Y, Csum = np.full((4, T, ld), np.nan), np.full(T, np.nan), C.c_double()
    slot, bad, msg = np.full(N, -1, np.int32), np.full(2, -1, np.int32), C.create_string_buffer(128)
    g = None if group is None else np.ascontiguousarray(group, dtype=np.int32)
    got = lib.survival_planes(N, T, len(xs), y.ctypes.data, e.ctypes.data, xs[0].ctypes.data, xs[1].ctypes.data if len(xs) > 1 else None,
                              None if g is None else g.ctypes.data, Gr, ld, planes.ctypes.data, Y.ctypes.data, C.addressof(Csum),
                              slot.ctypes.data, bad.ctypes.data, msg, 128)
    if got == 0:
        return 0, (int(bad[0]), int(bad[1])), msg.value.decode()
    return got, planes, Y, Csum.value, slot


def _pack_data(N, T, K, seed):
    """y in multiples of 1/4 (every partial sum of Y_t is exact), e > 0 wherever y > 0, cells without exposure, NaN cells."""
    rng = np.random.default_rng([seed, N, T, K])
    y = rng.integers(0, 6, size=(N, T)) / 4.0 * (rng.random((N, T)) < 0.6)
    e = rng.uniform(0.1, 2.0, size=(N, T))
    e[(rng.random((N, T)) < 0.2) & (y == 0)] = 0.0  # no exposure, y = 0
    xs = [rng.uniform(-1.0, 6.0, size=(N, T)) for _ in range(K)]
    y[rng.random((N, T)) < 0.1] = np.nan           # NaN in y alone, ...
    e[rng.random((N, T)) < 0.1] = np.nan           # ... in e alone, in both
    for x in xs:
        x[np.isnan(y) & (rng.random((N, T)) < 0.5)] = np.nan
    return y, e, xs


def _check_planes(got, y, e, xs, ld, slot_ref):
    got_ld, planes, Y, Csum, slot = got
    N, T = y.shape
    assert got_ld == ld
    np.testing.assert_array_equal(slot, slot_ref)
    yc, ec, xc = R.clean(y, e, xs)
    pad = np.setdiff1d(np.arange(ld), slot_ref)
    assert len(pad) == ld - N
    for k, src in enumerate([yc, ec] + xc):
        want = np.zeros((T, ld))
        want[:, slot_ref] = src.T
        assert planes[k].tobytes() == want.tobytes(), k  # bit for bit, the sign of a zero included
        assert (planes[k][:, pad] == 0).all() and not np.signbit(planes[k][:, pad]).any()
    if len(xs) == 1:
        assert np.isnan(planes[3]).all()  # no second titer: nothing written
    np.testing.assert_array_equal(Y, yc.sum(axis=0))  # multiples of 1/4: exact in any order
    terms = [float(v) * math.log(float(w)) for v, w in zip(yc.ravel(), ec.ravel()) if v > 0] + [-math.lgamma(float(v) + 1.0) for v in yc.ravel()]
    # Neumaier's sum: u |sum| + O(n u^2) sum |terms|, with room
    assert abs(Csum - math.fsum(terms)) <= 2 * R.U * math.fsum(abs(v) for v in terms)
    assert any(v > 0 for v in yc.ravel())


def test_planes_of_the_identity_layout(lib):
    N, T, K, ld = 67, 3, 2, 128
    y, e, xs = _pack_data(N, T, K, 0)
    assert np.isnan(y).any() and np.isnan(e).any() and ((e == 0) & (y == 0)).any()
    y[7, 1], e[7, 1], xs[0][7, 1], xs[1][7, 1] = 0.0, 0.0, np.inf, np.nan  # no follow-up: whatever the titers hold comes back as 0
    got = _pack(lib, y, e, xs, ld)
    _check_planes(got, y, e, xs, ld, np.arange(N))
    assert got[1][2][1, 7] == 0.0 and got[1][3][1, 7] == 0.0
    y[5, 2], e[5, 2] = 0.25, 0.0  # refused; a later cell that would be refused too is not reached
    y[9, 0] = -1.0
    assert _pack(lib, y, e, xs, ld) == (0, (5, 2), "infected > 0 with exposure 0 (the likelihood is -inf for every theta)")


def test_planes_of_the_grouped_layout(lib):
    N, T, Gr, ld = 130, 2, 3, 192
    group = np.where(np.arange(N) % 13 < 3, 2, 0)  # sizes 100 / 0 / 30, interleaved: 2 + 0 + 1 tiles
    y, e, xs = _pack_data(N, T, 1, 1)
    # the columns, restated: the individuals sorted by group (stable), every group from a multiple of 64
    start = np.concatenate([[0], np.cumsum((np.bincount(group, minlength=Gr) + 63) // 64 * 64)])
    slot_ref = np.empty(N, dtype=np.int64)
    for g in range(Gr):
        members = np.flatnonzero(group == g)
        slot_ref[members] = start[g] + np.arange(len(members))
    assert start[-1] == ld
    _check_planes(_pack(lib, y, e, xs, ld, group, Gr), y, e, xs, ld, slot_ref)
    y[100, 1], e[100, 1] = 0.5, 0.0
    assert _pack(lib, y, e, xs, ld, group, Gr) == (0, (100, 1), "infected > 0 with exposure 0 (the likelihood is -inf for every theta)")
