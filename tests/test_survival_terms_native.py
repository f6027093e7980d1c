"""abd_survival_terms.hpp on the CPU: the host half of a survival evaluation -- lambda_t, a, b for the kernel, and logp and the
gradient from the device sums -- against the NumPy restatement given the same sums; and the rule for one cell at creation."""
import ctypes as C
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
