"""abd_survival_periods_terms.hpp on the CPU: the host half of a survival evaluation by period -- lambda_t, a_t, b for the kernel,
the fold of W0_t into W0_p, and logp and the gradient from the device sums -- against the NumPy restatement given the same sums; a
period without intervals; the sizes of the form."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from tests import survival_periods_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("survival_periods") / "libsurvival_periods_harness.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror", "-I",
                           os.path.join(ROOT, "abdpymc_amd", "csrc"), os.path.join(ROOT, "tests", "native", "survival_periods_harness.cpp"),
                           "-o", str(out)])
    lib = C.CDLL(str(out))
    lib.survival_periods_terms.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_double] + [C.c_void_p] * 5
    lib.survival_periods_sizes.argtypes = [C.c_int, C.c_int, C.c_void_p]
    return lib


def _terms(lib, rs, q, sums):
    T, P = rs.T, rs.P
    pri = np.array(R.PRIORS)
    period = rs.period.astype(np.int32)
    par, gsums, g, lp = np.empty(2 * T + 1), np.empty(T + 2 + P), np.empty(rs.dim), C.c_double()
    D = lib.survival_periods_terms(T, P, period.ctypes.data, pri.ctypes.data, q.ctypes.data, rs.Y.ctypes.data, rs.C, sums.ctypes.data,
                                   par.ctypes.data, gsums.ctypes.data, C.addressof(lp), g.ctypes.data)
    assert D == rs.dim == T + P + 5
    return par, gsums, lp.value, g


@pytest.mark.parametrize("shape", [(67, 30, 3), (130, 65, 65), (67, 511, 4)])
@pytest.mark.parametrize("name", R.POINTS)
def test_host_terms_equal_the_restatement(lib, shape, name):
    N, T, P = shape
    rs, _ = R.model_of(N, T, P)
    q = R.make_point(name, T, P)
    sums = rs.sums(q)
    lp_ref, g_ref = rs.combine(q, sums)
    par, gsums, lp, g = _terms(lib, rs, q, sums)
    m, s, z, a_mu, a_sl, az, b = rs.split(q)
    # two libraries' exp (each within 1 ulp), one addition and one division each: a few u
    np.testing.assert_allclose(par[:T], R._invlogit(m + np.exp(s) * z), rtol=1e-15, atol=0)
    # a_p = a_mu + a_sd z_p: one exp, one product, one sum; the sum may cancel to the size of u (|a_mu| + a_sd |z_p|)
    a_p = a_mu + np.exp(a_sl) * az
    np.testing.assert_allclose(par[T:2 * T], a_p[rs.period], rtol=0, atol=4 * R.U * (abs(a_mu) + np.exp(a_sl) * np.abs(az).max()))
    for p in range(P):  # the expansion copies: every interval of a period reads the same bits
        assert len(set(par[T:2 * T][rs.period == p].tolist())) <= 1
    assert par[2 * T] == b
    # the fold: S_t, L, W_x pass through; W0_p is the compensated sum of its intervals in ascending t, within one rounding of the exact
    # sum of the same float64 terms
    np.testing.assert_array_equal(gsums[:T + 2], sums[:T + 2])
    for p in range(P):
        terms = sums[T + 2:][rs.period == p]
        exact = math.fsum(terms)
        assert abs(gsums[T + 2 + p] - exact) <= 2 * R.U * abs(exact) + 2 * R.U ** 2 * np.abs(terms).sum()
    assert np.isfinite(lp) and np.isfinite(g).all()
    # the same closed form in another order of additions: a few roundings of the largest addend
    assert abs(lp - lp_ref) <= 1e-13 * max(1.0, abs(lp_ref), np.abs(sums).max())
    np.testing.assert_allclose(g, g_ref, rtol=1e-12, atol=1e-13 * max(1.0, np.abs(g_ref).max()))


def test_a_period_without_intervals_sees_its_prior_alone(lib):
    N, T, P = 1000, 199, 5  # period 3 has no interval
    rs, _ = R.model_of(N, T, P)
    assert not (rs.period == 3).any()
    for name in ("typical", "a_spread", "b_plus_50"):
        q = R.make_point(name, T, P)
        _, gsums, _, g = _terms(lib, rs, q, rs.sums(q))
        assert gsums[T + 2 + 3] == 0.0 and not np.signbit(gsums[T + 2 + 3])
        assert g[T + 4 + 3] == -q[T + 4 + 3] / R.PRIORS[6] ** 2  # exactly -z_p / a_z_sd^2


def test_the_sizes_of_the_form(lib):
    for T, P in ((1, 1), (30, 3), (65, 65), (511, 4)):
        out = np.empty(6, dtype=np.int32)
        lib.survival_periods_sizes(T, P, out.ctypes.data)
        # dim, n_ab, par_stride, n_sums, out_stride, mode
        assert out.tolist() == [T + P + 5, T + 1, 2 * T + 1, 2 * T + 2, 2 * T + 2, 3]
