"""The perm sums of the dense gap loop as differences of the H sums, and the S boost by selects (abd_planes.hpp: abd_hc_open,
abd_hc_close, abd_s_boost_hi; plain C++) on the CPU: one lane group walks a range of rows in pieces as a wave of the dense kernel
does, with the plane form's and the legacy form's bookkeeping side by side, against the cf-weighted sum in long double.

Bound: with n additions into H, H carries at most n u sum|h| at either end of the difference and the (at most a few) adds
and subtracts on the perm sum itself round once each: |err| <= (2 n + 3) 2^-53 sum|h|."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "hc_sum_harness.cpp")
INC = os.path.join(ROOT, "abdpymc_amd", "csrc")
U = 2.0 ** -53


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = tmp_path_factory.mktemp("hc_sum") / "libhc_sum_harness.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-fvisibility-inlines-hidden", "-Wl,-Bsymbolic",
                           "-I", INC, SRC, "-o", str(out)])
    lib = C.CDLL(str(out))
    dp, u8p, ip = C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int)
    lib.hc_sum_run.argtypes = [dp, dp, u8p, u8p, C.c_int, ip, C.c_int, u8p, u8p, dp]
    lib.hc_sum_run.restype = C.c_longlong
    lib.hc_boost_check.restype = C.c_int
    return lib


def _run(harness, h_n, h_s, inf, vac, bounds, before_i, before_v):
    """-> out [64][8] (see hc_sum_harness.cpp); asserts that the two forms of the bookkeeping give the same bits"""
    n = h_n.shape[0]
    h_n, h_s = np.ascontiguousarray(h_n, np.float64), np.ascontiguousarray(h_s, np.float64)
    inf, vac = np.ascontiguousarray(inf, np.uint8), np.ascontiguousarray(vac, np.uint8)
    before_i, before_v = np.ascontiguousarray(before_i, np.uint8), np.ascontiguousarray(before_v, np.uint8)
    b = np.ascontiguousarray(bounds, np.int32)
    assert b[0] == 0 and b[-1] == n and np.all(np.diff(b) >= 1) and before_i.shape == (len(b) - 1, 64)
    out = np.empty((64, 8))
    dp, u8p, ip = C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int)
    bad = harness.hc_sum_run(h_n.ctypes.data_as(dp), h_s.ctypes.data_as(dp), inf.ctypes.data_as(u8p), vac.ctypes.data_as(u8p), n,
                             b.ctypes.data_as(ip), len(b) - 1, before_i.ctypes.data_as(u8p), before_v.ctypes.data_as(u8p), out.ctypes.data_as(dp))
    assert bad == 0  # plane form == legacy form, bit for bit
    return out


def _assert_bound(out, n):
    bound = (2 * n + 3) * U
    worst = 0.0
    for col, tot in ((2, 4), (3, 5)):
        assert np.all(np.abs(out[:, col]) <= bound * out[:, tot]), (n, np.abs(out[:, col]).max(), bound * out[:, tot].min())
        nz = out[:, tot] > 0
        if nz.any():
            worst = max(worst, float((np.abs(out[nz, col]) / (U * out[nz, tot])).max()))
    return worst


def _h(rng, n):
    """mixed sign, magnitudes spread over e^+-2"""
    return (rng.random((n, 64)) - 0.5) * np.exp(4.0 * rng.random((n, 64)) - 2.0)


def _bounds(rng, n, P):
    P = min(P, n)
    cuts = np.sort(rng.choice(np.arange(1, n), size=P - 1, replace=False)) if P > 1 else np.array([], int)
    return np.concatenate([[0], cuts, [n]]).astype(np.int32)


@pytest.mark.parametrize("n", [1, 2, 3, 33, 64, 65, 257, 491, 500])
@pytest.mark.parametrize("P", [1, 2, 3, 4])
def test_random_ranges_against_the_long_double_sum(harness, n, P):
    rng = np.random.default_rng(1000 * n + P)
    worst = 0.0
    for dens in (0.0, 0.004, 0.05, 0.5):
        b = _bounds(rng, n, P)
        inf = rng.random((n, 64)) < dens
        vac = rng.random((n, 64)) < dens / 2
        bi = rng.random((len(b) - 1, 64)) < 0.25
        bv = rng.random((len(b) - 1, 64)) < 0.25
        out = _run(harness, _h(rng, n), _h(rng, n), inf, vac, b, bi, bv)
        worst = max(worst, _assert_bound(out, n))
    print(f"n={n} P={P}: worst {worst:.2f} u sum|h|")


@pytest.mark.parametrize("n,bounds", [(1, [0, 1]), (7, [0, 7]), (200, [0, 60, 61, 200]), (500, [0, 1, 250, 499, 500])])
def test_named_lane_histories(harness, n, bounds):
    """lane l of every piece: 0 never exposed; 1 infected before the piece; 2 vaccinated before it (S only); 3 first infection at
    the piece's first gap; 4 at its last gap; 5 vaccination only, inside the piece; 6 infection and vaccination in one gap;
    7 vaccinated first and infected later (or in the same gap, where the piece has one gap); lanes 8 .. 63 repeat them."""
    rng = np.random.default_rng(n)
    P = len(bounds) - 1
    inf, vac = np.zeros((n, 64), bool), np.zeros((n, 64), bool)
    bi, bv = np.zeros((P, 64), bool), np.zeros((P, 64), bool)
    cf_n, cf_s = np.zeros((n, 64), bool), np.zeros((n, 64), bool)  # the definition: exposed in a gap <= g of the piece, or before it
    for p in range(P):
        a, e = bounds[p], bounds[p + 1]
        mid = (a + e - 1) // 2
        for l in range(64):
            k = l % 8
            bi[p, l], bv[p, l] = k == 1, k == 2
            if k == 3:
                inf[a, l] = True
            if k == 4:
                inf[e - 1, l] = True
            if k == 5:
                vac[mid, l] = True
            if k == 6:
                inf[mid, l] = vac[mid, l] = True
            if k == 7:
                vac[a, l] = inf[e - 1, l] = True
            cf_n[a:e, l] = bi[p, l] | (np.cumsum(inf[a:e, l]) > 0)
            cf_s[a:e, l] = bi[p, l] | bv[p, l] | (np.cumsum(inf[a:e, l] | vac[a:e, l]) > 0)
    h_n, h_s = _h(rng, n), _h(rng, n)
    out = _run(harness, h_n, h_s, inf, vac, np.array(bounds), bi, bv)
    _assert_bound(out, n)
    # the harness's own reference agrees with the definition restated here (float128 where the platform has it)
    ld = np.longdouble
    ref_n = (h_n.astype(ld) * cf_n).sum(axis=0)
    ref_s = (h_s.astype(ld) * cf_s).sum(axis=0)
    bound = (2 * n + 3) * U
    assert np.all(np.abs((out[:, 0].astype(ld) - ref_n).astype(float)) <= bound * np.abs(h_n).sum(axis=0))
    assert np.all(np.abs((out[:, 1].astype(ld) - ref_s).astype(float)) <= bound * np.abs(h_s).sum(axis=0))
    # never exposed: exactly +0.0; vaccinated only: N stays exactly 0.0 while S counts
    for l in range(0, 64, 8):
        assert out[l, 0] == 0.0 and not np.signbit(out[l, 0]) and out[l, 1] == 0.0 and not np.signbit(out[l, 1])
    for l in list(range(2, 64, 8)) + list(range(5, 64, 8)):
        assert out[l, 0] == 0.0 and not np.signbit(out[l, 0])
        assert out[l, 1] != 0.0
    # exposed before every piece: the whole range counts -- HC is H, to the bound
    for l in range(1, 64, 8):
        assert abs(out[l, 0] - h_n[:, l].sum()) <= bound * np.abs(h_n[:, l]).sum()


def test_nobody_exposed_is_exactly_zero_whatever_h_is(harness):
    rng = np.random.default_rng(5)
    n = 300
    z, zb = np.zeros((n, 64), bool), np.zeros((3, 64), bool)
    for scale in (1.0, 1e300, 1e-300):
        out = _run(harness, _h(rng, n) * scale, _h(rng, n) * scale, z, z, [0, 100, 101, n], zb, zb)
        assert np.all(out[:, :2] == 0.0) and not np.signbit(out[:, :2]).any()


def test_s_boost_select_is_the_fp64_add_bit_for_bit(harness):
    assert harness.hc_boost_check() == 0


def test_stand_alone_program_under_host_sanitizers(tmp_path):
    exe = tmp_path / "hc_sum_harness"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-DHC_SUM_HARNESS_MAIN", "-I", INC, SRC, "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "hc sum harness ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
