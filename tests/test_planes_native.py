"""The exposure planes of the dense gap loop (abd_planes.hpp, plain C++) on the CPU: the reference transpose against a
bit-by-bit definition, and the plane form's exposure bookkeeping stepped against the legacy form's per-lane OR chain."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "planes_harness.cpp")
INC = os.path.join(ROOT, "abdpymc_amd", "csrc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = tmp_path_factory.mktemp("planes") / "libplanes_harness.so"
    # (no contraction: the harness compares std::fma against std::fma; -Bsymbolic as in test_nuts_native.py)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-fvisibility-inlines-hidden", "-Wl,-Bsymbolic",
                           "-I", INC, SRC, "-o", str(out)])
    lib = C.CDLL(str(out))
    u64p, u8p, dp = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.POINTER(C.c_double)
    lib.planes_transpose.argtypes = [u64p, C.c_int, C.c_int, C.c_int, u64p]
    lib.planes_transpose.restype = C.c_longlong
    lib.planes_gaps.argtypes = [C.c_int]
    lib.planes_index.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    lib.planes_index.restype = C.c_longlong
    lib.planes_exposure_check.argtypes = [u8p, u8p, C.c_int, C.c_int, dp, dp]
    lib.planes_exposure_check.restype = C.c_longlong
    return lib


def _pack(bits):
    """bits (G, N) 0/1 -> words [nt][N], word t of individual j = gaps 64 t .. 64 t + 63"""
    G, N = bits.shape
    nt = (G + 63) // 64
    w = np.zeros((nt, N), dtype=np.uint64)
    for g in range(G):
        w[g >> 6] |= bits[g].astype(np.uint64) << np.uint64(g & 63)
    return w


# full, empty and random tiles; ragged at the last lane group (N % 64 in {1, 63}) and at the last word (G % 64 in {1, 33})
@pytest.mark.parametrize("N,G", [(64, 64), (128, 128), (65, 65), (127, 97), (1, 1), (129, 33), (191, 257)])
@pytest.mark.parametrize("fill", ["zeros", "ones", "random"])
def test_transpose_against_the_bit_by_bit_definition(harness, N, G, fill):
    rng = np.random.default_rng(N * 1000 + G)
    bits = {"zeros": np.zeros((G, N), np.uint8), "ones": np.ones((G, N), np.uint8), "random": (rng.random((G, N)) < 0.3).astype(np.uint8)}[fill]
    words = np.ascontiguousarray(_pack(bits))
    n_lg, Gp = (N + 63) // 64, harness.planes_gaps(G)
    assert Gp % 2 == 0 and Gp >= G + 2  # pairs of gaps are aligned; the loop fetches one pair ahead
    u64p = C.POINTER(C.c_uint64)
    for which in (0, 1):
        sentinel = np.uint64(0xA5A5A5A5A5A5A5A5)
        planes = np.full(n_lg * Gp * 2, sentinel, dtype=np.uint64)
        n_words = harness.planes_transpose(words.ctypes.data_as(u64p), N, G, which, planes.ctypes.data_as(u64p))
        assert n_words == planes.size
        p = planes.reshape(n_lg, Gp, 2)
        assert harness.planes_index(n_lg - 1, G - 1, G, which) == ((n_lg - 1) * Gp + G - 1) * 2 + which
        assert np.all(p[:, :, which ^ 1] == sentinel)  # the other masks are not this transpose's
        assert np.all(p[:, G:, which] == sentinel)     # nor are the padding gaps (the slot zeroes them once)
        padded = np.zeros((G, n_lg * 64), np.uint8)
        padded[:, :N] = bits
        for lg in range(n_lg):
            for g in range(G):
                mask = int(p[lg, g, which])
                got = np.array([(mask >> l) & 1 for l in range(64)], np.uint8)
                np.testing.assert_array_equal(got, padded[g, lg * 64:(lg + 1) * 64], err_msg=f"lg {lg} gap {g}")


K = np.array([float.fromhex("0x1.23456789abcdep+9"), float.fromhex("-0x1.fedcba9876543p+10"), float.fromhex("0x1.0f0f0f0f0f0f1p+8"), -0.0])


def _check(harness, inf, vac, g0, k=K):
    G = inf.shape[0]
    inf, vac = np.ascontiguousarray(inf, np.uint8), np.ascontiguousarray(vac, np.uint8)
    out = np.empty((G - g0, 64, 4))
    u8p, dp = C.POINTER(C.c_uint8), C.POINTER(C.c_double)
    bad = harness.planes_exposure_check(inf.ctypes.data_as(u8p), vac.ctypes.data_as(u8p), G, g0, k.ctypes.data_as(dp), out.ctypes.data_as(dp))
    # ... and against the definition in numpy: exposed = any exposure in gaps <= g (the gap of first exposure counts, abd.py:306)
    seen_n = np.cumsum(inf, axis=0)[g0:] > 0
    seen_s = np.cumsum(inf | vac, axis=0)[g0:] > 0
    np.testing.assert_array_equal(out[..., 0], seen_n.astype(float))
    np.testing.assert_array_equal(out[..., 1], seen_s.astype(float))  # a vaccination exposes S ...
    assert np.all(out[..., 0] <= out[..., 1])                        # ... but not N
    np.testing.assert_array_equal(out[..., 2], np.where(seen_n, k[0] + k[1], k[1]))  # (one rounding either way)
    assert bad == 0
    return out


@pytest.mark.parametrize("G", [1, 2, 33, 65, 130])
def test_exposure_bookkeeping_random_histories(harness, G):
    rng = np.random.default_rng(G)
    for dens in (0.0, 0.005, 0.03, 0.3):
        inf = rng.random((G, 64)) < dens
        vac = rng.random((G, 64)) < dens / 2
        for g0 in sorted({0, 1, 31, 32, 63, 64, G // 2, G - 1}):
            if g0 < G:
                _check(harness, inf, vac, g0)


def test_exposure_bookkeeping_adversarial_histories(harness):
    G = 130
    z = np.zeros((G, 64), bool)
    # first exposure at gap 0, at a piece's own g0, at gaps 31 / 32 / 63 / 64 (one lane each, the rest never exposed)
    for g_first in (0, 31, 32, 63, 64, G - 1):
        inf = z.copy()
        inf[g_first, g_first % 64] = True
        for g0 in sorted({0, g_first, max(0, g_first - 1), min(G - 1, g_first + 1)}):
            out = _check(harness, inf, z, g0)
            assert out[..., 0].sum() == max(0, G - max(g0, g_first)) if g0 <= g_first else out[..., 0].sum() == G - g0
    # vaccination before the first infection: S exposed from the dose on, N from the infection on
    inf, vac = z.copy(), z.copy()
    vac[10, 5] = True
    inf[40, 5] = True
    for g0 in (0, 10, 11, 40, 41):
        out = _check(harness, inf, vac, g0)
        assert out[max(0, 10 - g0):, 5, 1].all() and not out[:max(0, 10 - g0), 5, 1].any()
        assert out[max(0, 40 - g0):, 5, 0].all() and not out[:max(0, 40 - g0), 5, 0].any()
    # never exposed; everyone in every gap; infection and dose in the same gap
    _check(harness, z, z, 0)
    _check(harness, ~z, ~z, 0)
    _check(harness, ~z, z, 64)
    both = z.copy()
    both[32, :] = True
    for g0 in (0, 32, 33):
        _check(harness, both, both, g0)
    # every lane first exposed in another gap (a refresh in every gap), doses one gap earlier
    inf, vac = z.copy(), z.copy()
    for l in range(64):
        inf[2 * l + 1, l] = True
        vac[2 * l, l] = True
    for g0 in (0, 1, 64, 65, 127):
        _check(harness, inf, vac, g0)
    # signed zeros and specials in the constants: the refreshed base is fma(1.0, c perm, c init), the initial one fma(0.0, ...)
    for k in (np.array([-1.5, -0.0, 2.5, 0.0]), np.array([0.0, -0.0, -0.0, -0.0]), np.array([np.inf, 1.0, -np.inf, 2.0])):
        G2 = 8
        inf2 = np.zeros((G2, 64), np.uint8)
        inf2[3, ::2] = 1
        out = np.empty((G2, 64, 4))
        u8p, dp = C.POINTER(C.c_uint8), C.POINTER(C.c_double)
        assert harness.planes_exposure_check(inf2.ctypes.data_as(u8p), inf2.ctypes.data_as(u8p), G2, 0, k.ctypes.data_as(dp), out.ctypes.data_as(dp)) == 0


def test_stand_alone_program_under_host_sanitizers(tmp_path):
    exe = tmp_path / "planes_harness"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-DPLANES_HARNESS_MAIN", "-I", INC, SRC, "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "planes harness ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
