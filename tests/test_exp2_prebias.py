"""The dense kernels form the high word of 2^(j/1024) 2^e as entry[kc & 1023].hi + (kc << 10) from a PRE-BIASED table and a k
clamped once (abd_types.hpp).  Swept here on the CPU against the earlier form, hi(T[k & 1023]) + (clamp(k >> 10) << 20):

* every k inside the clamp, [-1022 * 1024, 510 * 1024 + 1023]: the same bits;
* k outside it, down to -1023 * 1024, up to 511 * 1024 and at the saturated ends of v_cvt_i32_f64: the exponent is the
  clamped one as before and the entry is that of the bound (j = 0 below, j = 1023 above) -- the earlier form kept k & 1023
  there, so the mantissas differ by design; such a term is below 2^-1021 or at least 2^510 either way.
"""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_MIN, K_MAX = -1022 * 1024, 510 * 1024 + 1023


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("exp2") / "libexp2_harness.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-fvisibility-inlines-hidden", "-Wl,-Bsymbolic", "-I", os.path.join(ROOT, "abdpymc_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "exp2_harness.cpp"), "-o", str(out)])
    lib = C.CDLL(str(out))
    for f in (lib.exp2_hi_plain, lib.exp2_hi_prebiased):
        f.argtypes = [C.c_int]
        f.restype = C.c_uint32
    lib.exp2_first_difference.argtypes = [C.c_int, C.c_int]
    lib.exp2_first_difference.restype = C.c_longlong
    lib.exp2_low_words_kept.restype = C.c_int
    for f in (lib.exp2_inverse_prebiased, lib.exp2_inverse_plain):
        f.argtypes = [C.c_int]
        f.restype = C.c_uint64
    return lib


def test_same_high_word_for_every_k_inside_the_clamp(lib):
    assert lib.exp2_low_words_kept() == 1
    assert lib.exp2_first_difference(K_MIN, K_MAX) == K_MAX + 1


def test_the_sweep_is_not_idle(lib):
    # just below the clamp the earlier form keeps k & 1023 and the new one reads the bound's entry
    assert lib.exp2_first_difference(K_MIN - 1024, K_MAX) == K_MIN - 1023
    assert lib.exp2_hi_plain(0) == 0x3FF00000 and lib.exp2_hi_plain(1024) == 0x40000000


def test_outside_the_clamp_the_exponent_is_the_clamped_one(lib):
    ks = list(range(-1023 * 1024, K_MIN)) + list(range(K_MAX + 1, 511 * 1024 + 1))
    ks += [-2 ** 31, -2 ** 31 + 1, 2 ** 31 - 1, 2 ** 31 - 1024, -2 ** 30, 2 ** 30]  # v_cvt_i32_f64 saturates to the first and third
    for k in ks:
        bound = K_MIN if k < K_MIN else K_MAX
        got = lib.exp2_hi_prebiased(k)
        assert got == lib.exp2_hi_plain(bound), k  # the bound's entry, the bound's exponent
        assert (got >> 20) == (lib.exp2_hi_plain(k) >> 20) == 0x3FF + (-1022 if k < K_MIN else 510), k


def test_the_sweeps_backward_read_of_the_table(lib):
    """2^(-j/1024) for the log of the acceptance uniform (abd_gibbs_dense.hpp: log_uniform_u32): the entry of k = -j, scaled,
    has the bits of T[1024 - j] / 2 (1 for j = 0, 1/2 for j = 1024)"""
    for j in range(0, 1025):
        assert lib.exp2_inverse_prebiased(j) == lib.exp2_inverse_plain(j), j
    assert lib.exp2_inverse_prebiased(0) == 0x3FF0000000000000 and lib.exp2_inverse_prebiased(1024) == 0x3FE0000000000000
