"""
The cohort simulator without a GPU: the parameter classes' validation, the library's argument errors, the step function of
abd_simulate.hpp compiled for the CPU (tests/native/simulate_harness.cpp) against the NumPy restatement
(tests/sim_restatement.py), the same harness under the sanitizers, and the restatement against the known answers of the
reference's own tests (abdpymc/test_simulation.py:190-356).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from abdpymc_amd import simulation as sim
from tests import sim_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "native", "simulate_harness.cpp")
INCLUDES = ["-I", os.path.join(ROOT, "tests", "native", "fake_hip"), "-I", os.path.join(ROOT, "abdpymc_amd", "csrc")]
WALK_FIELDS = ("protect_a", "protect_b", "init", "perm_rise", "temp_rise_i", "temp_rise_v", "temp_wane")  # SimWalkAb's order


# ---- 1. parameter validation and method errors ----

@pytest.mark.parametrize("make,field", [
    (lambda: sim.Protection(b=0.0), "b"), (lambda: sim.Protection(b=-1.0), "b"), (lambda: sim.Protection(a=float("inf")), "a"),
    (lambda: sim.Elisa(b=0.0), "b"), (lambda: sim.Elisa(b=1.0), "b"), (lambda: sim.Elisa(d=0.0), "d"), (lambda: sim.Elisa(sd=0.0), "sd"),
    (lambda: sim.Elisa(sd=float("nan")), "sd"),
    (lambda: sim.Dynamics(perm_rise=-0.1), "perm_rise"), (lambda: sim.Dynamics(temp_rise_i=-1.0), "temp_rise_i"),
    (lambda: sim.Dynamics(temp_rise_v=-1.0), "temp_rise_v"), (lambda: sim.Dynamics(temp_wane=1.5), "temp_wane"),
    (lambda: sim.Dynamics(temp_wane=0.0), "temp_wane"), (lambda: sim.Dynamics(init=float("nan")), "init"),
    (lambda: sim.Dynamics(init="x"), "init"),
])
def test_parameter_classes_validate_and_name_the_field(make, field):
    with pytest.raises(ValueError, match=rf"\b{field}\b"):
        make()


def test_parameter_classes_defaults_unknown_fields_and_p_protection():
    assert sim.Antibodies().as_native() == R.default_params()
    assert sim.Dynamics(temp_wane=1.0).temp_wane == 1.0 and sim.Dynamics(perm_rise=0).perm_rise == 0.0
    for cls in (sim.Protection, sim.Elisa, sim.Dynamics, sim.Antibody, sim.Antibodies):
        with pytest.raises((TypeError, ValueError)):
            cls(nonsense=1.0)
    with pytest.raises(ValueError, match="protection"):
        sim.Antibody(protection=sim.Elisa())
    p = sim.Protection(a=0.5, b=2.0)
    assert p.p_protection(0.5) == 0.5
    np.testing.assert_allclose(p.p_protection(np.array([-1.0, 2.0])), 1 / (1 + np.exp(-2.0 * (np.array([-1.0, 2.0]) - 0.5))), rtol=0)


def test_lam0_errors_are_the_references():
    with pytest.raises(ValueError, match="lam0 should be 1D"):
        sim.check_lam0(np.zeros((2, 3)), 3)
    with pytest.raises(ValueError, match="must have single infection rate for each time gap"):
        sim.check_lam0(np.zeros(4), 3)
    assert sim.check_lam0([0.1, 0.2, 0.3], 3).dtype == np.float64


def test_cohort_wants_exactly_one_source():
    with pytest.raises(ValueError, match="exactly one"):
        sim.Cohort(1)
    with pytest.raises(ValueError, match="antibodies"):
        sim.Cohort(1, "nowhere", antibodies=None)


def test_null_context_and_params_fail_without_a_device():
    from abdpymc_amd import _native

    lib = _native.load()
    lam = np.zeros(4)
    p = _native._SimParams()
    assert lib.abd_simulate(None, C.byref(p), lam.ctypes.data, 0, 0, 1, None, None, None, None, None, None) == -1
    assert b"ctx is NULL" in lib.abd_last_error()
    assert lib.abd_simulate_staged(None, C.byref(p), lam.ctypes.data, 0, 0, 1, 0, None, None, None, None, None, None) == -1
    assert lib.abd_simulate(C.c_void_p(1), None, lam.ctypes.data, 0, 0, 1, None, None, None, None, None, None) == -1
    assert b"params is NULL" in lib.abd_last_error()


def test_cli_parser():
    a = sim.build_parser().parse_args(["--cohort_data", "d", "--lam0", "0.04", "--seed", "42", "--replicate", "3", "--out", "o"])
    assert (a.cohort_data, a.lam0, a.seed, a.replicate, a.out) == ("d", [0.04], 42, 3, "o")


# ---- 2. the native step function against the restatement ----

@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = tmp_path_factory.mktemp("simulate") / "libsimulate_harness.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", *INCLUDES, HARNESS, "-o", str(out)])
    lib = C.CDLL(str(out))
    P = C.c_void_p
    lib.sim_walk_keyed.argtypes = [P, P, P, P, C.c_int, C.c_int, C.c_uint64, C.c_uint32, C.c_uint32, P, P, P]
    lib.sim_walk_injected.argtypes = [P, P, P, P, C.c_int, C.c_int, P, P, P, P, P, P]
    lib.sim_od_row.argtypes = [C.c_double, C.c_double, C.c_double, P, P, P, C.c_int, P]
    for f in (lib.sim_walk_keyed, lib.sim_walk_injected, lib.sim_od_row):
        f.restype = None
    return lib


def random_params(rng):
    def ab():
        return dict(protect_a=rng.normal(0.0, 1.5), protect_b=rng.uniform(0.2, 3.0), elisa_b=-rng.uniform(0.5, 3.0),
                    elisa_d=rng.uniform(0.5, 2.5), elisa_sd=rng.uniform(0.01, 0.3), init=rng.normal(-2.0, 1.0),
                    perm_rise=rng.uniform(0.0, 3.0), temp_rise_i=rng.uniform(0.0, 3.0), temp_rise_v=rng.uniform(0.0, 3.0),
                    temp_wane=rng.uniform(0.5, 1.0))
    return {"s": ab(), "n": ab()}


def walk_par(params):
    return np.array([params[ag][f] for ag in ("s", "n") for f in WALK_FIELDS])


@pytest.mark.parametrize("G", [5, 63, 64, 65, 300])
def test_native_step_function_equals_the_restatement(harness, G):
    rng = np.random.default_rng(G)
    N = 200
    params = random_params(rng)
    lam0 = rng.uniform(0.0, 0.3, G)
    vacs = (rng.random((N, G)) < 2.0 / G).astype(np.int8)
    pcr = (rng.random((N, G)) < 1.0 / G).astype(np.int8)
    par = walk_par(params)
    seed, rho, off = int(rng.integers(0, 2 ** 63)) * 2 + 1, 2 ** 31 + G, 2 ** 32 - 100  # the individual's index wraps at 2^32
    for pcrpos in (pcr, None):
        inf, s, n = np.empty((N, G), np.int8), np.empty((N, G)), np.empty((N, G))
        harness.sim_walk_keyed(par.ctypes.data, lam0.ctypes.data, vacs.ctypes.data, None if pcrpos is None else pcrpos.ctypes.data,
                               N, G, seed, rho, off, inf.ctypes.data, s.ctypes.data, n.ctypes.data)
        want = R.simulate(params, lam0, vacs, pcrpos, seed, rho, ind_offset=off)
        assert want["margin"] > 1e-9
        assert np.array_equal(inf, want["infections"])
        np.testing.assert_allclose(s, want["s_titer"], rtol=1e-13, atol=0)
        np.testing.assert_allclose(n, want["n_titer"], rtol=1e-13, atol=0)
        assert 0 < inf.sum() < inf.size
        # ... and with injected uniforms
        u = [rng.random((N, G)) for _ in range(3)]
        harness.sim_walk_injected(par.ctypes.data, lam0.ctypes.data, vacs.ctypes.data, None if pcrpos is None else pcrpos.ctypes.data,
                                  N, G, u[0].ctypes.data, u[1].ctypes.data, u[2].ctypes.data, inf.ctypes.data, s.ctypes.data, n.ctypes.data)
        w_inf, w_s, w_n, margin = R.walk(params, lam0, vacs, pcrpos, *u)
        assert margin > 1e-9
        assert np.array_equal(inf, w_inf)
        np.testing.assert_allclose(s, w_s, rtol=1e-13, atol=0)
        np.testing.assert_allclose(n, w_n, rtol=1e-13, atol=0)
    K = 500
    x, titer, z = rng.choice([0.0, 1.0, 2.0, 4.0], K), rng.normal(0.0, 2.0, K), rng.standard_normal(K)
    od = np.empty(K)
    e = params["s"]
    harness.sim_od_row(e["elisa_b"], e["elisa_d"], e["elisa_sd"], x.ctypes.data, titer.ctypes.data, z.ctypes.data, K, od.ctypes.data)
    np.testing.assert_allclose(od, R.od(e, x, titer, z), rtol=1e-13, atol=1e-15)


# ---- 3. the same harness as a stand-alone program under the sanitizers ----

def test_harness_is_clean_under_the_sanitizers(tmp_path):
    exe = tmp_path / "simulate_harness"
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-DSIM_HARNESS_MAIN", *INCLUDES, HARNESS, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == ""
    assert "simulate ok" in r.stdout


# ---- 4. known answers of the reference's own tests, on the restatement ----

@pytest.mark.parametrize("case", R.KNOWN_ANSWERS, ids=[c[0] for c in R.KNOWN_ANSWERS])
def test_known_answers_of_the_reference(case):
    _, s_over, n_over, vacs, pcrpos, infections, titers = case
    out = R.simulate(R.known_params(s_over, n_over), np.zeros(5), np.array([vacs]), np.array([pcrpos]), seed=7, rho=0)
    assert out["infections"][0].tolist() == infections
    assert out["n_infected"].tolist() == infections
    for ag, gap, want in titers:
        assert out[ag + "_titer"][0, gap] == pytest.approx(want, abs=1e-7), (ag, gap)  # assertAlmostEqual's 7 places
