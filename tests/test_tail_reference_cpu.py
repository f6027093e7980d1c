"""
The 40-digit reference of tests/mp_reference.py and its committed results (tests/golden/tail_parity.npz), without a GPU:

* the fixture is what the generator writes today (needs mpmath; everything else here does not);
* the reference is right where the float64 oracle can tell: O.logp_dlogp agrees within E_ORACLE u S_k at every output it
  returns finite, and the literal (G, G, N) form on logp at the typical points;
* the outputs the oracle does NOT return finite are listed, so that a change of the oracle shows up here;
* the case table reaches the regimes it is there for (a condition on the inputs, read from the stored extremes of t);
* abd_terms.hpp, serial and per-lane form, fed with the reference's sums, returns the reference's logp and gradient within the
  device budget C u S_k at every case -- sigmoid, softplus, the priors, the b = 0 guard and the HX scaling on the host side.

S_k is the sum of the absolute values of all addends of output k: an error relative to the VALUE cannot be asked for in the
tails, where the oracle's own is 0.61 on a gradient entry that cancels (b = -40, perm = e^3).
"""
import ctypes as C
import math
import os
import subprocess
import warnings

import numpy as np
import pytest

from oracle import abd_oracle as O
from tests import mp_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (set, storage, case) -> the outputs O.logp_dlogp returns NaN for: e * s = inf * 0 in lik() wherever exp(b (a - x)) overflows.
# Its logp (entry 17) is right there.  Everywhere else the oracle is finite, the rho logit of -800 included.
_B40 = [1, 2, 3, 4, 5, 6, 10, 11, 14]
ORACLE_NOT_FINITE = {
    ("65x33", "f64", "b=+40 perm=e^3"): _B40, ("65x33", "f32", "b=+40 perm=e^3"): _B40,
    ("65x33", "f64", "b=+300"): [5, 6, 10, 14], ("65x33", "f32", "b=+300"): [5, 6, 10, 14],
    ("7x65", "f64", "b=+40 perm=e^3"): _B40, ("65x33 distinct", "f64", "b=+40 perm=e^3"): _B40,
    ("20x13", "f64", "b=+40 perm=e^3"): _B40, ("sparse", "f64", "b=+40 perm=e^3"): _B40,
}


@pytest.fixture(scope="module")
def fx(golden_dir):
    return R.load_fixture(golden_dir)


def _all_cases():
    for name, (_, _, f32) in R.SETS.items():
        cases = R.set_cases(name)
        for st in ("f64", "f32") if f32 else ("f64",):
            for c, (cname, theta, i_raw, w, coh) in enumerate(cases):
                yield name, st, c, cname, theta, i_raw, w, (R.rounded_to_f32(coh) if st == "f32" else coh)


def test_the_fixture_is_what_the_generator_writes(fx):
    pytest.importorskip("mpmath")
    import multiprocessing
    from concurrent.futures import ProcessPoolExecutor

    from tests.golden import make_tail_fixtures as M

    # the parts side by side in fresh processes (a minute and a quarter of mpmath in one): the two halves of the full table first
    new = {}
    with ProcessPoolExecutor(max_workers=4, mp_context=multiprocessing.get_context("spawn")) as pool:
        for arrays in pool.map(M.generate_part, M.parts()):
            new.update(arrays)
    assert sorted(new) == sorted(fx)
    for k, v in new.items():
        assert v.dtype == fx[k].dtype and v.shape == fx[k].shape, k
        assert v.tobytes() == fx[k].tobytes(), k  # bit for bit, the signs of zeros included


def test_the_rebuilt_inputs_are_the_ones_the_references_were_made_on(fx):
    from tests.golden.make_tail_fixtures import case_check

    for name, st, c, cname, theta, i_raw, w, coh in _all_cases():
        assert fx[f"{name}.names"][c] == cname
        assert theta.tobytes() == fx[f"{name}.{st}.theta"][c].tobytes(), (name, cname)
        np.testing.assert_array_equal(case_check(i_raw, w, coh), fx[f"{name}.{st}.check"][c], err_msg=f"{name} {cname}")


def test_the_oracle_agrees_wherever_it_is_finite_and_where_it_is_not_is_pinned(fx):
    worst, where, not_finite = 0.0, None, {}
    for name, st, c, cname, theta, i_raw, w, coh in _all_cases():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # overflow in exp, invalid value in multiply: the cases pinned above
            lp, g = O.logp_dlogp(theta, i_raw, w, coh)
        got, ref, S = np.append(g, lp), fx[f"{name}.{st}.ref"][c], fx[f"{name}.{st}.S"][c]
        assert np.isfinite(ref).all() and np.isfinite(S).all() and (S > 0).all(), (name, cname)
        bad = np.flatnonzero(~np.isfinite(got)).tolist()
        if bad:
            not_finite[(name, st, cname)] = bad
        ok = np.isfinite(got)
        ratio = np.abs(got[ok] - ref[ok]) / (R.U * S[ok])
        if ratio.max() > worst:
            worst, where = float(ratio.max()), (name, st, cname, int(np.flatnonzero(ok)[ratio.argmax()]))
        if cname in ("base", "truth"):  # the literal (G, G, N) form, logp only
            lit = O.joint_logp(theta, i_raw, w, coh, dense=True)
            assert abs(lit - ref[17]) <= R.E_ORACLE * R.U * S[17], (name, st, cname, lit, ref[17])
    print(f"\nE_oracle measured: {worst:.1f} u S_k at {where}; E_ORACLE = {R.E_ORACLE}, C = {R.C_BUDGET}, C u = {R.C_BUDGET * R.U:.2e}")
    assert worst <= R.E_ORACLE <= 64.0
    assert R.C_BUDGET == 32.0 * R.E_ORACLE and R.C_BUDGET * R.U <= 1e-12
    assert not_finite == ORACLE_NOT_FINITE


def test_the_table_reaches_the_regimes(fx):
    t = np.concatenate([fx[k] for k in sorted(fx) if k.endswith(".t_ext")])
    tmin, tmax, tabs = t[:, 0], t[:, 1], t[:, 2]
    assert np.any((tmax > 510.0) & (tmax < 1021.0))  # between the dense kernels' clamp and the list kernels'
    assert np.any(tmax > 1021.0)
    assert np.any(tmin < -1022.0)
    assert np.any((tabs < 2.0 ** -40) & (tabs > 0.0)) and np.any(tabs == 0.0)  # b = 1e-300, and b = 0 itself
    # every set of the short table too: the observation lists and the per-reading kernels have clamps of their own
    for name in R.SETS:
        te = fx[f"{name}.f64.t_ext"]
        assert np.any((te[:, 1] > 510.0) & (te[:, 1] < 1021.0)) and np.any(te[:, 1] > 1021.0) and np.any(te[:, 0] < -1022.0), name


@pytest.fixture(scope="module")
def terms(tmp_path_factory):
    out = tmp_path_factory.mktemp("terms_tail") / "libterms_harness.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-fvisibility-inlines-hidden", "-Wl,-Bsymbolic", "-I", os.path.join(ROOT, "abdpymc_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "terms_harness.cpp"), "-o", str(out)])
    lib = C.CDLL(str(out))
    dp = C.POINTER(C.c_double)
    lib.terms_compare_const.argtypes = [dp, dp, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_double, dp, dp, dp, dp]
    lib.terms_compare_const.restype = C.c_int
    return lib


def prior_constant(G):
    """abd_context.hip: prior_constant, restated"""
    v = -(math.lgamma(1.0) + math.lgamma(G - 1.0) - math.lgamma(float(G))) - 2.0 * (math.lgamma(10.0) + math.lgamma(1.0) - math.lgamma(11.0))
    for mu in (2.0, 1.0, 2.0, 1.0, 1.0):
        al, be = mu * mu / 0.25, mu / 0.25
        v += al * math.log(be) - math.lgamma(al)
    for sd in (1.0, 1.0, 0.5, 0.5, 0.5, 0.5):
        v += -math.log(sd) - 0.5 * math.log(2.0 * math.pi)
    return v


@pytest.mark.parametrize("dense", [0, 1])
def test_abd_terms_on_the_references_sums(fx, terms, dense):
    """Both forms of abd_terms.hpp on the host, fed the reference's sums rounded to float64; dense = 1: HX scaled by
    c = 1024 log2(e) b as the dense kernel returns it (b = 0: by the guard's 1e-300), which the terms divide back."""
    dp = C.POINTER(C.c_double)
    kC = 1024.0 / math.log(2.0)
    worst = 0.0
    for name, st, c, cname, theta, i_raw, w, coh in _all_cases():
        ref, S, sums = fx[f"{name}.{st}.ref"][c], fx[f"{name}.{st}.S"][c], fx[f"{name}.{st}.sums"][c].copy()
        if dense:
            for hx, kb in ((5, 11), (11, 14)):  # A_N_HX, A_S_HX
                sums[hx] *= kC * (theta[kb] if theta[kb] != 0.0 else 1e-300)
        G, N = coh.n_gaps, coh.n_inds
        lp_s, lp_l, g_s, g_l = C.c_double(), C.c_double(), np.empty(17), np.empty(17)
        th = np.ascontiguousarray(theta, dtype=np.float64)
        rc = terms.terms_compare_const(th.ctypes.data_as(dp), sums.ctypes.data_as(dp), G, float(N), float(coh.n.od.size), float(coh.s.od.size),
                                       dense, prior_constant(G), C.byref(lp_s), g_s.ctypes.data_as(dp), C.byref(lp_l), g_l.ctypes.data_as(dp))
        assert rc == 0, (name, cname)
        for form, got in (("serial", np.append(g_s, lp_s.value)), ("lanes", np.append(g_l, lp_l.value))):
            assert np.isfinite(got).all(), (name, st, cname, form, got)
            ratio = np.abs(got - ref) / (R.U * S)
            worst = max(worst, float(ratio.max()))
            assert ratio.max() <= R.C_BUDGET, (name, st, cname, form, int(ratio.argmax()), float(ratio.max()), got, ref)
    print(f"\nabd_terms.hpp on the reference's sums, dense = {dense}: worst error {worst:.1f} u S_k (budget {R.C_BUDGET})")
