"""
Per-cell convergence diagnostics without a GPU (abdpymc_amd/diagnostics.py; include/abd_hip.h: abd_sampler_enable_diagnostics):
the hand case, from_draws against a direct two-pass computation and BDA3's split R-hat, the behaviour of rhat / ess on chains
whose answer is known, the merges, and the kernel's per-cell update compiled for the CPU (tests/native/diag_harness.cpp) as a
stand-alone program, plain and under the sanitizers, against from_draws.
"""
import os
import subprocess

import numpy as np
import pytest

from abdpymc_amd import diagnostics as dg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "native", "diag_harness.cpp")
INCLUDES = ["-I", os.path.join(ROOT, "abdpymc_amd", "csrc")]
EPS = 2.0 ** -52


# ---- the gates: derived, shared with tests/test_gpu_diagnostics.py ----

def mean_gate(n, xmax, delta=0.0):
    """|mean - reference| of n values bounded by xmax, each perturbed by at most delta: Welford rounding 4 n 2^-52 max|x|."""
    return delta + 4 * n * EPS * xmax


def m2_gate(n, m2, xmax, delta=0.0):
    """|M2 - reference|: a perturbation of at most delta per value moves each centred value by at most 2 delta
    (4 delta sqrt(n M2) + 4 n delta^2), plus rounding 8 n 2^-52 sqrt(M2 (M2 + n max|x|^2))."""
    return 4 * delta * np.sqrt(n * m2) + 4 * n * delta ** 2 + 8 * n * EPS * np.sqrt(m2 * (m2 + n * xmax ** 2))


def two_pass(x, L):
    """The moments of x (chains, D, ...) computed directly: np.mean / np.var per half, explicit reshaping into batches."""
    chains, D = x.shape[:2]
    H = D // 2
    B = H // L
    halves = [x[:, :H], x[:, H:2 * H]]
    out = []
    for h in halves:
        out += [h.mean(axis=1), h.var(axis=1) * H]
    bm = np.concatenate([h[:, :B * L].reshape((chains, B, L) + x.shape[2:]).mean(axis=2) for h in halves], axis=1)  # (chains, 2B, ...)
    out += [bm.mean(axis=1), bm.var(axis=1) * 2 * B]
    return np.stack(out, axis=1), bm


def check_moments(got, x, L, delta_of=lambda xmax, n: 0.0):
    """got (chains, 6, ...) against the two-pass moments of x by the gates; delta_of(max|x|, n): the per-value perturbation."""
    want, bm = two_pass(np.asarray(x, dtype=np.float64), L)
    H = x.shape[1] // 2
    nb = bm.shape[1]
    xmax, bmax = np.abs(x[:, :2 * H]).max(), np.abs(bm).max()
    for h in (0, 1):
        d = delta_of(xmax, H)
        assert (np.abs(got[:, 2 * h] - want[:, 2 * h]) <= mean_gate(H, xmax, d)).all(), f"mean of half {h}"
        assert (np.abs(got[:, 2 * h + 1] - want[:, 2 * h + 1]) <= m2_gate(H, want[:, 2 * h + 1], xmax, d)).all(), f"M2 of half {h}"
    d = delta_of(bmax, nb)
    assert (np.abs(got[:, 4] - want[:, 4]) <= mean_gate(nb, bmax, d)).all(), "bm_mean"
    assert (np.abs(got[:, 5] - want[:, 5]) <= m2_gate(nb, want[:, 5], bmax, d)).all(), "bm_M2"


def bda3_split_rhat(x):
    """Gelman et al., Bayesian Data Analysis 3rd ed., section 11.4, transcribed: x (chains, D, ...)."""
    H = x.shape[1] // 2
    psi = np.concatenate([x[:, :H], x[:, H:2 * H]], axis=0)  # m sequences of length n
    m, n = psi.shape[:2]
    psi_j = psi.mean(axis=1)
    Bv = n / (m - 1) * ((psi_j - psi_j.mean(axis=0)) ** 2).sum(axis=0)
    W = (((psi - psi_j[:, None]) ** 2).sum(axis=1) / (n - 1)).mean(axis=0)
    return np.sqrt(((n - 1) / n * W + Bv / n) / W)


# ---- 1. the hand case ----

def test_hand_case():
    x = np.array([[0.0, 1.0, 0.0, 1.0]])
    mo = dg.from_draws(x, 1)
    m = mo["moments"][0]
    assert m[0] == 0.5 and m[2] == 0.5          # the half means
    assert m[1] == 0.5 and m[3] == 0.5          # W = mean of M2_h / (H - 1) = 1/2
    assert m[5] == 1.0                          # bm_M2 of the batch means 0, 1, 0, 1
    assert mo["info"].tolist() == [[2, 2, 4, 1]]
    assert dg.rhat(mo) == pytest.approx(np.sqrt(0.5), abs=1e-15)
    assert dg.ess(mo) == pytest.approx(4.0, abs=1e-15)
    # the integer path of i
    mi = dg.from_draws(x.astype(np.int8), 1)
    assert mi["counts"][0].tolist() == [1, 1, 2, 2] and mi["counts"].dtype == np.int64
    assert abs(dg.rhat(mi) - dg.rhat(mo)) <= 1e-15
    assert abs(dg.ess(mi) - dg.ess(mo)) <= 1e-15
    e, se = dg.ess(mo, with_mcse=True)
    assert se == pytest.approx(np.sqrt((1.0 / 3.0) / 4.0), abs=1e-15)


# ---- 2. from_draws against a direct two-pass computation ----

def test_from_draws_equals_a_two_pass_computation():
    rng = np.random.default_rng(5)
    x = rng.normal(1.0, 2.0, (3, 21, 5, 4))  # D odd: the last draw is ignored; H = 10, L = 3: a trailing draw in each half
    mo = dg.from_draws(x, 3)
    assert mo["info"].tolist() == [[10, 10, 6, 3]] * 3
    check_moments(mo["moments"], x, 3)
    np.testing.assert_allclose(dg.rhat(mo), bda3_split_rhat(x), rtol=0, atol=1e-12)
    # the ignored draw and the trailing draws: changing draw 20 changes nothing, changing draw 9 no batch moment
    y = x.copy()
    y[:, 20] += 100.0
    assert dg.from_draws(y, 3)["moments"].tobytes() == mo["moments"].tobytes()
    y = x.copy()
    y[:, 9] += 100.0
    my = dg.from_draws(y, 3)["moments"]
    assert my[:, 4:].tobytes() == mo["moments"][:, 4:].tobytes() and (my[:, 0] != mo["moments"][:, 0]).all()
    # counts are exact
    b = rng.random((3, 21, 5, 4)) < 0.3
    mi = dg.from_draws(b.astype(np.int8), 3)
    H, B, L = 10, 3, 3
    halves = [b[:, :H], b[:, H:2 * H]]
    cb = np.concatenate([h[:, :B * L].reshape(3, B, L, 5, 4).sum(axis=2) for h in halves], axis=1)
    want = np.stack([halves[0].sum(axis=1), halves[1].sum(axis=1), cb.sum(axis=1), (cb * cb).sum(axis=1)], axis=1)
    np.testing.assert_array_equal(mi["counts"], want)
    np.testing.assert_array_equal(dg.from_draws(b, 3)["counts"], want)  # booleans are integers here
    np.testing.assert_allclose(dg.rhat(mi), bda3_split_rhat(b.astype(np.float64)), rtol=0, atol=1e-12)
    np.testing.assert_allclose(dg.ess(mi), dg.ess(dg.from_draws(b.astype(np.float64), 3)), rtol=1e-12)


def test_argument_errors():
    with pytest.raises(ValueError):
        dg.from_draws(np.zeros((2, 1)), 1)
    with pytest.raises(ValueError):
        dg.from_draws(np.zeros((2, 8)), 0)
    with pytest.raises(ValueError):
        dg.from_draws(np.zeros(8), 1)
    with pytest.raises(ValueError, match="diag_i_counts"):
        dg.summary({})
    assert dg.default_batch(21) == 3 and dg.default_batch(2) == 1 and dg.default_batch(20000) == 100
    assert dg.result_bytes(4, 200, 10000) == 4 * 16 * 8 * 2000000


# ---- 3. behaviour on chains whose answer is known ----

def test_rhat_tells_mixed_chains_from_a_shifted_one():
    """Four iid chains: below 1.01.  One chain of a pair shifted by two standard deviations: the half means are 0, 0, 2, 2, so
    B_over_H -> 4/3 and rhat -> sqrt(1 + 4/3) = 1.53 > 1.5.  With one of FOUR chains shifted the half means are six 0s and two
    2s, B_over_H -> 6/7 and rhat -> sqrt(13/7) = 1.363: it cannot pass 1.5, so that case is held to its own limit."""
    rng = np.random.default_rng(2024)
    x = rng.standard_normal((4, 20000, 6))
    r = dg.rhat(dg.from_draws(x, 100))
    assert (r < 1.01).all() and (r > 0.99).all()
    pair = x[:2].copy()
    pair[1] += 2.0
    r2 = dg.rhat(dg.from_draws(pair, 100))
    assert (r2 > 1.5).all() and (np.abs(r2 - np.sqrt(7.0 / 3.0)) < 0.03).all()
    x[3] += 2.0
    r4 = dg.rhat(dg.from_draws(x, 100))
    assert (r4 > 1.1).all() and (np.abs(r4 - np.sqrt(13.0 / 7.0)) < 0.03).all()


def test_constant_cells_are_nan_and_frozen_halves_are_inf():
    x = np.zeros((2, 8, 3))
    x[:, :, 0] = 1.5                 # constant
    x[:, 4:, 1] = 1.0                # constant within every half, the halves differ
    x[:, :, 2] = np.arange(8) % 3    # an ordinary cell
    for mo in (dg.from_draws(x, 2), dg.from_draws(x[:, :, 1:].astype(np.int64), 2)):
        r = dg.rhat(mo)
        if "moments" in mo:
            assert np.isnan(r[0]) and np.isinf(r[1]) and np.isfinite(r[2])
            assert np.isnan(dg.ess(mo)[0])  # no variance of the batch means
        else:
            assert np.isinf(r[0]) and np.isfinite(r[1])


# D, L and the seed were chosen here on the CPU: 4 chains x 200 batches = 800 batches, so the estimator's relative standard
# deviation is sqrt(2 / 800) = 0.05.  The run gives ess / n = 1.0563 for the iid chains and 0.0605 for AR(1) with phi = 0.9 (the
# limit is (1 - phi) / (1 + phi) = 0.0526; batches of 100 against an autocorrelation time of 19 bias it upwards): 0.8 x 1.0563 =
# 0.845 > 0.7 and 1.2 x 0.0605 = 0.0726 < 0.1, both 4 standard deviations inside.
def test_ess_of_an_autoregression_is_lower():
    rng = np.random.default_rng(31)
    chains, D, L, phi = 4, 20000, 100, 0.9
    z = rng.standard_normal((chains, D))
    ar = np.empty_like(z)
    ar[:, 0] = z[:, 0]
    for t in range(1, D):
        ar[:, t] = phi * ar[:, t - 1] + np.sqrt(1 - phi * phi) * z[:, t]
    n = chains * D
    iid = float(dg.ess(dg.from_draws(z, L))) / n
    dep = float(dg.ess(dg.from_draws(ar, L))) / n
    print(f"ess / n: iid {iid:.4f}, AR(1) {dep:.4f}")
    rel = 4 * np.sqrt(2.0 / (chains * 2 * (D // 2 // L)))
    assert iid * (1 - rel) > 0.7
    assert dep * (1 + rel) < 0.1


# ---- 4. merges and the summary ----

def _result(x_i, x_n, x_s, L):
    return {"diag_i_counts": dg.from_draws(x_i, L)["counts"], "diag_ab_n_mu": dg.from_draws(x_n, L)["moments"],
            "diag_ab_s_mu": dg.from_draws(x_s, L)["moments"], "diag_info": dg.from_draws(x_i, L)["info"]}


def test_merges_and_summary():
    rng = np.random.default_rng(9)
    G, N, D, L = 5, 7, 40, 4
    xi = (rng.random((4, D, G, N)) < 0.4).astype(np.int8)
    xi[:, :, 0, 0] = 0                                   # a constant cell
    xn, xs = rng.normal(0, 1, (4, D, G, N)), rng.normal(2, 3, (4, D, G, N))
    xs[3, :, 2, 5] += 50.0                               # a followed cell one chain disagrees about
    whole = _result(xi, xn, xs, L)
    merged = dg.merge_chains([_result(xi[:2], xn[:2], xs[:2], L), _result(xi[2:], xn[2:], xs[2:], L)])
    for k in dg.RESULT_KEYS:
        assert merged[k].tobytes() == whole[k].tobytes() and merged[k].shape == whole[k].shape, k
    shards = dg.merge_individual_shards([_result(xi[..., :3], xn[..., :3], xs[..., :3], L), _result(xi[..., 3:], xn[..., 3:], xs[..., 3:], L)])
    for k in dg.RESULT_KEYS:
        assert shards[k].tobytes() == whole[k].tobytes(), k
    last = np.array([4, 4, 2, -1, 0, 4, 3])
    from abdpymc_amd.model import THETA_NAMES

    res = dict(whole)
    res[THETA_NAMES[0]] = rng.normal(0, 1, (4, D))
    res["stat_lp"] = rng.normal(0, 1, (4, D))
    sm = dg.summary(res, last_gap=last)
    assert sm["i"]["rhat"].shape == (G, N) and sm["ab_s_mu"]["ess"].shape == (G, N) and sm["ab_n_mu"]["sd"].shape == (G, N)
    assert sm["i"]["n_constant"] == 1 and np.isnan(sm["i"]["rhat"][0, 0])
    assert sm["i"]["followed"]["n_cells"] == int((np.arange(G)[:, None] <= last[None, :]).sum())
    assert sm["ab_s_mu"]["worst_cells"][0].tolist() == [2, 5] and sm["ab_s_mu"]["max_rhat"] == sm["ab_s_mu"]["rhat"][2, 5] > 1.5
    assert sm["ab_s_mu"]["followed"]["max_rhat"] == sm["ab_s_mu"]["rhat"][2, 5] and sm["ab_s_mu"]["n_rhat_above_1.1"] >= 1
    assert sm["i"]["followed"]["n_constant"] == 1 and sm["ab_n_mu"]["followed"]["n_constant"] == 0
    assert set(sm["scalars"]) == {THETA_NAMES[0], "lp"} and np.isfinite(sm["scalars"]["lp"]["ess"])
    np.testing.assert_allclose(sm["ab_n_mu"]["sd"], xn.reshape(-1, G, N).std(axis=0, ddof=1), rtol=1e-12)
    e = sm["ab_n_mu"]["ess"]
    at = sm["ab_n_mu"]["min_ess_cell"]
    assert e[at] == np.nanmin(e) == sm["ab_n_mu"]["min_ess"]
    arrays = dg.summary_arrays(sm)
    assert arrays["diag_summary_i_rhat"].shape == (G, N) and arrays["diag_summary_scalars"].shape == (3, 2)


# ---- 5. the kernel's per-cell update on the CPU ----

def _replay(exe, tmp_path, x, bits, L):
    D, C = x.shape
    src, dst = tmp_path / "draws.bin", tmp_path / "moments.bin"
    with open(src, "wb") as f:
        f.write(np.array([D, L, C], dtype=np.int64).tobytes() + np.ascontiguousarray(x, dtype=np.float64).tobytes()
                + np.ascontiguousarray(bits, dtype=np.uint8).tobytes())
    r = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "" and "diag ok" in r.stdout
    raw = open(dst, "rb").read()
    m = np.frombuffer(raw, dtype=np.float64, count=6 * C).reshape(6, C)
    c = np.frombuffer(raw, dtype=np.int64, count=4 * C, offset=48 * C).reshape(4, C)
    info = np.frombuffer(raw, dtype=np.int64, count=4, offset=80 * C)
    return m, c, info


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitizers"])
def test_native_update_reproduces_from_draws(tmp_path, sanitize):
    exe = tmp_path / "diag_harness"
    flags = ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", *flags, "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", *INCLUDES, HARNESS, "-o", str(exe)])
    rng = np.random.default_rng(77)
    for D, L in ((21, 3), (8, 2), (4, 1), (9, 5), (2, 1)):  # trailing draws, none, one-draw batches, no whole batch, one draw per half
        C = 37
        x = rng.normal(-1.0, 3.0, (D, C))
        bits = rng.random((D, C)) < 0.35
        m, c, info = _replay(exe, tmp_path, x, bits, L)
        want = dg.from_draws(x[None], L)
        want_i = dg.from_draws(bits[None].astype(np.int8), L)
        assert info.tolist() == want["info"][0].tolist()
        np.testing.assert_array_equal(c, want_i["counts"][0])
        H, nb = D // 2, 2 * (D // 2 // L)
        xmax = np.abs(x).max()
        ref = want["moments"][0]
        for h in (0, 1):
            assert (np.abs(m[2 * h] - ref[2 * h]) <= mean_gate(H, xmax)).all()
            assert (np.abs(m[2 * h + 1] - ref[2 * h + 1]) <= m2_gate(H, ref[2 * h + 1], xmax)).all()
        assert (np.abs(m[4] - ref[4]) <= mean_gate(nb, xmax)).all()
        assert (np.abs(m[5] - ref[5]) <= m2_gate(nb, ref[5], xmax)).all()
        if D >= 4 and nb >= 2:
            check_moments(m[None], x[None], L)
