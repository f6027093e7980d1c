"""
Per-individual timelines without a GPU (abdpymc_amd/timelines.py; include/abd_hip.h: abd_sampler_enable_timelines): from_draws,
merge and quantiles on hand-made draws whose answers follow from the definition by hand, compute_chunked_cum_p, the exact
cumulative probability against the clipped sum of the marginals, and the kernel's bin rule, chunk mask and quantile compiled for
the CPU (tests/native/timeline_harness.cpp) as a stand-alone program, plain and under the sanitizers, against the NumPy side.
"""
import os
import subprocess

import numpy as np
import pytest

from abdpymc_amd import timelines as tl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "native", "timeline_harness.cpp")
INCLUDES = ["-I", os.path.join(ROOT, "abdpymc_amd", "csrc")]
LO, HI = -4.0, 8.0
W = (HI - LO) / 62


def _draws(i_cols, n_cols=None, s_cols=None):
    """(1, D, G, 1) arrays of one chain and one individual from per-draw rows over the gaps"""
    i = np.asarray(i_cols, dtype=np.int8)[None, :, :, None]
    n = np.zeros(i.shape) if n_cols is None else np.asarray(n_cols, dtype=np.float64)[None, :, :, None]
    s = np.zeros(i.shape) if s_cols is None else np.asarray(s_cols, dtype=np.float64)[None, :, :, None]
    return i, n, s


def test_bins_by_hand():
    x = np.array([-np.inf, -4.0 - 1e-12, -4.0, -4.0 + W / 2, -4.0 + 1.5 * W, 0.0, 8.0 - 1e-12, 8.0, 9.0, np.inf, np.nan])
    # 0.0 is (0 + 4) / w = 20.67 bins in: interior bin 20, counter 21
    assert tl.bins(x, LO, HI).tolist() == [0, 0, 1, 1, 2, 21, 62, 63, 63, 63, 63]
    with pytest.raises(ValueError):
        tl.bins(x, 1.0, 1.0)
    with pytest.raises(ValueError):
        tl.bins(x, 0.0, np.inf)


def test_a_cell_that_alternates_between_two_values():
    """ten draws, titer -1 in the even ones and 5 in the odd ones: counters 16 (= 1 + floor(3 / w) = 1 + 15) and 47 (= 1 + floor(9 / w)
    = 1 + 46) hold 5 each; t = q n = 0.25, 5, 9.75 fall into the first, the first (C = 5 >= 5) and the second mode"""
    D = 10
    x = np.where(np.arange(D) % 2 == 0, -1.0, 5.0)[:, None]
    i, n, s = _draws(np.zeros((D, 1)), x, x + 100.0)
    r = tl.from_draws(i, n, s, ((LO, HI), (LO, HI)))
    h = r["tl_hist_n"][0, 0, 0]
    assert r["tl_hist_n"].dtype == np.uint16 and r["tl_hist_n"].shape == (1, 1, 1, 64)
    assert h[16] == 5 and h[47] == 5 and h.sum() == D
    assert r["tl_hist_s"][0, 0, 0, 63] == D  # everything above the range: overflow
    q = tl.quantiles(h, (0.025, 0.5, 0.975), LO, HI)
    want = [LO + W * (15 + 0.25 / 5), LO + W * (15 + 5 / 5), LO + W * (46 + (9.75 - 5) / 5)]
    np.testing.assert_allclose(q, want, rtol=0, atol=4 * np.finfo(float).eps * 8)
    assert q[0] < -1.0 + W and q[2] > 5.0 - W  # the band spans both modes: what mean +- sd cannot show
    assert tl.quantiles(r["tl_hist_s"][0, 0, 0], (0.5,), LO, HI).tolist() == [HI]


def test_quantile_edge_cases():
    c = np.zeros(64, dtype=np.int64)
    assert np.isnan(tl.quantiles(c, (0.0, 0.5, 1.0), LO, HI)).all()  # n = 0
    c[0], c[30], c[63] = 4, 2, 4
    q = tl.quantiles(c, (0.0, 0.4, 0.5, 0.6, 0.61, 1.0), LO, HI)
    # t = 0, 4, 5, 6, 6.1, 10: bin 0 (C = 4 >= t) gives lo; bin 30 interpolates; bin 63 gives hi
    assert q[0] == LO and q[1] == LO and q[4] == HI and q[5] == HI
    assert q[2] == LO + W * (29 + (5 - 4) / 2) and q[3] == LO + W * (29 + (6 - 4) / 2)
    # a stack of histograms, an empty one among them; q = 0 skips empty leading bins
    many = np.stack([c, np.zeros(64, dtype=np.int64), np.eye(64, dtype=np.int64)[7] * 3])
    out = tl.quantiles(many, (0.0, 1.0), LO, HI)
    assert out.shape == (2, 3) and np.isnan(out[:, 1]).all()
    assert out[0, 2] == LO + W * 6 and out[1, 2] == LO + W * 7
    with pytest.raises(ValueError):
        tl.quantiles(c, (1.5,), LO, HI)
    with pytest.raises(ValueError):
        tl.quantiles(c.astype(float), (0.5,), LO, HI)
    with pytest.raises(ValueError):
        tl.quantiles(c[:63], (0.5,), LO, HI)


def test_infection_counters_by_hand():
    #          gap 0  1  2  3  4
    rows = [[0, 1, 0, 0, 1],   # infected at 1 and again at 4
            [0, 0, 0, 1, 0],
            [0, 0, 0, 0, 0],
            [1, 0, 0, 0, 0]]
    i, n, s = _draws(rows)
    r = tl.from_draws(i, n, s)
    assert r["tl_inf"][0, :, 0].tolist() == [1, 1, 0, 1, 1]
    assert r["tl_cum"][0, :, 0].tolist() == [1, 2, 2, 3, 3]           # one chunk
    assert r["tl_ninf"][0, 0].tolist() == [1, 2, 1, 0, 0, 0, 0, 0]    # draws with 0, 1, 2 infections
    assert r["tl_info"].tolist() == [[4]] and r["tl_info"].dtype == np.int64
    r2 = tl.from_draws(i, n, s, splits=(2,))                          # chunks {0, 1}, {2, 3, 4}
    assert r2["tl_cum"][0, :, 0].tolist() == [1, 2, 0, 1, 2]
    r3 = tl.from_draws(i, n, s, splits=(2, 4))                        # chunks {0, 1}, {2, 3}, {4}
    assert r3["tl_cum"][0, :, 0].tolist() == [1, 2, 0, 1, 1]
    # follow-up to gap 3: the second infection of draw 0 is not counted; never followed: the row stays 0; the planes ignore it
    r4 = tl.from_draws(i, n, s, last_gap=[3])
    assert r4["tl_ninf"][0, 0].tolist() == [1, 3, 0, 0, 0, 0, 0, 0]
    np.testing.assert_array_equal(r4["tl_cum"], r["tl_cum"])
    assert tl.from_draws(i, n, s, last_gap=[-1])["tl_ninf"].sum() == 0
    # 7 and more are pooled
    i9, n9, s9 = _draws(np.ones((2, 9)))
    assert tl.from_draws(i9, n9, s9)["tl_ninf"][0, 0].tolist() == [0, 0, 0, 0, 0, 0, 0, 2]
    with pytest.raises(ValueError):
        tl.from_draws(i, n, s, splits=(3, 2))
    with pytest.raises(ValueError):
        tl.from_draws(i[0], n, s)


def test_merge_is_the_sum_over_chains_and_parts():
    rng = np.random.default_rng(5)
    i = (rng.random((3, 12, 7, 4)) < 0.2).astype(np.int8)
    n, s = rng.normal(1, 3, i.shape), rng.normal(2, 4, i.shape)
    last = np.array([6, 3, -1, 0])
    whole = tl.from_draws(i, n, s, splits=(3,), last_gap=last)
    parts = [tl.from_draws(i[:1], n[:1], s[:1], splits=(3,), last_gap=last), tl.from_draws(i[1:], n[1:], s[1:], splits=(3,), last_gap=last)]
    a, b = tl.merge(whole), tl.merge(parts)
    assert a["draws"] == b["draws"] == 36
    for k in ("inf", "cum", "ninf", "hist_n", "hist_s"):
        np.testing.assert_array_equal(a[k], b[k])
        assert a[k].dtype == np.int64
    np.testing.assert_array_equal(a["hist_n"].sum(axis=-1), np.full((7, 4), 36))
    # pooled over the chains the histogram is that of all draws as one chain
    flat = tl.from_draws(i.reshape(1, 36, 7, 4), n.reshape(1, 36, 7, 4), s.reshape(1, 36, 7, 4), splits=(3,), last_gap=last)
    np.testing.assert_array_equal(a["hist_s"], flat["tl_hist_s"][0])
    np.testing.assert_array_equal(a["cum"], flat["tl_cum"][0])
    with pytest.raises(ValueError, match="timelines"):
        tl.merge({"i": i})
    # summary and individual read either
    sm = tl.summary(whole, last)
    np.testing.assert_array_equal(sm["p_inf"], i.mean(axis=(0, 1)))
    assert sm["ab_n_mu"]["median"].shape == (7, 4) and (sm["ab_n_mu"]["lower"] <= sm["ab_n_mu"]["upper"]).all()
    np.testing.assert_allclose(sm["n_infections"][[0, 1, 3]].sum(axis=1), 1.0)
    assert np.isnan(sm["n_infections"][2]).all()
    one = tl.individual(whole, 1, last)
    assert one["gaps"].tolist() == [0, 1, 2, 3] and one["ab_s_mu"].shape == (3, 4) and one["cum_p"].shape == (4,)
    np.testing.assert_array_equal(one["cum_p"], sm["cum_p"][:4, 1])
    assert tl.individual(whole, 2, last)["gaps"].size == 0
    assert tl.line(sm).startswith("timelines: ")
    assert tl.result_bytes(2, 7, 4) == 2 * (16 * 28 + 64 * 4) + 2 * 3 * 8 * 28
    assert tl.result_bytes(2, 7, 4, hist=True) - tl.result_bytes(2, 7, 4) == 2 * 256 * 28


def test_compute_chunked_cum_p():
    p = np.array([0.5, 0.4, 0.3])
    np.testing.assert_allclose(tl.compute_chunked_cum_p(p), [0.5, 0.9, 1.0], rtol=0, atol=1e-15)
    np.testing.assert_allclose(tl.compute_chunked_cum_p(p, splits=(2,)), [0.5, 0.9, 0.3], rtol=0, atol=1e-15)
    np.testing.assert_allclose(tl.compute_chunked_cum_p(p, splits=(1, 2)), p, rtol=0, atol=0)
    with pytest.raises(ValueError, match="p is not 1D"):
        tl.compute_chunked_cum_p(np.zeros((2, 3)))


def test_exact_cum_against_the_clipped_sum():
    # under splits, on draws with at most one infection per chunk, the clipped sum of the marginals IS the exact value
    rng = np.random.default_rng(9)
    D, G, splits = 40, 9, (3, 6)
    i = np.zeros((1, D, G, 1), dtype=np.int8)
    for d in range(D):
        for a, b in ((0, 3), (3, 6), (6, 9)):
            if rng.random() < 0.6:
                i[0, d, rng.integers(a, b), 0] = 1
    r = tl.from_draws(i, None, None, splits=splits)
    assert "tl_hist_n" not in r
    exact = r["tl_cum"][0, :, 0] / D
    approx = tl.compute_chunked_cum_p(r["tl_inf"][0, :, 0] / D, splits)
    np.testing.assert_allclose(exact, approx, rtol=0, atol=1e-12)
    assert exact.max() > 0
    # one chunk, a repeat infection: two of four draws are infected at gap 0 and the same two again at gap 1
    i = np.zeros((1, 4, 2, 1), dtype=np.int8)
    i[0, :2, :, 0] = 1
    r = tl.from_draws(i, None, None)
    exact = r["tl_cum"][0, :, 0] / 4
    approx = tl.compute_chunked_cum_p(r["tl_inf"][0, :, 0] / 4)
    assert exact.tolist() == [0.5, 0.5] and approx.tolist() == [0.5, 1.0]
    assert exact[1] < approx[1]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitizers"])
def test_native_rules_against_brute_force_and_numpy(tmp_path, sanitize):
    exe = tmp_path / "timeline_harness"
    flags = ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", *flags, "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", *INCLUDES, HARNESS, "-o", str(exe)])
    rng = np.random.default_rng(3)
    for lo, hi in ((LO, HI), (0.3, 0.9)):
        w = (hi - lo) / 62
        edges = lo + w * np.arange(63)
        x = np.concatenate([rng.normal((lo + hi) / 2, hi - lo, 500), edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf),
                            [np.nan, np.inf, -np.inf, lo, hi]])
        q = np.concatenate([[0.0, 1.0, 0.025, 0.5, 0.975], rng.random(20)])
        src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
        with open(src, "wb") as f:
            f.write(np.array([lo, hi]).tobytes() + np.array([x.size, q.size], dtype=np.int64).tobytes() + x.tobytes() + q.tobytes())
        r = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stderr == "" and "timeline ok" in r.stdout
        raw = open(dst, "rb").read()
        b = np.frombuffer(raw, dtype=np.int64, count=x.size)
        hist = np.frombuffer(raw, dtype=np.int64, count=64, offset=8 * x.size)
        got = np.frombuffer(raw, dtype=np.float64, count=q.size, offset=8 * (x.size + 64))
        np.testing.assert_array_equal(b, tl.bins(x, lo, hi))
        np.testing.assert_array_equal(hist, np.bincount(b, minlength=64))
        assert hist[0] > 0 and hist[63] > 0 and (hist[1:63] > 0).sum() > 30
        # the same formula in the same order on either side: a handful of roundings apart at most
        np.testing.assert_allclose(got, tl.quantiles(hist, q, lo, hi), rtol=0, atol=8 * np.finfo(float).eps * max(abs(lo), abs(hi)))


def test_cli_pools_gathered_histograms():
    """what rank 0 does with a result gathered from several ranks: per-chain histograms in, pooled quantiles out"""
    from abdpymc_amd import cli

    rng = np.random.default_rng(2)
    i = (rng.random((4, 9, 6, 5)) < 0.15).astype(np.int8)
    n, s = rng.normal(0, 3, i.shape), rng.normal(1, 3, i.shape)
    res = tl.from_draws(i, n, s, ((-3.0, 3.0), (-2.0, 4.0)), splits=(2,))
    res["tl_q"] = np.tile(np.array(tl.DEFAULT_Q), (4, 1))
    pooled_n = tl.merge(res)["hist_n"]
    sm = cli.add_timelines(res, np.full(5, 5))
    assert not any(k in res for k in tl.HIST_KEYS)
    np.testing.assert_array_equal(res["tl_q_n"], tl.quantiles(pooled_n, tl.DEFAULT_Q, -3.0, 3.0))
    np.testing.assert_array_equal(res["tl_summary_ab_n_mu"], res["tl_q_n"])
    np.testing.assert_array_equal(res["tl_summary_cum_p"], sm["cum_p"])
    assert set(tl.RESULT_KEYS) <= set(res)
    assert tl.line(sm).count("timelines:") == 1
    # ... and the same summary again from the pooled quantiles alone
    again = tl.summary(res, np.full(5, 5))
    np.testing.assert_array_equal(again["ab_s_mu"]["upper"], sm["ab_s_mu"]["upper"])


def test_summary_reads_the_band_from_the_levels_the_result_has():
    """a result without histograms carries the quantiles it was sampled with: summary reads the smallest level, the one nearest 0.5
    and the largest, whatever they are; one with histograms gives any levels"""
    rng = np.random.default_rng(8)
    i = (rng.random((2, 15, 4, 3)) < 0.2).astype(np.int8)
    n, s = rng.normal(0, 2, i.shape), rng.normal(1, 2, i.shape)
    full = tl.from_draws(i, n, s)
    m = tl.merge(full)
    levels = (0.9, 0.1, 0.45, 0.6)  # (in no order)
    lean = {k: v for k, v in full.items() if k not in tl.HIST_KEYS}
    lean["tl_q"] = np.tile(np.array(levels), (2, 1))
    lean["tl_q_n"] = tl.quantiles(m["hist_n"], levels, *tl.DEFAULT_RANGES[0])
    lean["tl_q_s"] = tl.quantiles(m["hist_s"], levels, *tl.DEFAULT_RANGES[1])
    assert tl.band_levels(levels) == (1, 2, 0) and tl.band_levels(tl.DEFAULT_Q) == (0, 1, 2) and tl.band_levels((0.3,)) == (0, 0, 0)
    sm = tl.summary(lean)
    assert sm["q"] == (0.1, 0.45, 0.9)
    want = tl.summary(full, q=(0.1, 0.45, 0.9))
    assert want["q"] == (0.1, 0.45, 0.9)
    for var in ("ab_n_mu", "ab_s_mu"):
        for k in ("lower", "median", "upper"):
            np.testing.assert_array_equal(sm[var][k], want[var][k])
    assert "80 % S band" in tl.line(sm) and "95 % N band" in tl.line(tl.summary(full))
    assert tl.individual(lean, 1)["ab_n_mu"].shape == (3, 4)
    with pytest.raises(ValueError, match="no histograms"):
        tl.summary(lean, q=tl.DEFAULT_Q)
    with pytest.raises(ValueError, match="no titer quantiles"):
        tl.summary({k: v for k, v in lean.items() if k != "tl_q_n"})
