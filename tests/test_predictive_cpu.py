"""
Posterior predictive checks without a GPU: the stream of the replicates' normals (abd_hip.h: abd_posterior_predictive) restated
in numpy against the C oracle's Philox4x32-10, the merge rules and summary of abdpymc_amd.predictive, and the CLI /
record-budget / output plumbing of the two options.
"""
import math
import sys

import numpy as np
import pytest

from abdpymc_amd import predictive, synthetic
from oracle import c_oracle
from tests.helpers import oracle_cohort_from_synth

M32 = np.uint64(0xFFFFFFFF)


def philox_np(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 over arrays of counters (uint32 words held in uint64) -> the four output words."""
    c = [np.asarray(v, dtype=np.uint64) & M32 for v in (c0, c1, c2, c3)]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = np.uint64(k0) & M32, np.uint64(k1) & M32
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return c


def stream_uniforms(seed, stream, draw, antigen, r):
    """u1, u2 of caller readings r (array) of one antigen: the counter and the 53-bit uniforms of abd_readings.hpp: Predictive."""
    r = np.asarray(r, dtype=np.uint64)
    c3 = 0x80000000 | (antigen << 30) | ((draw >> 32) & 0x3FFFFFFF)
    w = philox_np(r, stream, draw & 0xFFFFFFFF, c3, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)

    def u(a, b):
        return (((a >> np.uint64(5)) << np.uint64(26) | (b >> np.uint64(6))).astype(np.float64) + 0.5) * 2.0 ** -53

    return u(w[0], w[1]), u(w[2], w[3])


def stream_normals(seed, stream, draw, antigen, r):
    """z of caller readings r of one antigen (Box-Muller of the first uniform pair)."""
    u1, u2 = stream_uniforms(seed, stream, draw, antigen, r)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


@pytest.fixture(scope="module")
def co():
    return c_oracle.COracle(oracle_cohort_from_synth(synthetic.make_cohort(3, 4, seed=1)))


def test_philox_np_known_answers_and_random_counters(co):
    # Random123 kat_vectors, philox4x32-10 (as tests/test_gibbs.py)
    for args, want in (((0, 0, 0, 0, 0, 0), [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]),
                       (([0xFFFFFFFF] * 6), [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]),
                       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0),
                        [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1])):
        assert [int(v) for v in philox_np(*args)] == want == co.philox(*args)
    rng = np.random.default_rng(0)
    c = rng.integers(0, 2 ** 32, size=(4, 200), dtype=np.uint64)
    for k0, k1 in ((0, 0), (0xDEADBEEF, 0x12345678), (2 ** 32 - 1, 7)):
        got = philox_np(c[0], c[1], c[2], c[3], k0, k1)
        for i in range(0, 200, 7):
            want = co.philox(int(c[0, i]), int(c[1, i]), int(c[2, i]), int(c[3, i]), k0, k1)
            assert [int(g[i]) for g in got] == want


@pytest.mark.parametrize("seed,stream,draw,antigen", [(0, 0, 0, 0), (5, 3, 1234, 1), (2 ** 64 - 1, 2 ** 32 - 1, 2 ** 40 + 17, 0)])
def test_uniforms_and_normals_as_specified(co, seed, stream, draw, antigen):
    r = np.arange(0, 3000, 37)
    u1, u2 = stream_uniforms(seed, stream, draw, antigen, r)
    z = stream_normals(seed, stream, draw, antigen, r)
    for i in range(0, r.size, 5):
        c3 = 0x80000000 | (antigen << 30) | ((draw >> 32) & 0x3FFFFFFF)
        w = co.philox(int(r[i]), stream, draw & 0xFFFFFFFF, c3, seed & 0xFFFFFFFF, seed >> 32)
        a = ((w[0] >> 5) * 2 ** 26 + (w[1] >> 6) + 0.5) * 2.0 ** -53
        b = ((w[2] >> 5) * 2 ** 26 + (w[3] >> 6) + 0.5) * 2.0 ** -53
        assert u1[i] == a and u2[i] == b and 0.0 < a < 1.0 and 0.0 < b < 1.0
        assert z[i] == math.sqrt(-2.0 * math.log(a)) * math.cos(2.0 * math.pi * b)


def test_normals_are_standard_and_keys_separate_them():
    r = np.arange(200000)
    z = stream_normals(11, 2, 7, 0, r)
    assert abs(z.mean()) < 4 / math.sqrt(r.size) and abs(z.std() - 1.0) < 4 / math.sqrt(2 * r.size)
    assert abs(np.mean(z ** 4) - 3.0) < 0.05
    for other in (stream_normals(12, 2, 7, 0, r), stream_normals(11, 3, 7, 0, r), stream_normals(11, 2, 8, 0, r),
                  stream_normals(11, 2, 7, 1, r), stream_normals(11, 2, 7 + 2 ** 32, 0, r)):
        assert abs(np.corrcoef(z, other)[0, 1]) < 0.02 and not np.any(z == other)


@pytest.mark.parametrize("splits", [(37,), (1, 20, 16), (5, 5, 5, 5, 17)])
def test_merge_over_uneven_splits_equals_whole_matrix(splits):
    rng = np.random.default_rng(len(splits))
    K = 257
    m = 0.5 + rng.standard_normal((sum(splits), K)) * rng.uniform(0.01, 2.0, K)
    pit = rng.uniform(0.0, 1.0, m.shape)
    parts, lo = [], 0
    for s in splits:
        parts.append(predictive.stats_from_matrix(m[lo:lo + s], pit[lo:lo + s]))
        lo += s
    mean, m2, p, n = predictive.merge(*parts)
    assert n == m.shape[0]
    np.testing.assert_allclose(mean, m.mean(axis=0), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(m2, ((m - m.mean(axis=0)) ** 2).sum(axis=0), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(p, pit.mean(axis=0), rtol=1e-12, atol=1e-12)
    # an empty chain is neutral on either side
    e = predictive.stats_from_matrix(m[:0], pit[:0])
    for got in (predictive.merge(e, *parts), predictive.merge(*parts, e)):
        np.testing.assert_allclose(got[0], mean, rtol=1e-15)
        assert got[3] == n


def _welford(m, pit):
    """the accumulator update of the predictive kernel, draw by draw"""
    mean = m2 = pm = None
    for n, (x, p) in enumerate(zip(m, pit), start=1):
        if n == 1:
            mean, m2, pm = x.copy(), np.zeros_like(x), p.copy()
            continue
        d = x - mean
        mean = mean + d / n
        m2 = m2 + d * (x - mean)
        pm = pm + (p - pm) / n
    return mean, m2, pm, m.shape[0]


def test_summary_equals_direct_numpy():
    rng = np.random.default_rng(7)
    chains, draws, K_s, K_n = 3, 40, 50, 30
    m = 0.8 + 0.1 * rng.standard_normal((chains, draws, K_s + K_n))
    pit = rng.beta(0.3, 0.3, m.shape)
    res = {"it_s_sigma": rng.uniform(0.05, 0.2, (chains, draws)), "it_n_sigma": rng.uniform(0.05, 0.2, (chains, draws)),
           "ppc_n_obs": np.tile([K_s, K_n], (chains, 1))}
    st = [_welford(m[c], pit[c]) for c in range(chains)]
    for j, name in enumerate(("ppc_mean", "ppc_m2", "ppc_pit")):
        res[name] = np.stack([s[j] for s in st])
    res["ppc_n_draws"] = np.array([s[3] for s in st])
    sm = predictive.summary(res)
    assert sm["n_draws"] == chains * draws
    flat_m, flat_p = m.reshape(-1, K_s + K_n), pit.reshape(-1, K_s + K_n)
    for name, sl, sig in (("it_s_lik", slice(0, K_s), "it_s_sigma"), ("it_n_lik", slice(K_s, None), "it_n_sigma")):
        a = sm[name]
        sd = np.sqrt(flat_m[:, sl].var(axis=0) + np.mean(res[sig] ** 2))
        p = flat_p[:, sl].mean(axis=0)
        np.testing.assert_allclose(a["mean"], flat_m[:, sl].mean(axis=0), rtol=1e-12)
        np.testing.assert_allclose(a["sd"], sd, rtol=1e-12)
        np.testing.assert_allclose(a["p"], p, rtol=1e-12)
        assert a["n_low"] == int((p < 0.025).sum()) and a["n_high"] == int((p > 0.975).sum())
        assert a["n_extreme"] == a["n_low"] + a["n_high"] and a["share_extreme"] == a["n_extreme"] / p.size
        assert a["hist"].shape == (20,) and a["hist"].sum() == p.size
        assert list(a["hist"]) == [int(((p >= b / 20) & ((p < (b + 1) / 20) | (b == 19))).sum()) for b in range(20)]


def test_cli_parser_accepts_the_flags():
    from abdpymc_amd.cli import build_parser

    a = build_parser().parse_args(["--tune", "1", "--draws", "1", "--ppc", "--posterior_predictive"])
    assert a.ppc and a.posterior_predictive
    b = build_parser().parse_args(["--tune", "1", "--draws", "1"])
    assert not b.ppc and not b.posterior_predictive


def test_record_bytes_counts_the_matrix():
    from abdpymc_amd.sampler import record_bytes

    assert record_bytes(4, 100, 31, 1520, False, False, n_replicates=35709) == 4 * 100 * 35709 * 8
    assert record_bytes(2, 10, 3, 5, True, True, n_readings=7, n_replicates=7) == \
        record_bytes(2, 10, 3, 5, True, True, n_readings=7) + 2 * 10 * 7 * 8
    assert record_bytes(2, 10, 3, 5, True, True) == record_bytes(2, 10, 3, 5, True, True, n_replicates=0)


def test_host_sampler_refuses_the_options():
    from abdpymc_amd.sampler import sample

    class _M:
        n_chains = 1
        ctx = None

    for kw in ({"posterior_predictive": True}, {"ppc": True}):
        with pytest.raises(ValueError, match="native sampler"):
            sample(_M(), tune=1, draws=1, native=False, **kw)


def test_write_posterior_npz_carries_the_keys(tmp_path, monkeypatch):
    from abdpymc_amd import cli

    monkeypatch.setitem(sys.modules, "arviz", None)  # the .npz path, whether ArviZ is installed or not
    rng = np.random.default_rng(1)
    res = {"it_s_b": rng.standard_normal((2, 3)), "stat_lp": rng.standard_normal((2, 3)),
           "posterior_predictive_it_s_lik": rng.standard_normal((2, 3, 5)),
           "posterior_predictive_it_n_lik": rng.standard_normal((2, 3, 4)),
           "ppc_mean": rng.standard_normal((2, 9)), "ppc_m2": rng.random((2, 9)), "ppc_pit": rng.random((2, 9)),
           "ppc_n_draws": np.array([3, 3]), "ppc_n_obs": np.array([[5, 4], [5, 4]]),
           "ppc_p_it_s_lik": rng.random(5), "ppc_p_it_n_lik": rng.random(4),
           "observed_data_it_s_lik": rng.random(5), "observed_data_it_n_lik": rng.random(4)}
    out = cli.write_posterior(res, str(tmp_path / "post.npz"), {"gap": np.arange(2), "ind": np.arange(3)})
    z = np.load(out)
    for k, v in res.items():
        np.testing.assert_array_equal(z[k], v)
