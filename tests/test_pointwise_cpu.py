"""
WAIC from pointwise log-likelihood statistics (abdpymc_amd.compare) and the CLI / record-budget plumbing of the pointwise
log-likelihood, without a GPU: the device's accumulator update (abd_readings.hpp: LogLik) is restated here in numpy.
"""
import numpy as np
import pytest

from abdpymc_amd import compare


def _waic_direct(ll):
    """az.waic(scale="log") written out: draws of all chains pooled, variances with ddof 0."""
    ll = ll.reshape(-1, ll.shape[-1])
    S = ll.shape[0]
    lppd = np.log(np.mean(np.exp(ll), axis=0))
    pw = np.var(ll, axis=0)
    elpd = lppd - pw
    return elpd.sum(), pw.sum(), np.sqrt(elpd.size * np.var(elpd)), elpd, pw, S


def _device_rule(ll):
    """the accumulator update of the pointwise kernel, draw by draw: running max M, S = sum exp(ll - M), Welford mean / M2"""
    M = S = mean = M2 = None
    for n, x in enumerate(ll, start=1):
        if n == 1:
            M, S, mean, M2 = x.copy(), np.ones_like(x), x.copy(), np.zeros_like(x)
            continue
        up = x > M
        S = np.where(up, S * np.exp(M - x) + 1.0, S + np.exp(np.minimum(x - M, 0.0)))
        M = np.where(up, x, M)
        d = x - mean
        mean = mean + d / n
        M2 = M2 + d * (x - mean)
    return M + np.log(S), mean, M2, ll.shape[0]


def test_waic_matches_direct_numpy():
    rng = np.random.default_rng(0)
    ll = -1.0 + 0.7 * rng.standard_normal((4, 50, 300))
    w = compare.waic_from_matrix(ll)
    e, p, se, elpd_i, pw_i, S = _waic_direct(ll)
    assert w["n_draws"] == S == 200
    np.testing.assert_allclose([w["elpd_waic"], w["p_waic"], w["se"]], [e, p, se], rtol=1e-12)
    np.testing.assert_allclose(w["elpd_i"], elpd_i, rtol=1e-12)
    np.testing.assert_allclose(w["p_waic_i"], pw_i, rtol=1e-12)
    assert w["n_warn"] == int((pw_i > 0.4).sum()) > 0


@pytest.mark.parametrize("splits", [(37,), (1, 20, 16), (5, 5, 5, 5, 17)])
def test_device_rule_merged_over_uneven_splits_equals_whole_matrix(splits):
    rng = np.random.default_rng(len(splits))
    K = 257
    ll = -2.0 + rng.standard_normal((sum(splits), K)) * rng.uniform(0.1, 3.0, K)
    ll[:, 0] = -np.arange(ll.shape[0], dtype=float)  # falling: the running max never rises
    ll[:, 1] = np.arange(ll.shape[0], dtype=float)  # rising: rescaled at every draw
    parts, lo = [], 0
    for s in splits:
        parts.append(_device_rule(ll[lo:lo + s]))
        lo += s
    lse, mean, m2, n = compare.merge(*parts)
    r_lse, r_mean, r_m2, r_n = compare.stats_from_matrix(ll)
    assert n == r_n
    np.testing.assert_allclose(lse, r_lse, rtol=1e-12)
    np.testing.assert_allclose(mean, r_mean, rtol=1e-12)
    np.testing.assert_allclose(m2, r_m2, rtol=1e-9)
    res = {"waic_lse": np.stack([p[0] for p in parts]), "waic_mean": np.stack([p[1] for p in parts]),
           "waic_m2": np.stack([p[2] for p in parts]), "waic_n_draws": np.array([p[3] for p in parts]),
           "waic_n_obs": np.tile([200, 57], (len(parts), 1))}
    w, wd = compare.waic(res), _waic_direct(ll)
    np.testing.assert_allclose([w["elpd_waic"], w["p_waic"], w["se"]], wd[:3], rtol=1e-10)
    assert w["elpd_waic_i_s"].shape == (200,) and w["p_waic_i_n"].shape == (57,)


def test_compare_paired_se_by_hand():
    rng = np.random.default_rng(3)
    a = -1.0 + 0.3 * rng.standard_normal((2, 40, 30))
    b = a + 0.2 * rng.standard_normal((2, 40, 30)) - 0.1
    wa, wb = compare.waic_from_matrix(a), compare.waic_from_matrix(b)
    out = compare.compare({"A": wa, "B": wb})
    best, other = ("A", "B") if wa["elpd_waic"] >= wb["elpd_waic"] else ("B", "A")
    d = (wa if best == "A" else wb)["elpd_i"] - (wb if best == "A" else wa)["elpd_i"]
    dse = np.sqrt(sum((x - sum(d) / len(d)) ** 2 for x in d) / len(d) * len(d))  # sqrt(n var), ddof 0, written out
    assert out[best]["rank"] == 0 and out[best]["elpd_diff"] == 0.0 and out[best]["dse"] == 0.0
    assert out[other]["elpd_diff"] == pytest.approx(float(d.sum()), rel=1e-12)
    assert out[other]["dse"] == pytest.approx(dse, rel=1e-12)
    with pytest.raises(ValueError):
        compare.compare({"A": wa, "C": compare.waic_from_matrix(a[..., :10])})


def test_cli_parser_accepts_the_flags():
    from abdpymc_amd.cli import build_parser

    a = build_parser().parse_args(["--tune", "1", "--draws", "1", "--waic", "--log_likelihood"])
    assert a.waic and a.log_likelihood
    b = build_parser().parse_args(["--tune", "1", "--draws", "1"])
    assert not b.waic and not b.log_likelihood


def test_record_bytes_counts_the_matrix():
    from abdpymc_amd.sampler import record_bytes

    base = record_bytes(4, 100, 31, 1520, False, False)
    assert base == 0
    assert record_bytes(4, 100, 31, 1520, False, False, n_readings=35709) == 4 * 100 * 35709 * 8
    assert record_bytes(2, 10, 3, 5, True, True, n_readings=7) == record_bytes(2, 10, 3, 5, True, True) + 2 * 10 * 7 * 8


def test_host_sampler_refuses_the_options():
    from abdpymc_amd.sampler import sample

    class _M:
        n_chains = 1
        ctx = None

    for kw in ({"log_likelihood": True}, {"waic": True}):
        with pytest.raises(ValueError, match="native sampler"):
            sample(_M(), tune=1, draws=1, native=False, **kw)
