"""
risk.py on the CPU: the table of a binary draw against a literal per-individual loop of the reference's survival construction
(survival.py:72-100: NaN after the last sample, the window, at most one infection per individual, exposure = 1 - the lagged
running sum; 102-114: the titer of the gap before), the Mantel-Haenszel rate ratio, the merges, the refusals of ``spec`` and
``survival_arrays``.  Everything here is an integer or a hand-computed rational: comparisons are exact unless a bound is stated.
"""
import numpy as np
import pytest

from abdpymc_amd import risk


def _draw(G, N, seed, density=0.15):
    rng = np.random.default_rng(seed)
    i = (rng.random((G, N)) < density).astype(np.int8)
    mu_s, mu_n = rng.normal(2.0, 1.5, (G, N)), rng.normal(1.0, 1.0, (G, N))
    last = rng.integers(-1, G, N)
    last[0], last[-1] = G - 1, -1
    return i, mu_s, mu_n, last


def _literal(i, mu_s, mu_n, last, sp):
    """One individual at a time, as the reference builds `infected` and `exposure` from an (ind, gap) array"""
    G, N = i.shape
    start, end = sp["start"], sp["end"]
    table = np.zeros((2, 2, G, 8), dtype=np.int64)
    for j in range(N):
        row = i[:, j].astype(float)
        row[last[j] + 1:] = np.nan  # after the last sample
        win = row[start + 1:end]
        if sp["first_only"]:
            infected, run = [], 0.0
            for v in win:  # the values while their running sum is below 1
                if run > 1.0:
                    infected.append(0.0)
                else:
                    infected.append(1.0 - run if run + v > 1.0 else v)
                run += v
            infected = np.array(infected)
            exposure = np.ones_like(infected)
            exposure[1:] -= np.cumsum(infected)[:-1]
        else:
            infected, exposure = win.copy(), np.ones_like(win)
        exposure[np.isnan(infected)] = np.nan
        for t in range(end - start - 1):
            if np.isnan(exposure[t]) or exposure[t] == 0.0:
                continue
            assert exposure[t] == 1.0 and infected[t] in (0.0, 1.0)
            g = start + 1 + t
            for a, (mu, edges) in enumerate(((mu_s, sp["edges_s"]), (mu_n, sp["edges_n"]))):
                b = sum(1 for e in edges if mu[start + t, j] >= e)  # the titer one gap earlier
                table[a, 0, g, b] += 1
                table[a, 1, g, b] += int(infected[t])
    return table


@pytest.mark.parametrize("first_only", [0, 1])
@pytest.mark.parametrize("window", ["all", "inside", "two"])
def test_table_against_the_literal_loop(window, first_only):
    G, N = 23, 41
    i, mu_s, mu_n, last = _draw(G, N, 3)
    start, end = {"all": (0, G), "inside": (G // 3, G - 2), "two": (9, 11)}[window]
    sp = risk.spec(start, end, np.quantile(mu_s, np.arange(1, 8) / 8), np.quantile(mu_n, [0.3, 0.6, 0.9]), first_only, n_gaps=G)
    got = risk.from_deterministics(i, mu_s, mu_n, last, sp)
    want = _literal(i, mu_s, mu_n, last, sp)
    assert got.dtype == np.int64 and got.shape == (2, 2, G, 8)
    np.testing.assert_array_equal(got, want)
    assert want[:, 0].sum() > 0 and not got[:, :, :start + 1].any() and not got[:, :, end:].any()
    assert not got[1, :, :, 4:].any()  # three edges: bins 0 .. 3
    np.testing.assert_array_equal(got[0].sum(axis=-1), got[1].sum(axis=-1))  # the antigens only bin differently
    if window == "two":
        assert (got[:, :, np.arange(G) != start + 1] == 0).all()
    if first_only:
        assert got[0, 1].sum() <= N
    # leading axes, and last_gap None = everyone to the last gap
    stack = risk.from_deterministics(np.stack([i, i[:, ::-1]]), np.stack([mu_s, mu_s[:, ::-1]]), np.stack([mu_n, mu_n[:, ::-1]]),
                                     None, sp)
    np.testing.assert_array_equal(stack[0], _literal(i, mu_s, mu_n, np.full(N, G - 1), sp))
    np.testing.assert_array_equal(stack[0], stack[1])


def test_nan_titers_land_in_bin_zero():
    G, N = 12, 9
    i, mu_s, mu_n, last = _draw(G, N, 5)
    sp = risk.spec(0, G, [1.0, 2.0], [0.5], 1)
    ref = risk.from_deterministics(i, mu_s, mu_n, last, sp)
    nan = risk.from_deterministics(i, np.full((G, N), np.nan), np.full((G, N), np.nan), last, sp)
    assert not nan[..., 1:].any()
    np.testing.assert_array_equal(nan[..., 0], ref.sum(axis=-1))


def test_rate_ratio_by_hand_and_under_proportional_hazards():
    # two gaps, reference bin 0 against bin 1: (1 * 10 / 30 + 2 * 30 / 40) / (2 * 20 / 30 + 3 * 10 / 40) = (11 / 6) / (25 / 12)
    T, e = np.zeros((2, 8)), np.zeros((2, 8))
    T[:, :2], e[:, :2] = [[10, 20], [30, 10]], [[2, 1], [3, 2]]
    rr = risk.rate_ratio(T, e)
    assert abs(rr[1] - 22.0 / 25.0) <= 4 * 2.0 ** -52 and rr[0] == 1.0 and np.isnan(rr[2:]).all()
    assert abs(risk.rate_ratio(T, e, reference_bin=1)[0] - 25.0 / 22.0) <= 4 * 2.0 ** -52
    # a gap without person-gaps in either bin is left out; no events in the reference: NaN
    T2, e2 = np.vstack([T, np.zeros((1, 8))]), np.vstack([e, np.zeros((1, 8))])
    assert risk.rate_ratio(T2, e2)[1] == rr[1]
    e0 = e.copy()
    e0[:, 0] = 0
    assert np.isnan(risk.rate_ratio(T, e0)).all()
    # e[g, b] = c_g k_b T[g, b]: the gap effect c_g cancels and RR_b = k_b / k_r, whatever T is
    rng = np.random.default_rng(0)
    G = 30
    T = rng.integers(1, 500, (G, 8)).astype(float)
    c, k = rng.uniform(0.001, 0.05, G), rng.uniform(0.2, 3.0, 8)
    e = c[:, None] * k[None, :] * T
    for r in (0, 3):
        got = risk.rate_ratio(T, e, reference_bin=r)
        assert np.abs(got / (k / k[r]) - 1).max() <= 4 * G * 2.0 ** -52  # G terms on either side of the ratio
    with pytest.raises(ValueError):
        risk.rate_ratio(T, e, reference_bin=8)
    with pytest.raises(ValueError):
        risk.rate_ratio(T, e[:, :7])


def test_shards_add_and_chains_concatenate():
    G, N = 17, 30
    i, mu_s, mu_n, last = _draw(G, N, 7)
    sp = risk.spec(2, G - 1, [1.0, 2.0, 3.0], [0.5, 1.5], 1)

    def res_of(sl):
        t = risk.from_deterministics(i[None, None, :, sl], mu_s[None, None, :, sl], mu_n[None, None, :, sl], last[sl], sp)
        return risk.as_result(t, sp)

    whole, a, b = res_of(slice(None)), res_of(slice(0, 11)), res_of(slice(11, None))
    merged = risk.merge_individual_shards([a, b])
    for k in risk.RESULT_KEYS:
        np.testing.assert_array_equal(merged[k], whole[k])
    assert merged["risk_table"].dtype == np.int64 and whole["risk_table"].shape == (1, 1, 2, 2, G, 8)
    assert whole["risk_edges_s"].shape == (1, 7) and np.isnan(whole["risk_edges_s"][0, 3:]).all()
    np.testing.assert_array_equal(whole["risk_window"], [[2, G - 1, 1]])
    two = risk.merge_chains([whole, whole])
    assert two["risk_table"].shape == (2, 1, 2, 2, G, 8) and two["risk_window"].shape == (2, 3)
    other = risk.as_result(whole["risk_table"], risk.spec(2, G - 1, [1.0, 2.0], [0.5, 1.5], 1))
    for merge in (risk.merge_chains, risk.merge_individual_shards):
        with pytest.raises(ValueError):
            merge([whole, other])  # another spec
        with pytest.raises(ValueError):
            merge([whole, {"risk_table": whole["risk_table"]}])


def test_summary_counts_and_ignores_undefined_draws():
    G = 6
    t = np.zeros((2, 3, 2, 2, G, 8), dtype=np.int64)
    t[:, :, :, 0, 1:, :2] = 50           # 50 person-gaps in bins 0 and 1 of gaps 1 ..
    t[:, :, :, 1, 1:, 0] = 10            # rate 0.2 in bin 0
    t[:, :, :, 1, 1:, 1] = 5             # ... 0.1 in bin 1: RR 0.5
    t[0, 0, 0, 1, :, 0] = 0              # one draw without events in the reference bin of S: RR undefined there
    res = risk.as_result(t, risk.spec(0, G, [1.0], [1.0], 1))
    sm = risk.summary(res)
    assert sm["n_draws"] == 6 and sm["window"] == (0, G, 1) and sm["edges_s"].tolist() == [1.0]
    assert sm["s"]["rate_ratio"]["n_defined"][1] == 5 and sm["n"]["rate_ratio"]["n_defined"][1] == 6
    for ag in ("s", "n"):
        assert sm[ag]["rate_ratio"]["median"][1] == 0.5 and sm[ag]["protection"]["median"][1] == 0.5
        assert sm[ag]["person_gaps"]["median"][1] == 50 * (G - 1) and sm[ag]["events"]["median"][1] == 5 * (G - 1)
        assert sm[ag]["rate"]["median"][1] == 0.1 and sm[ag]["rate"]["n_defined"][2] == 0 and np.isnan(sm[ag]["rate"]["median"][2])
    arrs = risk.summary_arrays(sm)
    assert arrs["risk_summary_s_protection"].shape == (4, 8) and arrs["risk_summary_s_rate_ratio"][3, 1] == 5
    assert set(arrs) == {f"risk_summary_{a}_{q}" for a in ("s", "n") for q in risk.QUANTITIES}
    with pytest.raises(ValueError):
        risk.summary({"risk_table": t})
    with pytest.raises(ValueError):
        risk.summary(res, prob=1.0)


def test_spec_refusals():
    ok = risk.spec(0, 10, [1.0, 2.0], [], True)
    assert ok["first_only"] == 1 and ok["edges_n"].size == 0 and risk.spec(3, None, n_gaps=9)["end"] == 9
    assert risk.spec(4, 6)["end"] == 6 and risk.spec(0, 10, range(7))["edges_s"].size == 7
    bad = [dict(start=-1, end=5), dict(start=3, end=4), dict(start=0, end=11, n_gaps=10), dict(start=0, end=None),
           dict(start=0.5, end=5), dict(start=0, end=5, edges_s=range(8)), dict(start=0, end=5, edges_n=[1.0, 1.0]),
           dict(start=0, end=5, edges_s=[2.0, 1.0]), dict(start=0, end=5, edges_s=[np.nan]), dict(start=0, end=5, edges_n=[np.inf]),
           dict(start=0, end=5, first_only=2), dict(start=0, end=5, first_only=-1), dict(start=0, end=5, first_only=0.5),
           dict(start=0, end=5, edges_s=[[1.0, 2.0]])]
    for kw in bad:
        with pytest.raises(ValueError):
            risk.spec(**kw)
    i, mu_s, mu_n, last = _draw(8, 5, 1)
    with pytest.raises(ValueError):
        risk.from_deterministics(i, mu_s, mu_n, last, risk.spec(0, 9))  # a window beyond the draw's gaps
    with pytest.raises(ValueError):
        risk.from_deterministics(i, mu_s, mu_n[:-1], last, risk.spec(0, 8))


def test_survival_arrays():
    G, N = 20, 50
    rng = np.random.default_rng(11)
    i_mean = rng.random((G, N)) * (rng.random((G, N)) < 0.5)  # many individuals pass a total of 1
    mu_s, mu_n = rng.normal(size=(G, N)), rng.normal(size=(G, N))
    last = rng.integers(-1, G, N)
    last[0], last[1] = G - 1, -1
    for start, end in ((0, G), (4, 15), (7, 9)):
        sa = risk.survival_arrays(i_mean, mu_s, mu_n, last, start, end)
        n_int = end - start - 1
        for k in ("infected", "exposure", "s_titer", "n_titer"):
            assert sa[k].shape == (N, n_int), k
        inf, ex = sa["infected"], sa["exposure"]
        np.testing.assert_array_equal(np.isnan(inf), np.isnan(ex))
        # NaN after the last sample only -- and everywhere there, but that the reference's running-sum rule writes a single 0
        # (with exposure 0: no contribution to a Poisson term) into the first such cell of an individual already past the cap
        after = np.arange(start + 1, end)[None, :] > last[:, None]
        assert not (np.isnan(inf) & ~after).any()
        kept = after & ~np.isnan(inf)
        assert (inf[kept] == 0.0).all() and (ex[kept] <= 4 * G * 2.0 ** -52).all() and (kept.sum(axis=1) <= 1).all()
        assert (np.nansum(inf, axis=1) <= 1.0 + 4 * G * 2.0 ** -52).all()  # (a sum of up to G roundings)
        assert (np.nansum(inf, axis=1) >= 1.0 - 4 * G * 2.0 ** -52).any() or n_int < 3  # the cap is reached by some
        e = np.where(np.isnan(ex), -1.0, ex)
        assert ((ex[~np.isnan(ex)] >= 0) & (ex[~np.isnan(ex)] <= 1)).all()
        assert (np.diff(e, axis=1) <= 0).all()  # non-increasing (the NaN tail sits below)
        assert (ex[~np.isnan(ex[:, 0]), 0] == 1.0).all()
        # below the cap the probabilities are the means themselves; the titers are those of the gap before
        first = i_mean.T[:, start + 1]
        np.testing.assert_array_equal(inf[last >= start + 1, 0], first[last >= start + 1])
        np.testing.assert_array_equal(sa["s_titer"], mu_s.T[:, start:end - 1])
        np.testing.assert_array_equal(sa["n_titer"], mu_n.T[:, start:end - 1])
    # a binary "mean" gives the table's own cells: exposure 1 up to and including the first infection, 0 after it
    i, _, _, last = _draw(G, N, 2)
    sa = risk.survival_arrays(i, mu_s, mu_n, last, 2, G)
    t = risk.from_deterministics(i, mu_s, mu_n, last, risk.spec(2, G, first_only=1))
    assert np.nansum(sa["exposure"]) == t[0, 0].sum() and np.nansum(sa["infected"]) == t[0, 1].sum()
    with pytest.raises(ValueError):
        risk.survival_arrays(i_mean, mu_s, mu_n, last, 5, 6)
    with pytest.raises(ValueError):
        risk.survival_arrays(-i_mean - 1, mu_s, mu_n, last, 0, G)
