"""
PSIS-LOO by individual for the titer model (abdpymc_amd.loo) without a GPU: the plan's refusals, the host
sampler's refusal, ``loo.loo`` and the report line on fabricated values, ``compare.compare(ic="loo")`` against the formulas
written out, ``compare.compare`` without ``ic`` unchanged, and the command line's refusals.
"""
import os
import warnings
from types import SimpleNamespace

import numpy as np
import pytest

from abdpymc_amd import compare, loo, sampler, summaries
from tests.test_individual_waic_cpu import _grouped_case
from tests.test_summaries_plumbing_cpu import CHAINS, DRAWS, G, N, StubContext, StubModel, StubSampler

N_READINGS = np.array([3, 0, 1, 0, 2, 1, 4])  # of the stub's N = 7 individuals


class LooStubSampler(StubSampler):
    def enable_loo(self, draws, thin=1):
        self.calls.append(("enable_loo", draws, thin))

    def loo_stats(self):
        self.calls.append(("loo_stats",))
        has = N_READINGS > 0
        return {"elpd_loo": np.where(has, -2.0, 0.0), "pareto_k": np.where(has, 0.1, np.nan), "lppd": np.where(has, -1.5, 0.0),
                "n_tail": np.where(has, 3, 0).astype(np.int32), "n_readings": N_READINGS.copy(), "n_draws": CHAINS * -(-DRAWS // 2)}


class LooStubContext(StubContext):
    def sampler(self, chains, theta0, **kw):
        self.calls.append(("sampler", sorted(kw)))
        return LooStubSampler(self.calls, len(chains))


class LooStubModel(StubModel):
    def __init__(self):
        self.ctx = LooStubContext()


def _opts(**kw):
    return summaries.resolve(kw)


@pytest.mark.parametrize("kw, draws, chains, text", [
    (dict(loo=True, loo_thin=0), 10, 2, "loo_thin must be an integer >= 1, got 0"),
    (dict(loo=True, loo_thin=2.5), 10, 2, "loo_thin must be an integer >= 1, got 2.5"),
    (dict(loo=True), 6000, 3, "3 chains x 6000 draws = 18000 columns per individual, over the 16384 the device smooths: a larger "
                              "loo_thin fits (loo_thin >= 2)"),
    (dict(loo=True, loo_thin=2), 40000, 4, "loo_thin >= 10"),
])
def test_plan_refuses_before_any_device_call(kw, draws, chains, text):
    with pytest.raises(ValueError) as e:
        loo.SUMMARY.plan(_opts(**kw), draws, chains, G, N)
    assert text in str(e.value)
    m = LooStubModel()  # ... and through sample(): nothing is created, nothing enabled
    with pytest.raises(ValueError):
        sampler.sample(m, tune=1, draws=draws, chains=chains, **kw)
    assert m.ctx.calls == []


def test_plan_and_the_calls_of_a_run():
    assert loo.SUMMARY.plan(_opts(), 10, 2, G, N) is None
    p = loo.SUMMARY.plan(_opts(loo=True, loo_thin=3), 40, 3, G, N)
    assert p["kept"] == 14 and p["loo_thin"] == 3 and p["draws"] == 40
    m = LooStubModel()
    res = sampler.sample(m, tune=2, draws=DRAWS, chains=CHAINS, loo=True, loo_thin=2)
    assert [c for c in m.ctx.calls if c[0].startswith(("enable_", "loo_"))] == [("enable_loo", DRAWS, 2), ("loo_stats",)]
    assert sorted(k for k in res if k.startswith("loo_")) == sorted(loo.RESULT_KEYS)
    assert res["loo_elpd_i"].shape == (N,) and res["loo_n_draws"].tolist() == [CHAINS * 3] and res["loo_n_tail"].dtype == np.int32


def test_plan_cap_boundary():
    assert loo.SUMMARY.plan(_opts(loo=True), 4096, 4, G, N)["kept"] == 4096  # exactly 16384
    with pytest.raises(ValueError, match="16388"):
        loo.SUMMARY.plan(_opts(loo=True), 4097, 4, G, N)
    with pytest.raises(ValueError, match="16386"):
        loo.SUMMARY.plan(_opts(loo=True, loo_thin=3), 16384, 3, G, N)


def test_host_sampler_refuses():
    m = LooStubModel()
    with pytest.raises(ValueError) as e:
        sampler.sample(m, tune=1, draws=2, native=False, loo=True)
    assert str(e.value) == loo.SUMMARY.native_only and "native" in str(e.value) and m.ctx.calls == []


def _fabricated(seed=0, n=9, S=200, bad=()):
    """the loo_* keys of a result: individuals 2 and 6 have no readings; ``bad``: those with k = 0.9"""
    rng = np.random.default_rng(seed)
    cnt = rng.integers(1, 30, n)
    cnt[[2, 6]] = 0
    has = cnt > 0
    lppd = np.where(has, -3.0 + rng.standard_normal(n), 0.0)
    elpd = np.where(has, lppd - rng.uniform(0.05, 0.6, n), 0.0)
    k = np.where(has, rng.uniform(-0.1, 0.5, n), np.nan)
    k[list(bad)] = 0.9
    return {"loo_elpd_i": elpd, "loo_pareto_k": k, "loo_lppd_i": lppd, "loo_n_tail": np.where(has, 40, 0).astype(np.int32),
            "loo_n_readings": cnt.astype(np.int64), "loo_n_draws": np.array([S], dtype=np.int64)}


def test_loo_of_a_result_is_loo_from_individual():
    res = _fabricated(bad=(4,))
    w = loo.loo(res)
    ref = compare.loo_from_individual(res["loo_elpd_i"], res["loo_pareto_k"], res["loo_lppd_i"], res["loo_n_readings"], 200)
    assert set(w) == set(ref)
    for key, v in ref.items():
        np.testing.assert_array_equal(w[key], v)
    has = res["loo_n_readings"] > 0
    assert w["n_individuals"] == 7 and w["n_bad"] == 1 and w["worst"] == 4 and w["n_draws"] == 200
    assert w["elpd_loo"] == pytest.approx(res["loo_elpd_i"][has].sum()) and w["p_loo"] == pytest.approx((res["loo_lppd_i"] - res["loo_elpd_i"])[has].sum())
    with pytest.raises(ValueError, match="loo_lppd_i"):
        loo.loo({k: v for k, v in res.items() if k != "loo_lppd_i"})
    # a written and loaded posterior file
    idata = SimpleNamespace(constant_data=SimpleNamespace(data_vars={k: v for k, v in res.items()}))
    assert loo.loo(idata)["elpd_loo"] == w["elpd_loo"]


def test_report_line_and_warning():
    data = SimpleNamespace(coords={"ind": np.arange(100, 109)})
    res = _fabricated(bad=(4, 7))
    with pytest.warns(UserWarning, match="2 of 7 individuals have a Pareto k above 0.7"):
        lines = loo.SUMMARY.report(res, data)
    w = loo.loo(res)
    thr = min(1.0 - 1.0 / np.log10(200), 0.7)
    n_warn = int((res["loo_pareto_k"][res["loo_n_readings"] > 0] > thr).sum())
    assert lines == [f"LOO by individual: elpd_loo {w['elpd_loo']:.3f}  p_loo {w['p_loo']:.3f}  se {w['se']:.3f}  (7 individuals, 200 draws; "
                     f"2 with k > 0.7, {n_warn} above {thr:.2f}; worst: individual 104 k 0.90)"]
    assert n_warn >= 2 and thr < 0.7
    for key, ref in (("elpd_loo_ind", w["elpd_i"]), ("p_loo_ind", w["p_loo_i"]), ("pareto_k_ind", w["pareto_k"])):
        assert res[key].shape == (9,)
        np.testing.assert_array_equal(res[key], ref)
        assert loo.SUMMARY.owns(key) and loo.SUMMARY.group(key) == "constant_data" and loo.SUMMARY.dims[key] == ["ind"]
    assert np.isnan(res["pareto_k_ind"][[2, 6]]).all() and np.all(res["elpd_loo_ind"][[2, 6]] == 0.0)
    quiet = _fabricated()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        (line,) = loo.SUMMARY.report(quiet, SimpleNamespace())
    assert "; 0 with k > 0.7, " in line and "worst: individual " in line


def test_compare_ic_loo_against_the_formulas():
    a, b, c = _fabricated(1), _fabricated(1), _fabricated(1)
    rng = np.random.default_rng(5)
    has = a["loo_n_readings"] > 0
    b["loo_elpd_i"] = np.where(has, a["loo_elpd_i"] - rng.uniform(0.0, 0.3, has.size), 0.0)
    c["loo_elpd_i"] = np.where(has, a["loo_elpd_i"] + 0.2 * rng.standard_normal(has.size) + 0.1, 0.0)
    c["loo_pareto_k"] = np.where(has, 0.8, np.nan)
    variants = {"a": a, "b": b, "c": loo.loo(c)}  # a dictionary of loo_from_individual is taken as it is
    table = compare.compare(variants, ic="loo")
    tot = {name: float(v["loo_elpd_i"][has].sum()) for name, v in (("a", a), ("b", b), ("c", c))}
    order = sorted(tot, key=lambda k: -tot[k])
    best = {"a": a, "b": b, "c": c}[order[0]]["loo_elpd_i"]
    m = int(has.sum())
    assert m == 7 and [table[name]["rank"] for name in order] == [0, 1, 2]
    for name, v in (("a", a), ("b", b), ("c", c)):
        row = table[name]
        assert set(row) == {"rank", "elpd_loo", "p_loo", "se", "elpd_diff", "dse", "n_bad"}
        assert row["elpd_loo"] == pytest.approx(tot[name], rel=1e-13)
        assert row["p_loo"] == pytest.approx(float((v["loo_lppd_i"] - v["loo_elpd_i"])[has].sum()), rel=1e-12)
        assert row["se"] == pytest.approx(np.sqrt(m * np.var(v["loo_elpd_i"][has])), rel=1e-12)
        assert row["elpd_diff"] == pytest.approx(tot[order[0]] - tot[name], abs=1e-12) and row["elpd_diff"] >= 0.0
        d = (best - v["loo_elpd_i"])[has]
        assert row["dse"] == pytest.approx(np.sqrt(m * np.var(d)), rel=1e-12, abs=1e-15)
        assert row["dse"] != pytest.approx(np.sqrt(has.size * np.var(best - v["loo_elpd_i"])), rel=1e-6) or name == order[0]
        assert row["n_bad"] == (7 if name == "c" else 0)
    assert table[order[0]]["elpd_diff"] == 0.0 and table[order[0]]["dse"] == 0.0
    # what it refuses, by name
    with pytest.raises(ValueError, match=r"\['w', 'z'\]"):
        compare.compare({"a": a, "z": {"waic_lse": np.zeros((1, 3))}, "w": {}}, ic="loo")
    other = _fabricated(1)
    other["loo_n_readings"] = other["loo_n_readings"].copy()
    other["loo_n_readings"][2] = 5
    with pytest.raises(ValueError, match=r"\['other'\]"):
        compare.compare({"a": a, "b": b, "other": other}, ic="loo")
    fewer = {k: (v[:-1] if v.shape == (9,) else v) for k, v in _fabricated(1).items()}
    with pytest.raises(ValueError, match=r"\['fewer'\]"):
        compare.compare({"a": a, "b": b, "fewer": fewer}, ic="loo")
    with pytest.raises(ValueError, match="ic"):
        compare.compare({"a": a}, ic="dic")


def test_compare_without_ic_is_what_it_was():
    """the WAIC fixture of tests/test_individual_waic_cpu.py: the table's entries by hand, and ic="waic" the same dictionaries"""
    ll, groups, T, cnt, res_a = _grouped_case(1)
    _, _, _, _, res_b = _grouped_case(2)
    table = compare.compare({"a": res_a, "b": res_b})
    assert table == compare.compare({"a": res_a, "b": res_b}, ic="waic") == compare.compare({"a": res_a, "b": res_b}, by="individual")
    wa, wb = compare.waic(res_a, by="individual"), compare.waic(res_b, by="individual")
    best, other = (("a", wa), ("b", wb)) if wa["elpd_waic"] >= wb["elpd_waic"] else (("b", wb), ("a", wa))
    has = cnt > 0
    d = (best[1]["elpd_i"] - other[1]["elpd_i"])[has]
    assert table[best[0]] == dict(rank=0, elpd_waic=best[1]["elpd_waic"], p_waic=best[1]["p_waic"], se=best[1]["se"], elpd_diff=0.0, dse=0.0,
                                  n_warn=best[1]["n_warn"])
    assert table[other[0]] == dict(rank=1, elpd_waic=other[1]["elpd_waic"], p_waic=other[1]["p_waic"], se=other[1]["se"],
                                   elpd_diff=float(best[1]["elpd_waic"] - other[1]["elpd_waic"]),
                                   dse=float(np.sqrt(d.size * np.var(d))), n_warn=other[1]["n_warn"])
    assert list(table[other[0]]) == ["rank", "elpd_waic", "p_waic", "se", "elpd_diff", "dse", "n_warn"]


def test_cli_flags(golden_dir):
    from abdpymc_amd import cli

    base = ["--tune", "1", "--draws", "4"]
    a = cli.build_parser().parse_args(base + ["--loo", "--loo_thin", "2"])
    assert loo.SUMMARY.cli_options(a, None, 2, 1) == {"loo": True, "loo_thin": 2}
    assert loo.SUMMARY.cli_options(cli.build_parser().parse_args(base + ["--loo"]), None, 2, 1) == {"loo": True, "loo_thin": 1}
    assert loo.SUMMARY.cli_options(cli.build_parser().parse_args(base), None, 2, 2) == {"loo": False, "loo_thin": 1}
    with pytest.raises(SystemExit, match="--loo_thin needs --loo"):
        loo.SUMMARY.cli_options(cli.build_parser().parse_args(base + ["--loo_thin", "2"]), None, 2, 1)
    with pytest.raises(SystemExit, match="2 processes"):
        loo.SUMMARY.cli_options(cli.build_parser().parse_args(base + ["--loo"]), None, 2, 2)
    with pytest.raises(SystemExit, match="--loo"):  # before a model is built
        cli.main(base + ["--cores", "1", "--ititers_data", os.path.join(golden_dir, "test_cohort"), "--loo_thin", "2"])


def test_registry_and_keys():
    import re

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "abd_hip.h")).read()
    assert int(re.search(r"#define ABD_SAMPLER_LOO_MAX_DRAWS (\d+)", header).group(1)) == loo.MAX_DRAWS  # the plan's cap is the library's
    # the summaries kept per chain stay what they were; every() puts loo behind WAIC, and what the plumbing relies on holds over it
    reg = summaries.every()
    assert [s.name for s in reg] == ["waic", "loo"] + [s.name for s in summaries.registry()[1:]] and reg[1] is loo.SUMMARY
    prefixes = [s.prefix for s in reg]
    assert all(p and not q.startswith(p) for i, p in enumerate(prefixes) for j, q in enumerate(prefixes) if i != j)
    owned = [k for s in reg for k in s.options]
    assert len(owned) == len(set(owned)) and all(s.name in s.options for s in reg)
    assert loo.SUMMARY.options == {"loo": False, "loo_thin": 1} and loo.SUMMARY.prefix == "loo_"
    assert all(loo.SUMMARY.owns(k) and loo.SUMMARY.group(k) == "constant_data" for k in loo.RESULT_KEYS)
