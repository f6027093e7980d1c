"""
The per-individual timelines of the native sampler (abd_sampler_enable_timelines / abd_sampler_timelines /
abd_sampler_timeline_quantiles; sample(timelines=True); the CLI's --timelines) against timelines.from_draws of the draws the same
run recorded: the integer counters exactly, the histograms by cumulative counts within the Deterministics' per-titer gate, the
device's quantiles against timelines.quantiles of the read-out histograms; what the counters must not depend on, as byte
equality; the errors; the teardown.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest

from abdpymc_amd import synthetic
from abdpymc_amd import timelines as tl
from abdpymc_amd._native import AbdError
from abdpymc_amd.data import TiterData
from tests.test_gpu_pointwise import _same_trajectories

pytestmark = pytest.mark.gpu
TUNE, DRAWS = 6, 21
EPS = np.finfo(np.float64).eps


def _dense_model(N, G, n_chains, seed=11, splits=None, last_gap=None):
    from abdpymc_amd.model import AbdModel

    sc = synthetic.make_cohort(N, G, seed=seed)
    d = SimpleNamespace(n_gaps=sc.n_gaps, n_inds=sc.n_inds, vacs=sc.vacs, pcrpos=sc.pcrpos,
                        coords={"gap": np.arange(sc.n_gaps), "ind": np.arange(sc.n_inds)},
                        s=SimpleNamespace(obs=sc.s_obs), n=SimpleNamespace(obs=sc.n_obs))
    if last_gap is not None:
        d.last_gap = np.asarray(last_gap)
    return AbdModel(d, splits=splits, n_chains=n_chains)


def _model(which, golden_dir, n_chains):
    from abdpymc_amd.model import model

    if which == "test":  # observation lists
        return model(TiterData.from_disk(os.path.join(golden_dir, "test_cohort")), n_chains=n_chains)
    return _dense_model(100, 70, n_chains)


def delta(xmax):
    """what a titer of the accumulating kernel may differ by from the recorded one: the Deterministics tests' per-titer gate"""
    return 1e-12 * xmax + 1e-13


def check_integers(res, splits=None, last_gap=None):
    want = tl.from_draws(res["i"], None, None, splits=splits, last_gap=last_gap)
    for k in ("tl_inf", "tl_cum", "tl_ninf", "tl_info"):
        assert res[k].dtype == np.int64 and res[k].shape == want[k].shape, k
        np.testing.assert_array_equal(res[k], want[k], err_msg=k)
    assert (res["tl_cum"] > res["tl_inf"]).any()  # (not about zeros)
    assert (res["tl_cum"] >= res["tl_inf"]).all()


def check_histograms(res, ranges):
    """every cell and every bin edge e: #{x < e - d} <= C <= #{x < e + d} over the recorded draws; rows sum to the draws"""
    D = res["i"].shape[1]
    for key, var, (lo, hi) in (("tl_hist_n", "ab_n_mu", ranges[0]), ("tl_hist_s", "ab_s_mu", ranges[1])):
        h, x = res[key], res[var]
        assert h.dtype == np.uint16 and h.shape == (x.shape[0],) + x.shape[2:] + (64,), key
        np.testing.assert_array_equal(h.sum(axis=-1, dtype=np.int64), np.full(h.shape[:-1], D), err_msg=key)
        C = np.cumsum(h, axis=-1, dtype=np.int64)
        d = delta(np.abs(x).max())
        w = (hi - lo) / 62
        worst = 0
        for k in range(63):  # the edge between counters k and k + 1
            e = lo + w * k if k < 62 else hi
            below, above = (x < e - d).sum(axis=1), (x < e + d).sum(axis=1)
            worst = max(worst, int((above - below).max()))
            assert (below <= C[..., k]).all() and (C[..., k] <= above).all(), (key, k)
        print(f"{key}: gate {d:.3e}; at most {worst} draws of a cell inside it at one edge")
        assert (h[..., 0] > 0).any() and (h[..., 63] > 0).any() and (h[..., 1:63] > 0).any(), key


def check_quantiles(res, ranges):
    m = tl.merge(res)
    q = res["tl_q"][0]
    for key, hist, (lo, hi) in (("tl_q_n", m["hist_n"], ranges[0]), ("tl_q_s", m["hist_s"], ranges[1])):
        want = tl.quantiles(hist, q, lo, hi)
        got = res[key]
        assert got.shape == want.shape and got.dtype == np.float64, key
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=key)
        err = np.nanmax(np.abs(got - want))
        gate = 8 * EPS * max(abs(lo), abs(hi))
        print(f"{key}: largest difference {err:.3e} (gate {gate:.3e})")
        assert err <= gate, key
        # ascending in q, up to the same roundings: lo + 62 w, the end of the last interior bin, need not be hi to the last bit
        assert (np.diff(got, axis=0) >= -gate).all()


def _same_tl(a, b, keys=None):
    for k in keys or [k for k in a if k.startswith("tl_")]:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
        assert a[k].tobytes() == b[k].tobytes(), k


_runs = {}


def run(golden_dir, which, chains, **kw):
    """sample(...) of the main case, computed once per variant and left alone"""
    from abdpymc_amd.sampler import sample

    key = (which, chains, tuple(sorted(kw.items())))
    if key not in _runs:
        m = _model(which, golden_dir, chains)
        launch = kw.pop("launch_config", None)
        if launch:
            m.ctx.set_launch_config(*launch)
        _runs[key] = sample(m, tune=TUNE, draws=DRAWS, chains=chains, seed=7, **kw)
        m.close()
    return _runs[key]


def ranges_of(golden_dir, which):
    """the 10 % and 90 % quantiles of the titers a first run with the same seed recorded: under-, overflow and interior bins fill"""
    first = run(golden_dir, which, 2)
    return tuple((float(np.quantile(first[v], 0.1)), float(np.quantile(first[v], 0.9))) for v in ("ab_n_mu", "ab_s_mu"))


@pytest.mark.parametrize("chains", [2, 5])  # units of 1 and of 2 chains
@pytest.mark.parametrize("which", ["dense", "test"])
def test_counters_equal_from_draws_of_the_recorded_draws(golden_dir, which, chains):
    ranges = ranges_of(golden_dir, which)
    res = run(golden_dir, which, chains, timelines=True, timeline_ranges=ranges, timelines_hist=True)
    G, N = res["i"].shape[2:]
    assert res["tl_inf"].shape == (chains, G, N) and res["tl_ninf"].shape == (chains, N, 8) and res["tl_info"].tolist() == [[DRAWS]] * chains
    assert res["tl_q_n"].shape == (3, G, N) and res["tl_q"].tolist() == [[0.025, 0.5, 0.975]] * chains
    np.testing.assert_array_equal(res["tl_range"], np.tile(np.array(ranges), (chains, 1, 1)))
    last = None if which == "dense" else TiterData.from_disk(os.path.join(golden_dir, "test_cohort")).last_gap
    check_integers(res, last_gap=last)
    check_histograms(res, ranges)
    check_quantiles(res, ranges)
    sm = tl.summary(res, last)
    np.testing.assert_array_equal(sm["cum_p"], res["tl_cum"].sum(axis=0) / (chains * DRAWS))
    one = tl.individual(res, 0, last)
    assert one["ab_s_mu"].shape == (3, one["gaps"].size)


@pytest.mark.parametrize("splits", [(30,), (20, 50)])
def test_chunks_and_follow_up(splits):
    from abdpymc_amd.sampler import sample

    N, G = 100, 70
    last = np.full(N, G - 1)
    last[::7] = -1
    last[1::5] = np.arange(N)[1::5] % G
    m = _dense_model(N, G, 2, splits=splits, last_gap=last)
    res = sample(m, tune=TUNE, draws=DRAWS, chains=2, seed=7, timelines=True, timelines_hist=True)
    m.close()
    assert (last == -1).any() and (last == G - 1).any()
    check_integers(res, splits=splits, last_gap=last)
    assert not res["tl_ninf"][:, last < 0].any() and (res["tl_ninf"][:, last >= 0].sum(axis=-1) == DRAWS).all()
    one_chunk = tl.from_draws(res["i"], None, None, last_gap=last)
    assert (one_chunk["tl_cum"] != res["tl_cum"]).any()  # (the chunks matter in this run)
    for k in tl.HIST_KEYS:
        assert (res[k].sum(axis=-1, dtype=np.int64) == DRAWS).all()


@pytest.mark.parametrize("N,G", [(40, 300), (33, 65)])  # the 8-word form; two tiles of the export and a one-gap second word
def test_shapes_of_the_walker_and_the_read_out(N, G):
    from abdpymc_amd.sampler import sample

    m = _dense_model(N, G, 2, seed=3)
    assert m.ctx.is_dense
    first = sample(m, tune=2, draws=8, chains=2, seed=5)
    # (after two tuning steps a tenth of the titers and more sit at their smallest value, the uninfected cells': the range is the
    # middle half of the recorded titers' span, so that the smallest underflow and the largest overflow)
    span = [(float(first[v].min()), float(first[v].max())) for v in ("ab_n_mu", "ab_s_mu")]
    ranges = tuple((a + 0.25 * (b - a), a + 0.75 * (b - a)) for a, b in span)
    res = sample(m, tune=2, draws=8, chains=2, seed=5, timelines=True, timeline_ranges=ranges, timelines_hist=True,
                 timeline_q=(0.0, 0.1, 0.25, 0.5, 0.6, 0.75, 0.9, 1.0))
    m.close()
    assert res["tl_q_s"].shape == (8, G, N)
    check_integers(res)
    check_histograms(res, ranges)
    check_quantiles(res, ranges)


def test_more_individuals_than_the_grid_has_waves():
    """The accumulating kernel's grid is capped at 8 workgroups of 4 waves per CU -- 8 192 waves on the MI355X's 256 CUs -- and a
    wave strides over the individuals beyond it: with 8 300 of them the first 108 waves take a second one."""
    from abdpymc_amd.sampler import sample

    N, G = 8300, 20
    m = _dense_model(N, G, 1, seed=5)
    cus = int(m.ctx.device_name.split()[-2])  # "... <n> CUs"
    assert N > cus * 8 * 4, (N, cus)
    first = sample(m, tune=2, draws=5, chains=1, seed=3)
    span = [(float(first[v].min()), float(first[v].max())) for v in ("ab_n_mu", "ab_s_mu")]
    ranges = tuple((a + 0.25 * (b - a), a + 0.75 * (b - a)) for a, b in span)
    res = sample(m, tune=2, draws=5, chains=1, seed=3, timelines=True, timeline_ranges=ranges, timelines_hist=True)
    m.close()
    check_integers(res)
    check_histograms(res, ranges)
    check_quantiles(res, ranges)
    # the individuals of the second pass have counted like the others
    assert (res["tl_ninf"][0, cus * 32:].sum(axis=-1) == 5).all() and res["tl_inf"][0, :, cus * 32:].any()


def test_thin_recording_and_plain_run(golden_dir):
    ranges = ranges_of(golden_dir, "dense")
    kw = dict(timelines=True, timeline_ranges=ranges, timelines_hist=True)
    base = run(golden_dir, "dense", 2, **kw)
    thinned = run(golden_dir, "dense", 2, thin=5, **kw)
    assert thinned["i"].shape[1] == 5
    _same_tl(thinned, base)
    unrecorded = run(golden_dir, "dense", 2, record_deterministics=False, record_discrete=False, **kw)
    assert "i" not in unrecorded and "i_raw" not in unrecorded
    _same_tl(unrecorded, base)
    plain = run(golden_dir, "dense", 2)
    assert not any(k.startswith("tl_") for k in plain)
    _same_trajectories(base, plain, keys=("i_raw", "ab_s_waner", "i", "ab_s_mu", "ab_n_mu"))
    # without timelines_hist the histograms stay on the device, the rest is the same
    lean = run(golden_dir, "dense", 2, timelines=True, timeline_ranges=ranges)
    assert not any(k in lean for k in tl.HIST_KEYS)
    _same_tl(lean, base, keys=tl.RESULT_KEYS)
    # without timeline_q no pooled quantiles are read out (a caller that pools several processes' histograms itself)
    unpooled = run(golden_dir, "dense", 2, timelines=True, timeline_ranges=ranges, timelines_hist=True, timeline_q=None)
    assert not any(k in unpooled for k in ("tl_q", "tl_q_n", "tl_q_s"))
    _same_tl(unpooled, base, keys=tl.RESULT_KEYS[:5] + tl.HIST_KEYS)


@pytest.mark.parametrize("which", ["dense", "test"])
def test_launch_configuration_changes_nothing(golden_dir, which):
    ranges = ranges_of(golden_dir, which)
    kw = dict(timelines=True, timeline_ranges=ranges, timelines_hist=True)
    _same_tl(run(golden_dir, which, 2, launch_config=(3, 1), **kw), run(golden_dir, which, 2, **kw))


def _sampler(m, chains, tune, **kw):
    pt = m.initial_point()
    q0 = np.tile(m.ravel(pt), (chains, 1))
    for c in range(chains):
        m.ctx.set_discrete(c, pt["i_raw"].astype(np.int8), pt["ab_s_waner"].astype(np.int8))
    return m.ctx.sampler(list(range(chains)), q0, tune=tune, seed=1, **kw)


RANGES = ((-1.0, 3.0), (0.0, 5.0))
Q = (0.025, 0.5, 0.975)


def _read(smp, n):
    per = [smp.timelines(k, hist=True) for k in range(n)]
    return per, smp.timeline_quantiles(Q)


@pytest.mark.parametrize("which", ["dense", "test"])
def test_cutting_the_run_into_calls_changes_nothing(golden_dir, which):
    m = _model(which, golden_dir, 2)
    whole = _sampler(m, 2, 5, timelines=(22, *RANGES))
    whole.run(27)
    a, qa = _read(whole, 2)
    whole.close()
    cut = _sampler(m, 2, 5, timelines=(22, *RANGES))
    cut.run(3)  # inside tuning: nothing counted yet
    mid = cut.timelines(0, hist=True)
    assert mid["n_draws"] == 0 and not mid["hist_n"].any() and not mid["cum"].any()
    assert np.isnan(cut.timeline_quantiles(Q)[0]).all()
    cut.run(9)
    assert cut.timelines(1)["n_draws"] == 7  # readable between the calls
    cut.run(15)
    b, qb = _read(cut, 2)
    cut.close()
    m.close()
    for x, y in zip(a, b):
        assert x["n_draws"] == y["n_draws"] == 22
        for k in ("inf", "cum", "ninf", "hist_n", "hist_s"):
            assert x[k].tobytes() == y[k].tobytes(), k
        assert x["inf"].sum() > 0 and (x["hist_n"].sum(axis=-1) == 22).all()
    for x, y in zip(qa, qb):
        assert x.tobytes() == y.tobytes()


def test_errors(golden_dir):
    m = _dense_model(100, 70, 2)
    smp = _sampler(m, 2, TUNE, timelines=(9, *RANGES))
    smp.run(TUNE + 4)
    before, _ = _read(smp, 2)
    assert before[0]["n_draws"] == 4
    with pytest.raises(AbdError, match="planned"):
        smp.run(6)  # draws 4 .. 9 pass the planned 9: refused before anything is launched
    now, _ = _read(smp, 2)
    for x, y in zip(before, now):
        for k in ("inf", "cum", "ninf", "hist_n", "hist_s"):
            assert x[k].tobytes() == y[k].tobytes(), k
    smp.run(5)  # ... and the run goes on to its planned end
    assert smp.timelines(1)["n_draws"] == 9
    # the quantiles' arguments
    for bad in ((), tuple(np.linspace(0, 1, 9)), (-0.1,), (1.5,), (np.nan,)):
        with pytest.raises(ValueError):
            smp.timeline_quantiles(bad)
    assert smp.timeline_quantiles(tuple(np.linspace(0, 1, 8)))[0].shape == (8, 70, 100)
    # enabling after the first run is a state error
    lib, enable = smp._lib, smp._lib.abd_sampler_enable_timelines
    assert enable(smp._h, 20, -4.0, 8.0, -4.0, 8.0) == -3
    smp.close()
    # without the option there is nothing to read
    smp = _sampler(m, 2, 0)
    with pytest.raises(AbdError, match="not enabled"):
        smp.timelines(0)
    with pytest.raises(AbdError, match="not enabled"):
        smp.timeline_quantiles(Q)
    # argument errors; 0 releases
    assert enable(smp._h, 65536, -4.0, 8.0, -4.0, 8.0) == -1
    assert enable(smp._h, -1, -4.0, 8.0, -4.0, 8.0) == -1
    assert enable(smp._h, 8, 1.0, 1.0, -4.0, 8.0) == -1
    assert enable(smp._h, 8, -4.0, 8.0, 2.0, 1.0) == -1
    assert enable(smp._h, 8, float("nan"), 8.0, -4.0, 8.0) == -1
    assert enable(smp._h, 8, -4.0, float("inf"), -4.0, 8.0) == -1
    assert enable(smp._h, 8, -4.0, 8.0, -1e308, 1e308) == -1
    assert b"range" in lib.abd_last_error()
    assert enable(smp._h, 65535, -4.0, 8.0, -4.0, 8.0) == 0
    assert enable(smp._h, 8, -4.0, 8.0, -4.0, 8.0) == 0
    got = smp.timelines(0, hist=True)
    assert got["n_draws"] == 0 and not got["hist_s"].any() and not got["ninf"].any()
    assert enable(smp._h, 0, 0.0, 0.0, 0.0, 0.0) == 0
    with pytest.raises(AbdError, match="not enabled"):
        smp.timelines(0)
    smp.close()
    with pytest.raises(ValueError):
        _sampler(m, 2, 0, timelines=(-1, *RANGES))
    from abdpymc_amd.sampler import sample

    with pytest.raises(ValueError, match="native"):
        sample(m, tune=1, draws=4, chains=1, native=False, timelines=True)
    with pytest.raises(ValueError, match="65535"):
        sample(m, tune=1, draws=65536, chains=1, timelines=True, record_deterministics=False, record_discrete=False)
    with pytest.raises(ValueError, match="range"):
        sample(m, tune=1, draws=4, chains=1, timelines=True, timeline_ranges=((1, 1), (-4, 8)))
    with pytest.raises(ValueError, match="timeline_q"):
        sample(m, tune=1, draws=4, chains=1, timelines=True, timeline_q=())
    with pytest.raises(ValueError, match="budget"):
        sample(m, tune=1, draws=4, chains=2, timelines=True, record_deterministics=False, record_discrete=False,
               budget_bytes=tl.result_bytes(2, 70, 100) - 1)
    m.close()


@pytest.mark.parametrize("kind", ["dense", "test"])
def test_teardown_with_the_buffers_live(golden_dir, kind):
    """create / enable / destroy without running; destroy with the buffers live after a run; the context closed first; enabled,
    dropped and enabled again"""
    from abdpymc_amd._native import _check

    m = _model(kind, golden_dir, 2)
    for _ in range(3):
        smp = _sampler(m, 2, 2, timelines=(6, *RANGES))
        smp.close()
    smp = _sampler(m, 2, 2)
    for planned in (6, 0, 6):
        _check(smp._lib, smp._lib.abd_sampler_enable_timelines(smp._h, planned, -1.0, 3.0, 0.0, 5.0))
    smp.run(8)
    first = smp.timelines(1, hist=True)
    smp.close()
    smp.close()
    smp = _sampler(m, 2, 2, timelines=(6, *RANGES))
    smp.run(8)
    again = smp.timelines(1, hist=True)
    for k in ("inf", "cum", "ninf", "hist_n", "hist_s"):
        assert first[k].tobytes() == again[k].tobytes(), k
    m.ctx.close()  # the context while its sampler holds the buffers: Context.close closes the sampler first
    assert not smp._h.value
    smp.close()
    m.close()


def test_cli_writes_the_timelines(tmp_path, golden_dir, capsys):
    from abdpymc_amd import cli

    out = tmp_path / "post.npz"
    d = os.path.join(golden_dir, "test_cohort")
    rc = cli.main(["--tune", "6", "--draws", "8", "--cores", "1", "--ititers_data", d, "--timelines", "--timeline_range_s=-2,6", "--thin", "5",
                   "--netcdf", str(out)])
    assert rc == 0
    line = [ln for ln in capsys.readouterr().err.splitlines() if ln.startswith("timelines:")]
    assert len(line) == 1 and "P(ever infected within follow-up) > 0.5" in line[0] and "95 % S band" in line[0] and "95 % N band" in line[0]
    assert "under- or overflow bin" in line[0]
    z = np.load(out)
    td = TiterData.from_disk(d)
    G, N = td.n_gaps, td.n_inds
    assert z["tl_inf"].shape == (2, G, N) and z["tl_cum"].shape == (2, G, N) and z["tl_ninf"].shape == (2, N, 8)
    assert z["tl_info"].tolist() == [[8]] * 2 and z["tl_q_n"].shape == (3, G, N) and z["tl_q_s"].shape == (3, G, N)
    assert z["tl_range"][0].tolist() == [[-4.0, 8.0], [-2.0, 6.0]]
    assert z["i"].shape[1] == 2  # (the record is thinned, the counters are not)
    assert not any(k in z.files for k in tl.HIST_KEYS)
    res = {k: z[k] for k in z.files if not k.startswith("tl_summary_")}
    arrays = tl.summary_arrays(tl.summary(res, td.last_gap))
    assert arrays.keys() == {k for k in z.files if k.startswith("tl_summary_")}
    for k, v in arrays.items():
        np.testing.assert_array_equal(z[k], v, err_msg=k)
    with pytest.raises(SystemExit, match="timeline_range_n"):
        cli.main(["--tune", "1", "--draws", "2", "--ititers_data", d, "--timelines", "--timeline_range_n=3,1"])
