"""
Every transition and adaptation step of the NUTS host logic (abd_nuts.hpp), replayed from the leapfrog log on the CPU.

tests/nuts_restatement.py states the algorithm; here the classic driver and the restated train protocol of
tests/native/nuts_harness.cpp run on closed-form targets with the log on, and every transition of every run must be the
restatement's: the same leaves in the same order and nothing beyond them, the draw the selected leaf bit for bit, tree_depth,
n_steps, diverging and lp equal, energy, max_energy_error and mean_tree_accept within the energy budget, every junction of a
half with the tree end it starts from within the integrator's gates, the step size within 4 E_np of the restated dual average,
the metric within the Welford gate of the two-pass variance.  Every decision of every run must be pinned (the restatement's
docstring: the measures); the remedy for a miss is another seed, never a looser rule.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import nuts_restatement as R
from tests.test_nuts_native import _correlated_target, _run_logged, harness  # noqa: F401  (harness: the fixture that builds the library)

STAT_NAMES = ("lp", "tree_depth", "n_steps", "mean_tree_accept", "step_size", "diverging", "energy", "max_energy_error")
INST_COLS = 4 + R.D


def _mild_target():
    """17 independent normals within a factor four of each other: the unit metric and the initial step build real trees"""
    rng = np.random.default_rng(6)
    return rng.normal(size=17) * 3, np.exp(rng.uniform(np.log(0.5), np.log(2.0), size=17))


def _scaled_target():
    """... over a decade and a half: the diagonal adaptation has something to find"""
    rng = np.random.default_rng(5)
    return rng.normal(size=17) * 3, np.exp(rng.uniform(np.log(0.1), np.log(3.0), size=17))


def _run_adapt(lib_path, mean, sd, tune, draws, seed, chains, prec=None, dense=False, eval_first=False, max_depth=10, installs=()):
    """nuts_harness_run_adapt -> dict; installs: (iteration, chain, inv_mass or None, step size) each"""
    lib = C.CDLL(lib_path)
    dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_longlong)
    fn = lib.nuts_harness_run_adapt
    fn.argtypes = [dp, dp, dp, C.c_longlong, C.c_longlong, C.c_ulonglong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, dp, C.c_longlong,
                   dp, lp, dp, dp, dp, dp, dp]
    fn.restype = C.c_int
    T = tune + draws
    cap = 1 + T * (1 + 2 ** min(max_depth, 10))
    mean, sd = np.ascontiguousarray(mean, dtype=np.float64), np.ascontiguousarray(sd, dtype=np.float64)
    pp = None
    if prec is not None:
        prec = np.ascontiguousarray(prec, dtype=np.float64)
        pp = prec.ctypes.data_as(dp)
    inst = np.zeros((max(len(installs), 1), INST_COLS))
    for i, (it, c, im, eps) in enumerate(installs):
        inst[i, :4] = it, c, im is not None, eps
        if im is not None:
            inst[i, 4:] = im
    buf = np.full((chains * cap + 1, R.LOG_COLS), -7.0)
    n_total = np.full(chains, -1, dtype=np.longlong)
    q, st = np.empty((chains, T, 17)), np.empty((chains, T, 8))
    eps, im, met = np.empty((chains, T)), np.empty((chains, T, 17)), np.empty((chains, T, 17, 17))
    refused = fn(mean.ctypes.data_as(dp), sd.ctypes.data_as(dp), pp, tune, draws, seed, chains, int(dense), int(eval_first), max_depth,
                 len(installs), inst.ctypes.data_as(dp), cap, buf.ctypes.data_as(dp), n_total.ctypes.data_as(lp), q.ctypes.data_as(dp),
                 st.ctypes.data_as(dp), eps.ctypes.data_as(dp), im.ctypes.data_as(dp), met.ctypes.data_as(dp))
    assert np.all(buf[-1] == -7.0) and np.all(n_total <= cap) and np.all(n_total > 0)
    rows = [buf[c * cap:c * cap + int(n_total[c])] for c in range(chains)]
    return dict(rows=rows, q=q, stats=[{k: st[c, :, i] for i, k in enumerate(STAT_NAMES)} for c in range(chains)], eps=eps, inv_mass=im,
                metric=met, refused=refused, tune=tune, T=T, seed=seed, dense=dense, max_depth=max_depth, installs=installs, chains=chains)


def _replay(run):
    """every chain of a harness run against the restatement -> (Tally over the chains, the chains' adaptation events)"""
    total, events = R.Tally(), []
    for c in range(run["chains"]):
        inst = {it: (im, eps) for it, k, im, eps in run["installs"] if k == c}
        t, _, ev = R.replay_chain(run["rows"][c], run["stats"][c], run["seed"], c, run["tune"], run["max_depth"], run["T"], dense=run["dense"],
                                  installs=inst, eps_after=run["eps"][c], inv_mass_after=run["inv_mass"][c], metric_after=run["metric"][c],
                                  draws=run["q"][c])
        total.merge(t)
        events.append(ev)
    return total, events


INSTALLED_METRIC = 10.0 ** (((np.arange(17) * 5) % 17) / 16.0 - 0.5)


@functools.lru_cache(maxsize=None)
def _case(lib_path, name):
    """One committed case, run and replayed once -> (the run, its Tally, its adaptation events)"""
    if name == "fixed":  # tune 0: the initial step and the unit metric for all 300 transitions
        run = _run_adapt(lib_path, *_mild_target(), 0, 300, 11, 1)
    elif name == "diagonal":  # both window switches (101, 202), the depth cap of the first 200, the last tenth, the final step size
        run = _run_adapt(lib_path, *_scaled_target(), 260, 40, 12, 2)
    elif name == "dense":
        mean, cov = _correlated_target()
        run = _run_adapt(lib_path, mean, np.sqrt(np.diag(cov)), 200, 30, 21, 1, prec=np.linalg.inv(cov), dense=True, eval_first=True)
    elif name == "installed":  # set_adaptation while tuning: before the first transition and in the middle of a window
        mean, sd = _scaled_target()
        run = _run_adapt(lib_path, mean, sd, 260, 20, 14, 2, installs=((0, 0, sd ** 2, 0.4), (0, 1, None, 0.05), (120, 0, INSTALLED_METRIC, 0.2),
                                                                        (120, 1, INSTALLED_METRIC, 0.0)))
    elif name == "short":  # the cap ends the trees
        run = _run_adapt(lib_path, *_mild_target(), 0, 60, 15, 2, max_depth=2)
    elif name == "large step":  # chain 0: energy errors beyond 1000; chain 1: a first leaf so far out that logp is -inf
        run = _run_adapt(lib_path, *_mild_target(), 0, 40, 16, 2, installs=((0, 0, None, 1.3), (0, 1, None, 1e78)))
    else:
        raise KeyError(name)
    tally, events = _replay(run)
    print(f"\nNUTS replay [{name}]: {tally}")
    return run, tally, events


ADAPT_CASES = ("fixed", "diagonal", "dense", "installed", "short", "large step")


@pytest.mark.parametrize("name", ADAPT_CASES)
def test_every_transition_is_the_restatements_and_every_decision_is_pinned(harness, name):
    run, tally, _ = _case(harness.lib_path, name)
    assert run["refused"] == 0
    assert tally.events["transitions"] == run["T"] * run["chains"]
    assert tally.pinned(), str(tally)
    assert tally.n["divergence"] > 0 and (name == "large step" or tally.n["select"] > 0)


def test_trees_of_every_ending_occur(harness):
    """What the cases are there for: several doublings with halves that start from an end many leaves back, sub-tree and whole-tree
    U-turns, trees the cap ends, divergences by energy error and by a non-finite logp, transitions that keep their start point."""
    _, fixed, _ = _case(harness.lib_path, "fixed")
    assert fixed.events["later_half_junctions"] > 300 and fixed.events["subtree_turn"] > 10 and fixed.events["tree_turn"] > 10
    assert fixed.events["divergent"] == 0 and fixed.n["merge"] > 600
    _, short, _ = _case(harness.lib_path, "short")
    assert short.events["capped"] >= 1 and short.events["leaves"] <= 3 * short.events["transitions"]
    run, large, _ = _case(harness.lib_path, "large step")
    assert large.events["divergent"] >= 2 and large.events["non_finite"] >= 1 and large.events["divergent"] > large.events["non_finite"]
    assert run["stats"][0]["diverging"].any() and np.isinf(run["stats"][1]["max_energy_error"]).any()
    _, diag, _ = _case(harness.lib_path, "diagonal")
    assert diag.events["start_kept"] > 0
    _, dense, _ = _case(harness.lib_path, "dense")
    assert dense.events["capped"] > 0  # the early cap of 8, on a correlated target under a diagonal metric


def test_the_diagonal_adaptation_follows_its_closed_forms(harness):
    run, tally, events = _case(harness.lib_path, "diagonal")
    assert 0.0 < tally.worst["metric"] <= 1.0 and 0.0 < tally.worst["eps"] <= 4 * R.E_NP_STEP
    im = run["inv_mass"]
    last = R.diag_updates_end(run["tune"])
    assert np.all(im[:, last - 1] != im[:, last - 2]) and np.all(im[:, last:] == im[:, last - 1:last])  # updates stop where PyMC's do
    assert np.all(run["eps"][:, run["tune"] - 1:] == run["eps"][:, run["tune"] - 1:run["tune"]])


def test_the_dense_schedule_refuses_installs_restarts_and_stretches(harness):
    run, tally, events = _case(harness.lib_path, "dense")
    for ev in events:
        assert ev["windows"] == [(15, 25), (25, 45), (45, 85), (85, 190)]  # 10, 20, 40 draws; the last one stretched from 80 to 105
        assert ev["dense_refused"] == [(24, 10)]  # 10 draws are no more than 17: no metric
        assert ev["dense_installed"] == [(44, 20), (84, 40), (189, 105)]
        assert ev["da_restarts"] == [44, 84, 189]
    met = run["metric"]
    for c in range(run["chains"]):
        assert np.count_nonzero(met[c, 43] - np.diag(np.diag(met[c, 43]))) == 0 and np.count_nonzero(met[c, 44] - np.diag(np.diag(met[c, 44]))) > 200
    assert tally.worst["dense_p0"] > 0 and tally.worst["metric"] <= 1.0


def test_an_installation_while_tuning_is_what_the_chain_goes_on_from(harness):
    """AdaptiveNuts::install at iteration 0 and in the middle of a window at 120: the next transition logs the installed step size
    bit for bit and moves under the installed metric (both asserted by the replay: replay_chain's eps_exact and junction gates),
    and every later iteration follows the restated adaptation from the re-seeded state.  A chain given a metric alone keeps its
    dual average, a chain given a step size alone keeps its variance windows."""
    run, tally, events = _case(harness.lib_path, "installed")
    assert events[0]["da_restarts"] == [0, 120] and events[1]["da_restarts"] == [0]
    assert run["stats"][0]["step_size"][0] == 0.4 and run["stats"][0]["step_size"][120] == 0.2 and run["stats"][1]["step_size"][0] == 0.05
    assert run["stats"][1]["step_size"][120] == run["eps"][1, 119]
    # not gone after one transition: one draw on a prior of weight 10 leaves at least 10 / 11 of the installed variance, and adds to it
    assert np.all(run["inv_mass"][:, 120] >= INSTALLED_METRIC * (10.0 / 11.0) * (1 - 1e-12))
    assert tally.worst["metric"] <= 1.0


@pytest.mark.parametrize("eval_first", [0, 1])
def test_the_train_driver_builds_the_restatements_trees(harness, eval_first):
    """The restated device protocol (nuts_harness_run_logged, trains = 1): the device enters every half by itself, the host adopts
    its points -- the junctions of the halves are the device's arithmetic here."""
    mean, sd = _mild_target()
    chains, draws, seed = 2, 60, 17
    rows, n_total, q, st = _run_logged(harness.lib_path, mean, sd, 0, draws, seed, chains, 1, eval_first, 3, 1 + draws * 1025)
    total = R.Tally()
    for c in range(chains):
        assert n_total[c] == len(rows[c])
        stats = {k: st[c, :, i] for i, k in enumerate(STAT_NAMES[:6])}
        t, _, _ = R.replay_chain(rows[c], stats, seed, c, 0, 10, draws, draws=q[c])
        total.merge(t)
    print(f"\nNUTS replay [trains, eval_first={eval_first}]: {total}")
    assert total.pinned(), str(total)
    assert total.events["later_half_junctions"] > 100 and total.events["leaves"] > 1000


def test_E_np_of_the_restated_dual_average(harness):
    """The float64 dual average of the restatement against the same recursion in 40 digits, over every committed case that tunes"""
    worst = 0.0
    for name in ("diagonal", "dense", "installed"):
        _, _, events = _case(harness.lib_path, name)
        e = max(ev["E_np"] for ev in events)
        print(f"E_np[{name}] = {e:.3e}")
        worst = max(worst, e)
    assert 0.0 < worst <= R.E_NP_STEP, worst


def test_the_stream_restated_in_integers():
    """xoshiro256++ / splitmix64 known answers: the state after seeding is splitmix64's published sequence for the seed word"""
    r = R.Rng(0, 0)
    assert R.Rng(0, 2 ** 64 - 1).s == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F, 0xF88BB8A8724C81EC]  # splitmix64 from 0: (stream + 1) wraps to 0
    a = [r.next() for _ in range(3)]
    b = R.Rng(0, 1)
    assert a != [b.next() for _ in range(3)] and all(0 <= v < 2 ** 64 for v in a)
    n = [R.Rng(3, 4).normal() for _ in range(1)]
    g = R.Rng(3, 4)
    first, second = g.normal(), g.normal()
    assert first == n[0] and g.spare is None and abs(first) < 10 and abs(second) < 10
