"""
Every transition and adaptation step of the native sampler, replayed from its leapfrog log, through every driver.

tests/test_gpu_leapfrog_parity.py holds every logged evaluation to the oracle; tests/test_nuts_replay_cpu.py holds the host's
tree logic to tests/nuts_restatement.py on closed-form targets.  Here the same restatement replays what the sampler does with the
device's numbers on the model itself: dense train launches in units of 1, 2 and 4 chains, observation-list trains and
host-driven units -- the leaves of every tree and where it stops, the draw, the statistics, the junction of every half with the
tree END it starts from (the device enters a half by itself: abd_train.hpp), the first momentum from the restated stream, and,
with tuning on, the step size and metric after every iteration (calls of one iteration each).  Every case asserts the launch
shape, every decision must be pinned, and the worst errors are printed (pytest -s).
"""
import numpy as np
import pytest

from abdpymc_amd import synthetic
from tests import nuts_restatement as R
from tests.helpers import random_sparse_cohort
from tests.test_gpu_leapfrog_parity import INV_MASS, STEEPNESS_LISTS, _dense_case, _step_size

pytestmark = pytest.mark.gpu

SEED = 5
STATS = ("lp", "tree_depth", "n_steps", "mean_tree_accept", "step_size", "diverging", "energy", "max_energy_error")
# the step at which the ORACLE's own trajectories from the start points of the 67 x 33 cohort leave the energy shell: with
# _step_size(steepness = 100) (eps = 0.0308) the first leaves of chains 0, 1, 2 have energy errors +795, -608, -1024 and the
# second ones +11518, +5072, +13304, all at a finite logp (O.logp_dlogp, the restated stream's momenta; at steepness 200 the
# first leaf is at 1e10 already, and the second raises in the oracle)
STEEPNESS_DIVERGING = 100.0


def _sample(ctx, states, th0, n_iter, tune=0, depth=5, gibbs=False, installs=None, dense_metric=False, stepwise=False, log=True):
    """One sampler over all of the context's chains -> dict of the log, the draws, the stats and, for a stepwise run (calls of one
    iteration), adaptation(k) and metric(k) after every iteration.  installs: {iteration: (inv_mass or None, step size)}, applied
    to every chain before that iteration."""
    C = len(states)
    installs = installs or {}
    for c in range(C):
        ctx.set_discrete(c, *states[c])
    smp = ctx.sampler(np.arange(C), th0, tune=tune, seed=SEED, max_treedepth=depth, gibbs=gibbs, dense_metric=dense_metric)
    if log:
        smp.enable_leapfrog_log(1 + n_iter * 2 ** depth)  # per iteration at most 2^depth - 1 leaves and a start row
    theta, stats = np.empty((C, n_iter, 17)), {k: np.empty((C, n_iter)) for k in STATS}
    eps, im, met = np.empty((C, n_iter)), np.empty((C, n_iter, 17)), np.empty((C, n_iter, 17, 17))
    it = 0
    while it < n_iter:
        if it in installs:
            for c in range(C):
                smp.set_adaptation(c, *installs[it])
        n = 1 if stepwise else min([k for k in installs if k > it] + [n_iter]) - it
        th, st = smp.run(n)
        theta[:, it:it + n] = th
        for k in STATS:
            stats[k][:, it:it + n] = st[k]
        if stepwise:
            for c in range(C):
                im[c, it], eps[c, it] = smp.adaptation(c)
                met[c, it] = smp.metric(c)
        it += n
    out = dict(theta=theta, stats=stats, shape=smp.launch_shape(), fallbacks=ctx.wait_fallbacks, n_iter=n_iter, tune=tune, depth=depth,
               gibbs=gibbs, installs=installs, dense_metric=dense_metric, logs=[smp.leapfrog_log(c) for c in range(C)] if log else None,
               eps=eps if stepwise else None, inv_mass=im if stepwise else None, metric=met if stepwise else None)
    smp.close()
    return out


def _replay(run, label):
    """every chain of a run against the restatement -> (Tally, the chains' adaptation events); prints the worst errors seen"""
    total, events = R.Tally(), []
    for c, (rows, n_total) in enumerate(run["logs"]):
        assert n_total == len(rows), (label, c, n_total, len(rows))  # nothing was dropped
        t, _, ev = R.replay_chain(rows, {k: v[c] for k, v in run["stats"].items()}, SEED, c, run["tune"], run["depth"], run["n_iter"],
                                  dense=run["dense_metric"], installs=run["installs"], sweep=run["gibbs"], draws=run["theta"][c],
                                  eps_after=None if run["eps"] is None else run["eps"][c],
                                  inv_mass_after=None if run["inv_mass"] is None else run["inv_mass"][c],
                                  metric_after=None if run["metric"] is None else run["metric"][c])
        total.merge(t)
        events.append(ev)
    print(f"\nNUTS replay {label}: {total}; launch {run['shape']}")
    assert total.pinned(), (label, str(total))
    assert total.events["transitions"] == run["n_iter"] * len(run["logs"])
    return total, events


def _assert_shape(run, unit, trains, workgroups=None):
    assert run["shape"]["unit"] == unit and run["shape"]["trains"] == trains, run["shape"]
    assert workgroups is None or run["shape"]["workgroups"] == workgroups, run["shape"]
    assert run["fallbacks"] == 0


# dense 67 x 33, one-level sums: (chains, ABD_SAMPLER_UNIT, chains per unit, trains, storage, workgroups with a range)
DENSE = {
    "unit 1": (3, 1, 1, True, "f64", 4),
    "unit 2": (3, 2, 2, True, "f64", 8),
    "unit 4": (4, 4, 4, True, "f64", 16),
    "host-driven": (2, 2, 2, False, "f64", 8),
    "unit 2 f32": (3, 2, 2, True, "f32", 8),
}


def _fixed(eps):
    return {0: (INV_MASS, eps)}


@pytest.mark.parametrize("gibbs", [False, True])
@pytest.mark.parametrize("case", ["unit 1", "unit 2", "unit 4", "host-driven"])
def test_fixed_adaptation_on_every_dense_driver(monkeypatch, case, gibbs):
    """tune 0, the spread diagonal metric and the oracle's step size of the leapfrog parity test, trees up to depth 5, 12
    iterations: units of 1, 2 (as 2 + 1) and 4 chains on the train kernels, and a host-driven unit."""
    C, unit_env, unit, trains, storage, wg = DENSE[case]
    ctx, states, th0, eps, _, _ = _dense_case(monkeypatch, 67, 33, C, unit_env, storage=storage, trains=trains)
    run = _sample(ctx, states, th0, 12, gibbs=gibbs, installs=_fixed(eps))
    ctx.close()
    _assert_shape(run, unit, "dense" if trains else "none", wg)
    tally, _ = _replay(run, f"67x33 {case} gibbs {gibbs}")
    assert tally.events["later_half_junctions"] >= C and tally.events["leaves"] > 12 * C


def test_fixed_adaptation_on_f32_storage(monkeypatch):
    C, unit_env, unit, trains, storage, wg = DENSE["unit 2 f32"]
    ctx, states, th0, eps, _, _ = _dense_case(monkeypatch, 67, 33, C, unit_env, storage=storage, trains=trains)
    run = _sample(ctx, states, th0, 12, gibbs=True, installs=_fixed(eps))
    ctx.close()
    _assert_shape(run, unit, "dense", wg)
    _replay(run, "67x33 unit 2 f32")


def _list_case(monkeypatch, trains, C=2):
    from abdpymc_amd._native import Context

    G, N = 31, 29
    splits = (10, 21)
    coh = random_sparse_cohort(N, G, 420, 380, seed=78)
    monkeypatch.setenv("ABD_SAMPLER_UNIT", "1")
    monkeypatch.setenv("ABD_SAMPLER_TRAINS", "1" if trains else "0")
    ctx = Context(G, N, (coh.s.idx_gap, coh.s.idx_ind, coh.s.log_dilution, coh.s.od),
                  (coh.n.idx_gap, coh.n.idx_ind, coh.n.log_dilution, coh.n.od), coh.vacs, coh.pcrpos, splits=splits, n_chains=C)
    assert not ctx.is_dense
    rng = np.random.default_rng(5)
    states = [((rng.random((G, N)) < 2.0 / G).astype(np.int8), (rng.random(N) < 0.5).astype(np.int8)) for _ in range(C)]
    th0 = np.stack([synthetic.make_thetas(G, 1, c)[0] for c in range(C)])
    return ctx, states, th0, _step_size(coh, splits, states, th0, STEEPNESS_LISTS)


@pytest.mark.parametrize("gibbs", [False, True])
@pytest.mark.parametrize("trains", [True, False])
def test_fixed_adaptation_on_observation_lists(monkeypatch, trains, gibbs):
    """a sparse cohort of 29 x 31: list trains (one chain per unit, a train ends with its half) and host-driven"""
    ctx, states, th0, eps = _list_case(monkeypatch, trains)
    run = _sample(ctx, states, th0, 12, gibbs=gibbs, installs=_fixed(eps))
    ctx.close()
    _assert_shape(run, 1, "lists" if trains else "none")
    _replay(run, f"lists 29x31 trains {trains} gibbs {gibbs}")


def test_a_long_two_level_launch_with_stale_look_ahead(monkeypatch):
    """380 x 190, units of four (4 + 2), 285 workgroups summing in two levels, sweep on, depth 3: the launches run several steps
    ahead of the host, which stops them behind the end of a tree"""
    ctx, states, th0, eps, _, _ = _dense_case(monkeypatch, 380, 190, 6, 4)
    run = _sample(ctx, states, th0, 5, depth=3, gibbs=True, installs=_fixed(eps))
    ctx.close()
    _assert_shape(run, 4, "dense", 285)
    _replay(run, "380x190 unit 4")


def test_the_depth_cap_ends_trees(monkeypatch):
    C, unit_env, unit, trains, storage, wg = DENSE["unit 2"]
    ctx, states, th0, eps, _, _ = _dense_case(monkeypatch, 67, 33, C, unit_env)
    run = _sample(ctx, states, th0, 12, depth=2, gibbs=True, installs=_fixed(eps))
    ctx.close()
    _assert_shape(run, unit, "dense", wg)
    tally, _ = _replay(run, "67x33 unit 2 depth 2")
    assert tally.events["capped"] >= 1 and run["stats"]["n_steps"].max() == 3


def test_divergent_transitions(monkeypatch):
    """A step size at which the oracle's own trajectories exceed an energy error of 1000 at a finite logp (STEEPNESS_DIVERGING)."""
    C, unit_env, unit, trains, storage, wg = DENSE["unit 2"]
    ctx, states, th0, _, ref, splits = _dense_case(monkeypatch, 67, 33, C, unit_env)
    eps = _step_size(ref, splits, states, th0, STEEPNESS_DIVERGING)
    run = _sample(ctx, states, th0, 6, gibbs=False, installs=_fixed(eps))
    ctx.close()
    _assert_shape(run, unit, "dense", wg)
    tally, _ = _replay(run, "67x33 unit 2 diverging")
    assert tally.events["divergent"] - tally.events["non_finite"] >= 1 and run["stats"]["diverging"].any()
    assert tally.margin["divergence"] > 1.0


TUNE, DRAWS, TUNE_DEPTH = 230, 10, 4


def test_tuning_on_dense_trains_step_by_step(monkeypatch):
    """tune 230 and 10 draws in calls of one iteration, sweep on: the step size of every iteration against the restated dual
    average, adaptation(k) after every iteration against the two-pass variance, through both window switches and the last tenth.
    One twin sampler runs the 240 iterations in one call: the same draws, bit for bit."""
    C, unit_env, unit, trains, storage, wg = DENSE["unit 2"]
    ctx, states, th0, _, _, _ = _dense_case(monkeypatch, 67, 33, C, unit_env)
    run = _sample(ctx, states, th0, TUNE + DRAWS, tune=TUNE, depth=TUNE_DEPTH, gibbs=True, stepwise=True)
    twin = _sample(ctx, states, th0, TUNE + DRAWS, tune=TUNE, depth=TUNE_DEPTH, gibbs=True, log=False)
    ctx.close()
    _assert_shape(run, unit, "dense", wg)
    _assert_shape(twin, unit, "dense", wg)
    np.testing.assert_array_equal(run["theta"][0], twin["theta"][0])
    np.testing.assert_array_equal(run["theta"], twin["theta"])
    tally, _ = _replay(run, "67x33 unit 2 tuning")
    assert 0.0 < tally.worst["metric"] <= 1.0 and 0.0 < tally.worst["eps"] <= 4 * R.E_NP_STEP


def test_tuning_on_list_trains_step_by_step(monkeypatch):
    ctx, states, th0, _ = _list_case(monkeypatch, True)
    run = _sample(ctx, states, th0, TUNE + DRAWS, tune=TUNE, depth=TUNE_DEPTH, gibbs=True, stepwise=True)
    ctx.close()
    _assert_shape(run, 1, "lists")
    tally, _ = _replay(run, "lists 29x31 tuning")
    assert 0.0 < tally.worst["metric"] <= 1.0 and 0.0 < tally.worst["eps"] <= 4 * R.E_NP_STEP


def test_the_dense_metric_step_by_step(monkeypatch):
    """dense_metric: host-driven by construction; tune 200: the 10-draw window is refused, 20, 40 and the stretched 105 install,
    the dual average restarts, metric(k) stands still in between, and the momentum solves L^T p0 = z."""
    ctx, states, th0, _, _, _ = _dense_case(monkeypatch, 67, 33, 2, 2)
    run = _sample(ctx, states, th0, 210, tune=200, depth=TUNE_DEPTH, gibbs=True, dense_metric=True, stepwise=True)
    ctx.close()
    _assert_shape(run, run["shape"]["unit"], "none")
    tally, events = _replay(run, "67x33 dense metric")
    for ev in events:
        assert ev["dense_refused"] == [(24, 10)] and [n for _, n in ev["dense_installed"]] == [20, 40, 105], ev
    assert tally.worst["dense_p0"] > 0 and tally.worst["metric"] <= 1.0


def test_an_installation_while_tuning(monkeypatch):
    """set_adaptation before iteration 0 and, in the middle of a variance window, before iteration 120 of 230 tuning iterations:
    the next transition logs the installed step size bit for bit and moves under the installed metric, every later iteration
    follows the restated adaptation from the re-seeded state (abd_nuts.hpp: AdaptiveNuts::install)."""
    C, unit_env, unit, trains, storage, wg = DENSE["unit 2"]
    ctx, states, th0, eps, _, _ = _dense_case(monkeypatch, 67, 33, C, unit_env)
    installs = {0: (INV_MASS, eps), 120: (INV_MASS[::-1].copy(), 0.5 * eps)}
    run = _sample(ctx, states, th0, TUNE + DRAWS, tune=TUNE, depth=TUNE_DEPTH, gibbs=True, installs=installs, stepwise=True)
    ctx.close()
    _assert_shape(run, unit, "dense", wg)
    tally, events = _replay(run, "67x33 unit 2 installed while tuning")
    assert np.all(run["stats"]["step_size"][:, 0] == eps) and np.all(run["stats"]["step_size"][:, 120] == 0.5 * eps)
    assert all(ev["da_restarts"] == [0, 120] for ev in events)
    assert np.all(run["inv_mass"][:, 120] >= INV_MASS[::-1] * (10.0 / 11.0) * (1 - 1e-12))  # not gone after one transition
    assert tally.worst["metric"] <= 1.0
