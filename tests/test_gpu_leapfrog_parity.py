"""
Every evaluation the native sampler consumes, against the oracle, at the launch shapes the sampler really uses.

The sampler's leapfrog log (abd_hip.h: abd_sampler_enable_leapfrog_log; abd_nuts.hpp: LeapfrogLog) holds one row per
evaluation handed to a chain's NUTS state: the point, logp, the gradient, the half-kicked momentum.  Here every row of short
runs is compared with ``O.logp_dlogp`` at the row's point and discrete state -- logp and every gradient entry at the
project's 1e-6 (test_gpu_parity.assert_close), logp also at the 1e-9 the sampler tests use for a recorded logp -- and
consecutive leaves of a half with the leapfrog in plain numpy.  The shapes are the smallest that reach each branch of a dense
train launch on 256 CUs (ranges of about four rows): more than 256 workgroups sum their partial rows in two levels
(abd_dense.hpp: two_level_sums: 32 shards of uneven length, a step mask for the unit's chains that sit a launch out), and
units of 2 and 4 chains read the split panels in kernel forms no evaluation launch has.  Every case asserts the workgroup
count the sampler reports (abd_sampler_launch_shape), so a change of the launch plan cannot move it to another branch
unnoticed.

Step size and metric are fixed (tune = 0, set_adaptation): a diagonal metric spread over more than a decade and a step size
worked out from the ORACLE's gradient at the start points (_step_size), at which the seven leapfrogs of a tree of depth 3 move
the point by up to a few tenths and the gradient by some percent, the energy error stays far from a divergence, and -- a
factor 10 or more below the step at which the oracle's trajectories leave the finite range -- every logged logp is finite
(asserted, not filtered).
"""
import functools

import numpy as np
import pytest

from abdpymc_amd import synthetic
from oracle import abd_oracle as O
from tests.helpers import oracle_cohort_from_synth, random_sparse_cohort
from tests.test_gpu_exposure_planes import _cohort
from tests.test_gpu_parity import assert_close

pytestmark = pytest.mark.gpu

N_ITER, DEPTH = 5, 3  # up to 5 x 7 leaves per chain; many trees turn earlier: of the order of a hundred oracle evaluations per case
N_SAME = 3            # transitions a train run and a host-driven run are compared over (later ones may part ways: a decision on a knife's edge)
LP_RTOL = 1e-9
# diagonal of M^-1: 17 entries spread over a decade and a half, in no particular order
INV_MASS = 10.0 ** (((np.arange(17) * 7) % 17) / 16.0 * 1.5 - 0.75)
EPS_DOUBLE = 2.0 ** -52
# _step_size: oracle trajectories of seven leapfrogs from these starts -- dense cohorts: |energy error| < 30 at 30, non-finite at
# 1000; the observation lists below: |energy error| < 2 at 3, non-finite at 30
STEEPNESS, STEEPNESS_LISTS = 30.0, 3.0


@functools.lru_cache(maxsize=None)
def _dense_cohort(N, G, kind):
    """(synthetic cohort, the oracle's cohort, the oracle's cohort on fp32-rounded panels), made once per shape and kind"""
    sc = _cohort(N, G, kind)
    coh = oracle_cohort_from_synth(sc)
    r32 = lambda a: a.astype(np.float32).astype(np.float64)
    coh32 = O.Cohort(coh.n_gaps, coh.n_inds, coh.vacs, coh.pcrpos,
                     O.AntigenObs(coh.s.idx_gap, coh.s.idx_ind, r32(coh.s.log_dilution), r32(coh.s.od)),
                     O.AntigenObs(coh.n.idx_gap, coh.n.idx_ind, r32(coh.n.log_dilution), r32(coh.n.od)))
    return sc, coh, coh32


def _starts(N, G, C):
    states = [synthetic.make_chain_state(N, G, c) for c in range(C)]
    th0 = np.stack([synthetic.make_thetas(G, 1, c)[0] for c in range(C)])
    return states, th0


def _step_size(coh, splits, states, th0, steepness=None):
    """A leapfrog from rest moves logp by eps^2 / 2 * sum(M^-1 g^2), a momentum draw p ~ N(0, M) by eps sqrt(sum(M^-1 g^2)) z:
    eps = steepness / sqrt(sum(M^-1 g^2)) at the steepest start point (the oracle's gradient) makes the first of order
    steepness^2 / 2, the second of order steepness."""
    steep = max(float((INV_MASS * O.logp_dlogp(th0[c], *states[c], coh, splits)[1] ** 2).sum()) for c in range(len(states)))
    return (steepness or STEEPNESS) / np.sqrt(steep)


def _run(ctx, states, th0, eps, gibbs=False, log=True, n_iter=N_ITER, seed=5):
    """One sampler over all of the context's chains from the given starts -> dict of what it logged, drew and recorded"""
    C = len(states)
    G, N = states[0][0].shape
    for c in range(C):
        ctx.set_discrete(c, *states[c])
    smp = ctx.sampler(np.arange(C), th0, tune=0, seed=seed, max_treedepth=DEPTH, gibbs=gibbs)
    for c in range(C):
        smp.set_adaptation(c, INV_MASS, eps)
    if log:
        smp.enable_leapfrog_log(1 + n_iter * (2 ** DEPTH))  # the start point, then per iteration at most 2^DEPTH - 1 leaves and a start row
    rec = dict(i_raw=np.zeros((C, n_iter, G, N), np.int8), ab_s_waner=np.zeros((C, n_iter, N), np.int8))
    theta, stats = smp.run_record(n_iter, 0, **rec)
    out = dict(theta=theta, stats=stats, rec=rec, shape=smp.launch_shape(), fallbacks=ctx.wait_fallbacks, gibbs=gibbs, n_iter=n_iter,
               states=states, eps=eps, logs=[smp.leapfrog_log(c) for c in range(C)] if log else None)
    smp.close()
    return out


def _ulp(x):
    return EPS_DOUBLE * np.abs(x)


def _check_rows(run, coh, splits, label, integrator=True):
    """Every logged row of every chain against the oracle under the discrete state the iteration rule names; the structure of the
    log; the leapfrog between consecutive leaves of a half.  Prints the worst errors seen (pytest -s)."""
    n_iter, worst = run["n_iter"], dict(lp=0.0, g=0.0, q=0.0, p=0.0)
    for c, (rows, n_total) in enumerate(run["logs"]):
        assert n_total == len(rows), (label, c, n_total, len(rows))  # nothing was dropped
        kind, it = rows["kind"], rows["iteration"].astype(int)
        assert kind[0] == 0 and it[0] == 0 and np.all(kind[1:] > 0)
        assert np.all(np.diff(it) >= 0) and it.max() <= n_iter
        assert np.isfinite(rows["lp"]).all() and np.isfinite(rows["g"]).all() and np.isfinite(rows["q"]).all(), (label, c)
        # a transition's start point is evaluated again exactly when a sweep ran before it: behind every iteration of the run
        np.testing.assert_array_equal(it[kind == 1], np.arange(1, n_iter + 1) if run["gibbs"] else [])
        leaves = np.bincount(it[kind == 2], minlength=n_iter)
        np.testing.assert_array_equal(leaves[:n_iter], run["stats"]["n_steps"][c])
        assert np.all(rows["eps"] == run["eps"]) and np.all(np.abs(rows["dir"][kind == 2]) == 1)
        for r in rows:
            k = int(r["iteration"])
            if run["gibbs"] and k > 0:  # the state the sweep of iteration k - 1 left
                i_raw, w = run["rec"]["i_raw"][c, k - 1], run["rec"]["ab_s_waner"][c, k - 1]
            else:
                i_raw, w = run["states"][c]
            lp_ref, g_ref = O.logp_dlogp(r["q"], i_raw, w, coh, splits)
            assert np.isfinite(lp_ref) and np.isfinite(g_ref).all(), (label, c, k)
            worst["lp"] = max(worst["lp"], abs(r["lp"] - lp_ref) / abs(lp_ref))
            worst["g"] = max(worst["g"], float((np.abs(r["g"] - g_ref) / np.maximum(np.abs(g_ref), 1e-6 * np.abs(g_ref).max())).max()))
            assert_close(r["lp"], r["g"], lp_ref, g_ref)
            assert abs(r["lp"] - lp_ref) <= LP_RTOL * abs(lp_ref), (label, c, k, r["lp"], lp_ref)
        # the recorded logp of a draw is a logged row's: the leaf the tree proposed or the start point, evaluated again after a sweep
        if run["gibbs"]:
            np.testing.assert_array_equal(run["stats"]["lp"][c], rows["lp"][kind == 1])
        if not integrator:
            continue
        # consecutive leaves a, b of one half: q_b = q_a + ve M^-1 (p_half_a + ve g_a), p_half_b = p_half_a + ve g_a (abd_nuts.hpp:
        # stage_leapfrog; abd_train.hpp: train_stage).  The position within 16 ulp of max(|q_a|, |ve M^-1 p_half_b|) per entry: five
        # roundings, contracted or not.  The momentum within 8 ulp of max(|p_half_a|, |ve g_a|): the device adds the half kick
        # 0.5 ve g twice (four roundings, the sum in between up to twice as large), numpy one product and one sum
        a, b = rows[:-1], rows[1:]
        pair = (a["kind"] == 2) & (b["kind"] == 2) & (a["iteration"] == b["iteration"]) & (a["depth"] == b["depth"]) & (b["n_leaf"] == a["n_leaf"] + 1)
        a, b = a[pair], b[pair]
        ve = (a["dir"] * a["eps"])[:, None]
        q_np = a["q"] + ve * INV_MASS * (a["p_half"] + ve * a["g"])
        q_bound = 16 * _ulp(np.maximum(np.abs(a["q"]), np.abs(ve * INV_MASS * b["p_half"])))
        p_bound = 8 * _ulp(np.maximum(np.abs(a["p_half"]), np.abs(ve * a["g"])))
        p_np = a["p_half"] + ve * a["g"]
        if len(a):
            worst["q"] = max(worst["q"], float((np.abs(b["q"] - q_np) / (q_bound / 16)).max()))
            worst["p"] = max(worst["p"], float((np.abs(b["p_half"] - p_np) / (p_bound / 8)).max()))
        assert np.all(np.abs(b["q"] - q_np) <= q_bound), (label, c)
        assert np.all(np.abs(b["p_half"] - p_np) <= p_bound), (label, c)
        run.setdefault("pairs", 0)
        run["pairs"] += int(pair.sum())
    print(f"\nleapfrog parity {label}: {sum(len(r) for r, _ in run['logs'])} rows, worst rel. error lp {worst['lp']:.2e}, gradient {worst['g']:.2e}, "
          f"integrator q {worst['q']:.1f} ulp, p_half {worst['p']:.1f} ulp; launch {run['shape']}")
    if integrator:
        assert run["pairs"] >= len(run["logs"]), (label, run["pairs"])  # trees with halves of several leaves
    return worst


def _dense_case(monkeypatch, N, G, C, unit, kind="full", storage="f64", split_model=False, trains=True):
    """Set up one dense case -> (context, its starts, step size, the oracle's cohort, the model's splits); asserts the panel form"""
    from abdpymc_amd._native import Context

    if unit is None:
        monkeypatch.delenv("ABD_SAMPLER_UNIT", raising=False)
    else:
        monkeypatch.setenv("ABD_SAMPLER_UNIT", str(unit))
    if trains:
        monkeypatch.delenv("ABD_SAMPLER_TRAINS", raising=False)
    else:
        monkeypatch.setenv("ABD_SAMPLER_TRAINS", "0")
    sc, coh, coh32 = _dense_cohort(N, G, kind)
    splits = (G // 3, 2 * G // 3) if split_model else None
    ctx = Context(G, N, sc.s_obs, sc.n_obs, sc.vacs, sc.pcrpos, splits=splits, n_chains=C, storage=storage)
    assert ctx.is_dense
    # split panels (od + a one-byte dilution code) or pair panels: what a one-chain launch reads per cell tells
    R = 4 if storage == "f32" else 8
    assert (ctx.algorithmic_bytes(1) < G * N * 3 * R) == (kind != "distinct")
    ref = coh32 if storage == "f32" else coh
    states, th0 = _starts(N, G, C)
    return ctx, states, th0, _step_size(ref, splits, states, th0), ref, splits


def _assert_shape(run, unit, workgroups, trains="dense"):
    assert run["shape"]["unit"] == unit and run["shape"]["trains"] == trains and run["shape"]["workgroups"] == workgroups, run["shape"]
    assert run["fallbacks"] == 0


# (N, G, chains, ABD_SAMPLER_UNIT or None for the default, chains per unit, workgroups): the three smallest two-level shapes --
# 17 x 242 = 4114 rows in ranges of four for 4 ranges per workgroup: 257 workgroups, shard 0 holds 9 partial rows, the rest 8;
# 5 chains in the default units of two (2 + 2 + 1: a unit with an empty slot), 11 x 190 = 2090 rows, 2 ranges per workgroup: 261;
# 6 chains in units of four (4 + 2: a partly filled unit), 6 x 190 = 1140 rows, one range per workgroup: 285
SMALLEST = {1: (1080, 242, 3, None, 1, 257), 2: (700, 190, 5, None, 2, 261), 4: (380, 190, 6, 4, 4, 285)}


@pytest.mark.parametrize("kind", ["full", "distinct"])
@pytest.mark.parametrize("storage", ["f64", "f32"])
@pytest.mark.parametrize("per_unit", [1, 2, 4])
def test_every_train_kernel_form_against_the_oracle_at_the_smallest_two_level_shape(monkeypatch, per_unit, storage, kind):
    """abd_train_kernel<R, CB, XC> for R = double / float storage, CB = 1, 2, 4 chains per unit, XC = split panels (the default:
    three distinct dilutions) / pair panels (every dilution distinct): all twelve, each summing its partial rows in two levels.
    The pair-panel cases run the model with two splits."""
    N, G, C, unit_env, unit, wg = SMALLEST[per_unit]
    ctx, states, th0, eps, ref, splits = _dense_case(monkeypatch, N, G, C, unit_env, kind=kind, storage=storage, split_model=kind == "distinct")
    run = _run(ctx, states, th0, eps)
    ctx.close()
    _assert_shape(run, unit, wg)
    _check_rows(run, ref, splits, f"{N}x{G} unit {unit} {storage} {kind}")


@pytest.mark.parametrize("N,G,C,unit_env,unit,wg,kind", [
    (1400, 190, 3, None, 1, 261, "bare"),   # 22 x 190 = 4180 rows, the last lane group ragged (56 lanes); shards 0-4 one row longer
    (1400, 190, 4, 2, 2, 511, "full"),      # the shipped grid: two workgroups per CU minus the service workgroup's slot
    (1400, 190, 4, 4, 4, 511, "bare"),
    (1024, 256, 3, None, 1, 255, "full"),   # 16 x 256 = 4096 rows: 256 workgroups, one fewer as a multiple of the CU count -- one level
])
def test_train_launches_at_the_shipped_grid_and_the_one_level_boundary(monkeypatch, N, G, C, unit_env, unit, wg, kind):
    """The grid a default-sized cohort gets (511 workgroups with a range), a ragged last lane group, and for contrast the largest
    launch that still sums in one level; two of them on a bare cohort (no vaccinations, no PCR positives)."""
    ctx, states, th0, eps, ref, splits = _dense_case(monkeypatch, N, G, C, unit_env, kind=kind)
    run = _run(ctx, states, th0, eps)
    ctx.close()
    _assert_shape(run, unit, wg)
    _check_rows(run, ref, splits, f"{N}x{G} unit {unit} {kind}")


@pytest.mark.parametrize("per_unit", [1, 2, 4])
def test_with_the_sweep_on_every_row_is_the_oracles_under_the_state_of_its_iteration(monkeypatch, per_unit):
    """gibbs on: a chain's sweep runs on its side stream while the unit's other chains step, so launches carry partial step masks;
    every row -- the start points evaluated again behind a sweep included -- is the oracle's under the discrete state recorded
    for the iteration before, a draw's recorded logp is such a start row's, and two runs log the same rows."""
    N, G, C, unit_env, unit, wg = SMALLEST[per_unit]
    ctx, states, th0, eps, ref, splits = _dense_case(monkeypatch, N, G, C, unit_env, split_model=True)
    run = _run(ctx, states, th0, eps, gibbs=True)
    again = _run(ctx, states, th0, eps, gibbs=True)
    ctx.close()
    _assert_shape(run, unit, wg)
    _assert_shape(again, unit, wg)
    assert run["stats"]["gibbs_proposed"].min() > 0 and any(np.any(run["rec"]["i_raw"][c, -1] != states[c][0]) for c in range(C))
    for (rows, n), (rows2, n2) in zip(run["logs"], again["logs"]):
        assert n == n2
        np.testing.assert_array_equal(rows.view(np.float64), rows2.view(np.float64))
    np.testing.assert_array_equal(run["rec"]["i_raw"], again["rec"]["i_raw"])
    _check_rows(run, ref, splits, f"{N}x{G} unit {unit} sweep on")


@pytest.mark.parametrize("per_unit", [1, 2, 4])
def test_host_driven_units_against_the_oracle_and_the_train_run(monkeypatch, per_unit):
    """ABD_SAMPLER_TRAINS=0: one evaluation launch per leapfrog of a unit (Caller::Unit: one workgroup per CU, summed by the launch
    itself), the leapfrog on the host.  Every row against the oracle as for the trains; and the train run at the same two-level
    shape builds the same first trees (as many leaf rows per transition) through points within 1e-7 -- the closed forms of the
    transforms are the device's there, so to rounding, not bit for bit.  With the log off a run draws the same bits as with it on."""
    N, G, C, unit_env, unit, wg = SMALLEST[per_unit]
    ctx, states, th0, eps, ref, splits = _dense_case(monkeypatch, N, G, C, unit, trains=False)
    host = _run(ctx, states, th0, eps)
    ctx.close()
    _assert_shape(host, unit, 256, trains="none")
    _check_rows(host, ref, splits, f"{N}x{G} unit {unit} host-driven")
    ctx, *_ = _dense_case(monkeypatch, N, G, C, unit)
    train = _run(ctx, states, th0, eps)
    unlogged = _run(ctx, states, th0, eps, log=False)
    ctx.close()
    _assert_shape(train, unit, wg)
    np.testing.assert_array_equal(train["theta"], unlogged["theta"])
    for k in train["stats"]:
        if k != "t_done":
            np.testing.assert_array_equal(train["stats"][k], unlogged["stats"][k], err_msg=k)
    for c in range(C):
        a, b = (r["logs"][c][0] for r in (train, host))
        a, b = a[a["iteration"] < N_SAME], b[b["iteration"] < N_SAME]
        assert len(a) == len(b) and np.array_equal(a["kind"], b["kind"]) and np.array_equal(a["iteration"], b["iteration"]), (c, len(a), len(b))
        assert np.array_equal(a["n_leaf"], b["n_leaf"]) and np.array_equal(a["depth"], b["depth"]) and np.array_equal(a["dir"], b["dir"])
        np.testing.assert_allclose(a["q"], b["q"], rtol=1e-7, atol=1e-7)
    np.testing.assert_allclose(train["theta"][:, :N_SAME], host["theta"][:, :N_SAME], rtol=1e-7, atol=1e-7)


def test_observation_list_trains_against_the_oracle(monkeypatch):
    """Leapfrog trains of observation lists (one chain per unit, several host threads, a train ends with its half): every row
    against the oracle, sweep on, twice the same rows, no completion wait falling back."""
    from abdpymc_amd._native import Context

    G, N, C = 300, 29, 3
    splits = (100, 201)
    coh = random_sparse_cohort(N, G, 1500, 1200, seed=77)
    monkeypatch.setenv("ABD_SAMPLER_UNIT", "1")
    monkeypatch.setenv("ABD_SAMPLER_TRAINS", "1")
    ctx = Context(G, N, (coh.s.idx_gap, coh.s.idx_ind, coh.s.log_dilution, coh.s.od),
                  (coh.n.idx_gap, coh.n.idx_ind, coh.n.log_dilution, coh.n.od), coh.vacs, coh.pcrpos, splits=splits, n_chains=C)
    assert not ctx.is_dense
    rng = np.random.default_rng(5)
    states = [((rng.random((G, N)) < 2.0 / G).astype(np.int8), (rng.random(N) < 0.5).astype(np.int8)) for _ in range(C)]
    th0 = np.stack([synthetic.make_thetas(G, 1, c)[0] for c in range(C)])
    eps = _step_size(coh, splits, states, th0, STEEPNESS_LISTS)
    run = _run(ctx, states, th0, eps, gibbs=True)
    again = _run(ctx, states, th0, eps, gibbs=True)
    ctx.close()
    for r in (run, again):
        assert r["shape"]["unit"] == 1 and r["shape"]["trains"] == "lists" and r["shape"]["threads"] == 2 and r["fallbacks"] == 0, r["shape"]
    for (rows, n), (rows2, n2) in zip(run["logs"], again["logs"]):
        assert n == n2
        np.testing.assert_array_equal(rows.view(np.float64), rows2.view(np.float64))
    _check_rows(run, coh, splits, "observation lists 29x300")


def test_a_full_log_counts_what_it_drops_and_the_calls_refuse_what_they_must():
    """The log's bookkeeping through the C ABI: a buffer of five rows keeps the first five of the full log and counts the rest; the
    log cannot be switched on after the first run, read without being on, or read past what it holds; capacity 0 is off."""
    from abdpymc_amd._native import AbdError, Context

    N, G, C = 130, 65, 2
    sc, coh, _ = _dense_cohort(N, G, "full")
    states, th0 = _starts(N, G, C)
    eps = _step_size(coh, None, states, th0)
    ctx = Context(G, N, sc.s_obs, sc.n_obs, sc.vacs, sc.pcrpos, n_chains=C)
    full = _run(ctx, states, th0, eps)
    for c in range(C):
        ctx.set_discrete(c, *states[c])
    smp = ctx.sampler(np.arange(C), th0, tune=0, seed=5, max_treedepth=DEPTH, gibbs=False)
    with pytest.raises(AbdError):
        smp.leapfrog_log(0)  # not enabled
    for c in range(C):
        smp.set_adaptation(c, INV_MASS, eps)
    smp.enable_leapfrog_log(3)
    smp.enable_leapfrog_log(0)  # off again ...
    with pytest.raises(AbdError):
        smp.leapfrog_log(0)
    smp.enable_leapfrog_log(5)  # ... and on: row 0 is the start point once, not twice
    with pytest.raises(ValueError):
        smp.enable_leapfrog_log(-1)
    theta, _ = smp.run(N_ITER)
    np.testing.assert_array_equal(theta, full["theta"])
    for c in range(C):
        rows, n_total = smp.leapfrog_log(c)
        ref, n_ref = full["logs"][c]
        assert n_total == n_ref > 5 and len(rows) == 5
        np.testing.assert_array_equal(rows.view(np.float64), ref[:5].view(np.float64))
    with pytest.raises(ValueError):
        smp.leapfrog_log(C)
    out = np.zeros((6, smp.LEAPFROG_COLS))
    assert smp._lib.abd_sampler_leapfrog_log(smp._h, 0, 0, 6, out.ctypes.data, None) == -1 and not out.any()  # a dropped row: refused
    assert smp._lib.abd_sampler_leapfrog_log(smp._h, 0, 4, 1, out.ctypes.data, None) == 0 and out[0].any() and not out[1:].any()
    with pytest.raises(AbdError):
        smp.enable_leapfrog_log(10)  # after the first run
    smp.close()
    ctx.close()
