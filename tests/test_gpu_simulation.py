"""
The device cohort simulator (abd_simulate; abdpymc_amd.simulation) against the NumPy restatement of its definition
(tests/sim_restatement.py): the reference's known answers, parity on cohorts of both word counts, lists and dense panels and
both storages, the exact limits of the protection curves, the invariances the keyed streams promise, the round trip into the
model, and the module's command line.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from abdpymc_amd import simulation as sim
from abdpymc_amd import synthetic
from abdpymc_amd._native import SIM_OUTPUTS, Context
from abdpymc_amd.data import MEASUREMENT_N, MEASUREMENT_S, TiterData
from oracle import abd_oracle as O
from tests import sim_restatement as R
from tests.helpers import oracle_cohort_from_synth, random_sparse_cohort
from tests.test_data_loader import default_cohort

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIRST = 2 ** 31 + 5  # first replicate of the parity cases: the replicate counter beyond 2^31


def _cohort_of(td):
    return O.Cohort(td.n_gaps, td.n_inds, np.asarray(td.vacs, dtype=np.int8), np.asarray(td.pcrpos, dtype=np.int8),
                    O.AntigenObs(*td.s.obs), O.AntigenObs(*td.n.obs))


def _ctx(coh, ignore=False, storage="f64"):
    return Context(coh.n_gaps, coh.n_inds, (coh.s.idx_gap, coh.s.idx_ind, coh.s.log_dilution, coh.s.od),
                   (coh.n.idx_gap, coh.n.idx_ind, coh.n.log_dilution, coh.n.od), coh.vacs, None if ignore else coh.pcrpos,
                   storage=storage)


def dense(N, G, seed):
    return oracle_cohort_from_synth(synthetic.make_cohort(N, G, seed=seed))


# name -> (cohort, storage, dense?, seed of the simulation): the seeds were chosen on the CPU so that the restatement's smallest
# margin exceeds 1e-9 in all three replicates
CASES = {
    "golden test cohort": (lambda gd: _cohort_of(TiterData.from_disk(os.path.join(gd, "test_cohort"))), "f64", None, 11),
    "default cohort": (lambda gd: _cohort_of(default_cohort(gd)), "f64", False, 12),
    "sparse 60 x 40": (lambda gd: random_sparse_cohort(60, 40, 900, 700, seed=40), "f64", False, 13),
    "sparse 60 x 300": (lambda gd: random_sparse_cohort(60, 300, 900, 700, seed=300), "f64", False, 14),
    "dense 100 x 64": (lambda gd: dense(100, 64, 164), "f64", True, 15),
    "dense 257 x 65": (lambda gd: dense(257, 65, 322), "f64", True, 16),
    "dense 50 x 200": (lambda gd: dense(50, 200, 250), "f64", True, 17),
    "dense 100 x 60 f32 storage": (lambda gd: dense(100, 60, 160), "f32", True, 18),
}


def case_params(seed):
    """Random parameters around the defaults, protection curves steep enough to decide both ways"""
    rng = np.random.default_rng(seed)
    p = R.default_params()
    for ag in ("s", "n"):
        p[ag].update(protect_a=rng.normal(0.0, 1.0), protect_b=rng.uniform(0.5, 2.0), elisa_b=-rng.uniform(1.0, 3.0),
                     elisa_d=rng.uniform(1.0, 2.0), elisa_sd=rng.uniform(0.05, 0.2), init=rng.normal(-2.0, 0.3),
                     perm_rise=rng.uniform(0.5, 2.5), temp_rise_i=rng.uniform(0.5, 2.0), temp_rise_v=rng.uniform(0.5, 2.5),
                     temp_wane=rng.uniform(0.85, 1.0))
    return p


def case_lam0(G, seed):
    """varies by gap around 0.04"""
    return 0.04 * np.random.default_rng(seed).uniform(0.25, 1.75, G)


def restate(coh, params, lam0, seed, rho, storage="f64", pcrpos=True, ind_offset=0):
    x = (lambda a: np.asarray(a, np.float32).astype(np.float64)) if storage == "f32" else (lambda a: np.asarray(a, float))
    return R.simulate(params, lam0, coh.vacs, coh.pcrpos if pcrpos else None, seed, rho,
                      (coh.s.idx_gap, coh.s.idx_ind, x(coh.s.log_dilution)), (coh.n.idx_gap, coh.n.idx_ind, x(coh.n.log_dilution)),
                      ind_offset=ind_offset)


# ---- 1. the reference's known answers through the device ----

@pytest.mark.parametrize("case", R.KNOWN_ANSWERS, ids=[c[0] for c in R.KNOWN_ANSWERS])
def test_known_answers_of_the_reference(case):
    _, s_over, n_over, vacs, pcrpos, infections, titers = case
    N = 3  # the individual of the reference's test, padded by two who are never vaccinated or PCR+
    v, p = np.zeros((N, 5), np.int8), np.zeros((N, 5), np.int8)
    v[1], p[1] = vacs, pcrpos
    obs = (np.array([0, 4], np.int32), np.array([0, 1], np.int32), np.zeros(2), np.zeros(2))
    ctx = Context(5, N, obs, obs, v, p)
    out = ctx.simulate(R.known_params(s_over, n_over), np.zeros(5), seed=7)
    assert out["infections"][0, 1].tolist() == infections and not out["infections"][0, [0, 2]].any()
    assert out["n_infected"][0].tolist() == infections
    for ag, gap, want in titers:
        assert out[ag + "_titer"][0, 1, gap] == pytest.approx(want, abs=1e-7), (ag, gap)  # assertAlmostEqual's 7 places
    ctx.close()


# ---- 2. parity with the restatement ----

@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_the_restatement(golden_dir, name):
    make, storage, is_dense, seed = CASES[name]
    coh = make(golden_dir)
    params, lam0 = case_params(seed), case_lam0(coh.n_gaps, seed)
    want = [restate(coh, params, lam0, seed, FIRST + r, storage) for r in range(3)]
    for w in want:
        assert w["margin"] > 1e-9  # on the restatement alone: no decision of the walk hangs on a rounding
    ctx = _ctx(coh, storage=storage)
    if is_dense is not None:
        assert ctx.is_dense == is_dense
    got = ctx.simulate(params, lam0, seed=seed, first_replicate=FIRST, n_replicates=3)
    for r, w in enumerate(want):
        assert np.array_equal(got["infections"][r], w["infections"])
        assert np.array_equal(got["n_infected"][r], w["n_infected"])
        np.testing.assert_allclose(got["s_titer"][r], w["s_titer"], rtol=1e-12, atol=0)
        np.testing.assert_allclose(got["n_titer"][r], w["n_titer"], rtol=1e-12, atol=0)
        np.testing.assert_allclose(got["od_s"][r], w["od_s"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(got["od_n"][r], w["od_n"], rtol=0, atol=1e-12)
        # protection decisions occurred, both ways: of those exposed without a PCR+ some were infected and some were not
        exposed = (R.keyed_uniforms(seed, FIRST + r, coh.n_inds, coh.n_gaps)[0] < lam0[None]) & (np.asarray(coh.pcrpos) != 1)
        assert 0 < (exposed & (w["infections"] == 1)).sum() < exposed.sum()
    ctx.close()


# ---- 3. exact limits ----

def test_exact_limits_of_the_protection_curves():
    coh = random_sparse_cohort(70, 130, 500, 400, seed=3)
    lam0 = case_lam0(130, 3) * 3
    u_e = R.keyed_uniforms(21, 4, 70, 130)[0]
    exposed = u_e < lam0[None, :]
    pcr = np.asarray(coh.pcrpos) == 1
    never, always = R.default_params(), R.default_params()
    for ag in ("s", "n"):
        never[ag]["protect_a"], always[ag]["protect_a"] = 100.0, -100.0
    ctx, ctx_nopcr = _ctx(coh), _ctx(coh, ignore=True)
    kw = dict(seed=21, first_replicate=4, outputs=("infections",))
    assert np.array_equal(ctx.simulate(never, lam0, **kw)["infections"][0] == 1, exposed | pcr)  # nobody is ever protected
    assert np.array_equal(ctx_nopcr.simulate(never, lam0, **kw)["infections"][0] == 1, exposed)
    assert np.array_equal(ctx.simulate(always, lam0, **kw)["infections"][0] == 1, pcr)           # everybody always is
    assert not ctx_nopcr.simulate(always, lam0, **kw)["infections"].any()
    assert exposed.any() and pcr.any() and (exposed & ~pcr).any()
    ctx.close()
    ctx_nopcr.close()


# ---- 4. invariance ----

@pytest.fixture(scope="module")
def inv():
    coh = dense(150, 70, 9)
    ctx = _ctx(coh)
    params, lam0 = case_params(5), case_lam0(70, 5)
    yield coh, ctx, params, lam0, ctx.simulate(params, lam0, seed=99, first_replicate=3, n_replicates=4)
    ctx.close()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_a_replicate_does_not_depend_on_the_batch_and_a_call_repeats(inv):
    _, ctx, params, lam0, batch = inv
    again = ctx.simulate(params, lam0, seed=99, first_replicate=3, n_replicates=4)
    for name in SIM_OUTPUTS:
        assert same_bits(batch[name], again[name]), name
    for r in range(4):
        one = ctx.simulate(params, lam0, seed=99, first_replicate=3 + r, n_replicates=1)
        for name in SIM_OUTPUTS:
            assert same_bits(batch[name][r], one[name][0]), (name, r)
    assert not np.array_equal(batch["infections"][0], batch["infections"][1])
    assert not np.array_equal(batch["od_s"][0], batch["od_s"][1])


@pytest.mark.parametrize("keep", [("infections",), ("n_infected",), ("od_s",), ("od_n", "n_titer"), ("s_titer",), ("n_titer", "n_infected"),
                                  ("infections", "od_n"), ("s_titer", "n_titer", "od_s", "od_n")])
def test_dropping_outputs_leaves_the_others_unchanged(inv, keep):
    _, ctx, params, lam0, batch = inv
    got = ctx.simulate(params, lam0, seed=99, first_replicate=3, n_replicates=4, outputs=keep)
    assert sorted(got) == sorted(keep)
    for name in keep:
        assert same_bits(batch[name], got[name]), name


def test_staging_chunks_do_not_change_the_result(inv):
    coh, ctx, params, lam0, batch = inv
    per_rep = 70 * 150 * 17 + 2 * 70 * 150 * 8 + 70 * 8  # bytes of one replicate with every output (abd_simulate)
    for budget in (1, per_rep * 2, per_rep * 3 + 100):  # one, two, three replicates per chunk: 4, 2 and 2 chunks
        got = ctx.simulate(params, lam0, seed=99, first_replicate=3, n_replicates=4, staging_bytes=budget)
        for name in SIM_OUTPUTS:
            assert same_bits(batch[name], got[name]), (name, budget)
    with pytest.raises(ValueError, match="staging_bytes"):
        ctx.simulate(params, lam0, staging_bytes=-1)


def test_two_shards_give_the_unsharded_infections_and_titers(inv):
    coh, _, params, lam0, batch = inv
    cut = 83  # shards of 83 and 67 individuals: neither a multiple of 64
    for lo, hi in ((0, cut), (cut, 150)):
        def obs(o):
            m = (np.asarray(o.idx_ind) >= lo) & (np.asarray(o.idx_ind) < hi)
            return np.asarray(o.idx_gap)[m], np.asarray(o.idx_ind)[m] - lo, np.asarray(o.log_dilution)[m], np.asarray(o.od)[m]
        part = Context(70, hi - lo, obs(coh.s), obs(coh.n), coh.vacs[lo:hi], coh.pcrpos[lo:hi])
        part.set_individual_offset(lo)
        got = part.simulate(params, lam0, seed=99, first_replicate=3, n_replicates=4, outputs=("infections", "s_titer", "n_titer"))
        for name in got:
            assert same_bits(np.ascontiguousarray(batch[name][:, lo:hi]), got[name]), (name, lo)
        part.close()


def test_argument_errors(inv):
    _, ctx, params, lam0, _ = inv
    bad = R.default_params()
    bad["n"]["temp_wane"] = 1.5
    with pytest.raises(ValueError, match=r"n\.temp_wane"):
        ctx.simulate(bad, lam0)
    bad = R.default_params()
    bad["s"]["elisa_b"] = 0.5
    with pytest.raises(ValueError, match=r"s\.elisa_b"):
        ctx.simulate(bad, lam0)
    bad = R.default_params()
    bad["s"]["protect_a"] = float("nan")
    with pytest.raises(ValueError, match=r"s\.protect_a"):
        ctx.simulate(bad, lam0)
    nan = lam0.copy()
    nan[3] = np.inf
    with pytest.raises(ValueError, match=r"lam0\[3\]"):
        ctx.simulate(params, nan)
    with pytest.raises(ValueError, match="n_replicates"):
        ctx.simulate(params, lam0, n_replicates=0)
    with pytest.raises(ValueError, match="2\\^32"):
        ctx.simulate(params, lam0, first_replicate=2 ** 32 - 1, n_replicates=2)
    with pytest.raises(ValueError, match="lam0 should be 1D"):
        ctx.simulate(params, lam0[None])
    with pytest.raises(ValueError, match="must have single infection rate for each time gap"):
        ctx.simulate(params, lam0[:-1])
    last = ctx.simulate(params, lam0, first_replicate=2 ** 32 - 1, n_replicates=1, outputs=("n_infected",))  # the last replicate there is
    assert last["n_infected"].shape == (1, 70)


# ---- 5. round trip into the model ----

def test_round_trip_into_the_model(golden_dir):
    from abdpymc_amd.model import model

    td = default_cohort(golden_dir)
    with sim.Cohort(42, data=td) as cohort:
        assert not hasattr(cohort, "s_titer") and not hasattr(cohort, "infections")
        assert (cohort.n_inds, cohort.n_gaps) == (td.n_inds, td.n_gaps) and cohort.true is td
        with pytest.raises(ValueError, match="lam0 should be 1D"):
            cohort.simulate_responses(np.zeros((2, td.n_gaps)))
        with pytest.raises(ValueError, match="must have single infection rate for each time gap"):
            cohort.simulate_responses(np.zeros(td.n_gaps + 1))
        cohort.simulate_responses(np.full(td.n_gaps, 0.04))
        assert cohort.s_titer.shape == cohort.n_titer.shape == cohort.infections.shape == (td.n_inds, td.n_gaps)
        many = cohort.simulate_many(np.full(td.n_gaps, 0.04), 2, outputs=("s_titer", "od_n"))
        assert np.array_equal(many["s_titer"][0], cohort.s_titer)
        df = cohort.simulate_dataset()
        new = cohort.to_titer_data()
    assert len(df) == len(td.s) + len(td.n) and np.array_equal(df["od"].to_numpy()[:len(td.s)], new.s.od)
    assert np.array_equal(many["od_n"][0], new.n.od) and not np.array_equal(new.s.od, td.s.od)
    assert np.array_equal(new.s.idx_gap, td.s.idx_gap) and np.array_equal(new.n.log_dilution, td.n.log_dilution)
    m = model(new)
    theta = synthetic.theta_init(td.n_gaps)
    i_raw, w = synthetic.make_chain_state(td.n_inds, td.n_gaps, 0)
    m.ctx.set_discrete(0, i_raw, w)
    lp, g = m.ctx.logp_dlogp(0, theta)
    lp_ref, g_ref = O.logp_dlogp(theta, i_raw, w, _cohort_of(new), None)
    assert np.isfinite(lp)
    assert abs(lp - lp_ref) <= 1e-6 * abs(lp_ref), (lp, lp_ref)  # smoke()'s tolerance
    scale = np.maximum(np.abs(g_ref), 1e-6 * np.abs(g_ref).max())
    assert (np.abs(g - g_ref) / scale).max() <= 1e-6
    m.close()


# ---- 6. the module's command line ----

def test_command_line_writes_a_cohort_directory(golden_dir, tmp_path):
    src, out = os.path.join(golden_dir, "test_cohort"), tmp_path / "simulated"
    r = subprocess.run([sys.executable, "-m", "abdpymc_amd.simulation", "--cohort_data", src, "--lam0", "0.04", "--seed", "42",
                        "--replicate", "0", "--out", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    true, td = TiterData.from_disk(src), TiterData.from_disk(str(out))
    z = np.load(out / "truth.npz")
    assert (td.n_inds, td.n_gaps, td.t0) == (true.n_inds, true.n_gaps, true.t0)
    assert np.array_equal(td.vacs, true.vacs) and np.array_equal(td.pcrpos, true.pcrpos)
    assert np.array_equal(td.s.idx_gap, true.s.idx_gap) and np.array_equal(td.n.log_dilution, true.n.log_dilution)
    # %.17g round-trips a double: the file holds the simulated readings exactly, as a correctly rounding parser shows ...
    import pandas as pd

    df = pd.read_csv(out / "df.csv", index_col=0, float_precision="round_trip")
    assert np.array_equal(df["od"][df["measurement"] == MEASUREMENT_S].to_numpy(), z["od_s"])
    assert np.array_equal(df["od"][df["measurement"] == MEASUREMENT_N].to_numpy(), z["od_n"])
    # ... while the loader reads with pandas' default parser, which is fast and not correctly rounded: it takes the first 17
    # digits of the text, leading zeros after the point included (0.0001057699558493998 comes back as 0.0001057699558493,
    # 7 364 ulp away), so no bound in ulp holds for it.  In absolute terms: the digits it drops are worth less than 1e-16 for
    # |od| < 10, and the few roundings it makes are each half an ulp of a value below 4 (4.4e-16): 4e-15 covers both, and a
    # misplaced or misformatted reading is off by many orders of magnitude more
    np.testing.assert_allclose(td.s.od, z["od_s"], rtol=0, atol=4e-15)
    np.testing.assert_allclose(td.n.od, z["od_n"], rtol=0, atol=4e-15)
    assert np.abs(z["od_s"]).max() < 4 and np.abs(z["od_n"]).max() < 4
    assert z["infections"].shape == z["s_titer"].shape == z["n_titer"].shape == (true.n_inds, true.n_gaps)
    assert np.all(z["infections"][np.asarray(true.pcrpos) == 1] == 1)
    assert float(z["s_temp_wane"]) == 0.95 and np.array_equal(z["lam0"], np.full(true.n_gaps, 0.04))
    want = restate(_cohort_of(true), R.default_params(), np.full(true.n_gaps, 0.04), 42, 0)
    assert want["margin"] > 1e-9
    assert np.array_equal(z["infections"], want["infections"])
