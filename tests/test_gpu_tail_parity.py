"""
Parity off the typical point: every evaluator of the log-probability path against the 40-digit reference
(tests/mp_reference.py; results committed in tests/golden/tail_parity.npz, so no mpmath is needed here).

The other GPU tests evaluate at theta_init + 0.3 N(0, I) or at the simulation's truth and compare at 1e-6 relative to the value.
NUTS does not stay there: steep and reversed curves, rho at 0 or 1, tiny sigma, huge or vanishing perm / temp -- where the
library's several statements of the logistic term (table or polynomial 2^t, one reciprocal per reading or per pair, clamps at
510, 1021 or none) part ways.  Here, for EVERY output k of every case (17 gradient entries and logp):

    |got_k - ref_k| <= C u S_k,   u = 2^-53,   S_k = the sum of the absolute values of all addends of output k,

with C = 32 E_oracle (mp_reference.py: C_BUDGET; E_oracle is the float64 oracle's own worst error in the same measure).  A
measure relative to the value cannot be met in the tails by any float64 code: entries cancel (the oracle's own relative error
is 0.61 at b = -40, perm = e^3).  Every output must be finite: asserted, nothing skipped, no entry masked.  Each test prints the
worst ratio it saw (pytest -s) and fails with EVERY output over its budget, not the first.

What this check found: the kernels took 1 - s of h' = q s (1 - s) from the rounded s.  In the dense
kernels s = r B from the shared reciprocal is 1 +- 20 u where a reading is saturated, which made 20 u |q| of noise per reading:
1.7e6 u S_k at b = +40, 1.4e5 at b = -40, 1.2e5 at init +20 / -20, 2.0e4 at b = +300, 8.9e3 at perm, temp = e^5, against the
budget of 1536; the list kernels missed init +20 / -20 (2.8e4).  They carry e now (1 - s = e s), and every case passes.
"""
import functools
import os

import numpy as np
import pytest

from oracle import abd_oracle as O
from tests import fused_launches as F
from tests import mp_reference as R
from tests.golden.make_tail_fixtures import case_check

pytestmark = pytest.mark.gpu

C_U = R.C_BUDGET * R.U
FULL = [row[0] for row in R.case_table(33)]  # the names of the full table, and of the short one
SHORT = list(R.FIVE)
_FX = R.load_fixture(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))


class Cases:
    """One set of the fixture with its inputs rebuilt and checked against the stored checksums"""

    def __init__(self, name, st="f64"):
        assert C_U <= 1e-12
        self.name, self.st = name, st
        self.rows = []  # (case name, theta, i_raw, waner, cohort, index)
        for c, (cname, theta, i_raw, w, coh) in enumerate(R.set_cases(name)):
            ref_coh = R.rounded_to_f32(coh) if st == "f32" else coh
            assert _FX[f"{name}.names"][c] == cname and theta.tobytes() == _FX[f"{name}.{st}.theta"][c].tobytes()
            np.testing.assert_array_equal(case_check(i_raw, w, ref_coh), _FX[f"{name}.{st}.check"][c])
            self.rows.append((cname, theta, i_raw, w, coh, c))

    def get(self, key, c):
        return _FX[f"{self.name}.{self.st}.{key}"][c]

    def row(self, cname):
        return next(r for r in self.rows if r[0] == cname)

    def with_companions(self, cname, n):
        """the case and n - 1 typical cases on the same cohort (the case itself again where the cohort has no other)"""
        row = self.row(cname)
        others = [r for r in self.rows if r[4] is row[4] and r[0] in ("base", "truth", "b=+3", "b=-8") and r[0] != cname]
        return [row] + [(others or [row])[k % len(others or [row])] for k in range(n - 1)]


@functools.lru_cache(maxsize=None)
def cases(name, st="f64"):
    return Cases(name, st)


def _context(coh, n_chains=1, storage="f64"):
    from abdpymc_amd._native import Context

    return Context(coh.n_gaps, coh.n_inds, (coh.s.idx_gap, coh.s.idx_ind, coh.s.log_dilution, coh.s.od),
                   (coh.n.idx_gap, coh.n.idx_ind, coh.n.log_dilution, coh.n.od), coh.vacs, coh.pcrpos, n_chains=n_chains, storage=storage)


class Worst:
    """Collects every output over its budget (or not finite) and fails at the end with all of them: done()"""

    def __init__(self, family):
        self.family, self.ratio, self.where, self.n, self.over = family, 0.0, None, 0, []

    def check(self, label, lp, g, ref, S, factor=1.0):
        got = np.append(np.asarray(g, float), float(lp))
        assert (S > 0).all()
        with np.errstate(invalid="ignore"):
            ratio = np.where(np.isfinite(got), np.abs(got - ref) / (R.U * S), np.inf)
        k = int(ratio.argmax())
        if ratio[k] > self.ratio:
            self.ratio, self.where = float(ratio[k]), (label, k)
        self.n += 1
        self.over += [(label, int(k), float(ratio[k]), float(got[k]), float(ref[k])) for k in np.flatnonzero(ratio > factor * R.C_BUDGET)]

    def done(self):
        print(f"\ntail parity, {self.family}: {self.n} evaluations, worst error {self.ratio:.1f} u S_k at {self.where} (budget C = {R.C_BUDGET})")
        assert not self.over, (self.family, "(what, output k, error in u S_k, got, reference)", self.over)


def _dense_case(cs, cname, worst, storage="f64"):
    """one case through launches of 1, 2 and 4 chains, the case in slot 0"""
    coh = cs.row(cname)[4]
    ctx = _context(coh, n_chains=4, storage=storage)
    assert ctx.is_dense
    for n in (1, 2, 4):
        batch = cs.with_companions(cname, n)
        for slot, (_, _, i_raw, w, _, _) in enumerate(batch):
            ctx.set_discrete(slot, i_raw, w)
        if n == 1:  # the one-chain launch: split panels where the cohort has them
            lp, g = ctx.logp_dlogp(0, batch[0][1])
            lp, g = [lp], [g]
        else:
            lp, g = ctx.logp_dlogp_batch(np.arange(n), np.stack([r[1] for r in batch]))
        for slot, (name, _, _, _, _, c) in enumerate(batch):
            worst.check(f"{n} chains, slot {slot}: {name}", lp[slot], g[slot], cs.get("ref", c), cs.get("S", c))
    ctx.close()


_DENSE = [("65x33", c) for c in FULL] + [("7x65", c) for c in SHORT]


@pytest.mark.parametrize("planes", ["1", "0"])
@pytest.mark.parametrize("name,cname", _DENSE, ids=[f"{n}-{c}" for n, c in _DENSE])
def test_dense_evaluation(name, cname, planes, monkeypatch):
    """logp_dlogp_batch with 1, 2 and 4 chains per call (a one-chain launch reads the split panels), the full table on 65 x 33 (two
    lane groups, one lane in the second) and the short one on 7 x 65 (two 64-gap words), with the plane form of the gap loop and without"""
    monkeypatch.setenv("ABD_DENSE_PLANES", planes)
    worst = Worst(f"dense evaluation, ABD_DENSE_PLANES={planes}, {name}: {cname}")
    _dense_case(cases(name), cname, worst)
    worst.done()


@pytest.mark.parametrize("cname", SHORT)
def test_dense_evaluation_pair_panels(cname):
    """every log dilution another value: no split panels, one-chain launches read the pair panels"""
    cs = cases("65x33 distinct")
    coh = cs.rows[0][4]
    ctx = _context(coh, 1)
    assert ctx.algorithmic_bytes(1) >= coh.n_gaps * coh.n_inds * 3 * 8  # (as tests/test_gpu_leapfrog_parity.py tells the panel form)
    ctx.close()
    worst = Worst(f"dense evaluation, pair panels: {cname}")
    _dense_case(cs, cname, worst)
    worst.done()


@pytest.mark.parametrize("cname", FULL)
def test_dense_evaluation_f32_storage(cname):
    """panels held in float32, arithmetic in float64: against the reference on the rounded panels"""
    worst = Worst(f"dense evaluation, f32 storage: {cname}")
    _dense_case(cases("65x33", "f32"), cname, worst, storage="f32")
    worst.done()


@pytest.mark.parametrize("n", [4, 1])
def test_fused_steps(n):
    """logp_dlogp_many, every row of every chain at another case (the cases that share the table's discrete state): with K = 8, which
    is too short to fuse on a context of more than one pipe and pins the unfused stream-ordered rows, and with K = 16 pipes + 3, where
    the call must have run the fused launches of abd_fuse_plan.hpp (read back from the result slots: tests/fused_launches.py)"""
    cs = cases("65x33")
    rows = [r for r in cs.rows if r[4] is cs.rows[0][4] and r[2].tobytes() == cs.rows[0][2].tobytes()]
    assert len(rows) >= 24
    ctx = _context(rows[0][4], n_chains=5)  # (one more chain slot than chains: the result slots then tell the launches apart)
    for slot in range(4):
        ctx.set_discrete(slot, rows[0][2], rows[0][3])
    K_fused = F.k_fused(ctx)
    worst = Worst(f"fused steps, K = 8 and {K_fused}, {n} chains")
    for K in (8, K_fused):
        for start in range(0, len(rows), K * n):
            pick = [[rows[(start + k * n + s) % len(rows)] for s in range(n)] for k in range(K)]
            lp, g = ctx.logp_dlogp_many(np.arange(n), np.array([[r[1] for r in step] for step in pick]))
            if K == K_fused:
                F.assert_fused(ctx, K, n, 4, lp, g)
            else:
                assert F.observed_plan(ctx, K, n, lp, g) == F.fuse_plan(K, n, ctx.n_pipes, ctx.n_result_slots)
            for k in range(K):
                for s in range(n):
                    cname, c = pick[k][s][0], pick[k][s][5]
                    worst.check(f"K = {K}, row {k} chain {s}: {cname}", lp[k, s], g[k, s], cs.get("ref", c), cs.get("S", c))
    assert ctx.wait_fallbacks == 0
    ctx.close()
    worst.done()


_ALL_SETS = _DENSE + [("sparse", c) for c in SHORT]


@pytest.mark.parametrize("name,cname", _ALL_SETS, ids=[f"{n}-{c}" for n, c in _ALL_SETS])
def test_loglik_only(name, cname):
    """loglik_dlogp: the two observed Normals alone, against the reference minus its prior addends; S_k stays the one of the
    whole output, prior addends included (the clamps' substitutes -- 2^-510 for 2^-800 -- are measured against terms of order one)"""
    cs = cases(name)
    worst = Worst(f"log-likelihood only, {name}: {cname}")
    _, theta, i_raw, w, coh, c = cs.row(cname)
    ctx = _context(coh)
    ctx.set_discrete(0, i_raw, w)
    lp, g = ctx.loglik_dlogp(0, theta)
    worst.check(cname, lp, g, cs.get("ref_lik", c), cs.get("S", c))
    ctx.close()
    worst.done()


_LISTS = _ALL_SETS + [("65x33 distinct", c) for c in SHORT]


@pytest.mark.parametrize("lanes", ["1", "0"])
@pytest.mark.parametrize("name,cname", _LISTS, ids=[f"{n}-{c}" for n, c in _LISTS])
def test_observation_lists(name, cname, lanes, monkeypatch):
    """The dense cohorts kept as observation lists (ABD_FORCE_SPARSE) and the sparse list cohort, through the lane-per-observation
    kernel and the wave-per-individual one: obs_term, polynomial 2^t, the clamp at 1021; alone and in a launch of two chains"""
    monkeypatch.setenv("ABD_FORCE_SPARSE", "1")
    monkeypatch.setenv("ABD_OBS_LANES", lanes)
    cs = cases(name)
    worst = Worst(f"observation lists, ABD_OBS_LANES={lanes}, {name}: {cname}")
    batch = cs.with_companions(cname, 2)
    ctx = _context(batch[0][4], n_chains=2)
    assert not ctx.is_dense
    for slot, r in enumerate(batch):
        ctx.set_discrete(slot, r[2], r[3])
    lp, g = ctx.logp_dlogp_batch([0, 1], np.stack([r[1] for r in batch]))
    lp1, g1 = ctx.logp_dlogp(0, batch[0][1])
    for slot, r in enumerate(batch):
        worst.check(f"2 chains, slot {slot}: {r[0]}", lp[slot], g[slot], cs.get("ref", r[5]), cs.get("S", r[5]))
    worst.check(f"alone: {cname}", lp1, g1, cs.get("ref", batch[0][5]), cs.get("S", batch[0][5]))
    ctx.close()
    worst.done()


@pytest.mark.parametrize("name,force_lists", [("20x13", False), ("7x65", False), ("20x13", True), ("7x65", True), ("sparse", False)])
def test_per_reading_kernels_and_deterministics(name, force_lists, monkeypatch):
    """pointwise_loglik: every reading within C u (the sum of the absolute values of its own addends), and their sum is
    loglik_dlogp's logp within the logp budget; posterior_predictive's curve means within C u |d|; deterministics: ab_n_mu and ab_s_mu within C u (sum of |addends| of the titer),
    i bit for bit"""
    if force_lists:
        monkeypatch.setenv("ABD_FORCE_SPARSE", "1")
    cs = cases(name)
    coh = cs.rows[0][4]
    ctx = _context(coh)
    assert ctx.is_dense == (name != "sparse" and not force_lists)
    w_ll, w_sum, w_mu, w_m = 0.0, 0.0, 0.0, 0.0
    for cname, theta, i_raw, w, _, c in cs.rows:
        ctx.set_discrete(0, i_raw, w)
        ll_s, ll_n = ctx.pointwise_loglik(0, theta)
        for got, ref in ((ll_s, cs.get("pw_s", c)), (ll_n, cs.get("pw_n", c))):
            assert got.shape == ref[:, 0].shape and np.isfinite(got).all(), (name, cname)
            ratio = np.abs(got - ref[:, 0]) / (R.U * ref[:, 2])
            w_ll = max(w_ll, float(ratio.max()))
            assert ratio.max() <= R.C_BUDGET, (name, cname, int(ratio.argmax()), float(ratio.max()))
        ll, _ = ctx.loglik_dlogp(0, theta)
        S17 = cs.get("S_lik", c)[17]
        r_sum = abs(ll_s.sum() + ll_n.sum() - ll) / (R.U * S17)
        w_sum = max(w_sum, float(r_sum))
        assert r_sum <= 2.0 * R.C_BUDGET, (name, cname, r_sum)  # two evaluations, each within the budget of the reference
        assert abs(ll_s.sum() + ll_n.sum() - cs.get("ref_lik", c)[17]) <= C_U * S17, (name, cname)
        # the other walker of abd_readings.hpp: the curve mean m = d s of every reading (|m| <= |d|, and a clamp's substitute for s
        # is off by at most 2^-510 |d|: the budget is C u |d|)
        _, _, m_s, m_n = ctx.posterior_predictive(0, theta, mean=True)
        for got, ref, d in ((m_s, cs.get("pw_s", c), theta[15]), (m_n, cs.get("pw_n", c), theta[12])):
            assert np.isfinite(got).all(), (name, cname)
            ratio = np.abs(got - ref[:, 1]) / (R.U * abs(d))
            w_m = max(w_m, float(ratio.max()))
            assert ratio.max() <= R.C_BUDGET, (name, cname, int(ratio.argmax()), float(ratio.max()))
        i_dev, mu_n, mu_s = ctx.deterministics(0, theta)
        np.testing.assert_array_equal(i_dev, O.constrain_infections(i_raw, np.asarray(coh.pcrpos).T))
        for got, ref in ((mu_n, cs.get("det_n", c)), (mu_s, cs.get("det_s", c))):
            assert np.isfinite(got).all(), (name, cname)
            ratio = np.abs(got - ref[0]) / (R.U * ref[1])
            w_mu = max(w_mu, float(ratio.max()))
            assert ratio.max() <= R.C_BUDGET, (name, cname, float(ratio.max()))
    ctx.close()
    print(f"\ntail parity, per-reading kernels on {name}{' as lists' if force_lists else ''}: worst error of a reading {w_ll:.1f} u (its scale), "
          f"of the sum against loglik_dlogp {w_sum:.1f} u S, of a titer {w_mu:.1f} u (its scale), of a curve mean {w_m:.1f} u |d|; budget C = {R.C_BUDGET}")


@pytest.mark.parametrize("unit", [1, 2, 4])
def test_train_kernels(unit, monkeypatch):
    """The leapfrog-train launches at five tail points: a sampler with tune = 0, tree depth 1, one iteration, no sweep and a step
    size of 1e-9, its leapfrog log on.  Every logged row -- the start point and the one leaf -- must carry the logp and gradient
    logp_dlogp returns at the row's own q on a spare chain slot with the same discrete state, within 2 C u S_k (two evaluations,
    each within the budget the evaluation path is held to above), S_k the fixture's at the case the chain started from: 1e-9 away.
    65 x 33 is dense, and a dense cohort of any size runs trains: asserted."""
    monkeypatch.setenv("ABD_SAMPLER_UNIT", str(unit))
    monkeypatch.delenv("ABD_SAMPLER_TRAINS", raising=False)
    cs = cases("65x33")
    coh = cs.rows[0][4]
    rows = [cs.row(c) for c in SHORT]
    assert len(rows) == 5
    worst = Worst(f"train kernels, units of {unit}")
    ctx = _context(coh, n_chains=6)
    assert ctx.is_dense
    for slot in range(6):
        ctx.set_discrete(slot, rows[0][2], rows[0][3])
    th0 = np.stack([r[1] for r in rows])
    smp = ctx.sampler(np.arange(5), th0, tune=0, seed=3, max_treedepth=1, gibbs=False)
    for c in range(5):
        smp.set_adaptation(c, np.ones(17), 1e-9)
    smp.enable_leapfrog_log(4)
    smp.run(1)
    shape = smp.launch_shape()
    assert shape["trains"] == "dense" and shape["unit"] == unit, shape
    for c, (cname, _, _, _, _, idx) in enumerate(rows):
        log, n_total = smp.leapfrog_log(c)
        assert n_total == len(log) == 2 and log["kind"][0] == 0 and log["kind"][1] == 2, (cname, n_total, log["kind"])
        for r in log:
            assert np.isfinite(r["lp"]) and np.isfinite(r["g"]).all() and np.isfinite(r["q"]).all(), (cname, r)
            assert np.abs(r["q"] - th0[c]).max() <= 1e-6
            lp, g = ctx.logp_dlogp(5, r["q"])
            assert np.isfinite(lp) and np.isfinite(g).all()
            worst.check(f"{cname} kind {int(r['kind'])}", r["lp"], r["g"], np.append(g, lp), cs.get("S", idx), factor=2.0)
    assert ctx.wait_fallbacks == 0
    smp.close()
    ctx.close()
    worst.done()
