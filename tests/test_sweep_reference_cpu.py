"""
The 40-digit sweep of tests/mp_reference.py and its committed results (tests/golden/sweep_decisions.npz), without a GPU:

* named parts of the fixture are what the generator writes today (needs mpmath; nothing else here does) -- one case of every set,
  chosen to run in under a minute side by side; tests/golden/make_sweep_fixtures.py makes the whole;
* the 40-digit sweep leaves the states and counts the C restatement (oracle/abd_oracle.c) leaves, on every case and both sweeps;
* every decision is pinned: |delta - log u| > C u S_full + 8e-15, so no kernel within its budget may decide otherwise;
* the reference's deltas are the model's: summed over a sweep's accepted proposals they are the change of mp_reference.evaluate's
  logp between the sweep's start and end state (computed by other code: the joint log-probability, priors included);
* Philox restated in Python gives the known answers.
"""
import math

import numpy as np
import pytest

from oracle import c_oracle
from tests import mp_reference as R
from tests.golden import make_sweep_fixtures as M


@pytest.fixture(scope="module")
def fx(golden_dir):
    return R.load_fixture(golden_dir, R.SWEEP_FIXTURE)


def _sets():
    return [(name, st) for name, spec in R.SWEEP_SETS.items() for st in (("f64", "f32") if spec["f32"] else ("f64",))]


def test_philox_restated_in_python():
    # Random123 kat_vectors, philox4x32-10 (tests/test_gibbs.py holds the C restatement to the same three)
    assert R.philox4x32_10(0, 0, 0, 0, 0, 0) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert R.philox4x32_10(*[0xFFFFFFFF] * 6) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    assert R.philox4x32_10(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0) == (
        0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)


# one case of every set and storage: the cheap sets whole would take minutes
REGENERATED = [("65x33", "f64", 16), ("65x33", "f32", 7), ("7x65", "f64", 3), ("20x13", "f64", 0), ("20x13 one split", "f64", 1),
               ("20x13 two splits", "f64", 0), ("20x13 no pcrpos", "f64", 1), ("sparse", "f64", 2), ("4x257", "f64", 1)]


def test_named_parts_of_the_fixture_are_what_the_generator_writes(fx):
    pytest.importorskip("mpmath")
    assert {p[:2] for p in REGENERATED} == set(_sets()) and set(REGENERATED) <= set(M.parts())
    new, _ = M.generate(only=REGENERATED, workers=4)  # (asserts on its way that every decision is pinned and the deltas add up to logp's change)
    for (name, st, c) in REGENERATED:
        cs, one = R.SweepSet(fx, name, st), R.SweepSet(new, name, st)  # the regenerated set holds this case alone: its case 0
        last = cs.spec["sweeps"] - 1
        rows, rows1 = cs.rows(c, 0, last), one.rows(0, 0, last)
        assert rows1 == slice(0, len(one.get("gf")))
        for key in ("check", "n", "i_raw", "waner", "counts", "lp"):
            assert one.get(key).dtype == cs.get(key).dtype and one.get(key)[0].tobytes() == cs.get(key)[c].tobytes(), (name, st, c, key)
        for key in ("gf", "acc"):
            assert one.get(key).dtype == cs.get(key).dtype and one.get(key).tobytes() == cs.get(key)[rows].tobytes(), (name, st, c, key)
        (has, d, S, cr), (has1, d1, S1, cr1) = cs.numbers(rows), one.numbers(rows1)
        assert has.tobytes() == has1.tobytes() and d.tobytes() == d1.tobytes() and S.tobytes() == S1.tobytes(), (name, st, c)
        assert one.get("d").dtype == cs.get("d").dtype == np.float64 and one.get("S").dtype == cs.get("S").dtype == np.float32
        if cs.spec["per_gap"]:
            assert cr.tobytes() == cr1.tobytes() and cr.dtype == cr1.dtype
            a, b = np.flatnonzero(has)[[0, -1]] + rows.start
            stored = cs.get("new")[int(cs.new_first[cs.at[a]]):int(cs.new_first[cs.at[b] + 1])]
            assert len(stored) > 0 and stored.tobytes() == one.get("new").tobytes(), (name, st, c)


def test_the_fixture_holds_every_set_and_the_inputs_it_was_made_on(fx, golden_dir):
    import os

    from tests.golden.make_tail_fixtures import case_check

    assert os.path.getsize(os.path.join(golden_dir, R.SWEEP_FIXTURE)) < 1 << 20
    n_rows = n_numbers = 0
    for name, st in _sets():
        cs, cases = R.SweepSet(fx, name, st), R.sweep_cases(name)
        assert list(fx[f"{name}.names"]) == [c[0] for c in cases]
        assert cs.n.shape == (len(cases), cs.spec["sweeps"], cases[0][4].n_inds) and cs.G == cases[0][4].n_gaps
        for c, (cname, theta, i_raw, w, coh) in enumerate(cases):
            coh = R.rounded_to_f32(coh) if st == "f32" else coh
            np.testing.assert_array_equal(case_check(i_raw, w, coh), cs.get("check")[c], err_msg=f"{name} {cname}")
        assert len(cs.get("gf")) == len(cs.get("acc")) == cs.first[-1]  # (SweepSet checks the number rows against float_inds)
        np.testing.assert_array_equal(cs.n.sum(axis=2), cs.get("counts")[:, :, 1])
        n_rows, n_numbers = n_rows + int(cs.first[-1]), n_numbers + len(cs.get("d"))
    # what the fixture is to hold: splits, no PCR+, two storages, the wide kernel, all-ones states, the whole table and the short one
    specs = R.SWEEP_SETS.values()
    assert any(s["splits"] and len(s["splits"]) == 1 for s in specs) and any(s["splits"] and len(s["splits"]) == 2 for s in specs)
    assert any(s["ignore_pcrpos"] for s in specs) and R.sweep_cases("4x257")[0][4].n_gaps > 256
    assert len(R.sweep_cases("65x33")) == 27 and all(len(R.sweep_cases(n)) == 5 for n in ("7x65", "20x13", "sparse"))
    assert any(r[2].all() for r in R.sweep_cases("65x33")) and any(r[2].all() for r in R.sweep_cases("4x257"))
    print(f"\nsweep fixture: {n_rows} proposals, {n_numbers} of them with delta, log u and S")


def test_the_c_restatement_makes_the_same_decisions(fx):
    for name, st in _sets():
        cs = R.SweepSet(fx, name, st)
        for c, (cname, theta, i_raw, w, coh) in enumerate(R.sweep_cases(name)):
            co = c_oracle.COracle(R.rounded_to_f32(coh) if st == "f32" else coh, cs.spec["splits"], cs.spec["ignore_pcrpos"])
            for s in range(cs.spec["sweeps"]):
                i_raw, w, a, p = co.gibbs_sweep(theta, i_raw, w, chain=c, seed=cs.spec["seed"], sweep=s)
                np.testing.assert_array_equal(i_raw, cs.get("i_raw")[c, s], err_msg=f"{name} {st} {cname} sweep {s}")
                np.testing.assert_array_equal(w, cs.get("waner")[c, s], err_msg=f"{name} {st} {cname} sweep {s}")
                assert (a, p) == tuple(cs.get("counts")[c, s]), (name, st, cname, s)
                assert a == int(cs.get("acc")[cs.rows(c, s)].sum())


def test_every_decision_is_pinned(fx):
    """On the rows whose numbers are stored (the generator asserts it on every row it makes).  S_full is stored rounded towards zero
    to float32; the threshold here takes the next float32 up: at least the float64 value's."""
    worst = (np.inf, None)
    for name, st in _sets():
        cs = R.SweepSet(fx, name, st)
        for c in range(cs.n.shape[0]):
            rows = cs.rows(c, 0, cs.spec["sweeps"] - 1)
            has, d, S, _ = cs.numbers(rows)
            S_up = np.nextafter(S.astype(np.float32), np.float32(np.inf)).astype(np.float64)
            assert np.isfinite(d).all() and (d[:, 1] < 0).all() and (d[:, 1] >= -22.9).all() and np.isfinite(S_up).all()
            assert (S[:, 0] > 0).all() and (S[:, 0] <= S[:, 1]).all() and (np.abs(d[:, 0]) <= S_up[:, 1]).all()
            np.testing.assert_array_equal(cs.get("acc")[rows][has], d[:, 0] > d[:, 1])
            m = M.margin(d[:, 0], d[:, 1], S_up[:, 1])
            assert (m > 1.0).all(), (name, st, c, float(m.min()))
            if m.min() < worst[0]:
                worst = (float(m.min()), (name, st, str(fx[f"{name}.names"][c])))
    print(f"\nsweep fixture: the smallest |delta - log u| is {worst[0]:.3g} x the pinning threshold C u S_full + {R.LOG_U_TOL}, at {worst[1]}")


def test_the_deltas_of_the_accepted_proposals_add_up_to_the_change_of_logp(fx):
    """sum of delta over a sweep's accepted proposals = logp(end) - logp(start), logp from mp_reference.evaluate, on the sets that
    store every individual's numbers (the generator asserts it on every case it makes).  Each stored number carries its own rounding
    to float64, u |value| <= u S, and the sum of the deltas is exact (fsum): within 2 u (all S)."""
    worst, n = 0.0, 0
    for name, st in _sets():
        cs = R.SweepSet(fx, name, st)
        if cs.spec["float_inds"] is not None:
            continue
        acc, lp = cs.get("acc"), cs.get("lp")
        for c in range(cs.n.shape[0]):
            for s in range(cs.spec["sweeps"]):
                r = cs.rows(c, s)
                _, d, S, _ = cs.numbers(r)
                S_up = np.nextafter(S[:, 1].astype(np.float32), np.float32(np.inf)).astype(np.float64)
                got, ref = math.fsum(d[acc[r], 0]), lp[c, s + 1, 0] - lp[c, s, 0]
                scale = R.U * (math.fsum(S_up[acc[r]]) + lp[c, s, 1] + lp[c, s + 1, 1])
                worst, n = max(worst, abs(got - ref) / scale), n + 1
                assert abs(got - ref) <= 2.0 * scale, (name, st, c, s, got, ref)
    assert n >= 40
    print(f"\nsweep fixture: sum of accepted deltas against the change of logp, {n} sweeps, worst {worst:.3g} of the rounding scale")
