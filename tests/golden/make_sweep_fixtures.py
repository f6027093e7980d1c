"""
Writes tests/golden/sweep_decisions.npz: two Gibbs sweeps of every case of the sweep sets (tests/mp_reference.py: SWEEP_SETS -- the
case table and sets of the tail fixture, three of them again with splits or without PCR+, and one wide set) made at 40 digits
(mp_reference.sweep) and rounded to float64.

    python tests/golden/make_sweep_fixtures.py [out.npz]

Case k of a set runs in chain slot k, with the set's seed; the second sweep starts from the first one's end state.  Per set `<set>`
and storage `<st>` (f64; f32 too for 65x33: the panels rounded to float32), the proposals of all cases, sweeps and individuals in
one row each, in that order:

    <set>.names            (cases,)       the cases' names
    <set>.<st>.check       (cases, 8)     sums of vacs, pcrpos, x_s, y_s, x_n, y_n, i_raw, waner: the inputs of the first sweep
    <set>.<st>.n           (cases, sweeps, N)   proposals of each individual: the rows are split by these
    <set>.<st>.gf, .acc    (rows,)        int16 / bool: the first gap whose constrained infection changes (-1: none), the decision
                                          (the dims are not stored: mp_reference.gibbs_order, integers alone, makes them)
    <set>.<st>.i_raw       (cases, sweeps, G, N) int8, .waner (cases, sweeps, N) int8: the state each sweep leaves
    <set>.<st>.counts      (cases, sweeps, 2)   accepted, proposed
    <set>.<st>.lp          (cases, sweeps + 1, 2)   logp (mp_reference.evaluate) of the start state and of each end state, and the
                                                    sum of the absolute values of its addends
  and for the rows of the individuals that carry numbers (all; the set's `float_inds` where it names some: a proposal takes 24 bytes
  that do not compress, and 65x33 has 190,000), in the rows' order:
    <set>.<st>.d           (number rows, 2 or 3) float64: delta, log u, and with per-gap terms cur_tail
    <set>.<st>.S           (number rows, 2) float32: S_changed, S_full ROUNDED TOWARDS ZERO -- a budget C u S made from them is never
                                            wider than the one of the float64 value
  and in the PER_GAP sets, for those rows:
    <set>.<st>.crossed     (number rows,) int16: the first gap, counted from gf, at which the bound lies below log u; -1: none
    <set>.<st>.new         the per-gap new terms of the rows that cross within mp_reference.PER_GAP_CROSSED gaps, gaps gf .. gf + crossed + 2
                           (as far as there are gaps), end to end: an early stop's bound is made of them (a row that does not
                           cross is accepted: delta >= log u; the few that cross later would take most of the file)
  An f32 array that equals its f64 counterpart bit for bit is left out (mp_reference.SweepSet.get falls back).

Every decision must be PINNED: |delta - log u| > C u S_full + 8e-15 (mp_reference: C_BUDGET, U, LOG_U_TOL), so that no kernel
within its budget may decide otherwise.  The generator asserts it on every row, numbers stored or not, and fails otherwise; the
remedy is another seed for that set, never a looser rule.  It also asserts that the deltas of a sweep's accepted proposals add up
to the change of mp_reference.evaluate's logp.  tests/test_sweep_reference_cpu.py regenerates named parts and compares them bit for bit.
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import mp_reference as R  # noqa: E402
from tests.golden.make_tail_fixtures import case_check  # noqa: E402


def parts():
    """[(set, storage, case index)]: the pieces the file is made of, each generated on its own (generate_part)"""
    out = []
    for name, spec in R.SWEEP_SETS.items():
        for st in ("f64", "f32") if spec["f32"] else ("f64",):
            out += [(name, st, c) for c in range(len(R.sweep_cases(name)))]
    return out


def margin(delta, log_u, S_full):
    """|delta - log u| over the pinning threshold C u S_full + LOG_U_TOL: pinned iff > 1"""
    return np.abs(delta - log_u) / (R.C_BUDGET * R.U * S_full + R.LOG_U_TOL)


def f32_towards_zero(x):
    x = np.asarray(x, dtype=np.float64)
    y = x.astype(np.float32)
    return np.where(np.abs(y.astype(np.float64)) > np.abs(x), np.nextafter(y, np.float32(0)), y).astype(np.float32)


def generate_part(part):
    """one case: dict of its arrays (rows of both sweeps)"""
    name, st, c = part
    spec = R.SWEEP_SETS[name]
    cname, theta, i_raw, w, coh = R.sweep_cases(name)[c]
    coh = R.rounded_to_f32(coh) if st == "f32" else coh
    kw = dict(splits=spec["splits"], ignore_pcrpos=spec["ignore_pcrpos"])
    o = dict(check=case_check(i_raw, w, coh), n=[], gf=[], acc=[], d=[], S=[], i_raw=[], waner=[], counts=[], new=[], crossed=[], margin=np.inf)
    e = R.evaluate(theta, i_raw, w, coh, **kw)
    o["lp"] = [(e["ref"][17], e["S"][17])]
    for s in range(spec["sweeps"]):
        i_raw, w, a, p, recs = R.sweep(theta, i_raw, w, coh, chain=c, seed=spec["seed"], sweep=s, per_gap=spec["per_gap"], **kw)
        n = np.zeros(coh.n_inds, dtype=np.int32)
        order = {j: [d for d, _ in R.gibbs_order(coh.n_gaps, j, c, spec["seed"], s)] for j in range(coh.n_inds)}
        for r in recs:
            assert r["dim"] == order[r["ind"]][n[r["ind"]]]
            n[r["ind"]] += 1
            m = float(margin(r["delta"], r["log_u"], r["S_full"]))
            assert math.isfinite(m) and m > 1.0, (part, cname, "a decision is not pinned: change the set's seed", r)
            o["margin"] = min(o["margin"], m)
            o["gf"].append(r["gf"]), o["acc"].append(r["accepted"])
            if spec["float_inds"] is None or r["ind"] in spec["float_inds"]:
                o["d"].append((r["delta"], r["log_u"]) + ((r["cur_tail"],) if spec["per_gap"] else ()))
                o["S"].append((r["S_changed"], r["S_full"]))
                if spec["per_gap"]:
                    o["crossed"].append(r["crossed"])
                    if 0 <= r["crossed"] < R.PER_GAP_CROSSED:
                        o["new"].append(r["new"])
        o["n"].append(n), o["i_raw"].append(i_raw), o["waner"].append(w), o["counts"].append((a, p))
        e = R.evaluate(theta, i_raw, w, coh, **kw)
        o["lp"].append((e["ref"][17], e["S"][17]))
        # the deltas are the model's: over the accepted proposals they add up to the change of logp (every number rounded to float64)
        got, ref = math.fsum(r["delta"] for r in recs if r["accepted"]), o["lp"][-1][0] - o["lp"][-2][0]
        assert abs(got - ref) <= 2.0 * R.U * (math.fsum(r["S_full"] for r in recs if r["accepted"]) + o["lp"][-1][1] + o["lp"][-2][1]), (part, got, ref)
    return part, o


def assemble(results):
    """the file's arrays from [(part, arrays)] (any subset of the parts, in the order of parts())"""
    out, by = {}, {}
    for (name, st, c), o in results:
        by.setdefault((name, st), []).append(o)
    for (name, st), os_ in by.items():
        spec, k = R.SWEEP_SETS[name], f"{name}.{st}."
        nd = 3 if spec["per_gap"] else 2
        out[f"{name}.names"] = np.array([r[0] for r in R.sweep_cases(name)])
        out[k + "check"] = np.array([o["check"] for o in os_], dtype=np.float64)
        out[k + "n"] = np.array([o["n"] for o in os_], dtype=np.int32)
        out[k + "gf"] = np.concatenate([np.array(o["gf"], dtype=np.int16) for o in os_])
        out[k + "acc"] = np.concatenate([np.array(o["acc"], dtype=bool) for o in os_])
        out[k + "d"] = np.concatenate([np.array(o["d"], dtype=np.float64).reshape(-1, nd) for o in os_])
        out[k + "S"] = np.concatenate([f32_towards_zero(np.array(o["S"], dtype=np.float64).reshape(-1, 2)) for o in os_])
        out[k + "i_raw"] = np.array([o["i_raw"] for o in os_], dtype=np.int8)
        out[k + "waner"] = np.array([o["waner"] for o in os_], dtype=np.int8)
        out[k + "counts"] = np.array([o["counts"] for o in os_], dtype=np.int64)
        out[k + "lp"] = np.array([o["lp"] for o in os_], dtype=np.float64)
        if spec["per_gap"]:
            out[k + "crossed"] = np.concatenate([np.array(o["crossed"], dtype=np.int16) for o in os_])
            out[k + "new"] = np.concatenate([np.zeros(0)] + [v for o in os_ for v in o["new"]])
    for k in [k for k in out if ".f32." in k]:
        twin = out.get(k.replace(".f32.", ".f64."))
        if twin is not None and twin.dtype == out[k].dtype and twin.shape == out[k].shape and twin.tobytes() == out[k].tobytes():
            del out[k]
    return out, {key: min(o["margin"] for o in os_) for key, os_ in by.items()}


def generate(only=None, workers=None):
    """(the arrays of the given parts (default: all), {(set, storage): its smallest pinned margin}), the parts side by side in fresh processes"""
    import multiprocessing
    from concurrent.futures import ProcessPoolExecutor

    todo = parts() if only is None else [p for p in parts() if p in only]
    with ProcessPoolExecutor(max_workers=workers or min(8, os.cpu_count() or 1), mp_context=multiprocessing.get_context("spawn")) as pool:
        return assemble(list(pool.map(generate_part, todo)))


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", R.SWEEP_FIXTURE)
    arrays, worst = generate()
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes; the smallest |delta - log u| in units of the pinning threshold:",
          ", ".join("%s %s: %.3g" % (k + (v,)) for k, v in worst.items()))
