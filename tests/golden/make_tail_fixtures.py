"""
Writes tests/golden/tail_parity.npz: the case table of tests/mp_reference.py evaluated at 40 digits (mpmath) and rounded to float64.

    python tests/golden/make_tail_fixtures.py [out.npz]

Per set of cases `<set>` (65x33, 7x65, 65x33 distinct, 20x13, sparse) and storage `<st>` (f64; f32 too for 65x33: the panels rounded
to float32, which the f32-storage contexts hold):

    <set>.<st>.theta     (cases, 17)  the points
    <set>.<st>.ref       (cases, 18)  gradient entries 0..16 and logp (17)
    <set>.<st>.S         (cases, 18)  sum of the absolute values of all addends of each, priors included
    <set>.<st>.ref_lik, .S_lik        the same without the prior addends (the two observed Normals alone)
    <set>.<st>.sums      (cases, 16)  the sums a kernel hands to abd_terms.hpp
    <set>.<st>.t_ext     (cases, 3)   min, max and max |.| of t = b log2(e) (a - x) over all readings
    <set>.<st>.check     (cases, 8)   sums of vacs, pcrpos, x_s, y_s, x_n, y_n, i_raw, waner: the inputs the case was evaluated on
    <set>.names          (cases,)     the cases' names
    <set>.f64.pw_s, .pw_n (cases, K, 3)   per reading: ll, the curve mean, the sum of |ll's addends|     (20x13, 7x65, sparse)
    <set>.f64.det_n, .det_s (cases, 2, G, N)   ab_n_mu / ab_s_mu and the sum of the absolute values of their addends

The inputs are rebuilt from seeds by whoever reads the file (mp_reference.set_cases) and checked against `.check`.
tests/test_tail_reference_cpu.py regenerates the file's contents and compares them bit for bit.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import mp_reference as R  # noqa: E402


def case_check(i_raw, w, coh):
    return np.concatenate([R.checksum(coh), [float(np.sum(i_raw)), float(np.sum(w))]])


def parts():
    """[(set, storage)]: the pieces the file is made of, each generated on its own (generate_part)"""
    return [(name, st) for name, (_, _, f32) in R.SETS.items() for st in (("f64", "f32") if f32 else ("f64",))]


def generate_part(part):
    return generate([part])


def generate(only=None):
    """the file's arrays by name; only: a list of parts (default: all)"""
    out = {}
    for name, (_, table, f32) in R.SETS.items():
        todo = [st for st in ("f64", "f32") if (name, st) in (parts() if only is None else only)]
        if not todo:
            continue
        cases = R.set_cases(name)
        out[f"{name}.names"] = np.array([c[0] for c in cases])
        for st in todo:
            rows = {k: [] for k in ("theta", "ref", "S", "ref_lik", "S_lik", "sums", "t_ext", "check")}
            for _, theta, i_raw, w, coh in cases:
                coh = R.rounded_to_f32(coh) if st == "f32" else coh
                r = R.evaluate(theta, i_raw, w, coh)
                rows["theta"].append(theta)
                rows["check"].append(case_check(i_raw, w, coh))
                for k in ("ref", "S", "ref_lik", "S_lik", "sums", "t_ext"):
                    rows[k].append(r[k])
            for k, v in rows.items():
                out[f"{name}.{st}.{k}"] = np.array(v, dtype=np.float64)
        if table.endswith("pointwise") and "f64" in todo:
            pw_s, pw_n, det_n, det_s = [], [], [], []
            for _, theta, i_raw, w, coh in cases:
                a, b = R.pointwise(theta, i_raw, w, coh)
                _, dn, ds = R.deterministics(theta, i_raw, w, coh)
                pw_s.append(a), pw_n.append(b), det_n.append(dn), det_s.append(ds)
            for k, v in (("pw_s", pw_s), ("pw_n", pw_n), ("det_n", det_n), ("det_s", det_s)):
                out[f"{name}.f64.{k}"] = np.array(v, dtype=np.float64)
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", R.FIXTURE)
    np.savez_compressed(path, **generate())
    print(path, os.path.getsize(path), "bytes")
