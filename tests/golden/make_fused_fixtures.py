"""
Writes tests/golden/fused_parity.npz: the references of tests/test_gpu_fused_parity.py's layer B -- the smallest cohorts at which a
fused launch of abd_logp_dlogp_many gets a range partition of its own -- from tests/mp_reference.py at 40 digits, rounded to float64.

    python tests/golden/make_fused_fixtures.py [out.npz]

Per shape `<set>` (193x344: six 64-gap words, the 8-word kernel forms; 449x172: three words; both 1376 plane rows) and storage
`<st>` (f64; f32 too for 449x172: the panels rounded to float32), three cases of mp_reference.case_table(G) (CASES) at two discrete
states (0: mp_reference.state(N, G, "random"); 1: synthetic.make_chain_state(N, G, 5)):

    <set>.<st>.theta     (cases, 17)          the points
    <set>.<st>.ref       (cases, states, 18)  gradient entries 0..16 and logp (17)
    <set>.<st>.S         (cases, states, 18)  sum of the absolute values of all addends of each, priors included
    <set>.<st>.check     (cases, states, 8)   sums of vacs, pcrpos, x_s, y_s, x_n, y_n, i_raw, waner: the inputs of the evaluation
    <set>.names          (cases,)             the cases' names

The inputs are rebuilt from seeds by whoever reads the file (set_cases, states) and checked against `.check`.  The file is written
with fixed member dates, so the same inputs give the same bytes.  An evaluation takes about 25 s of mpmath in pure Python (66 392
and 77 228 readings per antigen against the 2 145 of 65 x 33); all 18 take seven and a half minutes of one core, 75 s side by side
in eight processes: tests/test_fused_reference_cpu.py regenerates one of them and compares it bit for bit.
"""
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from abdpymc_amd import synthetic  # noqa: E402
from tests import mp_reference as R  # noqa: E402
from tests.golden.make_tail_fixtures import case_check  # noqa: E402

FIXTURE = "fused_parity.npz"
SHAPES = {"193x344": (193, 344, False), "449x172": (449, 172, True)}  # name -> (N, G, f32 too)
CASES = ("base", "b=+40 perm=e^2.5", "rho -800/-800")
N_STATES = 2


def cohort(name):
    N, G, _ = SHAPES[name]
    return R.cohort(("dense", N, G, "full"))


def states(name):
    """[(i_raw, waner)]: the two discrete states the chain slots alternate between"""
    N, G, _ = SHAPES[name]
    return [R.state(N, G, "random"), synthetic.make_chain_state(N, G, 5)]


def set_cases(name):
    """[(case name, theta)] of one shape"""
    G = SHAPES[name][1]
    rows = {r[0]: r for r in R.case_table(G)}
    assert all(rows[c][2] == "random" and rows[c][3] == "full" for c in CASES)
    return [(c, rows[c][1]) for c in CASES]


def parts():
    """[(shape, storage, case, state)]: the evaluations the file is made of, each generated on its own (generate_part)"""
    return [(name, st, c, z) for name, (_, _, f32) in SHAPES.items() for st in (("f64", "f32") if f32 else ("f64",))
            for c in range(len(CASES)) for z in range(N_STATES)]


def generate_part(part):
    """(part, ref, S, check) of one evaluation"""
    name, st, c, z = part
    coh = cohort(name)
    coh = R.rounded_to_f32(coh) if st == "f32" else coh
    i_raw, w = states(name)[z]
    r = R.evaluate(set_cases(name)[c][1], i_raw, w, coh)
    return part, r["ref"], r["S"], case_check(i_raw, w, coh)


def assemble(results):
    """the file's arrays by name from the results of all parts"""
    out = {}
    for name, (_, _, f32) in SHAPES.items():
        cases = set_cases(name)
        out[f"{name}.names"] = np.array([c[0] for c in cases])
        for st in ("f64", "f32") if f32 else ("f64",):
            out[f"{name}.{st}.theta"] = np.array([c[1] for c in cases], dtype=np.float64)
            for k, width in (("ref", 18), ("S", 18), ("check", 8)):
                out[f"{name}.{st}.{k}"] = np.full((len(cases), N_STATES, width), np.nan)
    for (name, st, c, z), ref, S, check in results:
        out[f"{name}.{st}.ref"][c, z], out[f"{name}.{st}.S"][c, z], out[f"{name}.{st}.check"][c, z] = ref, S, check
    assert all(np.isfinite(v).all() for k, v in out.items() if not k.endswith(".names"))
    return out


def write(path, arrays):
    """an .npz with its members in sorted order and a fixed date: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


if __name__ == "__main__":
    import multiprocessing
    import time
    from concurrent.futures import ProcessPoolExecutor

    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", FIXTURE)
    t0 = time.time()
    with ProcessPoolExecutor(max_workers=min(8, os.cpu_count() or 1), mp_context=multiprocessing.get_context("spawn")) as pool:
        results = list(pool.map(generate_part, parts()))
    write(path, assemble(results))
    print(path, os.path.getsize(path), "bytes,", f"{time.time() - t0:.0f} s")
