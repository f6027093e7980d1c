"""
Every sweep of the native sampler, as the sampler launches it, against the CPU restatement (tests/compound_replay.py).

tests/test_gibbs.py and tests/test_gpu_sweep_decisions.py hold `abd_gibbs_sweep` called on its own; here the same restatement
replays the sweeps INSIDE `abd_sampler_run_record`: what `queue_sweep` hands the kernels (the point the tree ended on or the
unit's staged points, the key `(seed << 20) ^ 0x5EED`, the sweep number `it + k`, the stream `slot + chain_offset`), in every
launch form (one chain on its side stream beside the train launches; 2 or 4 chains of a unit in one launch; lists on host
threads), in order against the draw's recording kernels and the next transition.  From explicit start states the replay chains
through every iteration of a run made in several calls -- one of them of a single iteration, the end of tuning inside another --
and never takes over the device's state: counts of every sweep, `i_raw` / `ab_s_waner` / `i` of every recorded one and the
state read back at the end are equal, `lp` of every iteration is the restatement's at the replayed state within 1e-9.  Every
case asserts the path it means (`is_dense`, `launch_shape()`, no wait fall-back) and, on the reference's side, that it is
about something: every chain accepted proposals, at least half of the consecutive recorded states differ.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

from abdpymc_amd import synthetic
from abdpymc_amd.data import TiterData
from oracle import abd_oracle as O
from oracle import c_oracle
from tests import compound_replay as R
from tests.helpers import oracle_cohort_from_synth, random_sparse_cohort
from tests.test_data_loader import default_cohort

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = (7, 1, 16)  # 24 iterations, tune 10: a call of one iteration, and the end of tuning inside the third
CALLS_12 = (7, 1, 4)


def _source_int(header, pattern):
    src = open(os.path.join(ROOT, "abdpymc_amd", "csrc", header)).read()
    return int(re.search(pattern, src).group(1))


def _compute_units():
    """the device's CU count, asked of the HIP runtime the library has loaded (hipDeviceAttributeMultiprocessorCount = 63)"""
    from abdpymc_amd import _native

    _native.load()
    hip = ctypes.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))
    n = ctypes.c_int(0)
    assert hip.hipDeviceGetAttribute(ctypes.byref(n), 63, 0) == 0 and n.value > 0
    return n.value


def _rounded_to_f32(coh):
    r32 = lambda a: a.astype(np.float32).astype(np.float64)
    return O.Cohort(coh.n_gaps, coh.n_inds, coh.vacs, coh.pcrpos,
                    O.AntigenObs(coh.s.idx_gap, coh.s.idx_ind, r32(coh.s.log_dilution), r32(coh.s.od)),
                    O.AntigenObs(coh.n.idx_gap, coh.n.idx_ind, r32(coh.n.log_dilution), r32(coh.n.od)))


@functools.lru_cache(maxsize=None)
def _dense(N, G):
    return oracle_cohort_from_synth(synthetic.make_cohort(N, G, seed=N + G))


@functools.lru_cache(maxsize=None)
def _golden(name):
    golden = os.path.join(ROOT, "tests", "golden")
    td = default_cohort(golden) if name == "default" else TiterData.from_disk(os.path.join(golden, "test_cohort"))
    return O.Cohort(td.n_gaps, td.n_inds, np.asarray(td.vacs, dtype=np.int8), np.asarray(td.pcrpos, dtype=np.int8),
                    O.AntigenObs(*td.s.obs), O.AntigenObs(*td.n.obs))


def _run_and_replay(label, coh, n_chains, expect, splits=None, ignore=False, storage="f64", slots=None, n_slots=None, chain_offset=0,
                    seed=11, tune=10, calls=CALLS, thin=1, dense_metric=False, rate=None, state_seed=5):
    """One sampler run in `calls`, recorded, then replayed call by call -> (Replayed, the start states).  expect: (is_dense, unit,
    trains[, host threads])."""
    from abdpymc_amd._native import Context

    G, N = coh.n_gaps, coh.n_inds
    slots = list(range(n_chains)) if slots is None else list(slots)
    ctx = Context(G, N, (coh.s.idx_gap, coh.s.idx_ind, coh.s.log_dilution, coh.s.od),
                  (coh.n.idx_gap, coh.n.idx_ind, coh.n.log_dilution, coh.n.od), coh.vacs, None if ignore else coh.pcrpos,
                  splits=splits, n_chains=n_slots or n_chains, storage=storage)
    assert ctx.is_dense == expect[0]
    rng = np.random.default_rng(state_seed)
    rate = 2.0 / G if rate is None else rate
    i0 = np.stack([(rng.random((G, N)) < rate).astype(np.int8) for _ in slots])
    w0 = np.stack([(rng.random(N) < 0.5).astype(np.int8) for _ in slots])
    th0 = np.stack([synthetic.make_thetas(G, 1, c)[0] for c in range(n_chains)])
    for c, slot in enumerate(slots):
        ctx.set_discrete(slot, i0[c], w0[c])
    smp = ctx.sampler(slots, th0, tune=tune, seed=seed, gibbs=True, chain_offset=chain_offset, dense_metric=dense_metric)
    shape = smp.launch_shape()
    assert (shape["unit"], shape["trains"]) == tuple(expect[1:3]), shape
    assert len(expect) < 4 or shape["threads"] == expect[3], shape
    runs = []
    for n in calls:
        n_rec = (n + thin - 1) // thin
        rec = dict(i_raw=np.full((n_chains, n_rec, G, N), -1, np.int8), ab_s_waner=np.full((n_chains, n_rec, N), -1, np.int8),
                   i=np.full((n_chains, n_rec, G, N), -1, np.int8))
        th, st = smp.run_record(n, 0, thin=thin, **rec)
        runs.append((th, st, rec))
    final = [ctx.get_discrete(slot) for slot in slots]
    assert ctx.wait_fallbacks == 0
    smp.close()
    ctx.close()

    co = c_oracle.COracle(_rounded_to_f32(coh) if storage == "f32" else coh, splits, ignore)
    out, it = R.Replayed(i0, w0), 0
    for k, (th, st, rec) in enumerate(runs):
        out = R.replay(co, th, slots=slots, chain_offset=chain_offset, seed=seed, first_iteration=it, recorded=rec, thin=thin, stats=st,
                       start=out, final=final if k + 1 == len(runs) else None)
        it += th.shape[1]
    print(f"\ncompound replay {label}: {out}; launch {shape}")
    assert out.sweeps == n_chains * sum(calls)
    assert np.all(out.accepted > 0), out.accepted                               # every chain accepted a proposal
    assert np.all(2 * out.recorded_changed >= out.recorded_pairs), (out.recorded_changed, out.recorded_pairs)
    assert np.all(out.recorded_pairs == sum((n + thin - 1) // thin for n in calls) - 1)
    return out, (i0, w0, co)


def _knobs(monkeypatch, unit=None, trains=None):
    for name, value in (("ABD_SAMPLER_UNIT", unit), ("ABD_SAMPLER_TRAINS", trains)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(value))


def test_a_dense_train_units_of_one_chain(monkeypatch):
    """300 x 40, one split, 3 chains: the train loop's one-chain sweeps on side streams beside the other chains' launches"""
    _knobs(monkeypatch)
    _run_and_replay("a", _dense(300, 40), 3, (True, 1, "dense"), splits=(17,))


def test_b_dense_train_units_of_two(monkeypatch):
    """130 x 65 (a gap beyond the first mask word), 5 chains: the default train units of 2 + 2 + 1"""
    _knobs(monkeypatch)
    _run_and_replay("b", _dense(130, 65), 5, (True, 2, "dense"))


def test_c_dense_train_units_of_four(monkeypatch):
    _knobs(monkeypatch, unit=4)
    _run_and_replay("c", _dense(130, 65), 6, (True, 4, "dense"))


def test_d_dense_unit_loop_sweeps_four_and_two_chains_in_one_launch(monkeypatch):
    """trains off: the unit loop sweeps its 4 and its 2 chains in ONE launch each (grid.y = m) at the unit's staged points"""
    _knobs(monkeypatch, unit=4, trains=0)
    _run_and_replay("d", _dense(130, 65), 6, (True, 4, "none"))


def test_e_dense_metric_takes_the_unit_loop_at_its_default_unit(monkeypatch):
    _knobs(monkeypatch)
    _run_and_replay("e", _dense(130, 65), 4, (True, 2, "none"), dense_metric=True)


def test_f_dense_f32_storage(monkeypatch):
    """`gibbs_kernel<float>`: the reference runs on the f32-rounded panels"""
    _knobs(monkeypatch, unit=2)
    _run_and_replay("f", _dense(100, 60), 4, (True, 2, "dense"), splits=(20, 41), storage="f32")


def test_g_dense_beyond_256_gaps(monkeypatch):
    """40 x 300, two splits: the 8-word instantiation"""
    _knobs(monkeypatch)
    _run_and_replay("g", _dense(40, 300), 2, (True, 1, "dense"), splits=(100, 200), calls=CALLS_12)


@pytest.mark.parametrize("trains", [True, False])
def test_h_more_individuals_than_a_sweep_launch_has_waves(monkeypatch, trains):
    """2100 x 20, 2 chains: a chain's sweep launch has at most (CUs / chains of the launch) workgroups of at most ABD_G2_MAX_WAVES
    waves (8 for a one-chain launch: enqueue_gibbs), so waves take a second individual from the chain's work queue"""
    N, G = 2100, 20
    n_cu = _compute_units()
    waves = _source_int("abd_gibbs_dense.hpp", r"#define\s+ABD_G2_MAX_WAVES\s+(\d+)")
    if trains:
        _knobs(monkeypatch)
        m, waves = 1, min(waves, _source_int("abd_gibbs.hip", r'tune_int\("ABD_G2_WAVES_ONE",\s*(\d+)\)'))
    else:
        _knobs(monkeypatch, unit=2, trains=0)
        m = 2
    assert N > (n_cu // m) * waves, (n_cu, m, waves)
    _run_and_replay(f"h trains {trains}", _dense(N, G), 2, (True, m, "dense" if trains else "none"))


def test_i_states_full_of_infections(monkeypatch):
    """50 x 64 from a start state at rate 0.9: the whole-wave paths, early in a run"""
    _knobs(monkeypatch)
    kcap = _source_int("abd_gibbs_dense.hpp", r"#define\s+ABD_G2_KCAP\s+(\d+)")
    coh = _dense(50, 64)
    _, (i0, _, co) = _run_and_replay("i", coh, 2, (True, 1, "dense"), rate=0.9, calls=CALLS_12)
    kept = [O.constrain_infections(i0[c], co.pcr.T, None).sum(axis=0).max() for c in range(2)]
    assert max(kept) > kcap, (kept, kcap)  # more kept infections than a lane holds for its walk


def test_j_list_trains_on_four_host_threads(monkeypatch):
    """the golden test cohort (observation lists), two splits, 4 chains: list trains, units of one chain on four host threads"""
    _knobs(monkeypatch)
    monkeypatch.delenv("ABD_SAMPLER_THREADS", raising=False)
    _run_and_replay("j", _golden("test"), 4, (False, 1, "lists", 4), splits=(14, 20))


def test_k_list_lock_step_units_of_two(monkeypatch):
    _knobs(monkeypatch)
    _run_and_replay("k", _golden("test"), 6, (False, 2, "none"))


def test_l_lists_beyond_256_gaps_without_pcr(monkeypatch):
    """sparse 29 x 300, two splits, PCR+ ignored: the 8-word list kernel"""
    _knobs(monkeypatch)
    _run_and_replay("l", random_sparse_cohort(29, 300, 1500, 1200, seed=77), 3, (False, 1, "lists"), splits=(100, 201), ignore=True,
                    calls=CALLS_12)


def test_m_lists_f32_storage(monkeypatch):
    _knobs(monkeypatch)
    _run_and_replay("m", random_sparse_cohort(40, 30, 900, 800, seed=13), 2, (False, 1, "lists"), storage="f32")


def test_n_the_default_cohort(monkeypatch):
    """the reference's own shape: 2 chains, tune 4, 10 iterations in calls of 4 + 6"""
    _knobs(monkeypatch)
    _run_and_replay("n", _golden("default"), 2, (False, 1, "lists"), tune=4, calls=(4, 6))


def test_o_the_stream_is_slot_plus_offset_and_the_key_has_two_words(monkeypatch):
    """130 x 65, slots [3, 1] of a 4-slot context, chain_offset 5, seed 2^33 + 7: the stream is slot + offset, not the position in
    the sampler, and both words of the shifted key are non-trivial"""
    _knobs(monkeypatch)
    seed = 2**33 + 7
    assert R.sweep_seed(seed) >> 32 and R.sweep_seed(seed) & 0xFFFFFFFF and R.sweep_seed(seed) != seed
    _run_and_replay("o", _dense(130, 65), 2, (True, 1, "dense"), slots=[3, 1], n_slots=4, chain_offset=5, seed=seed)


@pytest.mark.parametrize("cohort", ["a", "j"])
def test_p_thinned_records_are_replayed_through_the_gaps(monkeypatch, cohort):
    """thin = 5, 23 iterations in calls of 9 + 14: the records are iterations 0, 5, 10, ... of each CALL; the replay goes through
    the iterations between them on the CPU, from the thetas and the counts alone"""
    _knobs(monkeypatch)
    if cohort == "a":
        out, _ = _run_and_replay("p as a", _dense(300, 40), 3, (True, 1, "dense"), splits=(17,), calls=(9, 14), thin=5)
    else:
        out, _ = _run_and_replay("p as j", _golden("test"), 4, (False, 1, "lists", 4), splits=(14, 20), calls=(9, 14), thin=5)
    assert np.all(out.recorded == 2 + 3)
