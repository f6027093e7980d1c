"""
The sweep half of every compound step, replayed on the CPU.  TEST INFRASTRUCTURE ONLY: imports nothing of the product.

A run of the native sampler returns the point of every iteration, the discrete state of the recorded ones and the counts of
every sweep.  `replay` chains `oracle.c_oracle.COracle.gibbs_sweep` -- the C restatement that tests/test_sweep_reference_cpu.py
holds to the 40-digit sweep -- from the run's start states through ALL its iterations, at the recorded points, with the random
stream the sampler documents (key `(seed << 20) ^ 0x5EED`, counter word `slot + chain_offset`, sweep number = iteration), and
holds the run to it:

 * counts   `gibbs_accepted` / `gibbs_proposed` of every iteration, recorded or not: equal;
 * state    `i_raw` / `ab_s_waner` of every recorded iteration: equal, every cell.  With thin = K the replay goes through the
            unrecorded iterations on the CPU, from the thetas alone; it never takes over the run's state;
 * i        where recorded: `O.constrain_infections` of the reference's `i_raw`, equal;
 * lp       of every iteration: the restatement's joint logp of the iteration's point at the reference's state, within
            `lp_rtol |lp|`;
 * final    the state the caller read back after the call (`final`), if given: the last replayed state.

A run in several calls is replayed call by call: `first_iteration` is the number of iterations before the call and the start
state is what the replay of the call before returned (a `Replayed`, which also adds up what the cases assert about
themselves: acceptances per chain, how many consecutive recorded states differ).
"""
import numpy as np

from oracle import abd_oracle as O

SWEEP_KEY = 0x5EED
MASK64 = (1 << 64) - 1


def sweep_seed(seed: int) -> int:
    """the sweep's Philox key of a sampler created with `seed` (uint64 arithmetic)"""
    return ((int(seed) << 20) ^ SWEEP_KEY) & MASK64


class ReplayMismatch(AssertionError):
    """kind: "counts" / "state" (either may come with the other: see the message) / "i" / "lp" / "final" """

    def __init__(self, kind, chain, iteration, message):
        super().__init__(f"compound replay, chain {chain} iteration {iteration}: {message}")
        self.kind, self.chain, self.iteration = kind, chain, iteration


class Replayed:
    """What a replay leaves: the reference's state per chain, and the tallies over all calls so far."""

    def __init__(self, i_raw, waner):
        C = len(i_raw)
        self.i_raw = [np.array(a, dtype=np.int8) for a in i_raw]
        self.waner = [np.array(a, dtype=np.int8) for a in waner]
        self.sweeps = 0
        self.accepted = np.zeros(C, np.int64)
        self.proposed = np.zeros(C, np.int64)
        self.recorded = np.zeros(C, np.int64)          # recorded iterations compared
        self.recorded_pairs = np.zeros(C, np.int64)    # consecutive recorded iterations ...
        self.recorded_changed = np.zeros(C, np.int64)  # ... whose reference states differ
        self.worst_lp = 0.0                            # worst |lp - ref| / |ref|
        self._last = [None] * C

    def __str__(self):
        return (f"{self.sweeps} sweeps, {int(self.proposed.sum())} proposals ({int(self.accepted.sum())} accepted), "
                f"{int(self.recorded.sum())} recorded states compared ({int(self.recorded_changed.sum())} of "
                f"{int(self.recorded_pairs.sum())} consecutive ones differ), worst lp error {self.worst_lp:.2e}")


def _state_diff(i_got, w_got, i_ref, w_ref):
    """(differing cells of i_raw, differing individuals of waner, first differing individual or None)"""
    di, dw = np.asarray(i_got) != i_ref, np.asarray(w_got) != w_ref
    who = np.flatnonzero(di.any(axis=0) | dw)
    return int(di.sum()), int(dw.sum()), (int(who[0]) if who.size else None)


def replay(co, theta, i_raw0=None, waner0=None, slots=None, chain_offset=0, seed=0, first_iteration=0, recorded=None, thin=1,
           stats=None, start=None, final=None, lp_rtol=1e-9, nthreads=16):
    """
    co                a COracle of the cohort as the device holds it (f32 storage: on the f32-rounded cohort)
    theta             (C, n_iter, 17): the points of the call's iterations
    i_raw0, waner0    (C, G, N), (C, N): the states before iteration `first_iteration`; or `start`, the Replayed of the call before
    slots             the chains' slot ids; chain c sweeps on stream slots[c] + chain_offset
    seed              the SAMPLER's seed
    recorded          {"i_raw": (C, R, G, N), "ab_s_waner": (C, R, N)[, "i": (C, R, G, N)]}: record r is iteration r * thin of the call,
                      R = ceil(n_iter / thin)
    stats             {"gibbs_accepted", "gibbs_proposed", "lp"}: (C, n_iter) each
    final             [(i_raw, waner)] per chain as read back after the call, or None
    -> Replayed; raises ReplayMismatch.
    """
    theta = np.asarray(theta)
    C, n_iter = theta.shape[:2]
    assert len(slots) == C and thin >= 1 and 1 <= nthreads <= 16
    out = start if start is not None else Replayed(i_raw0, waner0)
    assert len(out.i_raw) == C
    n_rec = (n_iter + thin - 1) // thin
    assert recorded["i_raw"].shape[:2] == (C, n_rec) and recorded["ab_s_waner"].shape[:2] == (C, n_rec)
    key = sweep_seed(seed)
    pcr_gn = np.zeros((co.G, co.N), np.int8) if co.pcr is None else co.pcr.T
    splits = tuple(int(x) for x in co.splits) or None
    for c in range(C):
        stream = int(slots[c]) + int(chain_offset)
        i_ref, w_ref = out.i_raw[c], out.waner[c]
        for k in range(n_iter):
            t = first_iteration + k
            i_ref, w_ref, acc, prop = co.gibbs_sweep(theta[c, k], i_ref, w_ref, chain=stream, seed=key, sweep=t, nthreads=nthreads)
            got = (int(stats["gibbs_accepted"][c, k]), int(stats["gibbs_proposed"][c, k]))
            counts_differ = got != (acc, prop)
            counts_msg = f"counts (accepted, proposed) {got}, reference {(acc, prop)}"
            is_rec = k % thin == 0
            if is_rec:
                r = k // thin
                n_i, n_w, who = _state_diff(recorded["i_raw"][c, r], recorded["ab_s_waner"][c, r], i_ref, w_ref)
                if n_i or n_w:
                    raise ReplayMismatch("state", c, t, f"record {r}: {n_i} cells of i_raw and {n_w} of ab_s_waner differ from the "
                                         f"reference, first differing individual {who}; "
                                         + (counts_msg if counts_differ else "the counts agree"))
            if counts_differ:
                raise ReplayMismatch("counts", c, t, counts_msg + ("; the recorded state agrees" if is_rec else "; iteration not recorded"))
            if is_rec and recorded.get("i") is not None:
                bad = recorded["i"][c, r] != O.constrain_infections(i_ref, pcr_gn, splits)
                if bad.any():
                    raise ReplayMismatch("i", c, t, f"record {r}: {int(bad.sum())} cells of i are not the constrained i_raw, first "
                                         f"individual {int(np.flatnonzero(bad.any(axis=0))[0])}")
            lp_ref = co.logp_dlogp(theta[c, k], i_ref, w_ref, nthreads=nthreads)[0]
            err = abs(float(stats["lp"][c, k]) - lp_ref)
            if not err <= lp_rtol * abs(lp_ref):
                raise ReplayMismatch("lp", c, t, f"lp {float(stats['lp'][c, k])!r}, reference {lp_ref!r} at the replayed state: "
                                     f"{err / abs(lp_ref):.3e} relative, allowed {lp_rtol:.1e}")
            out.worst_lp = max(out.worst_lp, err / abs(lp_ref))
            out.sweeps += 1
            out.accepted[c] += acc
            out.proposed[c] += prop
            if is_rec:
                out.recorded[c] += 1
                if out._last[c] is not None:
                    out.recorded_pairs[c] += 1
                    out.recorded_changed[c] += int(not (np.array_equal(out._last[c][0], i_ref) and np.array_equal(out._last[c][1], w_ref)))
                out._last[c] = (i_ref, w_ref)
        out.i_raw[c], out.waner[c] = i_ref, w_ref
        if final is not None:
            n_i, n_w, who = _state_diff(final[c][0], final[c][1], i_ref, w_ref)
            if n_i or n_w:
                raise ReplayMismatch("final", c, first_iteration + n_iter - 1, f"the state read back after the call differs from the last "
                                     f"replayed one in {n_i} cells of i_raw and {n_w} of ab_s_waner, first individual {who}")
    return out
