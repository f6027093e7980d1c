"""
The No-U-Turn transition and its two adaptations, stated literally, as a reference for replaying the leapfrog log.

NumPy, ``math`` and mpmath only; nothing of the product is imported.  The sampler's leapfrog log (abd_hip.h:
abd_sampler_enable_leapfrog_log) holds the point, logp, gradient and half-kicked momentum of every evaluation a chain consumed.
Given the log, the seed and the chain's stream, everything else a transition does is determined: which leaves form the tree and
where it stops, which leaf becomes the draw, the accept statistic, and the step size and metric that follow.  This file states
that, in the order of the algorithm's definition and not of any state machine: a tree is a list of leaves, a sub-tree is a slice
of it, rho of a sub-tree is the explicit sum over the slice.

The stream (per chain: ``Rng(seed, chain id + chain_offset)``; xoshiro256++ seeded through splitmix64, uniform = top 53 bits,
normals by Box-Muller with the second value kept), consumed per transition in this order:
  1. 17 normals for the momentum (the kept value survives from one transition to the next);
  2. one ``next() >> 32``: bit d is the direction of doubling d;
  3. one uniform per leaf that passed the divergence test;
  4. one uniform per completed half, only when the half's weight does not exceed the tree's.

The tree.  Leaf n of a half has p = p_half + 0.5 ve g (ve = dir eps; g = 0 at a non-finite logp), H = -lp + 0.5 p . M^-1 p,
weight w = exp(H0 - H).  Doubling d adds 2^d leaves at the end of the tree that bit d names.  The half ends -- and is thrown
away -- at the first leaf j at which H - H0 > 1000 or lp is not finite (a divergence: the tree keeps its depth), or some
aligned block [j + 1 - 2^s, j], 2^s | j + 1, s >= 1, has  rho . M^-1 p_first <= 0  or  rho . M^-1 p_last <= 0  (a U-turn: the
depth counts the half).  Leaf n replaces the half's candidate iff u_n < w_n / sum_{m <= n} w_m.  A completed half replaces the
tree's candidate iff W_half > W_tree or u < W_half / W_tree (biased progressive sampling); then the whole tree is tested with
its two end momenta, then the depth cap.

The measures (u = 2^-53).
  Energy budget  B = 64 u (S_0 + S_leaf),  S = |lp| + 0.5 sum |addends of p . M^-1 p|.  Derivation, to first order in u: the
  dense metric's kinetic energy is two products in sequence, v = M^-1 p (17 products and 16 in-order additions per entry) and
  p . v (17 and 16 again): every addend p_r M_rc p_c passes through at most 1 + 16 + 1 + 16 = 34 roundings, so the computed
  value errs by at most 34 u sum |addends|; the half kick that forms p adds 2 relative roundings to p, i.e. 4 u on every
  addend; halving and the subtraction from -lp add 2 more on the total.  40 u S per energy, and an energy ERROR is the
  difference of two energies: 40 u (S_0 + S_leaf) <= B.  The restated momentum of the diagonal metric (p0 from this file's
  stream, four libm calls) errs by up to 4 u relative, another 8 u on S_0's kinetic part; 64 leaves room for that.
  Decisions.  A selection or merge ``u < threshold`` is pinned when |log u - log threshold_ref| > 2 B + 8 u (B the largest of
  the leaves the threshold is made of), a U-turn test when |dot_ref| > 64 u sum |addends of the dot|, a divergence test when
  |dh_ref - 1000| > B.  No sampler within its budget may decide a pinned decision otherwise.
Energies and weights are formed in 40 digits from the logged float64 values; block sums and U-turn dots in x87 extended
precision (64-bit mantissa: 2^-11 of the budget they are compared with).
"""
import math

import mpmath as mp
import numpy as np

D = 17
U = 2.0 ** -53
LOG_COLS = 7 + 3 * D
KIND, ITER, DEPTH, N_LEAF, DIR, EPS, LP = range(7)
Q, P_HALF, G = slice(7, 7 + D), slice(7 + D, 7 + 2 * D), slice(7 + 2 * D, 7 + 3 * D)
_M64 = (1 << 64) - 1
LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the U-turn dots need an extended-precision long double"

# the float64 dual average below against the same recursion in 40 digits: the worst relative error of a step size over the
# committed CPU cases (tests/test_nuts_replay_cpu.py measures, prints and asserts it), rounded up
E_NP_STEP = 4.0e-15


class Rng:
    def __init__(self, seed, stream):
        x = (seed ^ (0xD1B54A32D192ED03 * (stream + 1))) & _M64
        self.s = []
        for _ in range(4):
            x = (x + 0x9E3779B97F4A7C15) & _M64
            z = x
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
            self.s.append(z ^ (z >> 31))
        self.spare = None

    @staticmethod
    def _rotl(x, k):
        return ((x << k) | (x >> (64 - k))) & _M64

    def next(self):
        s = self.s
        r = (self._rotl((s[0] + s[3]) & _M64, 23) + s[0]) & _M64
        t = (s[1] << 17) & _M64
        s[2] ^= s[0]
        s[3] ^= s[1]
        s[1] ^= s[2]
        s[0] ^= s[3]
        s[2] ^= t
        s[3] = self._rotl(s[3], 45)
        return r

    def uniform(self):
        return (self.next() >> 11) * 2.0 ** -53

    def normal(self):
        if self.spare is not None:
            v, self.spare = self.spare, None
            return v
        u = 1.0 - self.uniform()
        v = self.uniform()
        r = math.sqrt(-2.0 * math.log(u))
        a = 6.283185307179586476925 * v
        self.spare = r * math.sin(a)
        return r * math.cos(a)


# ---- adaptation, as closed forms ---------------------------------------------------------------------------------------------
GAMMA, T0, KAPPA, TARGET = 0.05, 10.0, 0.75, 0.8
WINDOW, PRIOR_WEIGHT, VAR_FLOOR = 101, 10.0, 1e-12
EARLY_DEPTH, EARLY_ITERATIONS, DIVERGENCE = 8, 200, 1000.0


def initial_step():
    return 0.25 / D ** 0.25


def depth_cap(it, tune, max_treedepth):
    return min(EARLY_DEPTH, max_treedepth) if it < min(tune, EARLY_ITERATIONS) else max_treedepth


class DualAverage:
    """Hoffman & Gelman (2014), eq. 6, around mu = log(10 eps0); ``lib`` is ``math`` (float64) or ``mpmath`` (40 digits)."""

    def __init__(self, eps0, lib=math, target=TARGET):
        self.lib = lib
        self.num = (lambda x: x) if lib is math else mp.mpf
        self.mu = lib.log(10 * self.num(eps0))
        self.target, self.m, self.h_bar, self.log_eps_bar = self.num(target), 0, self.num(0.0), self.num(0.0)

    def update(self, accept):
        """-> the step size of the next tuning transition"""
        num, lib = self.num, self.lib
        self.m += 1
        m = num(float(self.m))
        self.h_bar = (1 - 1 / (m + num(T0))) * self.h_bar + (self.target - num(accept)) / (m + num(T0))
        log_eps = self.mu - lib.sqrt(m) / num(GAMMA) * self.h_bar
        eta = m ** num(-KAPPA)
        self.log_eps_bar = eta * log_eps + (1 - eta) * self.log_eps_bar
        return lib.exp(log_eps)

    def final(self):
        return self.lib.exp(self.log_eps_bar)


def _m2_gate(m2, n, absmax):
    """a Welford M2 over n values against the two-pass one"""
    return 8 * n * 2.0 ** -52 * np.sqrt(m2 * (m2 + n * absmax ** 2))


def diag_metric(draws, prior_point, prior_var):
    """The diagonal of M^-1 after the n tuning draws ``draws`` (n, 17) of an epoch that began with the prior "10 pseudo-draws at
    prior_point with variance prior_var" -> (variance with the floor applied, the gate of the comparison): n <= 101: the two-pass
    scatter of the draws with the prior merged in by Chan's formula; beyond: the draws from ((n - 1) // 101 - 1) * 101 on."""
    x = np.asarray(draws, dtype=np.float64)
    n = len(x)
    if n <= WINDOW:
        mean = x.mean(0)
        m2 = ((x - mean) ** 2).sum(0)
        tot = PRIOR_WEIGHT + n
        m2 = PRIOR_WEIGHT * np.asarray(prior_var, dtype=np.float64) + m2 + (mean - prior_point) ** 2 * PRIOR_WEIGHT * n / tot
        absmax = np.maximum(np.abs(x).max(0), np.abs(prior_point))
    else:
        x = x[((n - 1) // WINDOW - 1) * WINDOW:]
        tot = float(len(x))
        m2 = ((x - x.mean(0)) ** 2).sum(0)
        absmax = np.abs(x).max(0)
    var = m2 / tot
    gate = _m2_gate(m2, tot, absmax) / tot
    return np.where(np.isfinite(var) & (var > VAR_FLOOR), var, VAR_FLOOR), gate


def diag_updates_end(tune):
    """the metric is updated by the draws of iterations < this"""
    return tune - tune // 10 - 1


def dense_windows(tune):
    """The slow windows [begin, end) of a dense-metric warm-up: 7.5 % of tuning before them, 5 % behind, the first
    max(2.5 %, 10) long, each twice as long as the one before, and a window behind which the next would not fit reaches to the end"""
    begin, end, length = tune * 75 // 1000, tune - tune * 50 // 1000, max(tune * 25 // 1000, 10)
    out = []
    while begin < end:
        stop = begin + length
        if stop + 2 * length > end:
            stop = end
        out.append((begin, stop))
        begin, length = stop, 2 * length
    return out


def dense_metric(draws):
    """-> (n / (n + 5) cov(ddof = 1) + 1e-3 * 5 / (n + 5) I, the gate per entry, whether it is installed: n > 17 and it factors)"""
    x = np.asarray(draws, dtype=np.float64)
    n = float(len(x))
    m = n / (n + 5.0) * np.cov(x.T, ddof=1) + 1e-3 * 5.0 / (n + 5.0) * np.eye(D)
    m2 = ((x - x.mean(0)) ** 2).sum(0)
    g = _m2_gate(m2, n, np.abs(x).max(0))  # per variable; an off-diagonal scatter entry is bounded by the geometric mean
    gate = np.sqrt(np.outer(g, g)) / (n - 1.0) * n / (n + 5.0)
    ok = n > D
    if ok:
        try:
            np.linalg.cholesky(m)
        except np.linalg.LinAlgError:
            ok = False
    return m, gate, ok


def cholesky_in_order(m):
    """Cholesky-Banachiewicz in float64, row by row, every sum in the order of its index: l_rc = (m_rc - sum_{k < c} l_rk l_ck) /
    l_cc.  Two correct float64 factorisations of one matrix differ by about cond(M) u (5e-15 relative between this one and
    LAPACK's on the metrics of the committed dense case, cond 1.6e4), which is more than a backward check of a solve with the
    factor can absorb: the check is made with this factor, and with NumPy's given the difference of the two as allowance."""
    low = np.zeros((D, D))
    for r in range(D):
        for c in range(r + 1):
            v = m[r, c]
            for k in range(c):
                v -= low[r, k] * low[c, k]
            low[r, c] = math.sqrt(v) if r == c else v / low[c, c]
    return low


# ---- the tree ----------------------------------------------------------------------------------------------------------------
class Tally:
    """decision counts, the smallest pinning margins (as multiples of the threshold that pins) and the worst errors seen"""

    def __init__(self):
        self.n = dict(select=0, merge=0, uturn=0, divergence=0)
        self.margin = dict(select=math.inf, merge=math.inf, uturn=math.inf, divergence=math.inf)
        self.worst = dict(junction_q=0.0, junction_p=0.0, p0=0.0, dense_p0=0.0, energy=0.0, dh=0.0, accept=0.0, eps=0.0, metric=0.0)
        self.events = dict(divergent=0, non_finite=0, capped=0, subtree_turn=0, tree_turn=0, transitions=0, leaves=0,
                           later_half_junctions=0, start_kept=0)

    def decide(self, kind, margin, threshold):
        self.n[kind] += 1
        self.margin[kind] = min(self.margin[kind], margin / threshold)

    def see(self, name, value, limit=None, where=None):
        self.worst[name] = max(self.worst[name], float(value))
        if limit is not None:
            assert value <= limit, (name, float(value), limit, where)

    def merge(self, other):
        for k in self.n:
            self.n[k] += other.n[k]
            self.margin[k] = min(self.margin[k], other.margin[k])
        for k in self.worst:
            self.worst[k] = max(self.worst[k], other.worst[k])
        for k in self.events:
            self.events[k] += other.events[k]

    def pinned(self):
        return all(m > 1.0 for m in self.margin.values())

    def __str__(self):
        return (f"decisions {self.n}, smallest margin / pinning threshold {({k: float(f'{v:.3g}') for k, v in self.margin.items()})}, "
                f"worst {({k: float(f'{v:.3g}') for k, v in self.worst.items()})}, {self.events}")


def _velocity(metric, p):
    """M^-1 p in extended precision, and the sums of the absolute addends per entry"""
    p = np.asarray(p, dtype=LD)
    if metric.ndim == 1:
        v = metric.astype(LD) * p
        return v, np.abs(v).astype(np.float64)
    m = metric.astype(LD)
    return m @ p, (np.abs(m) @ np.abs(p)).astype(np.float64)


def _energy(lp, p, metric):
    """-> (H = -lp + 0.5 p . M^-1 p in 40 digits, S)"""
    pm = [mp.mpf(float(x)) for x in p]
    if metric.ndim == 1:
        add = [mp.mpf(float(metric[d])) * pm[d] * pm[d] for d in range(D)]
    else:
        add = [pm[r] * mp.mpf(float(metric[r, c])) * pm[c] for r in range(D) for c in range(D)]
    kin = mp.fsum(add) / 2
    s = abs(lp) + 0.5 * float(mp.fsum(abs(a) for a in add)) if math.isfinite(lp) else math.inf
    return (-mp.mpf(lp) + kin if math.isfinite(lp) else mp.inf), s


def _turns(ps, metric, tally):
    """The U-turn test of the leaves ``ps`` (momenta, in the order they were built): rho the explicit sum; -> turning"""
    rho = np.sum(np.asarray(ps, dtype=LD), axis=0)
    dots = []
    for p in (ps[0], ps[-1]):
        v = _velocity(metric, p)[0]
        if metric.ndim == 1:
            addends = np.abs(rho * v).astype(np.float64).sum()
        else:
            addends = float(np.abs(rho) @ (np.abs(metric.astype(LD)) @ np.abs(np.asarray(p, dtype=LD))))
        dots.append((float(rho @ v), 64 * U * addends))
    turning = any(d <= 0.0 for d, _ in dots)
    if turning:  # one test that says so beyond doubt pins the outcome
        tally.decide("uturn", *max(((-d, b) for d, b in dots if d <= 0.0), key=lambda t: t[0] / t[1] if t[1] else math.inf))
    else:
        for d, b in dots:
            tally.decide("uturn", d, b)
    return turning


def _ulp(x):
    return 2.0 ** -52 * np.abs(x)


def replay_transition(start, leaves, p0, eps, metric, dir_bits, rng, max_depth, tally, check_p0=True):
    """One transition from the start row ``start`` = (q, lp, g) over its logged leaf rows ``leaves`` (n, 58), which must be exactly
    the reference's, in its order.  metric: the diagonal (17,) or M^-1 (17, 17).  -> dict(depth, n_steps, diverging, selected = index
    of the selected leaf or -1 for the start point, H0, S0, dh = energy errors, B = their budgets, accept = mean acceptance)."""
    metric = np.asarray(metric, dtype=np.float64)
    q0, lp0, g0 = start
    with mp.workdps(40):
        h0, s0 = _energy(lp0, p0, metric)
        # the tree: leaves from its backward end to its forward end; a leaf is (q, p, g, row index or -1)
        tree = [(q0, np.asarray(p0, dtype=np.float64), g0, -1)]
        log_w_tree, cand = mp.mpf(0), -1
        dh, bud = [], []
        used, depth, diverging, capped = 0, 0, False, False
        while True:
            d = depth
            direction = 1 if (dir_bits >> d) & 1 else -1
            ve = direction * eps
            half, ws, sub_cand, stop = [], [], None, None
            for j in range(1 << d):
                assert used < len(leaves), f"the log ends inside doubling {d} at leaf {j}"
                r = leaves[used]
                assert (r[DEPTH], r[N_LEAF], r[DIR]) == (d, j, direction), ("leaf row", used, r[DEPTH], r[N_LEAF], r[DIR], "expected", d, j, direction)
                assert r[EPS] == eps, ("step size of a leaf row", r[EPS], eps)
                # the junction: the leaf before this one in the half, or the end of the tree the half starts from
                a_q, a_p, a_g, a_row = half[-1] if half else (tree[-1] if direction > 0 else tree[0])
                if a_row < 0:
                    p_np = a_p + 0.5 * ve * a_g
                    if check_p0:  # 16 ulp: four libm calls at <= 1 ulp (log, sqrt, sin or cos, sqrt of the metric) and five roundings
                        tally.see("p0", (np.abs(r[P_HALF] - p_np) / _ulp(np.maximum(np.abs(a_p), np.abs(0.5 * ve * a_g)))).max(), 16, (d, j))
                else:
                    a = leaves[a_row]
                    p_np = a[P_HALF] + ve * a[G]
                    tally.see("junction_p", (np.abs(r[P_HALF] - p_np) / _ulp(np.maximum(np.abs(a[P_HALF]), np.abs(ve * a[G])))).max(), 8, (d, j))
                v, v_abs = _velocity(metric, r[P_HALF])
                q_np = (np.asarray(a_q, dtype=LD) + ve * v).astype(np.float64)
                tally.see("junction_q", (np.abs(r[Q] - q_np) / _ulp(np.maximum(np.abs(a_q), np.abs(ve) * v_abs))).max(), 16, (d, j))
                if not half and d > 0:
                    tally.events["later_half_junctions"] += 1
                used += 1
                finite = math.isfinite(r[LP])
                g = r[G] if finite else np.zeros(D)
                p = r[P_HALF] + 0.5 * ve * g
                h, s = _energy(float(r[LP]), p, metric)
                e = h - h0
                if mp.isnan(e):
                    e = mp.inf
                dh.append(e)
                bud.append(64 * U * (s0 + s))
                half.append((r[Q], p, g, used - 1))
                if not finite:
                    tally.events["non_finite"] += 1
                    stop = "divergence"
                    break
                tally.decide("divergence", abs(float(e) - DIVERGENCE), bud[-1])
                if e > DIVERGENCE:
                    stop = "divergence"
                    break
                u = rng.uniform()
                ws.append(-e)
                if j == 0:
                    sub_cand = used - 1  # w / w = 1: no decision
                else:
                    log_thr = -e - mp.log(mp.fsum(mp.exp(w) for w in ws))
                    b = 2 * max(bud[-(j + 1):]) + 8 * U
                    tally.decide("select", abs((math.log(u) if u > 0 else -math.inf) - float(log_thr)), b)
                    if (u == 0.0) or mp.log(mp.mpf(u)) < log_thr:
                        sub_cand = used - 1
                n, size = j + 1, 2
                while n % size == 0:
                    if _turns([x[1] for x in half[n - size:n]], metric, tally):
                        stop = "turn"
                        break
                    size *= 2
                if stop:
                    break
            if stop == "divergence":
                diverging = True
                tally.events["divergent"] += 1
                break
            if stop == "turn":
                depth += 1
                tally.events["subtree_turn"] += 1
                break
            # a completed half: the biased merge
            log_w_half = mp.log(mp.fsum(mp.exp(w) for w in ws))
            b = 2 * max(bud) + 8 * U
            tally.decide("merge", abs(float(log_w_half - log_w_tree)), b)  # (whether a uniform is drawn at all)
            if log_w_half > log_w_tree:
                cand = sub_cand
            else:
                u = rng.uniform()
                tally.decide("merge", abs((math.log(u) if u > 0 else -math.inf) - float(log_w_half - log_w_tree)), b)
                if u == 0.0 or mp.log(mp.mpf(u)) < log_w_half - log_w_tree:
                    cand = sub_cand
            log_w_tree = mp.log(mp.exp(log_w_tree) + mp.exp(log_w_half))
            tree = tree + half if direction > 0 else half[::-1] + tree
            depth += 1
            if _turns([x[1] for x in tree], metric, tally):
                tally.events["tree_turn"] += 1
                break
            if depth >= max_depth:
                capped = True
                tally.events["capped"] += 1
                break
        assert used == len(leaves), f"{len(leaves) - used} leaf rows beyond the end of the reference's tree (depth {depth})"
        accept = float(mp.fsum(mp.mpf(1) if e <= 0 else mp.exp(-e) for e in dh) / len(dh))
        tally.events["transitions"] += 1
        tally.events["leaves"] += used
        tally.events["start_kept"] += cand < 0
        return dict(depth=depth, n_steps=used, diverging=diverging, capped=capped, selected=cand, H0=float(h0), S0=s0,
                    dh=[float(e) for e in dh], B=bud, accept=accept)


def check_transition_stats(ref, reported, tally, where):
    """energy, max_energy_error and mean_tree_accept of a transition as reported (dict of floats) against the replay ``ref``"""
    assert reported["tree_depth"] == ref["depth"] and reported["n_steps"] == ref["n_steps"] and bool(reported["diverging"]) == ref["diverging"], \
        (where, reported, {k: ref[k] for k in ("depth", "n_steps", "diverging")})
    if "energy" not in reported:  # (a driver that reports the six classic stats only)
        return _check_accept(ref, reported, tally, where)
    b0 = 64 * U * ref["S0"]
    tally.see("energy", abs(reported["energy"] - ref["H0"]) / (U * ref["S0"]))
    assert abs(reported["energy"] - ref["H0"]) <= b0, (where, "energy", reported["energy"], ref["H0"], b0)
    got = reported["max_energy_error"]
    big = max(abs(e) for e in ref["dh"])
    if math.isinf(big):
        assert got == math.inf, (where, "max_energy_error", got)
    else:  # the reported one is the error of a leaf whose own is the largest to within its budget
        ok = [abs(got - e) / b for e, b in zip(ref["dh"], ref["B"]) if abs(got - e) <= b and abs(e) >= big - b]
        assert ok, (where, "max_energy_error", got, ref["dh"])
        tally.see("dh", 64 * min(ok))
    _check_accept(ref, reported, tally, where)


def _check_accept(ref, reported, tally, where):
    n = ref["n_steps"]
    tally.see("accept", abs(reported["mean_tree_accept"] - ref["accept"]) / (U * n))
    fin = [b for b in ref["B"] if math.isfinite(b)]
    assert abs(reported["mean_tree_accept"] - ref["accept"]) <= n * max(fin + [0.0]), (where, "mean_tree_accept", reported["mean_tree_accept"], ref["accept"])


def replay_chain(rows, stats, seed, stream, tune, max_treedepth, n_iter, dense=False, installs=None, eps_after=None,
                 inv_mass_after=None, metric_after=None, sweep=False, draws=None):
    """Replay iterations [0, n_iter) of one chain from its log ``rows`` (n, 58: the INIT row first).

    stats: dict name -> (n_iter,) as the sampler reported them; draws (n_iter, 17) the reported draws.  installs: {iteration:
    (inv_mass or None, step size or 0)} as set_adaptation was called before that iteration.  eps_after / inv_mass_after /
    metric_after: what adaptation(k) / metric(k) gave after each iteration (None: not read; then the metric of every iteration
    must be known from ``installs`` alone, i.e. tune = 0).  sweep: the discrete state changes between transitions, so the
    reported lp of a draw is the next START row's and not the selected leaf's.
    -> (Tally, list of per-iteration replays, dict of adaptation events)"""
    rows = np.ascontiguousarray(rows).view(np.float64).reshape(-1, LOG_COLS)
    installs = installs or {}
    tally, out = Tally(), []
    events = dict(dense_refused=[], dense_installed=[], da_restarts=[], windows=dense_windows(tune) if dense else [], floor_hits=0)
    assert rows[0, KIND] == 0 and np.all(rows[1:, KIND] > 0)
    rng = Rng(seed, stream)
    point = (rows[0, Q].copy(), float(rows[0, LP]), rows[0, G].copy())
    by_it = {}
    for i in range(1, len(rows)):
        by_it.setdefault(int(rows[i, ITER]), []).append(i)
    assert all(0 <= k <= n_iter for k in by_it), sorted(by_it)
    eps = initial_step()
    metric = np.ones(D)

    def new_average(eps0):  # the float64 recursion, and the same in 40 digits beside it (E_np)
        with mp.workdps(40):
            return DualAverage(eps0), DualAverage(eps0, mp)

    da, da_mp = new_average(eps)
    prior_point, prior_var, epoch_draws = point[0].copy(), np.ones(D), []
    window_draws, is_dense, eps_exact = [], False, True
    wins = dict((b, a) for a, b in events["windows"])  # end -> begin
    worst_np = 0.0
    for it in range(n_iter):
        if it in installs:
            im, e = installs[it]
            assert not is_dense
            if im is not None:
                metric = np.asarray(im, dtype=np.float64).copy()
                if it < tune:
                    prior_point, prior_var, epoch_draws = point[0].copy(), metric.copy(), []
            if e > 0:
                eps, eps_exact = float(e), True
                if it < tune:
                    da, da_mp = new_average(eps)
                    events["da_restarts"].append(it)
        idx = by_it.get(it, [])
        kinds = rows[idx, KIND]
        n_start = int((kinds == 1).sum())
        assert n_start <= 1 and np.all(kinds[n_start:] == 2), (it, kinds)
        if n_start:  # the start point evaluated again: the same point, bit for bit
            r = rows[idx[0]]
            assert np.array_equal(r[Q], point[0]), (it, "START row is not the chain's point")
            point = (point[0], float(r[LP]), r[G].copy())
            if sweep and it > 0:  # the reported logp of a draw is the one of its point under the state the sweep left
                assert float(stats["lp"][it - 1]) == point[1], (it, "lp of the draw before", stats["lp"][it - 1], point[1])
        leaves = rows[idx[n_start:]]
        assert len(leaves), (it, "a transition without a leaf")
        # the step size the transition ran with
        got_eps = float(leaves[0, EPS])
        if eps_exact:
            assert got_eps == eps, (it, "step size", got_eps, eps)
        else:
            tally.see("eps", abs(got_eps - eps) / eps)
            assert abs(got_eps - eps) <= 4 * E_NP_STEP * eps, (it, "step size", got_eps, eps, abs(got_eps - eps) / eps)
        if eps_after is not None and it > 0 and not (it in installs and installs[it][1] > 0):
            assert eps_after[it - 1] == got_eps, (it, "adaptation(k) and the log disagree on the step size")
        z = np.array([rng.normal() for _ in range(D)])
        dir_bits = rng.next() >> 32
        first = leaves[0]
        ve0 = float(first[DIR]) * got_eps
        if metric.ndim == 1:
            p0 = z / np.sqrt(metric)
        else:  # the momentum the first leaf was reached with, checked backward: L^T p0 = z
            kick = 0.5 * ve0 * point[2]
            p0 = first[P_HALF] - kick
            own = cholesky_in_order(metric)
            for low, allowance in ((own, 0.0), (np.linalg.cholesky(metric), np.abs(np.linalg.cholesky(metric) - own).T @ np.abs(p0))):
                # (p0 is a difference of two logged values: 2 ulp of the larger, carried through |L^T|)
                slack = np.abs(low.T) @ (4 * U * np.maximum(np.abs(first[P_HALF]), np.abs(kick)))
                bound = 64 * U * (np.abs(low.T) @ np.abs(p0)) + slack + allowance
                res = np.abs((low.T.astype(LD) @ p0.astype(LD)).astype(np.float64) - z)
                tally.see("dense_p0", (res / bound).max() * 64)
                assert np.all(res <= bound), (it, "L^T p0 = z", (res / bound).max())
        ref = replay_transition(point, leaves, p0, got_eps, metric, dir_bits, rng, depth_cap(it, tune, max_treedepth), tally,
                                check_p0=metric.ndim == 1)
        out.append(ref)
        where = f"iteration {it}"
        check_transition_stats(ref, {k: float(stats[k][it]) for k in ("tree_depth", "n_steps", "diverging", "energy", "max_energy_error", "mean_tree_accept") if k in stats},
                               tally, where)
        assert float(stats["step_size"][it]) == got_eps, (where, "the step_size stat")
        if ref["selected"] >= 0:
            r = leaves[ref["selected"]]
            point = (r[Q].copy(), float(r[LP]), r[G].copy())
        if draws is not None:
            assert np.array_equal(draws[it], point[0]), (where, "the draw is not the selected leaf", ref["selected"])
        if not sweep:
            assert float(stats["lp"][it]) == point[1], (where, "lp", stats["lp"][it], point[1])
        # ---- what follows from it ----
        if it < tune:
            acc = float(stats["mean_tree_accept"][it])
            eps, eps_exact = da.update(acc), False
            with mp.workdps(40):
                eps_mp = da_mp.update(acc)
                if it == tune - 1:
                    eps, eps_mp = da.final(), da_mp.final()
                worst_np = max(worst_np, abs(float((mp.mpf(eps) - eps_mp) / eps_mp)))
            if not dense:
                if it < diag_updates_end(tune):
                    epoch_draws.append(point[0].copy())
                    expect, gate = diag_metric(epoch_draws, prior_point, prior_var)
                    if inv_mass_after is not None:
                        got = inv_mass_after[it]
                        floor = expect == VAR_FLOOR
                        events["floor_hits"] += int(floor.sum())
                        assert np.all(got[floor] == VAR_FLOOR), (where, "the floor")
                        tally.see("metric", (np.abs(got - expect)[~floor] / gate[~floor]).max() if (~floor).any() else 0.0)
                        assert np.all(np.abs(got - expect)[~floor] <= gate[~floor]), (where, "metric", got, expect)
                elif inv_mass_after is not None and it > 0:
                    assert np.array_equal(inv_mass_after[it], inv_mass_after[it - 1]), (where, "the metric moved behind the last update")
            else:
                slow_begin, slow_end = tune * 75 // 1000, tune - tune * 50 // 1000
                was_dense = is_dense
                if not is_dense and it < slow_end:  # diagonal until the first window is installed
                    epoch_draws.append(point[0].copy())
                closes = False
                if slow_begin <= it < slow_end:
                    window_draws.append(point[0].copy())
                    if it + 1 in wins:
                        assert len(window_draws) == it + 1 - wins[it + 1]
                        m, gate, ok = dense_metric(window_draws)
                        if ok:
                            closes = True
                            events["dense_installed"].append((it, len(window_draws)))
                            if metric_after is not None:
                                tally.see("metric", (np.abs(metric_after[it] - m) / gate).max())
                                assert np.all(np.abs(metric_after[it] - m) <= gate), (where, "dense metric", (np.abs(metric_after[it] - m) / gate).max())
                            is_dense = True
                            da, da_mp = new_average(eps)  # the step size restarts around the one just found
                            events["da_restarts"].append(it)
                        else:
                            events["dense_refused"].append((it, len(window_draws)))
                        window_draws = []
                if was_dense and not closes and metric_after is not None:
                    assert np.array_equal(metric_after[it], metric_after[it - 1]), (where, "the dense metric moved in an iteration that closes no window")
                if not is_dense and inv_mass_after is not None:
                    if it < slow_end:
                        expect, gate = diag_metric(epoch_draws, prior_point, prior_var)
                        tally.see("metric", (np.abs(inv_mass_after[it] - expect) / gate).max())
                        assert np.all(np.abs(inv_mass_after[it] - expect) <= gate), (where, "metric", inv_mass_after[it], expect)
                    else:
                        assert np.array_equal(inv_mass_after[it], inv_mass_after[it - 1]), (where, "the metric moved behind the last update")
        else:  # constant from here on: exp(log_eps_bar) within the gate at the first draw, the same bits after it
            eps, eps_exact = got_eps, True
            if eps_after is not None:
                assert eps_after[it] == got_eps, (where, "the step size moved after tuning")
        # the metric the next transition runs with: as reported, so that nothing compounds
        if is_dense:
            assert metric_after is not None, "a dense metric has to be read after every iteration"
            metric = np.asarray(metric_after[it], dtype=np.float64).copy()
        elif inv_mass_after is not None:
            metric = np.asarray(inv_mass_after[it], dtype=np.float64).copy()
        else:
            assert tune == 0, "the metric of a tuning run has to be read after every iteration"
    events["E_np"] = worst_np
    return tally, out, events
