"""
The posterior predictive checks of the survival models (``abd_survival_predictive_*``, ``abd_survival_replicate``)
restated.  TEST INFRASTRUCTURE ONLY, like the other ``*_restatement.py`` modules, from which it takes the data, the points and the
helpers: the package never imports it.

For a model of any form (K = 1, K = 2, by group, by period), a point q in that model's layout used as draw d, and a cell (j, t):

    mu_jt = lambda_t (e_jt sigma_jt)                      NumPy float64, the products in the kernel's order
    u_jt  = sim_uniform(w0, w1),  w = Philox4x32-10(counter (j, t, d mod 2^32, 0x40000020), key (seed lo, seed hi))
    r_jt  = k = 0; p = exp(-mu); c = p; while u >= c and k < 32: k += 1; p *= mu / k; c += p
    bin   = #{edges <= x} of each binning variable; cells without follow-up (e = 0) belong to no bin

``expected`` gives E[v][b] = sum of mu over the cells of a bin and E_j = sum_t mu; ``replicates`` gives the per-cell r and the number
of BOUNDARY cells: those whose u lies within 2^-36 of a cumulative value c the inversion examined, the only cells where two
correctly working exponentials can disagree on k (expected share about 1e-11 per cell).  ``mp_expected`` is E at 40 digits from
the float64 inputs converted exactly.  Every addend of an E is non-negative, so the sum of the absolute values of its addends --
the S of the other restatements -- is E itself: the error a float64 evaluation is entitled to is u E.

``tests/golden/make_survival_predictive_fixtures.py`` evaluates the case table below and commits the 40-digit E rounded to float64
and the restatement's per-cell replicates (``tests/golden/survival_predictive_reference.npz``).
"""
import math
import os

import numpy as np

from tests import survival_groups_restatement as RG
from tests import survival_periods_restatement as RP
from tests import survival_restatement as R1
from tests.survival_restatement import U, _invlogit  # noqa: F401  (U is re-exported)

STREAM = 0x40000020  # kSurvReplicate (abd_types.hpp); the simulator's streams are 0x40000000, 0x40000001, 0x40000010 | antigen
CAP = 32
MAX_BINS = 8
BOUNDARY = 2.0 ** -36

# The worst error of ``expected`` against ``mp_expected`` over the case table, per class of point, in units of u E
# (tests/test_survival_predictive_cpu.py measures, prints and asserts each).  Measured: see MEASURED_E_NP below; each rounded up by
# a tenth and to the next integer, as E_NP of tests/survival_restatement.py.  As there, the figures at large |b| are far above the
# few u of a cell's own operations: E does not count the conditioning of sigma on eta = b (x - a), about |eta| roundings where
# eta << 0, and the worst bin is one whose cells all have eta << 0.
# At r_minus_800 lambda_t = e^-797 is below float64's range: every E is exactly 0 in the reference (rounded to float64) and in
# any float64 evaluation, and a zero reference asks for an exact zero; the class's figure is never a factor of a bound.
MEASURED_E_NP = {"typical": 6.02, "b_plus_50": 92.2, "b_minus_50": 235.96, "eta_800": 682.15, "r_plus_800": 9.58, "r_minus_800": 0.0,
                 "sd_e10": 5.03, "sd_em10": 5.11, "a_spread": 2.77}
E_NP = {"typical": 7.0, "b_plus_50": 102.0, "b_minus_50": 260.0, "eta_800": 751.0, "r_plus_800": 11.0, "r_minus_800": 1.0, "sd_e10": 6.0,
        "sd_em10": 6.0, "a_spread": 4.0}
# |got - ref| <= C u E for the device, C = C_FACTOR E_NP[class]: DESIGN 19's factor for the same cell chain (exp2_reduced on a
# two-term reduced argument, the twice-refined reciprocal) plus one product, fixed before the kernel ran.
C_FACTOR = 4.0


def c_device(name):
    return C_FACTOR * E_NP[name]


FIXTURE = "survival_predictive_reference.npz"


def load_fixture(golden_dir):
    with np.load(os.path.join(golden_dir, FIXTURE)) as f:
        return {k: f[k] for k in f.files}


# ---------------------------------------------------------------------------------------------------
# bins and constants
# ---------------------------------------------------------------------------------------------------


def bin_of(x, edges):
    """#{edges <= x}; NaN compares false throughout: bin 0"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return sum((np.float64(ed) <= x).astype(np.int64) for ed in edges) if len(edges) else np.zeros(x.shape, dtype=np.int64)


def bins_of(rs, variables, edges):
    """(n_var, N, T) int64: the bin of every cell, -1 for cells without follow-up"""
    return np.stack([np.where(rs.e > 0, bin_of(x, ed), -1) for x, ed in zip(variables, edges)])


def constants(rs, variables, edges):
    """(O, PT (n_var, 8), n_cells (n_var, 8) int64, O_j (N,)) of the model's cleaned data, by math.fsum"""
    bins = bins_of(rs, variables, edges)
    O, PT, cells = np.zeros((len(variables), MAX_BINS)), np.zeros((len(variables), MAX_BINS)), np.zeros((len(variables), MAX_BINS), np.int64)
    for v in range(len(variables)):
        for b in range(MAX_BINS):
            sel = bins[v] == b
            O[v, b], PT[v, b], cells[v, b] = math.fsum(rs.y[sel]), math.fsum(rs.e[sel]), int(sel.sum())
    return O, PT, cells, np.array([math.fsum(row[er > 0]) for row, er in zip(rs.y, rs.e)])


# ---------------------------------------------------------------------------------------------------
# mu, NumPy float64
# ---------------------------------------------------------------------------------------------------


def _eta_r(rs, q):
    """(eta (N, T), r (T,)) of a restatement object of any form at q"""
    q = np.asarray(q, dtype=np.float64)
    if hasattr(rs, "P"):
        m, s, z, a_mu, a_sl, az, b = rs.split(q)
        return b * (rs.x - rs.a_t(q)[None, :]), m + np.exp(s) * z
    if hasattr(rs, "Gr"):
        m, s, z, a_mu, a_sl, az, b = rs.split(q)
        return b * (rs.x - (a_mu + np.exp(a_sl) * az)[rs.group][:, None]), m + np.exp(s) * z
    a, b, m, s, z = rs.split(q)
    return sum(b[k] * (rs.xs[k] - a[k]) for k in range(rs.K)), m + np.exp(s) * z


def mu_of(rs, q):
    """(N, T): e lambda_t sigma, +0.0 in cells without follow-up"""
    with np.errstate(over="ignore", under="ignore"):
        eta, r = _eta_r(rs, q)
        return _invlogit(r)[None, :] * (rs.e * _invlogit(eta))


def expected(rs, q, variables, edges):
    """(E (n_var, 8), E_j (N,)) of one point"""
    mu, bins = mu_of(rs, q), bins_of(rs, variables, edges)
    E = np.array([[mu[bins[v] == b].sum() for b in range(MAX_BINS)] for v in range(len(variables))])
    return E, mu.sum(axis=1)


# ---------------------------------------------------------------------------------------------------
# the keyed uniform (Philox4x32-10 in 64-bit integers) and the inversion
# ---------------------------------------------------------------------------------------------------

_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """arrays (or scalars) of counters < 2^32 -> four arrays of words, uint64 holding 32 bits"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _M32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def uniform(seed, N, T, draw):
    """(N, T): the uniform of every cell of draw ``draw`` under ``seed`` (64 bits), j the caller's index"""
    j, t = np.arange(N, dtype=np.uint64)[:, None], np.arange(T, dtype=np.uint64)[None, :]
    w0, w1, _, _ = philox4x32_10(j, t, int(draw) & 0xFFFFFFFF, STREAM, int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    # sim_uniform: ((double)(53-bit integer) + 0.5) 2^-53, the addition rounded as the device rounds it
    return ((((w0 >> np.uint64(5)) << np.uint64(26)) | (w1 >> np.uint64(6))).astype(np.float64) + 0.5) * 2.0 ** -53


def poisson_inverse(mu, u):
    """(k int64, boundary bool) elementwise: the sequential inversion and whether u came within 2^-36 of a cumulative value"""
    mu, u = np.broadcast_arrays(np.asarray(mu, dtype=np.float64), np.asarray(u, dtype=np.float64))
    k = np.zeros(mu.shape, dtype=np.int64)
    p = np.exp(-mu)
    c = p.copy()
    near = np.abs(u - c) < BOUNDARY
    active = u >= c
    for i in range(1, CAP + 1):
        if not active.any():
            break
        p = np.where(active, p * (mu / i), p)
        c = np.where(active, c + p, c)
        k += active
        near |= active & (np.abs(u - c) < BOUNDARY)
        active = active & (u >= c)
    return k, near


def replicates(rs, q, seed, draw):
    """(r (N, T) int64, the number of boundary cells) of the point q as draw ``draw``"""
    N, T = rs.y.shape
    k, near = poisson_inverse(mu_of(rs, q), uniform(seed, N, T, draw))
    return k, int(near.sum())


def replicate_callable(rs, seed):
    """The callable ``survival.predictive(..., replicate=)`` takes: (q (n, D), draw0) -> (mu, r), both (n, N, T)"""
    def fn(Q, draw0):
        Q = np.atleast_2d(Q)
        return (np.stack([mu_of(rs, q) for q in Q]), np.stack([replicates(rs, q, seed, draw0 + d)[0] for d, q in enumerate(Q)]))
    return fn


# ---------------------------------------------------------------------------------------------------
# 40 digits
# ---------------------------------------------------------------------------------------------------


def mp_expected(rs, q, variables, edges):
    """(E, S), each (n_var, 8), at 40 digits, rounded to float64 at the end: S, the sum of the absolute addends, equals E"""
    import mpmath as mp

    mp.mp.dps = 40
    F = mp.mpf
    N, T = rs.y.shape
    t = [F(float(v)) for v in q]
    sig = lambda v: 1 / (1 + mp.exp(-v))  # noqa: E731
    if hasattr(rs, "Gr") or hasattr(rs, "P"):
        n_a = rs.P if hasattr(rs, "P") else rs.Gr
        m, s, z, a_mu, a_sl, az, b = t[0], t[1], t[2:2 + T], t[T + 2], t[T + 3], t[T + 4:T + 4 + n_a], t[T + 4 + n_a]
        a = [a_mu + mp.exp(a_sl) * v for v in az]
        if hasattr(rs, "P"):
            eta = lambda j, k: b * (F(float(rs.x[j, k])) - a[int(rs.period[k])])  # noqa: E731
        else:
            eta = lambda j, k: b * (F(float(rs.x[j, k])) - a[int(rs.group[j])])  # noqa: E731
    else:
        K = rs.K
        a, b, m, s, z = t[:K], t[K:2 * K], t[2 * K], t[2 * K + 1], t[2 * K + 2:]
        eta = lambda j, k: sum(b[c] * (F(float(rs.xs[c][j, k])) - a[c]) for c in range(K))  # noqa: E731
    lam = [sig(m + mp.exp(s) * z[k]) for k in range(T)]
    bins = bins_of(rs, variables, edges)
    E = [[F(0)] * MAX_BINS for _ in variables]
    for j in range(N):
        for k in range(T):
            if not rs.e[j, k] > 0:
                continue
            mu = F(float(rs.e[j, k])) * lam[k] * sig(eta(j, k))
            for v in range(len(variables)):
                E[v][int(bins[v, j, k])] += mu
    out = np.array([[float(x) for x in row] for row in E])
    return out, out.copy()


# ---------------------------------------------------------------------------------------------------
# The case table: the smallest shapes at which the kernel can go wrong
# ---------------------------------------------------------------------------------------------------

# (form, N, T, n): form "k" with n = K, "groups" with n = Gr (interleaved labels), "periods" with n = P.  One cell; one full tile
# of one interval; a second tile with one live lane; three tiles; by group; by period with eras and monthly; the longest walk.
SHAPES = [("k", 1, 1, 1), ("k", 1, 1, 2), ("k", 64, 1, 1), ("k", 64, 1, 2), ("k", 65, 3, 1), ("k", 65, 3, 2), ("k", 130, 65, 1),
          ("k", 130, 65, 2), ("groups", 130, 65, 4), ("periods", 130, 65, 3), ("periods", 130, 65, 65), ("k", 67, 511, 1)]
LONG = ("k", 67, 511, 1)  # for the walk's length: in one parity test only
EDGES_OWN = (0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 5.5)  # of the model's first titer, uniform on [-1, 6): 8 bins
EDGES_OTHER = (1.0, 2.5, 7.0)                    # of the other variable: the last bin holds no cell
# the cases whose per-cell replicates the fixture holds: (shape, seed, draw0); the draws draw0 .. draw0 + 2 are the points
# REPLICATE_POINTS.  One seed needs its high word, one draw0 is past 0.
REPLICATE_POINTS = ("typical", "b_plus_50", "b_minus_50")
REPLICATE_CASES = [(("k", 1, 1, 1), 1, 0), (("k", 65, 3, 2), 2, 5), (("k", 130, 65, 2), (7 << 32) | 3, 0), (("groups", 130, 65, 4), 4, 1000),
                   (("periods", 130, 65, 3), 5, 0)]


def tag(shape):
    form, N, T, n = shape
    return f"N{N}_T{T}_" + {"k": "K", "groups": "G", "periods": "P"}[form] + str(n)


def points_of(shape):
    return R1.POINTS if shape[0] == "k" else RG.POINTS


def point_of(shape, name, seed=0):
    form, N, T, n = shape
    return R1.make_point(name, T, n, seed) if form == "k" else RG.make_point(name, T, n, seed)


def model_of(shape):
    """(rs, made, variables, edges): the restatement object of a shape, what creates the device handle of it -- ("k", y, e, xs),
    ("groups", y, e, x, group, Gr) or ("periods", y, e, x, period, P) -- and its binning variables (N, T) with their edges: the
    model's first titer, and where N > 64 a second one (the model's second titer, or an independent one)."""
    form, N, T, n = shape
    if form == "k":
        y, e, xs = R1.make_data(N, T, n)
        rs, made, own, other = R1.Restatement(y, e, xs), ("k", y, e, xs), xs[0], xs[1] if n == 2 else None
    elif form == "groups":
        y, e, x, group = RG.make_case(N, T, n)
        rs, made, own, other = RG.GroupsRestatement(y, e, x, group, n), ("groups", y, e, x, group, n), x, None
    else:
        y, e, x, period = RP.make_case(N, T, n)
        rs, made, own, other = RP.PeriodsRestatement(y, e, x, period, n), ("periods", y, e, x, period, n), x, None
    if N <= 64:
        return rs, made, [own], [EDGES_OWN]
    if other is None:
        other = np.random.default_rng([N, T, 99]).uniform(-1.0, 6.0, size=(N, T))
    return rs, made, [own, other], [EDGES_OWN, EDGES_OTHER]


def cases():
    """(key, shape, point name) of every case of the expected tables"""
    for shape in SHAPES:
        for name in points_of(shape):
            yield f"{tag(shape)}_{name}", shape, name
