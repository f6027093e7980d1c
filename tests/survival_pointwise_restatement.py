"""
The per-individual log-likelihood of the survival models (``abd_survival_individual_loglik``) restated twice.  TEST
INFRASTRUCTURE ONLY, like ``tests/survival_restatement.py`` and ``tests/survival_groups_restatement.py``, from which it takes the
data, the points and the helpers: the package never imports it.

For a model of either kind (K = 1, K = 2, by group) and a point in that model's layout, with lambda_t, sigma, y, e, x as there:

    ll_j = C_j + A_j - B_j
    A_j  = sum_t [ y > 0 ? y (log lambda_t + log sigma_jt) : 0 ]
    B_j  = sum_t e lambda_t sigma_jt
    C_j  = sum_{t: y > 0} ( y log e - lgamma(y + 1) )

PyMC's Poisson log-probability with fractional y, summed over individual j's intervals; sum_j ll_j is the data part of logp.

``pointwise`` is NumPy float64.  ``mp_pointwise`` is ``mpmath`` at 40 digits from the float64 inputs converted exactly and returns
with every ll_j the sum of the absolute values of its addends, S_j (per followed cell: e lambda sigma, and where y > 0
y log lambda, y log sigma, y log e, lgamma(y + 1)): ``u * S_j`` is the error a float64 evaluation is entitled to.  An individual
without a followed cell has no addend: S_j = 0 and ll_j = 0 exactly.

``tests/golden/make_survival_pointwise_fixtures.py`` evaluates the case table below with ``mp_pointwise`` and commits the results
rounded to float64 (``tests/golden/survival_pointwise_reference.npz``); the GPU tests read that file and need no mpmath.
"""
import math
import os

import numpy as np

from tests import survival_groups_restatement as RG
from tests import survival_restatement as R1
from tests.survival_restatement import U, _invlogit, _log_invlogit  # noqa: F401  (U is re-exported)

# The worst error of ``pointwise`` against ``mp_pointwise`` over the case table, per class of point, in units of u * S_j
# (tests/test_survival_pointwise_cpu.py measures, prints and asserts each).  Measured: typical 5.95, b_plus_50 9.73, b_minus_50
# 4.34, eta_800 8.85, r_plus_800 9.74, r_minus_800 3.24, sd_e10 6.20, sd_em10 5.87, a_spread 6.63; each rounded up by a tenth and
# to the next integer, as E_NP of tests/survival_restatement.py.  Above the 3 u of a cell's own operations for that table's
# reason -- S_j does not count the conditioning of sigma on eta = b (x - a), about |eta| roundings where eta << 0 -- and far
# below that table's figures at large |b|: an individual's S_j holds all its cells, those with eta > 0 and the y log sigma ~ y eta
# of an infected cell among them, so the worst output is no longer a sum of few cells with eta << 0 and nothing else (the one
# place where it still is: the single cell of the shape (1, 1), where four classes have their worst case).
E_NP = {"typical": 7.0, "b_plus_50": 11.0, "b_minus_50": 5.0, "eta_800": 10.0, "r_plus_800": 11.0, "r_minus_800": 4.0,
        "sd_e10": 7.0, "sd_em10": 7.0, "a_spread": 8.0}
# |got_j - ref_j| <= C u S_j for the device, C = C_FACTOR E_NP[class]: DESIGN 19's factor for the same cell chain (exp2_reduced on
# a two-term reduced argument, the twice-refined reciprocal, the device library's log1p), fixed before the kernel ran.
C_FACTOR = 4.0


def c_device(name):
    return C_FACTOR * E_NP[name]


FIXTURE = "survival_pointwise_reference.npz"


def load_fixture(golden_dir):
    """Every array of the fixture, keyed ``<case>/ll`` and ``<case>/ll_S``."""
    with np.load(os.path.join(golden_dir, FIXTURE)) as f:
        return {k: f[k] for k in f.files}


# ---------------------------------------------------------------------------------------------------
# NumPy float64
# ---------------------------------------------------------------------------------------------------


def _eta_r(rs, q):
    """(eta (N, T), r (T,)) of a ``Restatement`` or a ``GroupsRestatement`` at q"""
    if hasattr(rs, "Gr"):
        m, s, z, a_mu, a_sl, az, b = rs.split(q)
        a = a_mu + np.exp(a_sl) * az
        eta = b * (rs.x - a[rs.group][:, None])
    else:
        a, b, m, s, z = rs.split(q)
        eta = sum(b[k] * (rs.xs[k] - a[k]) for k in range(rs.K))
    return eta, m + np.exp(s) * z


def constants(rs):
    """(C_j (N,), n_cells (N,) int64) of the model's cleaned data"""
    C = np.array([math.fsum(v for yy, ee in zip(yr, er) if yy > 0 for v in (yy * math.log(ee), -math.lgamma(yy + 1.0)))
                  for yr, er in zip(rs.y, rs.e)])
    return C, (rs.e > 0).sum(axis=1).astype(np.int64)


def pointwise(rs, q):
    """ll_j (N,) of one point"""
    with np.errstate(over="ignore", under="ignore"):
        eta, r = _eta_r(rs, np.asarray(q, dtype=np.float64))
        lam, loglam = _invlogit(r), _log_invlogit(r)
        A = np.where(rs.y > 0, rs.y * (loglam[None, :] + _log_invlogit(eta)), 0.0).sum(axis=1)
        B = (lam[None, :] * (rs.e * _invlogit(eta))).sum(axis=1)
    return (constants(rs)[0] + A) - B


def pointwise_matrix(rs):
    """The callable ``survival.waic(..., pointwise=)`` takes: (n, D) -> (n, N)"""
    return lambda Q: np.stack([pointwise(rs, q) for q in np.atleast_2d(Q)])


def parameter_row(rs, q, n_draw):
    """lambda[T], log lambda[T], ab, 1 / n_draw: what one point gives the kernels (abd_survival_pointwise_terms.hpp)"""
    q = np.asarray(q, dtype=np.float64)
    if hasattr(rs, "Gr"):
        m, s, z, a_mu, a_sl, az, b = rs.split(q)
        ab = np.concatenate([a_mu + np.exp(a_sl) * az, [b]])
    else:
        a, b, m, s, z = rs.split(q)
        ab = np.concatenate([a, b])
    r = m + np.exp(s) * z
    with np.errstate(over="ignore", under="ignore"):
        return np.concatenate([_invlogit(r), _log_invlogit(r), ab, [1.0 / n_draw if n_draw > 0 else 0.0]])


# ---------------------------------------------------------------------------------------------------
# 40 digits
# ---------------------------------------------------------------------------------------------------


def _mp_setup(rs, q):
    import mpmath as mp

    mp.mp.dps = 40
    F = mp.mpf
    t = [F(float(v)) for v in q]
    sig = lambda v: 1 / (1 + mp.exp(-v))  # noqa: E731
    N, T = rs.y.shape
    if hasattr(rs, "Gr"):
        Gr = rs.Gr
        m, s, z, a_mu, a_sl, az, b = t[0], t[1], t[2:2 + T], t[T + 2], t[T + 3], t[T + 4:T + 4 + Gr], t[T + 4 + Gr]
        a = [a_mu + mp.exp(a_sl) * v for v in az]
        eta = lambda j, k: b * (F(float(rs.x[j, k])) - a[int(rs.group[j])])  # noqa: E731
    else:
        K = rs.K
        a, b, m, s, z = t[:K], t[K:2 * K], t[2 * K], t[2 * K + 1], t[2 * K + 2:]
        eta = lambda j, k: sum(b[c] * (F(float(rs.xs[c][j, k])) - a[c]) for c in range(K))  # noqa: E731
    r = [m + mp.exp(s) * z[k] for k in range(T)]
    return mp, F, sig, eta, r


def mp_pointwise(rs, q, raw=False):
    """{"ll", "ll_S"} (N,) at 40 digits, rounded to float64 at the end (``raw``: the mpmath numbers themselves)"""
    mp, F, sig, eta, r = _mp_setup(rs, q)
    N, T = rs.y.shape
    lam = [sig(v) for v in r]
    loglam = [-mp.log1p(mp.exp(-v)) for v in r]
    ll, S = [], []
    for j in range(N):
        v, sabs = F(0), F(0)
        for k in range(T):
            yy, ee = F(float(rs.y[j, k])), F(float(rs.e[j, k]))
            if yy == 0 and ee == 0:
                continue
            h = eta(j, k)
            terms = [-ee * lam[k] * sig(h)]
            if yy > 0:
                terms += [yy * loglam[k], -yy * mp.log1p(mp.exp(-h)), yy * mp.log(ee), -mp.loggamma(yy + 1)]
            for val in terms:
                v += val
                sabs += abs(val)
        ll.append(v)
        S.append(sabs)
    if raw:
        return {"ll": ll, "ll_S": S}
    return {"ll": np.array([float(v) for v in ll]), "ll_S": np.array([float(v) for v in S])}


def mp_data_loglik(rs, q):
    """The data log-likelihood of the whole cohort at 40 digits, written the other way round: interval by interval, every cell's
    Poisson log-probability y log mu - mu - lgamma(y + 1) from mu = e lambda_t sigma itself (an mpmath number)."""
    mp, F, sig, eta, r = _mp_setup(rs, q)
    N, T = rs.y.shape
    total = F(0)
    for k in range(T):
        lam = sig(r[k])
        for j in range(N):
            yy, ee = F(float(rs.y[j, k])), F(float(rs.e[j, k]))
            if yy == 0 and ee == 0:
                continue
            mu = ee * lam * sig(eta(j, k))
            total += (yy * mp.log(mu) if yy > 0 else 0) - mu - mp.loggamma(yy + 1)
    return total


# ---------------------------------------------------------------------------------------------------
# The case table: the smallest shapes at which the kernel can go wrong
# ---------------------------------------------------------------------------------------------------

# (N, T): the smallest; a second tile that is mostly padding; three tiles; the largest T -- for K = 1 and K = 2
SHAPES = [(1, 1), (67, 30), (130, 65), (67, 511)]
# (N, T, Gr): groups of sizes 1 / 2 / 64 (the slot permutation); one empty group, one group without follow-up, interleaved labels
SHAPES_GROUPS = [(67, 30, 3), (130, 65, 4)]
POINTS = R1.POINTS
POINTS_GROUPS = RG.POINTS


def model_of(N, T, K=None, Gr=None):
    """The restatement object of one shape (its cleaned data are the case's data) and what creates the device handle of it:
    (rs, ("k", y, e, xs)) or (rs, ("groups", y, e, x, group, Gr))"""
    if Gr is None:
        y, e, xs = R1.make_data(N, T, K)
        return R1.Restatement(y, e, xs), ("k", y, e, xs)
    y, e, x, group = RG.make_case(N, T, Gr)
    return RG.GroupsRestatement(y, e, x, group, Gr), ("groups", y, e, x, group, Gr)


def point_of(name, T, K=None, Gr=None, seed=0):
    return R1.make_point(name, T, K, seed) if Gr is None else RG.make_point(name, T, Gr, seed)


def cases():
    """(key, N, T, K, Gr, point name) of every case of the table; K is None for a grouped case, Gr for an ungrouped one"""
    for N, T in SHAPES:
        for K in (1, 2):
            for name in POINTS:
                yield f"N{N}_T{T}_K{K}_{name}", N, T, K, None, name
    for N, T, Gr in SHAPES_GROUPS:
        for name in POINTS_GROUPS:
            yield f"N{N}_T{T}_G{Gr}_{name}", N, T, None, Gr, name
