"""
The survival model by period of ``abdpymc_amd.survival`` (``model_alone_periods``) restated twice.  TEST INFRASTRUCTURE
ONLY, like ``tests/survival_groups_restatement.py``, from which it takes the closed forms of the host side, the points and the
helpers: the package never imports it.

``PeriodsRestatement`` is NumPy float64: logp, gradient, the raw sums the device returns and every individual's log-likelihood.
``mp_evaluate_periods`` is ``mpmath`` at 40 digits from the float64 inputs converted exactly, and returns with every output the
sum of the absolute values of its addends, S (``u * S`` is the error a float64 evaluation is entitled to).

Model, for (N, T) arrays y = infected, e = exposure, x = titer, NaN cells as y = e = 0, and p(t) in [0, P) the period of interval t:

    theta = m, s, z[T], a_mu, a_sd_log__, _a_z[P], b             D = T + P + 5 (the grouped model's layout with Gr -> P)
    sd = exp(s);  r_t = m + sd z_t;  lambda_t = invlogit(r_t);  a_sd = exp(a_sd_log__);  a_p = a_mu + a_sd _a_z_p
    eta = b (x - a_p(t));  sigma = invlogit(eta);  mu = e lambda_t sigma
    logp = sum_t [Y_t log lambda_t - lambda_t S_t] + L + C + priors
    S_t = sum_j e sigma;  L = sum_{y>0} y log sigma;  w = (y - mu)(1 - sigma);  W_x = sum w x;  W0_t = sum_j w
    W0_p = sum_{t in p} W0_t;  d/da_p = -b W0_p;  d/db = W_x - sum_p a_p W0_p
    priors: m ~ N(-3, 0.5) (hyper_mu = -3, as model_alone), sd ~ Exp(2), z ~ N(0, 1); a_mu ~ N(0, 0.5), a_sd ~ Exp(2),
            _a_z ~ N(0, 1); b ~ N(0, 0.5)

After the fold of W0_t into W0_p the host side is the grouped model's with (T, P, W0_p, a_p) in the places of (T, Gr, W0_g, a_g):
``PeriodsRestatement.combine`` calls ``GroupsRestatement.combine``.

``tests/golden/make_survival_periods_fixtures.py`` evaluates the case table below with ``mp_evaluate_periods`` and commits the
results rounded to float64 (``tests/golden/survival_periods_reference.npz``); the GPU tests read that file and need no mpmath.
"""
import math
import os

import numpy as np

from tests import survival_groups_restatement as RG
from tests import survival_pointwise_restatement as RP
from tests.survival_groups_restatement import _Acc
from tests.survival_restatement import U, _invlogit, _log_invlogit, clean, make_data  # noqa: F401  (U and clean are re-exported)

# lam0_mu_mean, lam0_mu_sd, lam0_sd_rate, lam0_z_sd, a_mu_sd, a_sd_rate, a_z_sd, b_sd
PRIORS = (-3.0, 0.5, 2.0, 1.0, 0.5, 2.0, 1.0, 0.5)

# The worst error of PeriodsRestatement against mp_evaluate_periods over the case table, per class of point, in units of u * S_k
# (tests/test_survival_periods_cpu.py measures, prints and asserts each).  Measured: typical 4.99, b_plus_50 195.40, b_minus_50
# 215.27, eta_800 297.85, r_plus_800 3.40, r_minus_800 4.64, sd_e10 5.60, sd_em10 5.52, a_spread 64.63; each rounded up by a
# tenth and to the next integer, as E_NP_GROUPS of tests/survival_groups_restatement.py, and above the 3 u of a cell's own
# operations for its reason: S does not count the conditioning of sigma on eta.  a_spread stands far above the grouped table's
# 4.00 for the same reason: with a_sd = e^3 the monthly shape has intervals whose midpoint lies 20 and more from every titer, so
# that an S_t or a W0_t -- a sum over one interval's cells alone, which the grouped model does not have -- holds only cells at
# eta << 0, as the worst outputs of the classes with a large |b| do.
E_NP_PERIODS = {"typical": 6.0, "b_plus_50": 215.0, "b_minus_50": 237.0, "eta_800": 328.0, "r_plus_800": 4.0, "r_minus_800": 6.0,
                "sd_e10": 7.0, "sd_em10": 7.0, "a_spread": 72.0}
# |got_k - ref_k| <= C u S_k for the device, C = C_FACTOR E_NP_PERIODS[class]: DESIGN 19's derivation for the same cell chain
# (the kernel by period runs the ungrouped kernel's cell function), fixed before the kernel ran.
C_FACTOR = 4.0


def c_device(name):
    return C_FACTOR * E_NP_PERIODS[name]


# The per-individual log-likelihood: the worst error of ``PeriodsRestatement.pointwise`` against the fixture's ``ll`` at the two
# pointwise shapes stays within E_NP of tests/survival_pointwise_restatement.py class by class (tests/test_survival_periods_cpu.py
# measures, prints and asserts each); the device's budget is that file's, C = 4 E_NP[class], for the same cell chain.
def c_device_pointwise(name):
    return RP.c_device(name)


FIXTURE = "survival_periods_reference.npz"


def load_fixture(golden_dir):
    """Every array of the fixture, keyed ``<case>/<output>``."""
    with np.load(os.path.join(golden_dir, FIXTURE)) as f:
        return {k: f[k] for k in f.files}


class PeriodsRestatement:
    """NumPy float64.  ``logp_dlogp(q)`` takes (D,) and returns (logp, grad): the callable ``survival.sample(evaluator=)`` takes."""

    def __init__(self, infected, exposure, titer, period, n_periods, priors=None):
        self.period = np.asarray(period, dtype=np.int64)
        self.P = int(n_periods)
        self.priors = PRIORS if priors is None else tuple(priors)
        # the host side after the fold: the grouped restatement of the same data with P "groups" (its labels are not read there)
        self._host = RG.GroupsRestatement(infected, exposure, titer, np.zeros(np.asarray(infected).shape[0], dtype=np.int64), self.P,
                                          self.priors)
        self.y, self.e, self.x = self._host.y, self._host.e, self._host.x
        self.N, self.T = self.y.shape
        assert self.period.shape == (self.T,) and self.period.min() >= 0 and self.period.max() < self.P and 1 <= self.P <= self.T
        self.dim = self.T + self.P + 5
        self.Y, self.C = self._host.Y, self._host.C

    def split(self, q):
        """m, s, z[T], a_mu, a_sd_log__, _a_z[P], b"""
        return self._host.split(q)

    def a_t(self, q):
        """the midpoint of every interval, (T,)"""
        m, s, z, a_mu, a_sl, az, b = self.split(q)
        return (a_mu + np.exp(a_sl) * az)[self.period]

    def sums(self, q):
        """S_t (T), L, W_x, W0_t (T) as the device returns them."""
        m, s, z, a_mu, a_sl, az, b = self.split(q)
        lam = _invlogit(m + np.exp(s) * z)
        eta = b * (self.x - self.a_t(q)[None, :])
        sig, oms = _invlogit(eta), _invlogit(-eta)
        es = self.e * sig
        S = np.ascontiguousarray(es.T).sum(axis=1)  # along the contiguous axis: NumPy's pairwise sum
        pos = self.y > 0
        L = (self.y[pos] * _log_invlogit(eta)[pos]).sum()
        w = (self.y - lam[None, :] * es) * oms
        return np.concatenate([S, [L, (w * self.x).sum()], np.ascontiguousarray(w.T).sum(axis=1)])

    def fold(self, sums):
        """S_t (T), L, W_x, W0_p (P): the sums the grouped host side takes.  A period without intervals gets exactly 0."""
        T = self.T
        W0_t = sums[T + 2:]
        W0_p = [math.fsum(W0_t[self.period == p]) for p in range(self.P)]
        return np.concatenate([sums[:T + 2], W0_p])

    def combine(self, q, sums):
        return self._host.combine(q, self.fold(np.asarray(sums, dtype=np.float64)))

    def logp_dlogp(self, q):
        with np.errstate(over="ignore", under="ignore"):
            return self.combine(q, self.sums(q))

    def logp(self, q):
        return self.logp_dlogp(q)[0]

    def pointwise(self, q):
        """ll_j (N,) of one point: C_j + A_j - B_j of tests/survival_pointwise_restatement.py"""
        q = np.asarray(q, dtype=np.float64)
        with np.errstate(over="ignore", under="ignore"):
            m, s, z, a_mu, a_sl, az, b = self.split(q)
            r = m + np.exp(s) * z
            eta = b * (self.x - self.a_t(q)[None, :])
            lam, loglam = _invlogit(r), _log_invlogit(r)
            A = np.where(self.y > 0, self.y * (loglam[None, :] + _log_invlogit(eta)), 0.0).sum(axis=1)
            B = (lam[None, :] * (self.e * _invlogit(eta))).sum(axis=1)
        return (RP.constants(self)[0] + A) - B

    def pointwise_matrix(self):
        """The callable ``survival.waic(..., pointwise=)`` takes: (n, D) -> (n, N)"""
        return lambda Q: np.stack([self.pointwise(q) for q in np.atleast_2d(Q)])

    def data_logp(self, q):
        """The data part of logp: C + L + sum_t [Y_t log lambda_t - lambda_t S_t]"""
        m, s, z = self.split(q)[:3]
        r = m + np.exp(s) * z
        sums = self.sums(q)
        with np.errstate(over="ignore", under="ignore"):
            return float(self.C + sums[self.T] + (self.Y * _log_invlogit(r) - _invlogit(r) * sums[:self.T]).sum())


# ---------------------------------------------------------------------------------------------------
# 40 digits
# ---------------------------------------------------------------------------------------------------


def mp_evaluate_periods(infected, exposure, titer, period, n_periods, q, priors=None, pointwise=False):
    """{"sums", "sums_S" (2 T + 2), "logp", "logp_S", "grad", "grad_S" (D)} at 40 digits, rounded to float64 at the end; with
    ``pointwise`` also {"ll", "ll_S"} (N,), every individual's log-likelihood with the addends of
    tests/survival_pointwise_restatement.py."""
    import mpmath as mp

    mp.mp.dps = 40
    F = mp.mpf
    y, e, (x,) = clean(infected, exposure, [titer])
    N, T = y.shape
    P = int(n_periods)
    period = [int(v) for v in period]
    D = T + P + 5
    mu_mean, mu_sd, sd_rate, z_sd, a_mu_sd, a_sd_rate, a_z_sd, b_sd = (F(float(v)) for v in (PRIORS if priors is None else priors))
    t = [F(float(v)) for v in q]
    m, s, z, a_mu, a_sl, az, b = t[0], t[1], t[2:2 + T], t[T + 2], t[T + 3], t[T + 4:T + 4 + P], t[T + 4 + P]
    sd, a_sd = mp.exp(s), mp.exp(a_sl)
    a = [a_mu + a_sd * v for v in az]
    sig = lambda v: 1 / (1 + mp.exp(-v))  # noqa: E731
    lam = [sig(m + sd * z[k]) for k in range(T)]
    loglam = [-mp.log1p(mp.exp(-(m + sd * z[k]))) for k in range(T)]
    sums = _Acc(mp, 2 * T + 2)
    lp = _Acc(mp, 1)
    ll = _Acc(mp, N)
    Y = [F(0)] * T
    for j in range(N):
        for k in range(T):
            yy, ee = F(float(y[j, k])), F(float(e[j, k]))
            if yy == 0 and ee == 0:
                continue
            xx = F(float(x[j, k]))
            eta = b * (xx - a[period[k]])
            sg = sig(eta)
            oms = sig(-eta)
            sums.add(k, ee * sg)
            if yy > 0:
                ls = -yy * mp.log1p(mp.exp(-eta))  # y log sigma, without the logarithm of 1 - tiny
                sums.add(T, ls)
                lp.add(0, yy * mp.log(ee))
            lp.add(0, -mp.loggamma(yy + 1))
            Y[k] += yy
            for val in (yy * oms, -ee * lam[k] * sg * oms):  # w = (y - mu)(1 - sigma): two addends per cell
                sums.add(T + 1, val * xx)
                sums.add(T + 2 + k, val)
            if pointwise:
                ll.add(j, -ee * lam[k] * sg)
                if yy > 0:
                    for val in (yy * loglam[k], ls, yy * mp.log(ee), -mp.loggamma(yy + 1)):
                        ll.add(j, val)
    S, S_abs = sums.v[:T], sums.s[:T]
    L = sums.v[T]
    Wx, Wx_abs = sums.v[T + 1], sums.s[T + 1]
    W0 = [sum((sums.v[T + 2 + k] for k in range(T) if period[k] == c), F(0)) for c in range(P)]
    W0_abs = [sum((sums.s[T + 2 + k] for k in range(T) if period[k] == c), F(0)) for c in range(P)]
    g = _Acc(mp, D)
    lp.add(0, L)
    lp.s[0] += sums.s[T] - abs(L)  # the addends of L are addends of logp

    def normal(acc_k, v, mean, sd_):
        zz = (v - mean) / sd_
        for val in (-zz * zz / 2, -mp.log(sd_), -mp.log(2 * mp.pi) / 2):
            lp.add(0, val)
        g.add(acc_k, -zz / sd_)

    for k in range(T):
        lp.add(0, Y[k] * loglam[k])
        lp.add(0, -lam[k] * S[k])
        lp.s[0] += lam[k] * (S_abs[k] - abs(S[k]))
        oml = 1 - lam[k]
        dr = (Y[k] - lam[k] * S[k]) * oml
        dr_abs = (Y[k] + lam[k] * S_abs[k]) * oml
        for idx, f in ((0, F(1)), (1, sd * z[k]), (2 + k, sd)):
            g.v[idx] += f * dr
            g.s[idx] += abs(f) * dr_abs
        normal(2 + k, z[k], F(0), z_sd)
    normal(0, m, mu_mean, mu_sd)
    for val in (mp.log(sd_rate), -sd_rate * sd, s):
        lp.add(0, val)
    g.add(1, -sd_rate * sd)
    g.add(1, F(1))
    # the a block: d/da_p = -b W0_p, and the chain rule through a_p = a_mu + a_sd z_p
    i_mu, i_sl, i_z, i_b = T + 2, T + 3, T + 4, T + 4 + P
    g.v[i_b] += Wx
    g.s[i_b] += Wx_abs
    for c in range(P):
        da, da_abs = -b * W0[c], abs(b) * W0_abs[c]
        for idx, f in ((i_mu, F(1)), (i_sl, a_sd * az[c]), (i_z + c, a_sd)):
            g.v[idx] += f * da
            g.s[idx] += abs(f) * da_abs
        g.v[i_b] += -a[c] * W0[c]
        g.s[i_b] += abs(a[c]) * W0_abs[c]
        normal(i_z + c, az[c], F(0), a_z_sd)
    normal(i_mu, a_mu, F(0), a_mu_sd)
    for val in (mp.log(a_sd_rate), -a_sd_rate * a_sd, a_sl):
        lp.add(0, val)
    g.add(i_sl, -a_sd_rate * a_sd)
    g.add(i_sl, F(1))
    normal(i_b, b, F(0), b_sd)
    f64 = lambda seq: np.array([float(v) for v in seq])  # noqa: E731
    out = {"sums": f64(sums.v), "sums_S": f64(sums.s), "logp": float(lp.v[0]), "logp_S": float(lp.s[0]),
           "grad": f64(g.v), "grad_S": f64(g.s)}
    if pointwise:
        out.update(ll=f64(ll.v), ll_S=f64(ll.s))
    return out


# ---------------------------------------------------------------------------------------------------
# The case table: the smallest shapes at which the kernel by period can go wrong
# ---------------------------------------------------------------------------------------------------

# (N, T, P): one cell; unequal periods, one of a single interval; monthly, with two finalize workgroups for S_t and for W0_t; two
# intervals; the largest T with labels that are not monotone; several tiles with a period that has no interval; 33 tiles, where
# ceil(4096 / 33) = 125 < 129 makes ranges of two intervals and a last range of one
SHAPES = [(1, 1, 1), (67, 30, 3), (130, 65, 65), (200, 2, 2), (67, 511, 4), (1000, 199, 5), (2100, 129, 4)]
POINTS = RG.POINTS
# the shapes whose cases also hold the per-individual log-likelihood
SHAPES_POINTWISE = [(67, 30, 3), (130, 65, 65)]


def plan(N, T):
    """(ntile, seg_len, nseg) of the launches, as creation plans them from N and T alone (abd_survival.hip)"""
    ntile = (N + 63) // 64
    want = max(1, min(T, (4096 + ntile - 1) // ntile))
    seg_len = (T + want - 1) // want
    return ntile, seg_len, (T + seg_len - 1) // seg_len


def make_periods(N, T, P):
    """Labels (T,) in [0, P)."""
    t = np.arange(T)
    if (T, P) == (30, 3):       # lengths 12 / 1 / 17
        lab = np.where(t < 12, 0, np.where(t == 12, 1, 2))
    elif (T, P) == (511, 4):    # not monotone
        lab = (3 * t + t // 64) % 4
    elif (T, P) == (199, 5):    # period 3 has no interval
        lab = np.minimum(t // 50, 3)
        lab[lab == 3] = 4
    elif P == T:
        lab = t
    else:
        lab = np.minimum(t // -(-T // P), P - 1)
    return lab.astype(np.int64)


def make_case(N, T, P):
    """(y, e, x, period) of one shape: ``make_data`` of the ungrouped table with the labels of ``make_periods``."""
    y, e, (x,) = make_data(N, T, 1)
    return y, e, x, make_periods(N, T, P)


def make_point(name, T, P, seed=0):
    """m, s, z[T], a_mu, a_sd_log__, _a_z[P], b: the grouped table's point of the same class (Gr -> P)"""
    return RG.make_point(name, T, P, seed)


def model_of(N, T, P):
    y, e, x, period = make_case(N, T, P)
    return PeriodsRestatement(y, e, x, period, P), (y, e, x, period)


def cases():
    """(key, N, T, P, point name) of every case of the table."""
    for N, T, P in SHAPES:
        for name in POINTS:
            yield f"N{N}_T{T}_P{P}_{name}", N, T, P, name
