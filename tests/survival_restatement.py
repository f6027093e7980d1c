"""
The Poisson hazard models of ``abdpymc_amd.survival`` restated twice.  TEST INFRASTRUCTURE ONLY, like ``oracle/`` and
``tests/mp_reference.py``: the package never imports it.

``Restatement`` is NumPy float64: logp, gradient and the raw sums the device returns.  ``mp_evaluate`` is ``mpmath`` at 40 digits
from the float64 inputs converted exactly, and returns with every output the sum of the absolute values of its addends, S:
``u * S`` is the error a float64 evaluation is entitled to, whatever the value cancels to.

Model (reference survival.py:116-153), for (N, T) arrays y = infected, e = exposure, x_k = titer(s), NaN cells as y = e = 0:

    theta = a[K], b[K], m, s, z[T];  sd = exp(s);  r_t = m + sd z_t;  lambda_t = invlogit(r_t)
    eta = sum_k b_k (x_k - a_k);  sigma = invlogit(eta);  mu = e lambda_t sigma
    logp = sum_t [Y_t log lambda_t - lambda_t S_t] + L + C + priors        (Poisson, a cell with y = 0 has no log term)
    S_t = sum_j e sigma;  L = sum_{y>0} y log sigma;  C = sum_{y>0} y log e - sum lgamma(y + 1);  Y_t = sum_j y
    w = (y - mu)(1 - sigma);  W_0 = sum w;  W_k = sum w x_k

``tests/golden/make_survival_fixtures.py`` evaluates the case table below with ``mp_evaluate`` and commits the results rounded to
float64 (``tests/golden/survival_reference_k1.npz``, ``_k2.npz``); the GPU tests read that file and need no mpmath.
"""
import math

import numpy as np

U = 2.0 ** -53
# The worst error of Restatement against mp_evaluate over the case table, per class of point, in units of u * S_k
# (tests/test_survival_cpu.py measures, prints and asserts each).  Measured: typical 9.55, b_plus_50 248.7, b_minus_50 571.2,
# eta_800 732.9, r_plus_800 16.05, r_minus_800 11.86, sd_e10 13.66, sd_em10 19.25; each rounded up by a tenth and to the next
# integer, room for another libm's last bits.  The figures are far above the 3 u of a cell's own operations because S does not
# count the conditioning of sigma on eta = b (x - a): sigma = e^eta / (1 + e^eta) inherits about |eta| roundings of eta, and the
# worst output of a class is an S_t whose column holds one or few followed cells with eta << 0 (|eta| ~ 730 for eta_800, ~ 10 at
# the typical points).
E_NP = {"typical": 11.0, "b_plus_50": 274.0, "b_minus_50": 629.0, "eta_800": 807.0, "r_plus_800": 18.0, "r_minus_800": 14.0,
        "sd_e10": 16.0, "sd_em10": 22.0}
# |got_k - ref_k| <= C u S_k for the device, C = C_FACTOR E_NP[class].  4: the kernel's documented per-term errors against libm
# and a correctly rounded division -- DESIGN 19 derives it (exp2_reduced 3.1e-16 ~ 2.8 u on a two-term reduced argument, the
# twice-refined reciprocal 1.1e-16 ~ 1 u, the device library's log1p <= 2 ulp: about 7 u per term where the restatement's chain is
# about 3 u; eta itself is formed by the same operations in both, with an fma in place of one multiply-add).
C_FACTOR = 4.0


def c_device(name):
    return C_FACTOR * E_NP[name]


def _worst(got, ref, S, what):
    """max |got - ref| / (u S); where S = 0 the value is an empty sum and must be exactly 0"""
    got, ref, S = np.atleast_1d(got), np.atleast_1d(ref), np.atleast_1d(S)
    assert np.isfinite(got).all(), what
    assert (got[S == 0] == 0).all(), what
    m = S > 0
    return float((np.abs(got - ref)[m] / S[m] / U).max()) if m.any() else 0.0


FIXTURES = {1: "survival_reference_k1.npz", 2: "survival_reference_k2.npz"}  # one file per K: each stays below 1 MiB


def load_fixtures(golden_dir):
    """Every array of both fixture files, keyed ``<case>/<output>``."""
    import os

    out = {}
    for name in FIXTURES.values():
        with np.load(os.path.join(golden_dir, name)) as f:
            out.update({k: f[k] for k in f.files})
    return out

PRIORS = {1: (1.0, -3.0, 0.5, 2.0, 1.0), 2: (0.5, -3.0, 0.5, 2.0, 1.0)}  # ab_sd, mu_mean, mu_sd, sd_rate, z_sd


def clean(y, e, xs):
    """NaN cells as y = e = 0 and the titers of cells without follow-up as 0 (what creation does)."""
    y, e = np.array(y, dtype=np.float64), np.array(e, dtype=np.float64)
    bad = np.isnan(y) | np.isnan(e)
    y[bad] = 0.0
    e[bad] = 0.0
    off = (y == 0) & (e == 0)
    xs = [np.where(off, 0.0, np.asarray(x, dtype=np.float64)) for x in xs]
    return y, e, xs


def _log_invlogit(r):
    return np.minimum(r, 0.0) - np.log1p(np.exp(-np.abs(r)))


def _invlogit(r):
    en = np.exp(-np.abs(r))
    return np.where(r >= 0, 1.0, en) / (1.0 + en)


class Restatement:
    """NumPy float64.  ``logp_dlogp(q)`` takes (D,) and returns (logp, grad): the callable ``survival.sample(evaluator=)`` takes."""

    def __init__(self, infected, exposure, titers, priors=None):
        self.y, self.e, self.xs = clean(infected, exposure, titers)
        self.K = len(self.xs)
        self.N, self.T = self.y.shape
        self.dim = 2 * self.K + 2 + self.T
        self.priors = PRIORS[self.K] if priors is None else tuple(priors)
        self.Y = np.ascontiguousarray(self.y.T).sum(axis=1)
        pos = self.y > 0
        self.C = math.fsum(list(self.y[pos] * np.log(self.e[pos])) + [-math.lgamma(v + 1.0) for v in self.y.ravel()])

    def split(self, q):
        K = self.K
        q = np.asarray(q, dtype=np.float64)
        return q[:K], q[K:2 * K], q[2 * K], q[2 * K + 1], q[2 * K + 2:]

    def sums(self, q):
        """S_t (T), L, W_0, W_k (K) as the device returns them."""
        a, b, m, s, z = self.split(q)
        lam = _invlogit(m + np.exp(s) * z)
        eta = sum(b[k] * (self.xs[k] - a[k]) for k in range(self.K))
        sig, oms = _invlogit(eta), _invlogit(-eta)
        es = self.e * sig
        S = np.ascontiguousarray(es.T).sum(axis=1)  # along the contiguous axis: NumPy's pairwise sum, not N roundings in a row
        pos = self.y > 0
        L = (self.y[pos] * _log_invlogit(eta)[pos]).sum()
        w = (self.y - lam[None, :] * es) * oms
        return np.concatenate([S, [L, w.sum()], [(w * x).sum() for x in self.xs]])

    def combine(self, q, sums):
        K, T = self.K, self.T
        a, b, m, s, z = self.split(q)
        ab_sd, mu_mean, mu_sd, sd_rate, z_sd = self.priors
        sd = np.exp(s)
        r = m + sd * z
        lam, loglam, oml = _invlogit(r), _log_invlogit(r), _invlogit(-r)
        S, L, W0, W = sums[:T], sums[T], sums[T + 1], sums[T + 2:]
        half_log_2pi = 0.9189385332046727

        def normal(v, mean, sd_):
            zz = (v - mean) / sd_
            return -0.5 * zz * zz - np.log(sd_) - half_log_2pi, -zz / sd_

        lp = self.C + L + (self.Y * loglam - lam * S).sum()
        dr = (self.Y - lam * S) * oml
        g = np.empty(self.dim)
        la, ga = normal(a, 0.0, ab_sd)
        lb, gb = normal(b, 0.0, ab_sd)
        lm, gm = normal(m, mu_mean, mu_sd)
        lz, gz = normal(z, 0.0, z_sd)
        lp += la.sum() + lb.sum() + lm + lz.sum() + math.log(sd_rate) - sd_rate * sd + s
        g[:K] = -b * W0 + ga
        g[K:2 * K] = (W - a * W0) + gb
        g[2 * K] = dr.sum() + gm
        g[2 * K + 1] = sd * (z * dr).sum() - sd_rate * sd + 1.0
        g[2 * K + 2:] = sd * dr + gz
        return float(lp), g

    def logp_dlogp(self, q):
        with np.errstate(over="ignore", under="ignore"):
            return self.combine(q, self.sums(q))

    def logp(self, q):
        return self.logp_dlogp(q)[0]


# ---------------------------------------------------------------------------------------------------
# 40 digits
# ---------------------------------------------------------------------------------------------------


def _mp():
    import mpmath

    mpmath.mp.dps = 40
    return mpmath


class _Acc:
    def __init__(self, mp, n):
        self.v = [mp.mpf(0)] * n
        self.s = [mp.mpf(0)] * n

    def add(self, k, val):
        self.v[k] += val
        self.s[k] += abs(val)


def mp_evaluate(infected, exposure, titers, q, priors=None):
    """{"sums", "sums_S" (T + 2 + K), "logp", "logp_S", "grad", "grad_S" (D)} at 40 digits, rounded to float64 at the end."""
    mp = _mp()
    F = mp.mpf
    y, e, xs = clean(infected, exposure, titers)
    K = len(xs)
    N, T = y.shape
    D = 2 * K + 2 + T
    ab_sd, mu_mean, mu_sd, sd_rate, z_sd = (F(float(v)) for v in (PRIORS[K] if priors is None else priors))
    t = [F(float(v)) for v in q]
    a, b, m, s, z = t[:K], t[K:2 * K], t[2 * K], t[2 * K + 1], t[2 * K + 2:]
    sd = mp.exp(s)
    sig = lambda v: 1 / (1 + mp.exp(-v))  # noqa: E731
    lam = [sig(m + sd * z[k]) for k in range(T)]
    sums = _Acc(mp, T + 2 + K)
    lp = _Acc(mp, 1)
    Y = [F(0)] * T
    for j in range(N):
        for k in range(T):
            yy, ee = F(float(y[j, k])), F(float(e[j, k]))
            if yy == 0 and ee == 0:
                continue
            x = [F(float(xs[c][j, k])) for c in range(K)]
            eta = sum(b[c] * (x[c] - a[c]) for c in range(K))
            sg = sig(eta)
            oms = sig(-eta)
            sums.add(k, ee * sg)
            if yy > 0:
                sums.add(T, -yy * mp.log1p(mp.exp(-eta)))  # y log sigma, without the logarithm of 1 - tiny
                lp.add(0, yy * mp.log(ee))
            lp.add(0, -mp.loggamma(yy + 1))
            Y[k] += yy
            # w = (y - mu)(1 - sigma): two addends per cell
            for val in (yy * oms, -ee * lam[k] * sg * oms):
                sums.add(T + 1, val)
                for c in range(K):
                    sums.add(T + 2 + c, val * x[c])
    S, S_abs = sums.v[:T], sums.s[:T]
    L, W0 = sums.v[T], sums.v[T + 1]
    g = _Acc(mp, D)
    lp.add(0, L)
    lp.s[0] += sums.s[T] - abs(L)  # the addends of L are addends of logp

    def normal(acc_k, v, mean, sd_):
        zz = (v - mean) / sd_
        for val in (-zz * zz / 2, -mp.log(sd_), -mp.log(2 * mp.pi) / 2):
            lp.add(0, val)
        g.add(acc_k, -zz / sd_)

    for k in range(T):
        lp.add(0, -Y[k] * mp.log1p(mp.exp(-(m + sd * z[k]))))  # Y_t log lambda_t
        lp.add(0, -lam[k] * S[k])
        lp.s[0] += lam[k] * (S_abs[k] - abs(S[k]))
        oml = 1 - lam[k]
        # d/dr_t = (Y_t - lambda_t S_t)(1 - lambda_t), its addends Y_t (1 - lambda_t) and those of lambda_t S_t (1 - lambda_t)
        dr = (Y[k] - lam[k] * S[k]) * oml
        dr_abs = (Y[k] + lam[k] * S_abs[k]) * oml
        for idx, f in ((2 * K, F(1)), (2 * K + 1, sd * z[k]), (2 * K + 2 + k, sd)):
            g.v[idx] += f * dr
            g.s[idx] += abs(f) * dr_abs
        normal(2 * K + 2 + k, z[k], F(0), z_sd)
    for c in range(K):
        g.v[c] += -b[c] * W0
        g.s[c] += abs(b[c]) * sums.s[T + 1]
        normal(c, a[c], F(0), ab_sd)
        g.v[K + c] += sums.v[T + 2 + c] - a[c] * W0
        g.s[K + c] += sums.s[T + 2 + c] + abs(a[c]) * sums.s[T + 1]
        normal(K + c, b[c], F(0), ab_sd)
    normal(2 * K, m, mu_mean, mu_sd)
    for val in (mp.log(sd_rate), -sd_rate * sd, s):
        lp.add(0, val)
    g.add(2 * K + 1, -sd_rate * sd)
    g.add(2 * K + 1, F(1))
    f64 = lambda seq: np.array([float(v) for v in seq])  # noqa: E731
    return {"sums": f64(sums.v), "sums_S": f64(sums.s), "logp": float(lp.v[0]), "logp_S": float(lp.s[0]),
            "grad": f64(g.v), "grad_S": f64(g.s)}


# ---------------------------------------------------------------------------------------------------
# The case table: shapes, data and points of the parity tests (tests/test_gpu_survival.py reads the fixture made from it)
# ---------------------------------------------------------------------------------------------------

SHAPES = [(N, T) for N in (1, 67, 130, 1000) for T in (1, 2, 30, 63, 64, 65, 199, 511) if N <= 67 or T < 511]
POINTS = ("typical", "b_plus_50", "b_minus_50", "eta_800", "r_plus_800", "r_minus_800", "sd_e10", "sd_em10")


def make_data(N, T, K, seed=0):
    """Data with what the kernel has to get right: NaN tails and an individual NaN throughout (where N > 2), exposure-0 / y-0 cells,
    a column with Y_t = 0 (where T > 1), fractional y; y <= e wherever y > 0."""
    rng = np.random.default_rng([seed, N, T, K])
    raw = rng.uniform(0.0, 0.25, size=(N, T)) * (rng.random((N, T)) < 0.5)
    y = np.empty_like(raw)
    run = np.zeros(N)
    for t in range(T):
        v = raw[:, t]
        y[:, t] = np.where(run > 1.0, 0.0, np.where(run + v > 1.0, 1.0 - run, v))
        run = run + v
    e = np.ones_like(y)
    e[:, 1:] -= np.cumsum(y, axis=1)[:, :-1]
    e = np.clip(e, 0.0, 1.0)
    if T > 2:
        e[rng.random((N, T)) < 0.05] = 0.0  # exposure 0 ...
    y[e == 0] = 0.0                         # ... only with y 0
    if T > 1:
        y[:, T // 2] = 0.0                  # Y_t = 0
    last = rng.integers(max(1, T // 2), T + 1, size=N)
    if N > 2:
        last[1] = 0                         # NaN throughout
    nan = np.arange(T)[None, :] >= last[:, None]
    if N == 1:
        nan[:] = False
    y[nan] = np.nan
    e[nan] = np.nan
    xs = [rng.uniform(-1.0, 6.0, size=(N, T)) for _ in range(K)]
    for x in xs:
        x[nan] = np.nan
    return y, e, xs


def make_point(name, T, K, seed=0):
    rng = np.random.default_rng([seed, T, K, sum(map(ord, name))])
    a = rng.normal(1.5, 0.5, K)
    b = rng.normal(-1.0, 0.5, K)
    m, s, z = -3.0 + 0.3 * rng.normal(), math.log(0.4) + 0.2 * rng.normal(), rng.normal(size=T)
    if name == "b_plus_50":
        b[:] = 50.0
    elif name == "b_minus_50":
        b[:] = -50.0
    elif name == "eta_800":      # |eta| up to 800 at x in [-1, 6]: b (x - a) with a = 2.5, |x - a| <= 3.5
        a[:] = 2.5
        b[:] = 800.0 / 3.5 / K
    elif name == "r_plus_800":
        m = 800.0 - 3.0
        z = z * 0.0 + rng.uniform(0.0, 1.0, T) * 3.0 / math.exp(s)
    elif name == "r_minus_800":
        m = -800.0 + 3.0
        z = z * 0.0 - rng.uniform(0.0, 1.0, T) * 3.0 / math.exp(s)
    elif name == "sd_e10":
        s = 10.0
        z = z * 1e-4
    elif name == "sd_em10":
        s = -10.0
    elif name != "typical":
        raise KeyError(name)
    return np.concatenate([a, b, [m, s], z])


def points_of(N, T):
    """Every point at every shape."""
    return POINTS


def cases():
    """(key, N, T, K, point name) of every case of the table."""
    for N, T in SHAPES:
        for K in (1, 2):
            for name in points_of(N, T):
                yield f"N{N}_T{T}_K{K}_{name}", N, T, K, name
