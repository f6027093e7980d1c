"""
The survival model by group of ``abdpymc_amd.survival`` (``model_alone_groups``; reference survival.py:155-174) restated twice.
TEST INFRASTRUCTURE ONLY, like ``tests/survival_restatement.py``, from which it takes the data generator and the helpers: the
package never imports it.

``GroupsRestatement`` is NumPy float64: logp, gradient and the raw sums the device returns.  ``mp_evaluate_groups`` is ``mpmath``
at 40 digits from the float64 inputs converted exactly, and returns with every output the sum of the absolute values of its
addends, S (``u * S`` is the error a float64 evaluation is entitled to).

Model, for (N, T) arrays y = infected, e = exposure, x = titer, NaN cells as y = e = 0, and g(j) in [0, Gr) the group of j:

    theta = m, s, z[T], a_mu, a_sd_log__, _a_z[Gr], b            D = T + Gr + 5 (PyMC's creation order: lam0 comes first)
    sd = exp(s);  r_t = m + sd z_t;  lambda_t = invlogit(r_t);  a_sd = exp(a_sd_log__);  a_g = a_mu + a_sd _a_z_g
    eta = b (x - a_g(j));  sigma = invlogit(eta);  mu = e lambda_t sigma
    logp = sum_t [Y_t log lambda_t - lambda_t S_t] + L + C + priors
    S_t = sum_j e sigma;  L = sum_{y>0} y log sigma;  w = (y - mu)(1 - sigma);  W_x = sum w x;  W0_g = sum_{j in g} w
    priors: m ~ N(0, 0.5) (no hyper_mu in this model), sd ~ Exp(2), z ~ N(0, 1); a_mu ~ N(0, 0.5), a_sd ~ Exp(2), _a_z ~ N(0, 1);
            b ~ N(0, 0.5)

``tests/golden/make_survival_groups_fixtures.py`` evaluates the case table below with ``mp_evaluate_groups`` and commits the
results rounded to float64 (``tests/golden/survival_groups_reference.npz``); the GPU tests read that file and need no mpmath.
"""
import math

import numpy as np

from tests.survival_restatement import U, _invlogit, clean, make_data  # noqa: F401  (U and clean are re-exported)
from tests.survival_restatement import _log_invlogit

# lam0_mu_mean, lam0_mu_sd, lam0_sd_rate, lam0_z_sd, a_mu_sd, a_sd_rate, a_z_sd, b_sd
PRIORS = (0.0, 0.5, 2.0, 1.0, 0.5, 2.0, 1.0, 0.5)

# The worst error of GroupsRestatement against mp_evaluate_groups over the case table, per class of point, in units of u * S_k
# (tests/test_survival_groups_cpu.py measures, prints and asserts each).  Measured: typical 3.25, b_plus_50 195.4, b_minus_50
# 190.82, eta_800 294.85, r_plus_800 3.91, r_minus_800 4.86, sd_e10 4.77, sd_em10 3.42, a_spread 4.00; each rounded up by a
# tenth and to the next integer, as E_NP of tests/survival_restatement.py, and above the 3 u of a cell's own operations for its
# reason: S does not count the conditioning of sigma on eta.  The figures are smaller than E_NP's because this table has six
# shapes where that one has thirty: fewer columns with a single followed cell at a large |eta|.
E_NP_GROUPS = {"typical": 4.0, "b_plus_50": 215.0, "b_minus_50": 210.0, "eta_800": 325.0, "r_plus_800": 5.0, "r_minus_800": 6.0,
               "sd_e10": 6.0, "sd_em10": 4.0, "a_spread": 5.0}
# |got_k - ref_k| <= C u S_k for the device, C = C_FACTOR E_NP_GROUPS[class]: DESIGN 19's derivation for the same cell chain
# (the grouped kernel runs the ungrouped kernel's cell function), fixed before the kernel ran.
C_FACTOR = 4.0


def c_device(name):
    return C_FACTOR * E_NP_GROUPS[name]


FIXTURE = "survival_groups_reference.npz"


def load_fixture(golden_dir):
    """Every array of the fixture, keyed ``<case>/<output>``."""
    import os

    with np.load(os.path.join(golden_dir, FIXTURE)) as f:
        return {k: f[k] for k in f.files}


class GroupsRestatement:
    """NumPy float64.  ``logp_dlogp(q)`` takes (D,) and returns (logp, grad): the callable ``survival.sample(evaluator=)`` takes."""

    def __init__(self, infected, exposure, titer, group, n_groups, priors=None):
        self.y, self.e, (self.x,) = clean(infected, exposure, [titer])
        self.group = np.asarray(group, dtype=np.int64)
        self.Gr = int(n_groups)
        self.N, self.T = self.y.shape
        assert self.group.shape == (self.N,) and self.group.min() >= 0 and self.group.max() < self.Gr
        self.dim = self.T + self.Gr + 5
        self.priors = PRIORS if priors is None else tuple(priors)
        self.Y = np.ascontiguousarray(self.y.T).sum(axis=1)
        pos = self.y > 0
        self.C = math.fsum(list(self.y[pos] * np.log(self.e[pos])) + [-math.lgamma(v + 1.0) for v in self.y.ravel()])

    def split(self, q):
        """m, s, z[T], a_mu, a_sd_log__, _a_z[Gr], b"""
        T, Gr = self.T, self.Gr
        q = np.asarray(q, dtype=np.float64)
        return q[0], q[1], q[2:2 + T], q[T + 2], q[T + 3], q[T + 4:T + 4 + Gr], q[T + 4 + Gr]

    def sums(self, q):
        """S_t (T), L, W_x, W0_g (Gr) as the device returns them."""
        m, s, z, a_mu, a_sl, az, b = self.split(q)
        lam = _invlogit(m + np.exp(s) * z)
        a = a_mu + np.exp(a_sl) * az
        eta = b * (self.x - a[self.group][:, None])
        sig, oms = _invlogit(eta), _invlogit(-eta)
        es = self.e * sig
        S = np.ascontiguousarray(es.T).sum(axis=1)  # along the contiguous axis: NumPy's pairwise sum
        pos = self.y > 0
        L = (self.y[pos] * _log_invlogit(eta)[pos]).sum()
        w = (self.y - lam[None, :] * es) * oms
        W0 = [w[self.group == g].sum() if (self.group == g).any() else 0.0 for g in range(self.Gr)]
        return np.concatenate([S, [L, (w * self.x).sum()], W0])

    def combine(self, q, sums):
        T, Gr = self.T, self.Gr
        m, s, z, a_mu, a_sl, az, b = self.split(q)
        mu_mean, mu_sd, sd_rate, z_sd, a_mu_sd, a_sd_rate, a_z_sd, b_sd = self.priors
        sd, a_sd = np.exp(s), np.exp(a_sl)
        a = a_mu + a_sd * az
        r = m + sd * z
        lam, loglam, oml = _invlogit(r), _log_invlogit(r), _invlogit(-r)
        S, L, Wx, W0 = sums[:T], sums[T], sums[T + 1], sums[T + 2:]
        half_log_2pi = 0.9189385332046727

        def normal(v, mean, sd_):
            zz = (v - mean) / sd_
            return -0.5 * zz * zz - np.log(sd_) - half_log_2pi, -zz / sd_

        lp = self.C + L + (self.Y * loglam - lam * S).sum()
        dr = (self.Y - lam * S) * oml
        g = np.empty(self.dim)
        lm, gm = normal(m, mu_mean, mu_sd)
        lz, gz = normal(z, 0.0, z_sd)
        lam_, gam = normal(a_mu, 0.0, a_mu_sd)
        laz, gaz = normal(az, 0.0, a_z_sd)
        lb, gb = normal(b, 0.0, b_sd)
        lp += lm + lz.sum() + math.log(sd_rate) - sd_rate * sd + s
        lp += lam_ + laz.sum() + math.log(a_sd_rate) - a_sd_rate * a_sd + a_sl + lb
        da = -b * W0
        g[0] = dr.sum() + gm
        g[1] = sd * (z * dr).sum() - sd_rate * sd + 1.0
        g[2:2 + T] = sd * dr + gz
        g[T + 2] = da.sum() + gam
        g[T + 3] = a_sd * (az * da).sum() - a_sd_rate * a_sd + 1.0
        g[T + 4:T + 4 + Gr] = a_sd * da + gaz
        g[T + 4 + Gr] = (Wx - (a * W0).sum()) + gb
        return float(lp), g

    def logp_dlogp(self, q):
        with np.errstate(over="ignore", under="ignore"):
            return self.combine(q, self.sums(q))

    def logp(self, q):
        return self.logp_dlogp(q)[0]


# ---------------------------------------------------------------------------------------------------
# 40 digits
# ---------------------------------------------------------------------------------------------------


class _Acc:
    def __init__(self, mp, n):
        self.v = [mp.mpf(0)] * n
        self.s = [mp.mpf(0)] * n

    def add(self, k, val):
        self.v[k] += val
        self.s[k] += abs(val)


def mp_evaluate_groups(infected, exposure, titer, group, n_groups, q, priors=None):
    """{"sums", "sums_S" (T + 2 + Gr), "logp", "logp_S", "grad", "grad_S" (D)} at 40 digits, rounded to float64 at the end."""
    import mpmath as mp

    mp.mp.dps = 40
    F = mp.mpf
    y, e, (x,) = clean(infected, exposure, [titer])
    N, T = y.shape
    Gr = int(n_groups)
    D = T + Gr + 5
    mu_mean, mu_sd, sd_rate, z_sd, a_mu_sd, a_sd_rate, a_z_sd, b_sd = (F(float(v)) for v in (PRIORS if priors is None else priors))
    t = [F(float(v)) for v in q]
    m, s, z, a_mu, a_sl, az, b = t[0], t[1], t[2:2 + T], t[T + 2], t[T + 3], t[T + 4:T + 4 + Gr], t[T + 4 + Gr]
    sd, a_sd = mp.exp(s), mp.exp(a_sl)
    a = [a_mu + a_sd * v for v in az]
    sig = lambda v: 1 / (1 + mp.exp(-v))  # noqa: E731
    lam = [sig(m + sd * z[k]) for k in range(T)]
    sums = _Acc(mp, T + 2 + Gr)
    lp = _Acc(mp, 1)
    Y = [F(0)] * T
    for j in range(N):
        gj = int(group[j])
        for k in range(T):
            yy, ee = F(float(y[j, k])), F(float(e[j, k]))
            if yy == 0 and ee == 0:
                continue
            xx = F(float(x[j, k]))
            eta = b * (xx - a[gj])
            sg = sig(eta)
            oms = sig(-eta)
            sums.add(k, ee * sg)
            if yy > 0:
                sums.add(T, -yy * mp.log1p(mp.exp(-eta)))  # y log sigma, without the logarithm of 1 - tiny
                lp.add(0, yy * mp.log(ee))
            lp.add(0, -mp.loggamma(yy + 1))
            Y[k] += yy
            for val in (yy * oms, -ee * lam[k] * sg * oms):  # w = (y - mu)(1 - sigma): two addends per cell
                sums.add(T + 1, val * xx)
                sums.add(T + 2 + gj, val)
    S, S_abs = sums.v[:T], sums.s[:T]
    L = sums.v[T]
    Wx, Wx_abs = sums.v[T + 1], sums.s[T + 1]
    W0, W0_abs = sums.v[T + 2:], sums.s[T + 2:]
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
    # the a block: d/da_g = -b W0_g, and the chain rule through a_g = a_mu + a_sd z_g
    i_mu, i_sl, i_z, i_b = T + 2, T + 3, T + 4, T + 4 + Gr
    g.v[i_b] += Wx
    g.s[i_b] += Wx_abs
    for c in range(Gr):
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
    return {"sums": f64(sums.v), "sums_S": f64(sums.s), "logp": float(lp.v[0]), "logp_S": float(lp.s[0]),
            "grad": f64(g.v), "grad_S": f64(g.s)}


# ---------------------------------------------------------------------------------------------------
# The case table: the smallest shapes at which the grouped kernel can go wrong
# ---------------------------------------------------------------------------------------------------

# (N, T, Gr): one cell; a full tile beside tiny groups (sizes 1 / 2 / 64); an empty group and a group without follow-up; more groups
# than a workgroup has waves or lanes and tiles that are mostly padding; the largest T; groups of several tiles (700 / 129 / 128
# / 42 / 1) over several ranges of intervals
SHAPES = [(1, 1, 1), (67, 30, 3), (130, 65, 4), (200, 2, 70), (67, 511, 2), (1000, 199, 5)]
POINTS = ("typical", "b_plus_50", "b_minus_50", "eta_800", "r_plus_800", "r_minus_800", "sd_e10", "sd_em10", "a_spread")


def make_groups(N, T, Gr):
    """Labels (N,) in [0, Gr): interleaved, never pre-sorted, wherever Gr > 1."""
    j = np.arange(N)
    if (N, Gr) == (67, 3):      # sizes 1 / 2 / 64
        lab = np.full(N, 2)
        lab[33] = 0
        lab[[10, 50]] = 1
    elif (N, Gr) == (130, 4):   # group 1 is empty; group 3 (13 individuals) has no follow-up at all (make_case)
        lab = np.where(j % 10 == 4, 3, np.where(j % 2 == 1, 0, 2))
    elif (N, Gr) == (1000, 5):  # sizes 700 / 129 / 128 / 42 / 1, shuffled
        lab = np.repeat(np.arange(5), (700, 129, 128, 42, 1))
        np.random.default_rng([N, T, Gr]).shuffle(lab)
    else:
        lab = j % Gr
    return lab.astype(np.int64)


def make_case(N, T, Gr):
    """(y, e, x, group) of one shape: ``make_data`` of the ungrouped table with the labels of ``make_groups``."""
    y, e, (x,) = make_data(N, T, 1)
    group = make_groups(N, T, Gr)
    if (N, Gr) == (130, 4):
        y[group == 3] = np.nan
        e[group == 3] = np.nan
        x[group == 3] = np.nan
    return y, e, x, group


def make_point(name, T, Gr, seed=0):
    """m, s, z[T], a_mu, a_sd_log__, _a_z[Gr], b with a_g around 1.5 (eta_800: all a_g = 2.5; a_spread: a_sd = e^3)."""
    rng = np.random.default_rng([seed, T, Gr, sum(map(ord, name))])
    b = rng.normal(-1.0, 0.5)
    m, s, z = -3.0 + 0.3 * rng.normal(), math.log(0.4) + 0.2 * rng.normal(), rng.normal(size=T)
    a_mu, a_sl, az = 1.5 + 0.2 * rng.normal(), math.log(0.5) + 0.2 * rng.normal(), rng.normal(size=Gr)
    if name == "b_plus_50":
        b = 50.0
    elif name == "b_minus_50":
        b = -50.0
    elif name == "eta_800":      # |eta| up to 800 at x in [-1, 6]: b (x - a) with a = 2.5, |x - a| <= 3.5
        a_mu, az = 2.5, az * 0.0
        b = 800.0 / 3.5
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
    elif name == "a_spread":
        a_sl = 3.0
    elif name != "typical":
        raise KeyError(name)
    return np.concatenate([[m, s], z, [a_mu, a_sl], az, [b]])


def cases():
    """(key, N, T, Gr, point name) of every case of the table."""
    for N, T, Gr in SHAPES:
        for name in POINTS:
            yield f"N{N}_T{T}_G{Gr}_{name}", N, T, Gr, name
