"""
A 40-digit restatement of the joint log-probability.  TEST INFRASTRUCTURE ONLY, like ``oracle/``: the package never imports it.

The float64 oracle (``oracle/abd_oracle.py``) is the yardstick at typical parameter values.  Away from them -- steep or reversed
curves, rho at 0 or 1, tiny sigma, huge or vanishing perm / temp -- it loses digits to cancellation like any float64 code,
returns NaN (``e * s = inf * 0`` in ``lik``) or raises (``math.exp`` in ``_sigmoid``).  This file states the same model in
``mpmath`` at 40 digits, from the float64 inputs converted exactly, and returns with every output the sum of the absolute values
of its addends, S: ``u * S`` is the error a float64 evaluation is entitled to, whatever the value cancels to.

Rules: the integer pre-pass (``i``) is ``O.constrain_infections`` (exact, pinned by the reference's known answers); the model
is the one ``O.logp_dlogp`` states (unit S boosts, ``rho_j = rho_s`` if waner else 1, ``cum`` on ``i`` for N and on ``i + v`` for
S); ``b == 0`` is the limit ``s = 1/2``.

``tests/golden/make_tail_fixtures.py`` evaluates the case table below with it and commits the results rounded to float64
(``tests/golden/tail_parity.npz``); the GPU tests read that file and need no mpmath.
"""
import math

import numpy as np

from abdpymc_amd import synthetic
from oracle import abd_oracle as O
from tests.helpers import oracle_cohort_from_synth, random_sparse_cohort

U = 2.0 ** -53
# The worst error of O.logp_dlogp against this reference over the case table, in units of u * S_k (tests/test_tail_reference_cpu.py measures,
# prints and asserts it: 40.7 at b = +300 on fp32-rounded panels, entry 3; rounded up with room for another libm's last bits).  The device budget derives from it.
E_ORACLE = 48.0
# |got_k - ref_k| <= C u S_k.  32: the kernels' documented per-term errors against a correctly rounded division and libm
# (rcp_newton 2.2e-15 ~ 20 u, the table 2^t 3.5e-16 ~ 3 u; abd_device.hpp), with the sums' own rounding on top.
C_BUDGET = 32.0 * E_ORACLE
FIXTURE = "tail_parity.npz"

LIK_ENTRIES = {"n": (1, 2, 3, 4, 11, 12, 13), "s": (5, None, 6, 10, 14, 15, 16)}  # perm, temp, rho, init, b, d, sigma


def _mp():
    import mpmath

    mpmath.mp.dps = 40
    return mpmath


class _Acc:
    """18 sums (17 gradient entries, logp at 17) and the sums of the absolute values of what went into them"""

    def __init__(self, mp):
        self.v = [mp.mpf(0)] * 18
        self.s = [mp.mpf(0)] * 18

    def add(self, k, val):
        self.v[k] += val
        self.s[k] += abs(val)


def _theta_mp(mp, theta):
    return [mp.mpf(float(x)) for x in theta]  # exact


def _priors(mp, acc, t, G, N, cells, n1, m1):
    F = mp.mpf
    sig = lambda z: 1 / (1 + mp.exp(-z))  # noqa: E731
    lsig = lambda z: -mp.log(1 + mp.exp(-z))  # noqa: E731

    def lbeta(a, b):
        return mp.loggamma(a) + mp.loggamma(b) - mp.loggamma(a + b)

    L0, L1, p = lsig(t[0]), lsig(-t[0]), sig(t[0])
    bm1 = G - 2
    for val in (bm1 * L1, -lbeta(1, G - 1), L0, L1, n1 * L0, (cells - n1) * L1):
        acc.add(17, val)
    acc.add(0, (1 + n1) * (1 - p))
    acc.add(0, -p * (bm1 + 1 + cells - n1))
    for k, mu in ((1, 2), (2, 1), (5, 2), (8, 1), (9, 1)):
        a, b, x = F(mu * mu) * 4, F(mu) * 4, mp.exp(t[k])
        for val in (a * mp.log(b), -mp.loggamma(a), a * t[k], -b * x):
            acc.add(17, val)
        acc.add(k, a)
        acc.add(k, -b * x)
    for k in (3, 6):
        L0, L1, r = lsig(t[k]), lsig(-t[k]), sig(t[k])
        for val in (9 * L0, -lbeta(10, 1), L0, L1):
            acc.add(17, val)
        acc.add(k, 10 * (1 - r))
        acc.add(k, -r)
    L0, L1, q = lsig(t[7]), lsig(-t[7]), sig(t[7])
    for val in (L0, L1, m1 * L0, (N - m1) * L1):
        acc.add(17, val)
    acc.add(7, (1 + m1) * (1 - q))
    acc.add(7, -q * (1 + N - m1))
    for k, mu, sd in ((4, -2, 1), (10, -2, 1), (11, -1, F(1) / 2), (12, 2, F(1) / 2), (14, -1, F(1) / 2), (15, 2, F(1) / 2)):
        z = (t[k] - mu) / sd
        for val in (-z * z / 2, -mp.log(sd), -mp.log(2 * mp.pi) / 2):
            acc.add(17, val)
        acc.add(k, -z / sd)
    for k in (13, 16):
        x = mp.exp(t[k])
        acc.add(17, -x)
        acc.add(17, t[k])
        acc.add(k, -x)
        acc.add(k, F(1))


class _Model:
    """The titers of one (theta, discrete state): per individual the scans U (response) and D (dU / d rho), made when first asked for"""

    def __init__(self, mp, theta, i_raw, waner, cohort, splits, ignore_pcrpos):
        self.mp = mp
        F = mp.mpf
        t = self.t = _theta_mp(mp, theta)
        sig = lambda z: 1 / (1 + mp.exp(-z))  # noqa: E731
        self.G, self.N = cohort.n_gaps, cohort.n_inds
        self.v = np.asarray(cohort.vacs).T.astype(np.int64)
        pcr = np.zeros(self.v.shape) if ignore_pcrpos else np.asarray(cohort.pcrpos, dtype=float).T
        self.i = O.constrain_infections(np.asarray(i_raw), pcr, splits)
        self.ii = self.i.astype(np.int64)
        self.waner = np.asarray(waner).astype(bool)
        self.cum = {"n": np.cumsum(self.ii, axis=0) > 0, "s": np.cumsum(self.ii + self.v, axis=0) > 0}
        self.perm = {"n": mp.exp(t[1]), "s": mp.exp(t[5])}
        self.temp_n = mp.exp(t[2])
        self.rho = {"n": sig(t[3]), "s": sig(t[6])}
        self.init = {"n": t[4], "s": t[10]}
        self.b = {"n": t[11], "s": t[14]}
        self.d = {"n": t[12], "s": t[15]}
        self.sg = {"n": mp.exp(t[13]), "s": mp.exp(t[16])}
        self._scans = {}
        self.zero = F(0)

    def scan(self, ag, j):
        key = (ag, j)
        if key not in self._scans:
            F = self.mp.mpf
            if ag == "n":
                e, rho, sens = self.ii[:, j], self.rho["n"], True
            else:
                e, rho, sens = self.ii[:, j] + self.v[:, j], (self.rho["s"] if self.waner[j] else F(1)), bool(self.waner[j])
            Us, Ds, u, d = [], [], F(0), F(0)
            for g in range(self.G):
                d = rho * d + u
                u = rho * u + int(e[g])
                Us.append(u)
                Ds.append(d if sens else F(0))
            self._scans[key] = (Us, Ds)
        return self._scans[key]

    def titer(self, ag, g, j):
        """(a, sum of |addends| of a, U, D) of antigen ag at cell (g, j)"""
        Us, Ds = self.scan(ag, j)
        pm = self.perm[ag] if self.cum[ag][g, j] else self.zero
        resp = self.temp_n * Us[g] if ag == "n" else Us[g]
        return pm + resp + self.init[ag], pm + resp + abs(self.init[ag]), Us[g], Ds[g]

    def reading(self, ag, g, j, x, y):
        """One OD reading -> dict of the curve mean, the log-density, its addends' absolute sum, and what the gradient needs"""
        mp = self.mp
        a, _, Ug, Dg = self.titer(ag, g, j)
        b, d, sg = self.b[ag], self.d[ag], self.sg[ag]
        z = b * (a - x)
        if b == 0:
            s, one_minus_s = mp.mpf(1) / 2, mp.mpf(1) / 2
        else:
            e = mp.exp(z)
            s, one_minus_s = 1 / (1 + e), e / (1 + e)
        m = d * s
        r = (y - m) / sg
        adds = (-r * r / 2, -mp.log(sg), -mp.log(2 * mp.pi) / 2)
        return dict(a=a, z=z, s=s, oms=one_minus_s, m=m, r=r, adds=adds, U=Ug, D=Dg)


def _lik(mp, acc, mdl, obs, ag, per_reading=None, t_ext=None, dev=None):
    """dev: a list of 7 zeros -> the sums a kernel hands to abd_terms.hpp (abd_types.hpp): Q2, H, HC, HU, HD, HX, QS with
    q = od - d s and h' = q s (1 - s)"""
    F = mp.mpf
    k_perm, k_temp, k_rho, k_init, k_b, k_d, k_sig = LIK_ENTRIES[ag]
    b, d, sg = mdl.b[ag], mdl.d[ag], mdl.sg[ag]
    rho = mdl.rho[ag]
    log2e = 1 / mp.log(2)
    for g, j, x, y in zip(np.asarray(obs.idx_gap), np.asarray(obs.idx_ind), np.asarray(obs.log_dilution, float), np.asarray(obs.od, float)):
        g, j, x, y = int(g), int(j), F(float(x)), F(float(y))
        q = mdl.reading(ag, g, j, x, y)
        for val in q["adds"]:
            acc.add(17, val)
        wgt = q["r"] / sg  # d ll / d m
        dm_du = -d * q["s"] * q["oms"]
        ga = wgt * dm_du * b
        if mdl.cum[ag][g, j]:
            acc.add(k_perm, ga * mdl.perm[ag])
        if ag == "n":
            acc.add(k_temp, ga * q["U"] * mdl.temp_n)
            acc.add(k_rho, ga * q["D"] * mdl.temp_n * rho * (1 - rho))
        else:
            acc.add(k_rho, ga * q["D"] * rho * (1 - rho))
        acc.add(k_init, ga)
        acc.add(k_b, wgt * dm_du * (q["a"] - x))
        acc.add(k_d, wgt * q["s"])
        acc.add(k_sig, q["r"] * q["r"])
        acc.add(k_sig, F(-1))
        if dev is not None:
            qq = y - q["m"]
            h = qq * q["s"] * q["oms"]
            for n, val in enumerate((qq * qq, h, h if mdl.cum[ag][g, j] else 0, h * q["U"], h * q["D"], h * (q["a"] - x), qq * q["s"])):
                dev[n] += val
        if per_reading is not None:
            per_reading.append((sum(q["adds"]), q["m"], sum(abs(v) for v in q["adds"])))
        if t_ext is not None:
            tt = q["z"] * log2e
            t_ext[0] = tt if t_ext[0] is None else min(t_ext[0], tt)
            t_ext[1] = tt if t_ext[1] is None else max(t_ext[1], tt)
            t_ext[2] = abs(tt) if t_ext[2] is None else max(t_ext[2], abs(tt))


def evaluate(theta, i_raw, waner, cohort, splits=None, ignore_pcrpos=False):
    """Everything about one point, rounded to float64: dict of
    ref (18,): the 17 gradient entries and logp (entry 17); S (18,): the absolute sums of their addends, priors included;
    ref_lik, S_lik (18,): the same without the prior addends (the two observed Normals alone);
    sums (16,): the 13 sums of abd_types.hpp (HX as the list kernels return it: not scaled), n1, m1 and a zero;
    t_ext (3,): min t, max t, max |t| of t = b log2(e) (a - x) over all readings (max |t| keeps magnitudes below float64's)."""
    mp = _mp()
    i_raw, waner = np.asarray(i_raw), np.asarray(waner)
    mdl = _Model(mp, theta, i_raw, waner, cohort, splits, ignore_pcrpos)
    lik, t_ext = _Acc(mp), [None, None, None]
    dev_n, dev_s = [mp.mpf(0)] * 7, [mp.mpf(0)] * 7
    _lik(mp, lik, mdl, cohort.n, "n", t_ext=t_ext, dev=dev_n)
    _lik(mp, lik, mdl, cohort.s, "s", t_ext=t_ext, dev=dev_s)
    sums = dev_n + [dev_s[n] for n in (0, 1, 2, 4, 5, 6)] + [mp.mpf(int(i_raw.sum())), mp.mpf(int(waner.sum())), mp.mpf(0)]
    full = _Acc(mp)
    _priors(mp, full, mdl.t, mdl.G, mdl.N, i_raw.size, int(i_raw.sum()), int(waner.sum()))
    for k in range(18):
        full.v[k] += lik.v[k]
        full.s[k] += lik.s[k]
    f = lambda xs: np.array([float(x) for x in xs])  # noqa: E731
    return dict(ref=f(full.v), S=f(full.s), ref_lik=f(lik.v), S_lik=f(lik.s), sums=f(sums), t_ext=f([mp.mpf(0) if x is None else x for x in t_ext]))


def logp_dlogp(theta, i_raw, waner, cohort, splits=None, ignore_pcrpos=False):
    """(logp, grad (17,), S (18,)): S[k] the sum of the absolute values of all addends of gradient entry k, S[17] of logp"""
    r = evaluate(theta, i_raw, waner, cohort, splits, ignore_pcrpos)
    return float(r["ref"][17]), r["ref"][:17].copy(), r["S"]


def pointwise(theta, i_raw, waner, cohort, splits=None, ignore_pcrpos=False):
    """Per reading, S list then N list, each (K, 3): the log-density ll, the curve mean m, and the sum of |ll's addends|"""
    mp = _mp()
    mdl = _Model(mp, theta, np.asarray(i_raw), np.asarray(waner), cohort, splits, ignore_pcrpos)
    out = []
    for ag, obs in (("s", cohort.s), ("n", cohort.n)):
        rows = []
        _lik(mp, _Acc(mp), mdl, obs, ag, per_reading=rows)
        out.append(np.array([[float(v) for v in row] for row in rows]).reshape(-1, 3))
    return out[0], out[1]


def deterministics(theta, i_raw, waner, cohort, splits=None, ignore_pcrpos=False):
    """i (G, N) int8, then ab_n_mu and ab_s_mu as (2, G, N): [0] the titer, [1] the sum of the absolute values of its addends"""
    mp = _mp()
    mdl = _Model(mp, theta, np.asarray(i_raw), np.asarray(waner), cohort, splits, ignore_pcrpos)
    out = {}
    for ag in ("n", "s"):
        mu = np.empty((2, mdl.G, mdl.N))
        for j in range(mdl.N):
            for g in range(mdl.G):
                a, sa, _, _ = mdl.titer(ag, g, j)
                mu[0, g, j], mu[1, g, j] = float(a), float(sa)
        out[ag] = mu
    return mdl.i.astype(np.int8), out["n"], out["s"]


# --------------------------------------------------------------------------------------------------------------------------
# The case table (shared by the generator and by every test, which rebuild the inputs and check them against the checksums)
# --------------------------------------------------------------------------------------------------------------------------


def rounded_to_f32(coh):
    r32 = lambda a: np.asarray(a).astype(np.float32).astype(np.float64)  # noqa: E731
    return O.Cohort(coh.n_gaps, coh.n_inds, coh.vacs, coh.pcrpos,
                    O.AntigenObs(coh.s.idx_gap, coh.s.idx_ind, r32(coh.s.log_dilution), r32(coh.s.od)),
                    O.AntigenObs(coh.n.idx_gap, coh.n.idx_ind, r32(coh.n.log_dilution), r32(coh.n.od)))


def synth_cohort(N, G, kind="full"):
    """the cohorts of tests/test_gpu_exposure_planes.py: 'bare' has no vaccinations and no PCR positives; 'distinct' gives every
    reading another log dilution (no split panels, one-chain launches read the pair panels)"""
    from tests.test_gpu_exposure_planes import _cohort

    return _cohort(N, G, kind)


def cohort(shape):
    """shape: ('dense', N, G, kind) or ('sparse',) -> the oracle's Cohort"""
    if shape[0] == "sparse":
        return random_sparse_cohort(23, 31, 300, 250)
    _, N, G, kind = shape
    return oracle_cohort_from_synth(synth_cohort(N, G, kind))


def checksum(coh):
    """sums of vacs, pcrpos, x_*, y_* (S then N): tells a rebuilt cohort from the one the references were made on"""
    return np.array([float(np.sum(coh.vacs)), float(np.sum(coh.pcrpos)), math.fsum(coh.s.log_dilution), math.fsum(coh.s.od),
                     math.fsum(coh.n.log_dilution), math.fsum(coh.n.od)])


def state(N, G, which):
    i_raw, w = synthetic.make_chain_state(N, G, 3)
    if which == "ones":
        i_raw = np.ones_like(i_raw)
    if which == "zeros":
        i_raw = np.zeros_like(i_raw)
    return i_raw, w


def _th(G, **kw):
    t = synthetic.make_thetas(G, 1, 0)[0].copy()  # not theta_init: its prior gradients are exactly zero
    for k, v in kw.items():
        t[int(k[1:])] = v
    return t


def case_table(G):
    """[(name, theta, state, cohort kind)]: the full table"""
    T = [
        ("base", _th(G), "random", "full"),
        ("truth", synthetic.truth_theta(G), "random", "full"),
        ("b=-8", _th(G, k11=-8.0, k14=-8.0), "random", "full"),
        ("b=+3", _th(G, k11=3.0, k14=3.0), "random", "full"),
        ("b=-40 perm=e^3", _th(G, k11=-40.0, k14=-40.0, k1=3.0, k5=3.0), "random", "full"),
        ("b=+40 perm=e^3", _th(G, k11=40.0, k14=40.0, k1=3.0, k5=3.0), "random", "full"),
        ("b=+40 perm=e^2.5", _th(G, k11=40.0, k14=40.0, k1=2.5, k5=2.5), "random", "full"),  # max t between the two clamps, 510 and 1021
        ("b=+300", _th(G, k11=300.0, k14=300.0), "random", "full"),
        ("b=0", _th(G, k11=0.0, k14=0.0), "random", "full"),
        ("b=-0.0", _th(G, k11=-0.0, k14=-0.0), "random", "full"),
        ("b=+-1e-9", _th(G, k11=1e-9, k14=-1e-9), "random", "full"),
        ("b=1e-300", _th(G, k11=1e-300, k14=1e-300), "random", "full"),
        ("rho +40/+40", _th(G, k3=40.0, k6=40.0), "random", "full"),
        ("rho -40/-40", _th(G, k3=-40.0, k6=-40.0), "random", "full"),
        ("rho -800/-800", _th(G, k3=-800.0, k6=-800.0), "random", "full"),
        ("rho +40/-40", _th(G, k3=40.0, k6=-40.0), "random", "full"),
        ("sigma=e^-12", _th(G, k13=-12.0, k16=-12.0), "random", "full"),
        ("sigma=e^+12", _th(G, k13=12.0, k16=12.0), "random", "full"),
        ("perm,temp=e^-30", _th(G, k1=-30.0, k2=-30.0, k5=-30.0), "random", "full"),
        ("perm,temp=e^+5", _th(G, k1=5.0, k2=5.0, k5=5.0), "random", "full"),
        ("p +30/-30", _th(G, k0=30.0, k7=-30.0), "random", "full"),
        ("p -30/+30", _th(G, k0=-30.0, k7=30.0), "random", "full"),
        ("d=0", _th(G, k12=0.0, k15=0.0), "random", "full"),
        ("d=-1.5", _th(G, k12=-1.5, k15=-1.5), "random", "full"),
        ("init +20/-20", _th(G, k4=20.0, k10=-20.0), "random", "full"),
        ("ones b=-8", _th(G, k11=-8.0, k14=-8.0), "ones", "full"),
        ("zeros, nobody exposed", _th(G), "zeros", "bare"),
    ]
    return T


# the short table: t below -1022, between 510 and 1021, above 1021; rho = 0 to the last bit; t below -510 through the titers
FIVE = ("b=-40 perm=e^3", "b=+40 perm=e^2.5", "b=+40 perm=e^3", "rho -800/-800", "perm,temp=e^+5")

# name -> (shape, kind of table, f32 too); 'bare' cohorts are derived per case
SETS = {
    "65x33": (("dense", 65, 33, "full"), "full", True),
    "7x65": (("dense", 7, 65, "full"), "five+pointwise", False),
    "65x33 distinct": (("dense", 65, 33, "distinct"), "five", False),
    "20x13": (("dense", 20, 13, "full"), "five+pointwise", False),
    "sparse": (("sparse",), "five+pointwise", False),
}


def set_cases(name):
    """[(case name, theta, i_raw, waner, cohort)] of one set, inputs rebuilt from the seeds"""
    shape, table, _ = SETS[name]
    base = cohort(shape)
    G, N = base.n_gaps, base.n_inds
    rows = case_table(G)
    if table != "full":
        rows = [r for r in rows if r[0] in FIVE]
    out = []
    for cname, theta, st, kind in rows:
        coh = base
        if kind == "bare":
            coh = O.Cohort(G, N, np.zeros_like(base.vacs), np.zeros_like(base.pcrpos), base.s, base.n)
        i_raw, w = state(N, G, st)
        out.append((cname, theta, i_raw, w, coh))
    return out


def load_fixture(golden_dir):
    import os

    return dict(np.load(os.path.join(golden_dir, FIXTURE)))
