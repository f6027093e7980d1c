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

The binary Gibbs-Metropolis sweep is restated here too (``sweep``: Philox in Python, the order and rule of ``abd_gibbs.hpp``, per-gap
likelihood terms at 40 digits): ``tests/golden/make_sweep_fixtures.py`` runs it over the same table and commits per proposal what a
kernel decides with (``tests/golden/sweep_decisions.npz``, read through ``SweepSet``).
"""
import functools
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
# The binary Gibbs-Metropolis sweep (abdpymc_amd/csrc/abd_gibbs.hpp) at 40 digits: same random stream, same order, and per
# proposal what a kernel decides with
# --------------------------------------------------------------------------------------------------------------------------

GIBBS_TRANSIT_U32 = 3435973836  # floor(0.8 * 2^32): a dim is proposed iff word 1 of its draw is below
LOG_U_TOL = 8e-15  # |log u| <= 32 log 2 + log 2 = 22.9: 2 ulp there (3.55e-15 each), rounded up


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    m = 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & m, p1 & m, ((p0 >> 32) ^ c3 ^ k1) & m, p0 & m
        k0, k1 = (k0 + 0x9E3779B9) & m, (k1 + 0xBB67AE85) & m
    return c0, c1, c2, c3


def gibbs_order(G, j, chain, seed, sweep):
    """[(dim, acceptance word)] of individual j's PROPOSED dims in the sweep's order (dim G: ab_s_waner)"""
    k0 = (seed & 0xFFFFFFFF) ^ ((sweep * 0x9E3779B9) & 0xFFFFFFFF)
    k1 = (seed >> 32) & 0xFFFFFFFF
    r = [philox4x32_10(d, j, chain, 0, k0, k1) for d in range(G + 1)]
    return [(d, r[d][2]) for d in sorted(range(G + 1), key=lambda d: (r[d][0] & ~0x1FF) | d) if r[d][1] < GIBBS_TRANSIT_U32]


class _SweepTerms:
    """Per gap of one individual: both antigens' likelihood terms -1/2 (q / sigma)^2 that depend on the discrete state"""

    def __init__(self, mp, theta, obs_n, obs_s, vac, G):
        t = _theta_mp(mp, theta)
        sig = lambda z: 1 / (1 + mp.exp(-z))  # noqa: E731
        self.mp, self.G, self.vac = mp, G, [int(v) for v in vac]
        self.perm_n, self.temp_n, self.rho_n, self.init_n = mp.exp(t[1]), mp.exp(t[2]), sig(t[3]), t[4]
        self.perm_s, self.rho_s, self.init_s = mp.exp(t[5]), sig(t[6]), t[10]
        self.n = (t[11], t[12], 2 * mp.exp(2 * t[13]), obs_n)
        self.s = (t[14], t[15], 2 * mp.exp(2 * t[16]), obs_s)

    def _gap(self, par, g, a):
        b, d, two_s2, obs = par
        acc = self.mp.mpf(0)
        for x, y in obs.get(g, ()):
            q = y - d / (1 + self.mp.exp(b * (a - x)))
            acc -= q * q / two_s2
        return acc

    def run(self, inf, waner, g0=0, carry=None):
        """terms and scan states of gaps g0 .. G-1; carry: the state (tn, ts, ci, civ) after gap g0 - 1"""
        F = self.mp.mpf
        tn, ts, ci, civ = carry if carry is not None else (F(0), F(0), 0, 0)
        rj = self.rho_s if waner else F(1)
        terms, states = [], []
        for g in range(g0, self.G):
            e_i, e_v = int(inf[g]), self.vac[g]
            tn = tn * self.rho_n + e_i
            ts = ts * rj + e_i + e_v
            ci += e_i
            civ += e_i + e_v
            a_n = (self.perm_n if ci else 0) + self.temp_n * tn + self.init_n
            a_s = (self.perm_s if civ else 0) + ts + self.init_s
            terms.append(self._gap(self.n, g, a_n) + self._gap(self.s, g, a_s))
            states.append((tn, ts, ci, civ))
        return terms, states


def sweep(theta, i_raw, waner, cohort, splits=None, ignore_pcrpos=False, chain=0, seed=0, sweep=0, per_gap=False, individuals=None):
    """One sweep of chain slot `chain` -> (i_raw, waner, accepted, proposed, records).  records: one dict per proposal, individual by
    individual in the sweep's order, floats rounded to float64:
      ind, dim, accepted;
      gf         the first gap whose constrained infection differs (0 for the ab_s_waner flip, -1 if none does);
      delta      the log-ratio; log_u: the log of the acceptance uniform (w + 1/2) / 2^32; the rule is delta > log_u (log_u < 0);
      S_changed  |prior| + sum over g >= gf of |current term| + |new term|: the addends the dense kernel forms delta from;
      S_full     the same over all gaps (= |prior| if nothing changes): the list kernel's and the C restatement's addends;
      cur_tail   the sum of the current terms of gaps >= gf;
      new, crossed (per_gap): the new terms of gaps gf, gf + 1, ... up to two gaps past the first one -- index `crossed` of `new`,
                 -1 if there is none -- at which the bound prior - cur_tail + (new terms so far) lies below log_u
    individuals: only these (default all); the others keep their state."""
    mp = _mp()
    F = mp.mpf
    i_raw, waner = np.array(i_raw, dtype=np.int8), np.array(waner, dtype=np.int8)
    G, N = cohort.n_gaps, cohort.n_inds
    pcr = np.zeros((G, N)) if ignore_pcrpos else np.asarray(cohort.pcrpos, dtype=float).T
    vacs = np.asarray(cohort.vacs)
    by_ind = []
    for obs in (cohort.n, cohort.s):
        d = {}
        for g, i, x, y in zip(np.asarray(obs.idx_gap), np.asarray(obs.idx_ind), np.asarray(obs.log_dilution, float), np.asarray(obs.od, float)):
            d.setdefault(int(i), {}).setdefault(int(g), []).append((F(float(x)), F(float(y))))
        by_ind.append(d)
    th0, th7 = F(float(theta[0])), F(float(theta[7]))
    records, accepted, proposed = [], 0, 0
    for j in range(N) if individuals is None else individuals:
        T = _SweepTerms(mp, theta, by_ind[0].get(j, {}), by_ind[1].get(j, {}), vacs[j], G)
        con = lambda r: O.constrain_infections(r[:, None], pcr[:, j:j + 1], splits)[:, 0].astype(np.int64)  # noqa: E731
        raw, w = i_raw[:, j].copy(), int(waner[j])
        inf = con(raw)
        cur, states = T.run(inf, w)
        for d, word in gibbs_order(G, j, chain, seed, sweep):
            proposed += 1
            raw_n, w_n, inf_n, gf = raw, w, inf, -1
            if d < G:
                prior = -th0 if raw[d] else th0
                raw_n = raw.copy()
                raw_n[d] ^= 1
                inf_n = con(raw_n)
                if not np.array_equal(inf, inf_n):
                    gf = int(np.argmax(inf != inf_n))
            else:
                w_n, gf = 1 - w, 0
                prior = th7 if w_n else -th7
            delta, S_changed, S_full, cur_tail, new, new_states = prior, abs(prior), abs(prior), F(0), [], []
            if gf >= 0:
                new, new_states = T.run(inf_n, w_n, gf, states[gf - 1] if gf > 0 else None)
                cur_tail = sum(cur[gf:], F(0))
                delta = prior + (sum(new, F(0)) - cur_tail)
                S_changed += sum((abs(v) for v in cur[gf:]), F(0)) + sum((abs(v) for v in new), F(0))
                S_full = S_changed + 2 * sum((abs(v) for v in cur[:gf]), F(0))
            log_u = mp.log((F(word) + F(1) / 2) / F(2) ** 32)
            acc = bool(delta > log_u)
            rec = dict(ind=j, dim=d, gf=gf, accepted=acc, delta=float(delta), log_u=float(log_u), S_changed=float(S_changed),
                       S_full=float(S_full), cur_tail=float(cur_tail))
            if per_gap:
                bound, crossed = prior - cur_tail, -1
                for k, v in enumerate(new):
                    bound += v
                    if bound < log_u:
                        crossed = k
                        break
                rec["crossed"] = crossed
                rec["new"] = np.array([float(v) for v in (new if crossed < 0 else new[:crossed + 3])])
            records.append(rec)
            if acc:
                accepted += 1
                raw, w, inf = raw_n, w_n, inf_n
                if gf >= 0:
                    cur, states = cur[:gf] + new, states[:gf] + new_states
        i_raw[:, j], waner[j] = raw, w
    return i_raw, waner, accepted, proposed, records


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


def load_fixture(golden_dir, name=FIXTURE):
    import os

    return dict(np.load(os.path.join(golden_dir, name)))


# The sets of the sweep fixture (tests/golden/make_sweep_fixtures.py -> sweep_decisions.npz): sets of SETS by name -- 20x13 again with
# one split, two splits and without PCR+, two of the five cases each -- and one wide set for the sweep kernels' 8-word instantiations.
# per_gap: the per-gap new terms are stored (what an early stop's bound is made of); float_inds: the individuals whose proposals'
# numbers are stored (None: all; every individual's decisions, first changed gaps and end state are).  Case k of a set runs in chain slot k.
SWEEP_FIXTURE = "sweep_decisions.npz"
PER_GAP_CROSSED = 14  # per-gap terms are stored for the rows whose bound crosses log u within this many gaps of the first changed one
_SWEEP_DEFAULT = dict(splits=None, ignore_pcrpos=False, f32=False, per_gap=False, sweeps=2, seed=2024, float_inds=None, only=None)
_TWO = ("b=+40 perm=e^2.5", "rho -800/-800")
SWEEP_SETS = {
    "65x33": dict(_SWEEP_DEFAULT, of="65x33", f32=True, float_inds=(0, 1, 2, 64)),
    "7x65": dict(_SWEEP_DEFAULT, of="7x65", per_gap=True),
    "20x13": dict(_SWEEP_DEFAULT, of="20x13", per_gap=True),
    "20x13 one split": dict(_SWEEP_DEFAULT, of="20x13", splits=(5,), per_gap=True, only=_TWO),
    "20x13 two splits": dict(_SWEEP_DEFAULT, of="20x13", splits=(4, 9), per_gap=True, only=_TWO),
    "20x13 no pcrpos": dict(_SWEEP_DEFAULT, of="20x13", ignore_pcrpos=True, per_gap=True, only=_TWO),
    "sparse": dict(_SWEEP_DEFAULT, of="sparse"),
    "4x257": dict(_SWEEP_DEFAULT, of=None, per_gap=True, sweeps=1),
}


class SweepSet:
    """One set and storage of the sweep fixture: the rows of a case's sweep, individual by individual in the sweep's order"""

    def __init__(self, fx, name, st="f64"):
        self.name, self.st, self.spec, self.fx, self.k = name, st, SWEEP_SETS[name], fx, f"{name}.{st}."
        self.n = self.get("n")  # (cases, sweeps, N)
        self.G = self.get("i_raw").shape[2]
        self.first = np.concatenate([[0], np.cumsum(self.n.sum(axis=2).reshape(-1))])  # by case * sweeps + sweep
        # which rows carry numbers, and where: row r's numbers are at at[r] of d, S and crossed
        keep = np.ones(self.n.shape[2], dtype=bool)
        if self.spec["float_inds"] is not None:
            keep[:] = False
            keep[list(self.spec["float_inds"])] = True
        self.has = np.repeat(np.broadcast_to(keep, self.n.shape).reshape(-1), self.n.reshape(-1))
        self.at = np.cumsum(self.has) - 1
        assert int(self.has.sum()) == len(self.get("d")) == len(self.get("S")) and len(self.has) == len(self.get("gf"))
        if self.spec["per_gap"]:
            cr, gf = self.get("crossed").astype(np.int64), self.get("gf")[self.has].astype(np.int64)
            self.new_first = np.concatenate([[0], np.cumsum(np.where((cr >= 0) & (cr < PER_GAP_CROSSED), np.minimum(cr + 3, self.G - gf), 0))])
            assert self.new_first[-1] == len(self.get("new"))

    def get(self, key):
        k = self.k + key
        return self.fx[k] if k in self.fx else self.fx[k.replace(".f32.", ".f64.")]  # (an f32 array equal to its f64 twin is stored once)

    def rows(self, c, s0, s1=None):
        """the slice of the set's rows that is sweep s0 (sweeps s0 .. s1) of case c"""
        n_s = self.n.shape[1]
        return slice(int(self.first[c * n_s + s0]), int(self.first[c * n_s + (s0 if s1 is None else s1) + 1]))

    def dims(self, c, s):
        """the dims of those rows: the sweep's order of every individual"""
        return np.array([d for j in range(self.n.shape[2]) for d, _ in gibbs_order(self.G, j, c, self.spec["seed"], s)], dtype=np.int16)

    def numbers(self, rows):
        """(mask of the rows of the slice that carry numbers, d, S, crossed or None of those)"""
        has = self.has[rows]
        at = self.at[rows][has]
        cr = self.get("crossed")[at] if self.spec["per_gap"] else None
        return has, self.get("d")[at], self.get("S")[at].astype(np.float64), cr

    def new_terms(self, row):
        """the stored per-gap new terms of a row (absolute index) that carries numbers: gaps gf, gf + 1, ... (none unless it crosses
        within PER_GAP_CROSSED gaps)"""
        k = int(self.at[row])
        return self.get("new")[int(self.new_first[k]):int(self.new_first[k + 1])]


@functools.lru_cache(maxsize=None)
def sweep_cases(name):
    """[(case name, theta, i_raw, waner, cohort)] of one sweep set"""
    of, only = SWEEP_SETS[name]["of"], SWEEP_SETS[name]["only"]
    if of is not None:
        return [r for r in set_cases(of) if only is None or r[0] in only]
    coh, out = cohort(("dense", 4, 257, "full")), []  # the wide set: two rows of the table, and an all-ones state at the typical point
    for cname, theta, st, _ in case_table(257):
        if cname in ("b=+40 perm=e^3", "sigma=e^-12"):
            out.append((cname, theta) + state(4, 257, st) + (coh,))
    out.append(("ones", _th(257)) + state(4, 257, "ones") + (coh,))
    return out
