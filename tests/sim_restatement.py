"""
NumPy restatement of the cohort simulator (include/abd_hip.h: abd_simulate), written from its equations: the keyed Philox
streams (in the style of tests/test_predictive_cpu.py: stream_normals), the walk with keyed or injected uniforms, the OD
readings, and the smallest |u - threshold| over every comparison the walk made.  A helper, not a test file.

Parameters are the dict ``Antibodies.as_native()`` gives: {"s": {...}, "n": {...}} with the ten fields of abd_sim_antibody.
"""
import numpy as np

from tests.test_predictive_cpu import philox_np

C3_EXPOSURE, C3_PROTECTION, C3_NOISE = 0x40000000, 0x40000001, 0x40000010
FIELDS = ("protect_a", "protect_b", "elisa_b", "elisa_d", "elisa_sd", "init", "perm_rise", "temp_rise_i", "temp_rise_v", "temp_wane")
DEFAULT_AB = dict(protect_a=0.0, protect_b=1.0, elisa_b=-2.2, elisa_d=1.6, elisa_sd=0.1, init=-2.0, perm_rise=2.0,
                  temp_rise_i=1.5, temp_rise_v=2.0, temp_wane=0.95)  # simulation.py:43-44, 76-78, 104-108


def default_params():
    return {"s": dict(DEFAULT_AB), "n": dict(DEFAULT_AB)}


def _u(a, b):
    return (((a >> np.uint64(5)) << np.uint64(26) | (b >> np.uint64(6))).astype(np.float64) + 0.5) * 2.0 ** -53


def _key(seed):
    return seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF


def keyed_uniforms(seed, rho, n_inds, n_gaps, ind_offset=0):
    """u_e, u_s, u_n, each (n_inds, n_gaps): exposure counter (ind_offset + j, rho, t, 0x40000000), words 0, 1; protection
    counter (.., 0x40000001), u_s of words 0, 1 and u_n of words 2, 3."""
    j = ((np.arange(n_inds, dtype=np.uint64) + np.uint64(ind_offset)) & np.uint64(0xFFFFFFFF))[:, None]
    t = np.arange(n_gaps, dtype=np.uint64)[None, :]
    e = philox_np(j, rho, t, C3_EXPOSURE, *_key(seed))
    p = philox_np(j, rho, t, C3_PROTECTION, *_key(seed))
    return _u(e[0], e[1]), _u(p[0], p[1]), _u(p[2], p[3])


def reading_normals(seed, rho, antigen, n_readings):
    """z of caller readings 0 .. n_readings - 1 of one antigen (S 0, N 1): counter (r, rho, 0, 0x40000010 | antigen), the first
    Box-Muller value."""
    w = philox_np(np.arange(n_readings, dtype=np.uint64), rho, 0, C3_NOISE | antigen, *_key(seed))
    return np.sqrt(-2.0 * np.log(_u(w[0], w[1]))) * np.cos(2.0 * np.pi * _u(w[2], w[3]))


def walk(params, lam0, vacs, pcrpos, u_e, u_s, u_n):
    """The walk with the given uniforms, all (n_inds, n_gaps); pcrpos None: no forced infections.
    -> infections (int8), s_titer, n_titer, margin: the smallest |u - threshold| over every comparison made (u_e against lam0 and
    u_s, u_n against p_s, p_n, in every gap of every individual)."""
    s, n = params["s"], params["n"]
    vacs = np.asarray(vacs) == 1
    N, G = vacs.shape
    pcr = np.zeros((N, G), bool) if pcrpos is None else np.asarray(pcrpos) == 1
    lam0 = np.asarray(lam0, float)
    inf = np.zeros((N, G), np.int8)
    st, nt = np.empty((N, G)), np.empty((N, G))
    s_temp, n_temp = np.zeros(N), np.zeros(N)
    s_prev, n_prev = np.full(N, float(s["init"])), np.full(N, float(n["init"]))
    any_i, any_v = np.zeros(N, bool), np.zeros(N, bool)
    margin = np.inf
    for t in range(G):
        exposed = u_e[:, t] < lam0[t]
        p_s = 1.0 / (1.0 + np.exp(-s["protect_b"] * (s_prev - s["protect_a"])))
        p_n = 1.0 / (1.0 + np.exp(-n["protect_b"] * (n_prev - n["protect_a"])))
        protected = (u_s[:, t] < p_s) | (u_n[:, t] < p_n)
        margin = min(margin, np.abs(u_e[:, t] - lam0[t]).min(), np.abs(u_s[:, t] - p_s).min(), np.abs(u_n[:, t] - p_n).min())
        infected = pcr[:, t] | (exposed & ~protected)
        s_temp = s_temp * s["temp_wane"] + infected * s["temp_rise_i"] + vacs[:, t] * s["temp_rise_v"]
        n_temp = n_temp * n["temp_wane"] + infected * n["temp_rise_i"]
        any_i |= infected
        any_v |= vacs[:, t]
        s_prev = s["init"] + s_temp + np.where(any_i | any_v, s["perm_rise"], 0.0)
        n_prev = n["init"] + n_temp + np.where(any_i, n["perm_rise"], 0.0)
        inf[:, t], st[:, t], nt[:, t] = infected, s_prev, n_prev
    return inf, st, nt, float(margin)


def od(ab, log_dilution, titer, z):
    """abd.logistic plus Normal noise: d / (1 + exp(-b (log_dilution - titer))) + sd z"""
    return ab["elisa_d"] / (1.0 + np.exp(-ab["elisa_b"] * (np.asarray(log_dilution, float) - titer))) + ab["elisa_sd"] * z


def simulate(params, lam0, vacs, pcrpos, seed, rho, s_obs=None, n_obs=None, ind_offset=0):
    """One replicate from the keyed streams.  s_obs / n_obs: (idx_gap, idx_ind, log_dilution) of the readings in the caller's order.
    -> dict(infections, s_titer, n_titer, n_infected, margin[, od_s, od_n])"""
    N, G = np.asarray(vacs).shape
    inf, st, nt, margin = walk(params, lam0, vacs, pcrpos, *keyed_uniforms(seed, rho, N, G, ind_offset))
    out = dict(infections=inf, s_titer=st, n_titer=nt, n_infected=inf.sum(axis=0, dtype=np.int64), margin=margin)
    for ag, (name, obs, titer) in enumerate((("s", s_obs, st), ("n", n_obs, nt))):
        if obs is not None:
            g, j, x = (np.asarray(v) for v in obs)
            out["od_" + name] = od(params[name], x, titer[j, g], reading_normals(seed, rho, ag, g.size))
    return out


# Known answers of the reference's own tests (abdpymc/test_simulation.py:190-356), all at lam0 = 0 over five gaps:
# (name, overrides of S's and of N's fields, vacs, pcrpos, expected infections, [(antigen, gap, expected titer), ...])
KNOWN_ANSWERS = (
    ("no change with lam0 = 0", dict(init=0.123), dict(init=0.456), [0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0],
     [("s", g, 0.123) for g in range(5)] + [("n", g, 0.456) for g in range(5)]),
    ("a PCR+ is an infection; S and N at and after it", dict(temp_rise_i=0.3, perm_rise=0.34, temp_wane=0.94, init=-1.0),
     dict(temp_rise_i=0.89, perm_rise=2.34, temp_wane=0.87), [0, 0, 0, 0, 0], [0, 0, 1, 0, 0], [0, 0, 1, 0, 0],
     [("s", 0, -1.0), ("s", 1, -1.0), ("s", 2, -1 + 0.3 + 0.34), ("s", 3, -1 + 0.3 * 0.94 + 0.34),
      ("n", 0, -2.0), ("n", 1, -2.0), ("n", 2, -2 + 0.89 + 2.34), ("n", 3, -2 + 0.89 * 0.87 + 2.34)]),
    ("vaccination raises S only", dict(temp_rise_v=0.3, perm_rise=0.34, temp_wane=0.94, init=-1.0), dict(), [0, 0, 1, 0, 0],
     [0, 0, 0, 0, 0], [0, 0, 0, 0, 0],
     [("s", 0, -1.0), ("s", 1, -1.0), ("s", 2, -1 + 0.3 + 0.34), ("s", 3, -1 + 0.3 * 0.94 + 0.34)] + [("n", g, -2.0) for g in range(5)]),
    ("vaccination then infection", dict(temp_rise_i=0.21, temp_rise_v=0.3, perm_rise=0.34, temp_wane=0.94, init=-1.0),
     dict(temp_rise_v=0.0, temp_rise_i=0.89, perm_rise=2.34, temp_wane=0.87), [0, 0, 1, 0, 0], [0, 0, 0, 1, 0], [0, 0, 0, 1, 0],
     [("s", 1, -1.0), ("s", 2, -1 + 0.3 + 0.34), ("s", 3, -1 + 0.3 * 0.94 + 0.34 + 0.21),
      ("n", 0, -2.0), ("n", 1, -2.0), ("n", 2, -2.0), ("n", 3, -2 + 0.89 + 2.34)]),
)


def known_params(s_over, n_over):
    p = default_params()
    p["s"].update(s_over)
    p["n"].update(n_over)
    return p
