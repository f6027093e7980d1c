"""
PSIS-LOO of one column of a log-likelihood matrix, restated twice from the definition in DESIGN.md §27 (not from
``abdpymc_amd/compare.py``): ``psis_column`` in plain Python loops over fp64, ``psis_column_mp`` in ``mpmath`` at 40 digits.
Also the matrices the CPU and the GPU tests share, and their 40-digit values, computed once per process.

The definition, for the S values ll_s of one individual in draw order:
    x_s = (-ll_s) - max_s(-ll_s);   M = min(S // 5, ceil(3 sqrt(S)));   cut = max((M+1)-th largest x, log(DBL_MIN))
    tail = {s : x_s > cut}, n of them.  n <= 4: k = +inf, the weights are x.  Else, with the tail ascending (ties in draw order)
    and t_i = exp(x_(i)) - exp(cut):  m = 30 + floor(sqrt(n));  b_j = (1 - sqrt(m / (j - 0.5))) / (3 t_q) + 1 / t_max, j = 1..m,
    t_q = t[int(n / 4 + 0.5) - 1];  k_j = mean_i log1p(-b_j t_i);  L_j = n (log(-b_j / k_j) - k_j - 1);  w_j = 1 / sum_i exp(L_i - L_j);
    b = sum_j b_j w_j;  k_raw = mean_i log1p(-b t_i);  sigma = -k_raw / b;  k = (n k_raw + 5) / (n + 10);
    x_(i) <- min(log(sigma expm1(-k log1p(-p_i)) / k + exp(cut)), 0), p_i = (i + 0.5) / n  (k == 0: -sigma log1p(-p_i) for the quantile)
    lw = x - logsumexp(x);  elpd = logsumexp(ll + lw);  lppd = logsumexp(ll) - log S

In the 40-digit version the comparisons that decide the tail and its order are those of the fp64 x (they are exact operations on
fp64 numbers, and every implementation makes the same ones); every value -- x itself, the fit, the sums -- is carried at 40 digits.
"""
import functools
import math
import sys

import numpy as np

DBL_MIN = sys.float_info.min
S_VALUES = (24, 25, 64, 65, 257, 1000, 4000)  # 64 | 65: a wave; 257: more than one draw per thread; 1000: M = 95; 4000: M = 190
S_TIES = 404    # 101 rows, each four times: M = 61 and the 62nd largest is tied with the 61st
S_WIDE = 4097   # past 4096 draws


def tail_len(S):
    return min(S // 5, int(math.ceil(3.0 * math.sqrt(S))))


def _tail(x64):
    """From the fp64 x: (cut, the tail's draws ascending in x with ties in draw order)."""
    S = len(x64)
    M = tail_len(S)
    desc = sorted(x64, reverse=True)
    cut = max(desc[M], math.log(DBL_MIN))
    tail = [s for s in range(S) if x64[s] > cut]
    tail.sort(key=lambda s: (x64[s], s))
    return cut, tail


def _x64(ll):
    a = [-float(v) for v in ll]
    mx = max(a)
    return [v - mx for v in a]


def _lse(v):
    m = max(v)
    s = 0.0
    for u in v:
        s += math.exp(u - m)
    return m + math.log(s)


def psis_column(ll):
    """fp64, plain loops: (elpd, k, lppd, n_tail)."""
    ll = [float(v) for v in ll]
    S = len(ll)
    x = _x64(ll)
    cut, tail = _tail(x)
    n = len(tail)
    k = math.inf
    if n > 4:
        ecut = math.exp(cut)
        t = [math.exp(x[s]) - ecut for s in tail]
        m = 30 + int(math.floor(math.sqrt(n)))
        t_q, t_max = t[int(n / 4 + 0.5) - 1], t[-1]
        b, L = [], []
        for j in range(1, m + 1):
            bj = (1.0 - math.sqrt(m / (j - 0.5))) / (3.0 * t_q) + 1.0 / t_max
            acc = 0.0
            for ti in t:
                acc += math.log1p(-bj * ti)
            kj = acc / n
            b.append(bj)
            L.append(n * (math.log(-bj / kj) - kj - 1.0))
        bh = 0.0
        for j in range(m):
            acc = 0.0
            for i in range(m):
                acc += math.exp(L[i] - L[j])
            bh += b[j] * (1.0 / acc)
        acc = 0.0
        for ti in t:
            acc += math.log1p(-bh * ti)
        k_raw = acc / n
        sigma = -k_raw / bh
        k = (n * k_raw + 5.0) / (n + 10.0)
        for i, s in enumerate(tail):
            lp = math.log1p(-(i + 0.5) / n)
            q = -sigma * lp if k == 0.0 else sigma * math.expm1(-k * lp) / k
            x[s] = min(math.log(q + ecut), 0.0)
    lx = _lse(x)
    elpd = _lse([ll[s] + (x[s] - lx) for s in range(S)])
    return elpd, k, _lse(ll) - math.log(S), n


def psis_column_mp(ll):
    """40 digits: (elpd, k, lppd, n_tail) as floats (k = inf where the tail has at most 4 draws)."""
    import mpmath as mp

    with mp.workdps(40):
        ll = [float(v) for v in ll]
        S = len(ll)
        cut64, tail = _tail(_x64(ll))
        a = [-mp.mpf(v) for v in ll]
        mx = max(a)
        x = [v - mx for v in a]
        n = len(tail)
        k = mp.inf

        def lse(v):
            m_ = max(v)
            return m_ + mp.log(mp.fsum(mp.exp(u - m_) for u in v))

        if n > 4:
            ecut = mp.exp(mp.mpf(cut64))
            t = [mp.exp(x[s]) - ecut for s in tail]
            m = 30 + int(math.floor(math.sqrt(n)))
            t_q, t_max = t[int(n / 4 + 0.5) - 1], t[-1]
            b, L = [], []
            for j in range(1, m + 1):
                bj = (1 - mp.sqrt(mp.mpf(m) / (mp.mpf(j) - mp.mpf("0.5")))) / (3 * t_q) + 1 / t_max
                kj = mp.fsum(mp.log1p(-bj * ti) for ti in t) / n
                b.append(bj)
                L.append(n * (mp.log(-bj / kj) - kj - 1))
            bh = mp.fsum(b[j] / mp.fsum(mp.exp(L[i] - L[j]) for i in range(m)) for j in range(m))
            k_raw = mp.fsum(mp.log1p(-bh * ti) for ti in t) / n
            sigma = -k_raw / bh
            k = (n * k_raw + 5) / (n + 10)
            for i, s in enumerate(tail):
                lp = mp.log1p(-(mp.mpf(i) + mp.mpf("0.5")) / n)
                q = -sigma * lp if k == 0 else sigma * mp.expm1(-k * lp) / k
                x[s] = min(mp.log(q + ecut), mp.mpf(0))
        lx = lse(x)
        elpd = lse([mp.mpf(ll[s]) + (x[s] - lx) for s in range(S)])
        lppd = lse([mp.mpf(v) for v in ll]) - mp.log(S)
        return float(elpd), float(k), float(lppd), n


def matrix_of(fn, ll, unfollowed=()):
    """``fn`` over the columns of ll (S, N): (elpd, k, lppd, n_tail) arrays; the columns ``unfollowed`` by the rule of §27."""
    N = ll.shape[1]
    elpd, k, lppd, n_tail = np.zeros(N), np.full(N, np.nan), np.zeros(N), np.zeros(N, dtype=np.int64)
    for j in range(N):
        if j not in unfollowed:
            elpd[j], k[j], lppd[j], n_tail[j] = fn(ll[:, j])
    return elpd, k, lppd, n_tail


# ---- the matrices the tests share ----

COLUMNS = ("normal", "exp_0.5", "exp_1.0", "wide_normal", "underflow", "unfollowed")
UNFOLLOWED = (5,)


def matrix(S, seed=0):
    """(S, 6): four random shapes of tail, a column whose spread passes 750 so that the cut is clipped at log(DBL_MIN) (fewer than M
    draws lie near the largest x, all others 800 below), and an unfollowed individual (exactly 0)."""
    rng = np.random.default_rng([27, S, seed])
    out = np.zeros((S, len(COLUMNS)))
    out[:, 0] = rng.normal(-3.0, 0.5, S)
    out[:, 1] = -0.5 * rng.exponential(1.0, S)
    out[:, 2] = -1.0 * rng.exponential(1.0, S)
    out[:, 3] = rng.normal(-40.0, 3.0, S)
    out[:, 4] = -np.abs(rng.normal(0.0, 1.0, S))
    far = rng.choice(S, size=max(1, tail_len(S) // 2), replace=False)
    out[far, 4] = -(800.0 + 10.0 * rng.random(far.size))
    return out


def matrix_ties():
    """(404, 6): 101 rows, every one four times (interleaved): ties sit on the cut-off and n_tail < M."""
    return np.tile(matrix(S_TIES // 4, seed=1), (4, 1))


def known_k(k0, S=4000, N=64, seed=3):
    """(S, N): ll = -k0 Exp(1), whose importance ratios exp(-ll) have a generalised Pareto tail of shape k0."""
    rng = np.random.default_rng([27, seed, int(round(100 * k0))])
    return -k0 * rng.exponential(1.0, (S, N))


@functools.lru_cache(maxsize=None)
def case(name):
    """name: an S of S_VALUES, S_WIDE, or "ties" -> (ll, the 40-digit (elpd, k, lppd, n_tail)).  Shared; do not write to it."""
    ll = matrix_ties() if name == "ties" else matrix(int(name))
    ll.setflags(write=False)
    return ll, matrix_of(psis_column_mp, ll, UNFOLLOWED)


CASES = tuple(S_VALUES) + ("ties", S_WIDE)


# ---- past a tail of 256 and up to the cap of 16 384 draws (tests/test_psis_wide_cpu.py, tests/test_gpu_psis_wide.py) ----
# Their 40-digit values are not computed when the tests run (about 20 s): tests/golden/psis_wide_reference.npz holds them.

COLUMNS_WIDE = ("positive", "huge", "constant", "few_high", "uniform", "heavy", "unfollowed")
UNFOLLOWED_WIDE = (6,)
# M = 8 | 48 | 64 | 96 | 97 | 128 | 192 | 256 | 257 | 384: a full sort array at 8, 64, 128 and 256; the last S of one, four and
# sixteen draws per thread (256, 1024, 4096) and the first of sixteen (1025); the last tail of the 256-slot sort (7281) and the
# first of the 512-slot one (7282); the cap
S_WIDE_VALUES = (40, 256, 442, 1024, 1025, 1793, 4096, 7281, 7282, 16384)
S_PLAIN_WIDE = (7282, 16384)  # ``matrix`` where the tail passes 256: its clipped column then has a tail of 128 and 192
S_TIES_WIDE = 7512            # 1878 rows, each four times: M = 261 and the 262nd largest is tied with the 261st


def n_few_high(S):
    """the draws of the column ``few_high`` that stand out: fewer than M, so that they alone are the tail"""
    return max(5, tail_len(S) // 3)


def matrix_wide(S, seed=0):
    """(S, 7): the kinds of column ``matrix`` has none of -- positive values (sums of densities), |ll| near 2e4, a constant, a
    tail whose members are all equal, bounded ratios (k < 0), a heavy tail (k > 1) -- and an unfollowed individual (exactly 0)."""
    rng = np.random.default_rng([28, S, seed])
    out = np.zeros((S, len(COLUMNS_WIDE)))
    out[:, 0] = rng.normal(35.0, 0.5, S)
    out[:, 1] = rng.normal(-2.0e4, 3.0, S)
    out[:, 2] = -1.25
    out[:, 3] = -0.5
    out[rng.choice(S, size=n_few_high(S), replace=False), 3] = -1.5
    out[:, 4] = rng.uniform(-1.0, 0.0, S)
    out[:, 5] = -1.5 * rng.exponential(1.0, S)
    return out


def matrix_ties_wide():
    """(7512, 6): 1878 rows of ``matrix``, every one four times: the ties on the cut-off leave n_tail = 260, below M = 261 and
    above 256."""
    return np.tile(matrix(S_TIES_WIDE // 4, seed=1), (4, 1))


WIDE_CASES = tuple(f"wide_{S}" for S in S_WIDE_VALUES) + tuple(f"plain_{S}" for S in S_PLAIN_WIDE) + ("ties_wide",)


@functools.lru_cache(maxsize=None)
def wide_case(name):
    """name of WIDE_CASES -> (ll, the unfollowed columns).  Shared; do not write to it."""
    if name == "ties_wide":
        ll, out = matrix_ties_wide(), UNFOLLOWED
    elif name.startswith("plain_"):
        ll, out = matrix(int(name[6:])), UNFOLLOWED
    else:
        ll, out = matrix_wide(int(name[5:])), UNFOLLOWED_WIDE
    ll.setflags(write=False)
    return ll, out


def rel_gap(got, want):
    """max |got - want| / max(1, |want|) over the finite entries; the non-finite ones must agree exactly (asserted)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isposinf(got), np.isposinf(want)), (got, want)
    assert np.array_equal(np.isfinite(got), fin), (got, want)
    if not fin.any():
        return 0.0
    return float((np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin]))).max())


if __name__ == "__main__":  # the restatement's own gap g to the 40-digit values (tests/golden/NOTICE_survival_loo.md)
    worst = {}
    for name in CASES:
        ll, ref = case(name)
        got = matrix_of(psis_column, ll, UNFOLLOWED)
        gaps = [rel_gap(got[i], ref[i]) for i in range(3)]
        assert np.array_equal(got[3], ref[3])
        print(name, "elpd %.3g  k %.3g  lppd %.3g" % tuple(gaps), "n_tail", ref[3].tolist(), "k", np.round(ref[1], 3).tolist())
        for key, g in zip(("elpd", "k", "lppd"), gaps):
            worst[key] = max(worst.get(key, 0.0), g)
    print("worst", worst)
