"""
Model comparison of per-draw survival fits on the device (abd_survival_draws_individual_loglik, _waic_*, _loo_*;
abd_survival_pointwise.hpp; abdpymc_amd.survival.waic_draws / loo_draws / compare_draws).

Every device check is bit equality against the plug-in handle of the form made of ``SurvivalDraws.arrays(m)``: the rows of
``draws_individual_loglik``, the WAIC statistics per dataset under any batching and interleaving, PSIS-LOO per dataset with its own
number of draws.  The plug-in kernels are the ones tests/test_gpu_survival_pointwise.py and tests/test_gpu_survival_loo.py tie to
the 40-digit fixtures.  The two tolerances that appear (``waic_draws`` / ``loo_draws`` on the device against the ``pointwise=`` host
path) are those tests' own gates for the same comparison, see ``test_waic_draws_and_loo_draws_against_the_host_path``.
"""
import os

import numpy as np
import pytest

from abdpymc_amd import _native, survival
from abdpymc_amd.data import TiterData
from tests import survival_groups_restatement as RG
from tests import survival_loo_restatement as RL
from tests import survival_periods_restatement as RPD
from tests import survival_restatement as R
from tests.survival_draws_cases import datasets
from tests.test_survival_loo_cpu import bound

pytestmark = pytest.mark.gpu

NS, TS, MS = (1, 63, 64, 65, 130), (1, 2, 7, 30), (1, 3, 17)  # the tile and batch edges


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _dataset_vector(n, M):
    return ((np.arange(n) * 5 + 2) % M).astype(np.int32)  # not monotone; M = 17: the first 16 rows on 16 different datasets


def _labels_of_groups(N):
    """(group (N,), Gr): a group of one (where N > 1), sizes that are no multiple of 64, the labels interleaved"""
    if N == 1:
        return np.zeros(1, np.int32), 1
    g = (1 + np.arange(N) % 2).astype(np.int32)
    g[N // 2] = 0
    return g, 3


class _Case:
    """One form at one shape: the datasets, the points (far from the origin included: large |b|, saturated eta, lambda at 0 and
    at 1), the ensemble handle and the plug-in handle of a dataset."""

    def __init__(self, form, N, T, M, labels=None):
        self.form, self.N, self.T, self.M = form, N, T, M
        d = datasets(M, N, T)
        if form == "groups":
            self.group, self.n_labels = _labels_of_groups(N)
            if N > 1:  # a group in which no individual is ever at risk in dataset 0 (its tiles skip their whole range)
                n_risk, event = d.n_risk.copy(), d.event.copy()
                n_risk[0, self.group == 2] = 0
                event[0, self.group == 2] = -1
                d = survival.SurvivalDraws(n_risk, event, d.s_titer, d.n_titer, d.source)
        elif form == "periods":
            self.n_labels = labels
            self.period = RPD.make_periods(N, T, labels).astype(np.int32)
        self.d = d
        if form in ("groups", "periods"):
            self.points = np.stack([RG.make_point(name, T, self.n_labels, seed=s) for s in (0, 1) for name in RG.POINTS])  # 18
        else:
            K = 1 if form == "k1" else 2
            self.K = K
            self.points = np.stack([R.make_point(name, T, K, seed=s) for s in (0, 1, 2) for name in R.POINTS][:18])

    def ensemble(self):
        d = self.d
        if self.form == "groups":
            return _native.SurvivalDrawsGroups(d.n_risk, d.event, d.s_titer, self.group, self.n_labels, RG.PRIORS)
        if self.form == "periods":
            return _native.SurvivalDrawsPeriods(d.n_risk, d.event, d.s_titer, self.period, self.n_labels, RPD.PRIORS)
        return _native.SurvivalDraws(d.n_risk, d.event, [d.s_titer, d.n_titer][:self.K], R.PRIORS[self.K])

    def plug_in(self, m):
        y, e, xs, xn = self.d.arrays(m)
        if self.form == "groups":
            return _native.SurvivalGroups(y, e, xs, self.group, self.n_labels, RG.PRIORS)
        if self.form == "periods":
            return _native.SurvivalPeriods(y, e, xs, self.period, self.n_labels, RPD.PRIORS)
        return _native.Survival(y, e, [xs, xn][:self.K], R.PRIORS[self.K])

    def draws(self, n, seed=7):
        """n draws that really differ: jittered typical points"""
        rng = np.random.default_rng([seed, self.N, self.T])
        return self.points[0] + 0.1 * rng.normal(size=(n, self.points.shape[1]))


def _cases_of(form, N):
    """every T with every M at this N; by period every T with P = 1, 3 and T"""
    for T in TS:
        for M in MS:
            if form == "periods":
                for P in sorted({1, min(3, T), T}):
                    yield _Case(form, N, T, M, P)
            else:
                yield _Case(form, N, T, M)


# ---- 1. kernel rows ----


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("form", ["k1", "k2", "groups", "periods"])
def test_rows_are_bit_equal_to_the_plug_in_kernel_on_every_dataset(form, N):
    """18 points (launches of 16 + 2), each on its own dataset: every row equals BITWISE what abd_survival_individual_loglik returns
    on the plug-in handle of that dataset, in the caller's order of individuals; with M = 17 the first launch mixes 16 different
    datasets and equals 16 single-point launches."""
    for case in _cases_of(form, N):
        pts, M = case.points, case.M
        ds = _dataset_vector(len(pts), M)
        h = case.ensemble()
        try:
            ll = h.draws_individual_loglik(ds, pts)
            assert ll.shape == (len(pts), N) and np.isfinite(ll).all()
            never = case.d.n_risk[ds] == 0  # (n, N): never at risk in the row's dataset: an exact 0
            assert (ll[never] == 0).all()
            for m in range(M):
                p = case.plug_in(m)
                try:
                    rows = np.flatnonzero(ds == m)
                    np.testing.assert_array_equal(_bits(ll[rows]), _bits(p.individual_loglik(pts[rows])), err_msg=f"{form} N{N} T{case.T} M{M} m{m}")
                finally:
                    p.close()
            if M == 17:
                assert len(set(ds[:16].tolist())) == 16
                for r in range(16):
                    np.testing.assert_array_equal(_bits(h.draws_individual_loglik(int(ds[r]), pts[r])[0]), _bits(ll[r]))
            if M > 1 and N > 4 and case.T > 1:  # the datasets differ: the index is read
                assert (h.draws_individual_loglik((ds + 1) % M, pts) != ll).any()
        finally:
            h.close()


# ---- 2. WAIC statistics ----

FORMS_AT = [("k1", 65, 30, 17, None), ("k2", 130, 7, 3, None), ("groups", 130, 7, 3, None), ("periods", 130, 30, 3, 3)]


@pytest.mark.parametrize("form,N,T,M,labels", FORMS_AT, ids=[f[0] for f in FORMS_AT])
def test_waic_statistics_per_dataset_are_the_plug_in_handles(form, N, T, M, labels):
    """72 draws with the datasets' rows interleaved, folded in calls of 1, 5, 16, 17 and 33 rows: per dataset lse, mean, m2, n_draws
    and n_cells equal BITWISE the plug-in handle's waic_accumulate of that dataset's rows in that order; the same bits from one call
    of 72, and with the rows sorted by dataset (each dataset's own order kept)."""
    case = _Case(form, N, T, M, labels)
    q = case.draws(72)
    ds = _dataset_vector(72, M)
    h = case.ensemble()
    try:
        with pytest.raises(ValueError, match="no draws accumulated"):
            h.draws_waic_stats()
        at = 0
        for n in (1, 5, 16, 17, 33):
            h.draws_waic_accumulate(ds[at:at + n], q[at:at + n])
            at += n
        assert at == 72
        got = h.draws_waic_stats()
        np.testing.assert_array_equal(got[3], np.bincount(ds, minlength=M))
        np.testing.assert_array_equal(got[4], case.d.n_risk)
        for m in range(M):
            p = case.plug_in(m)
            try:
                p.waic_accumulate(q[ds == m])
                (lse, mean, m2, n), cells = p.waic_stats()
            finally:
                p.close()
            assert n == got[3][m]
            np.testing.assert_array_equal(cells, got[4][m])
            for a, b, what in zip((lse, mean, m2), (got[0][m], got[1][m], got[2][m]), ("lse", "mean", "m2")):
                np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=f"{what} of dataset {m}")
        order = np.argsort(ds, kind="stable")
        for dss, qq in ((ds, q), (ds[order], q[order])):
            h.draws_waic_reset()
            with pytest.raises(ValueError, match="no draws accumulated"):
                h.draws_waic_stats()
            h.draws_waic_accumulate(dss, qq)
            for a, b in zip(h.draws_waic_stats(), got):
                np.testing.assert_array_equal(_bits(a) if a.dtype == np.float64 else a, _bits(b) if b.dtype == np.float64 else b)
        h.draws_waic_reset()  # a dataset nothing was folded into: NaN and 0 draws, the others untouched by it
        if M > 1:
            h.draws_waic_accumulate(ds[ds != 0], q[ds != 0])
            part = h.draws_waic_stats()
            assert part[3][0] == 0 and np.isnan(part[0][0]).all() and np.isnan(part[2][0]).all()
            np.testing.assert_array_equal(_bits(part[0][1:]), _bits(got[0][1:]))
            np.testing.assert_array_equal(_bits(part[2][1:]), _bits(got[2][1:]))
    finally:
        h.close()


# ---- 3. PSIS-LOO ----


@pytest.mark.parametrize("form,N,T,M,labels", FORMS_AT[1:], ids=[f[0] for f in FORMS_AT[1:]])
def test_loo_per_dataset_is_the_plug_in_handles(form, N, T, M, labels):
    """A different S per dataset in one handle -- 16, the smallest S tests/test_gpu_survival_loo.py smooths; 19, no multiple of 16;
    70 -- with the rows interleaved: elpd_loo, pareto_k, lppd and n_tail per dataset equal BITWISE the plug-in handle's loo_stats on
    the same draws; reset and re-accumulate in another order of the datasets gives the same bits."""
    case = _Case(form, N, T, M, labels)
    S = np.array([16, 19, 70])
    ds = np.random.default_rng(3).permutation(np.repeat(np.arange(3), S)).astype(np.int32)
    q = case.draws(len(ds))
    h = case.ensemble()
    try:
        h.draws_loo_reserve(70)
        with pytest.raises(ValueError, match="no draws held"):
            h.draws_loo_stats()
        at = 0
        for n in (1, 16, 19, 34, 35):
            h.draws_loo_accumulate(ds[at:at + n], q[at:at + n])
            at += n
        assert at == len(ds)
        got = h.draws_loo_stats()
        np.testing.assert_array_equal(got[4], S)
        for m in range(3):
            p = case.plug_in(m)
            try:
                p.loo_reserve(int(S[m]))
                p.loo_accumulate(q[ds == m])
                elpd, k, lppd, n_tail, n, cells = p.loo_stats()
            finally:
                p.close()
            assert n == S[m]
            np.testing.assert_array_equal(cells, case.d.n_risk[m])
            np.testing.assert_array_equal(n_tail, got[3][m])
            for a, b, what in zip((elpd, k, lppd), (got[0][m], got[1][m], got[2][m]), ("elpd", "k", "lppd")):
                np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=f"{what} of dataset {m}")
            followed = cells > 0
            assert np.isnan(k[~followed]).all() and (elpd[~followed] == 0).all() and (n_tail[followed] > 0).all()
        for a, b in zip(h.draws_loo_stats(), got):  # _stats consumes nothing
            np.testing.assert_array_equal(_bits(a) if a.dtype == np.float64 else a, _bits(b) if b.dtype == np.float64 else b)
        h.draws_loo_reset()
        order = np.argsort(-ds, kind="stable")  # the datasets one after the other, the last first
        h.draws_loo_accumulate(ds[order], q[order])
        for a, b in zip(h.draws_loo_stats(), got):
            np.testing.assert_array_equal(_bits(a) if a.dtype == np.float64 else a, _bits(b) if b.dtype == np.float64 else b)
    finally:
        h.close()


# ---- 4. refusals ----


def test_refusals_by_code_and_text_and_the_handle_still_works():
    case = _Case("k2", 65, 7, 3)
    q = case.draws(24)
    ds = _dataset_vector(24, 3)
    lib = _native.load()
    h = case.ensemble()
    try:
        ll = h.draws_individual_loglik(ds, q)

        def refused(call, code, text):
            with pytest.raises(_native.AbdError if code == -3 else ValueError, match=text):
                call()
            np.testing.assert_array_equal(_bits(h.draws_individual_loglik(ds[:3], q[:3])), _bits(ll[:3]))  # the handle still works

        bad = ds.copy()
        for v in (-1, 3):
            bad[2] = v
            for call in (lambda: h.draws_individual_loglik(bad, q), lambda: h.draws_waic_accumulate(bad, q), lambda: h.draws_loo_accumulate(bad, q)):
                refused(call, -1, rf"point 2: dataset {v} outside \[0, 3\)")
        refused(lambda: h.draws_loo_accumulate(ds, q), -3, "no matrix reserved")
        refused(lambda: h.draws_loo_stats(), -3, "no matrix reserved")
        refused(lambda: h.draws_loo_reserve(_native.SurvivalDraws.LOO_MAX_DRAWS + 1), -1, r"capacity=16385 outside \[0, 16384\]")
        refused(lambda: h.draws_loo_reserve(-1), -1, "outside")
        h.draws_loo_reserve(8)
        refused(lambda: h.draws_loo_stats(), -1, "no draws held")
        h.draws_loo_accumulate(ds[:15], q[:15])  # five rows each
        before = h.draws_loo_stats()
        np.testing.assert_array_equal(before[4], [5, 5, 5])
        # 24 rows would be 8 each with nothing held, but five are: refused before anything is launched, nothing stored
        refused(lambda: h.draws_loo_accumulate(ds, q), -3, "dataset 0: 5 draws held and 8 more would pass the capacity of 8")
        for a, b in zip(h.draws_loo_stats(), before):
            np.testing.assert_array_equal(_bits(a) if a.dtype == np.float64 else a, _bits(b) if b.dtype == np.float64 else b)
        h.draws_loo_accumulate(ds[15:24], q[15:24])  # to the brim
        np.testing.assert_array_equal(h.draws_loo_stats()[4], [8, 8, 8])
        h.draws_loo_reserve(0)
        refused(lambda: h.draws_loo_stats(), -3, "no matrix reserved")
        # the codes themselves, and NULL pointers on a live handle
        p = q.ctypes.data
        assert lib.abd_survival_draws_loo_accumulate(h._h, 1, ds.ctypes.data, p) == -3 and b"no matrix reserved" in lib.abd_last_error()
        assert lib.abd_survival_draws_loo_reserve(h._h, 16385) == -1 and b"outside" in lib.abd_last_error()
        assert lib.abd_survival_draws_individual_loglik(h._h, 1, bad.ctypes.data + 8, p, p) == -1 and b"outside" in lib.abd_last_error()
        for call in (lambda: lib.abd_survival_draws_individual_loglik(h._h, 1, None, p, p), lambda: lib.abd_survival_draws_individual_loglik(h._h, 1, ds.ctypes.data, p, None),
                     lambda: lib.abd_survival_draws_waic_accumulate(h._h, 1, ds.ctypes.data, None), lambda: lib.abd_survival_draws_loo_accumulate(h._h, 1, None, p),
                     lambda: lib.abd_survival_draws_waic_stats(h._h, p, p, p, None, p), lambda: lib.abd_survival_draws_loo_stats(h._h, p, p, p, p, None)):
            assert call() == -1 and b"NULL" in lib.abd_last_error()
        np.testing.assert_array_equal(_bits(h.draws_individual_loglik(ds, q)), _bits(ll))
    finally:
        h.close()


# ---- 5. Python: waic_draws / loo_draws on the device against the host path ----


def _fit_of(model, case, chains_per_dataset, draws):
    """a fit as sample_draws lays it out (dataset-major chains) of jittered typical points: no sampler needed"""
    M = case.M
    q = case.draws(M * chains_per_dataset * draws).reshape(M * chains_per_dataset, draws, -1)
    fit = {name: q[:, :, k].copy() for k, name in enumerate(model.names)}
    fit["dataset"] = np.repeat(np.arange(M), chains_per_dataset)
    fit["source"] = np.asarray(model.source)
    return fit


def test_waic_draws_and_loo_draws_against_the_host_path():
    """``waic_draws`` / ``loo_draws`` on the device against their ``pointwise=`` host path fed with the device's own rows
    (``individual_loglik``) -- the comparison tests/test_gpu_survival_pointwise.py (test_accumulators_fold_draws_in_order) and
    tests/test_gpu_survival_loo.py (test_loo_of_a_fit_of_the_golden_cohort) make for the plug-in models, with their gates:
      WAIC  the statistics against compare.stats_from_matrix of the same values: lse and mean within 1e-12 relative, m2 within 1e-9
            relative (waic_update's streaming mean and M2 against NumPy's two-pass ones).  In terms of what waic_draws returns:
            p_waic_j = m2 / n within 1e-9 relative, and elpd_j = lse - log n - p_waic_j within 1e-12 |lse_j| + 1e-9 p_waic_j.
      LOO   elpd_j, lppd_j and pareto_k_j within bound(what, S) = max(64 g, S 2^-53) relative to max(1, |value|), g the host
            estimator's own recorded gap to the 40-digit values (tests/test_survival_loo_cpu.py), and n_bad / n_warn equal.
    Both carry over unchanged: per dataset the ensemble's statistics ARE the plug-in handle's bits (the tests above)."""
    case = _Case("k2", 130, 7, 3)
    d = case.d
    model = survival.SurvivalDrawsModel(d, [d.s_titer, d.n_titer], ("S", "N"), priors=R.PRIORS[2])
    try:
        model.start, model.end = 2, 10
        fit = _fit_of(model, case, 2, 40)
        host_fit = dict(fit)
        w = survival.waic_draws(model, fit)
        lo = survival.loo_draws(model, fit)
        with pytest.raises(_native.AbdError, match="no matrix reserved"):
            model.draws_loo_stats()  # released
        w_host = survival.waic_draws(model, host_fit, pointwise=model.draws_individual_loglik)
        lo_host = survival.loo_draws(model, host_fit, pointwise=model.draws_individual_loglik)
    finally:
        model.close()
    assert all(k in fit for k in survival.DRAWS_WAIC_FIT_KEYS + survival.DRAWS_LOO_FIT_KEYS) and (int(fit["start"]), int(fit["end"])) == (2, 10)
    assert fit["draws_elpd_waic_ind"].shape == (3, 130) and fit["draws_waic_n_draws"].tolist() == [80, 80, 80]
    np.testing.assert_array_equal(fit["draws_waic_n_cells"], d.n_risk)
    np.testing.assert_array_equal(fit["draws_loo_n_cells"], d.n_risk)
    for m in range(3):
        a, b = w["datasets"][m], w_host["datasets"][m]
        followed = d.n_risk[m] > 0
        assert (a["elpd_i"][~followed] == 0).all() and (a["p_waic_i"][~followed] == 0).all() and (a["p_waic_i"][followed] > 0).all()
        gap_p = np.abs(a["p_waic_i"] - b["p_waic_i"])[followed] / b["p_waic_i"][followed]
        lse = b["elpd_i"] + b["p_waic_i"] + np.log(80)
        gap_e = np.abs(a["elpd_i"] - b["elpd_i"])[followed] / (1e-12 * np.abs(lse) + 1e-9 * b["p_waic_i"])[followed]
        print(f"dataset {m}: p_waic rel gap {gap_p.max():.3g} (1e-9), elpd gap over its bound {gap_e.max():.3g} (1)")
        assert gap_p.max() <= 1e-9 and gap_e.max() <= 1.0
        a, b = lo["datasets"][m], lo_host["datasets"][m]
        np.testing.assert_array_equal(np.isnan(a["pareto_k"]), ~followed)
        for key, what in (("elpd_i", "elpd"), ("lppd_i", "lppd"), ("pareto_k", "k")):
            gap = RL.rel_gap(a[key], b[key])
            print(f"dataset {m}: {key} device against host {gap:.3g} (bound {bound(what, 80):.3g})")
            assert gap <= bound(what, 80)
        assert (a["n_bad"], a["n_warn"], a["worst"]) == (b["n_bad"], b["n_warn"], b["worst"])
    for got, host in ((w, w_host), (lo, lo_host)):
        assert abs(got["elpd"] - host["elpd"]) <= 1e-9 * abs(host["elpd"]) and abs(got["se"] - host["se"]) <= 1e-6 * host["se"]
        assert 0.0 <= got["frac_between"] <= 1.0 and got["B"] > 0 and got["n_datasets"] == 3
    assert abs(lo["elpd"] - w["elpd"]) < 0.05 * abs(w["elpd"])  # two estimates of one quantity


# ---- 6. the command line, end to end on the golden cohort ----


def test_per_draw_ic_of_the_golden_cohort_end_to_end(tmp_path, golden_dir, capsys):
    """--per_draw 4 --per_draw_ic both for s, n and combined, then --compare of the three files (no GPU in that step): the table's
    pooled elpd_diff is compare_draws' in Python."""
    from abdpymc_amd.model import model
    from abdpymc_amd.sampler import sample

    cohort = os.path.join(golden_dir, "test_cohort")
    data = TiterData.from_disk(cohort)
    m = model(data, n_chains=2)
    res = sample(m, tune=20, draws=20, chains=2, seed=1, record_deterministics=True, record_discrete=False)
    m.close()
    post = tmp_path / "posterior.npz"
    np.savez(post, **{k: res[k] for k in ("i", "ab_s_mu", "ab_n_mu", "mean_i", "mean_ab_s_mu", "mean_ab_n_mu")})
    paths, fits = [], {}
    for name in ("s", "n", "combined"):
        out = tmp_path / f"{name}.npz"
        capsys.readouterr()
        rc = survival.main(["--posterior", str(post), "--ititers_data", cohort, "--start", "2", "--end", "20", "--model", name, "--out", str(out),
                            "--tune", "60", "--draws", "40", "--per_draw", "4", "--per_draw_ic", "both"])
        assert rc == 0
        lines = capsys.readouterr().out.splitlines()
        assert len(lines) == 3 and "per-draw fits of 4 datasets" in lines[0], lines
        assert lines[1].startswith("survival per-draw WAIC: elpd_waic ") and "frac_between" in lines[1] and "p_waic_j > 0.4" in lines[1]
        assert lines[2].startswith("survival per-draw PSIS-LOO: elpd_loo ") and "frac_between" in lines[2] and "pareto_k > 0.7" in lines[2]
        with np.load(out) as f:
            fits[name] = {k: f[k] for k in f.files}
        fit = fits[name]
        assert all(k in fit for k in survival.DRAWS_WAIC_FIT_KEYS + survival.DRAWS_LOO_FIT_KEYS + ("source", "dataset"))
        assert fit["draws_elpd_waic_ind"].shape == (4, data.n_inds) and fit["draws_pareto_k_ind"].shape == (4, data.n_inds)
        assert fit["draws_waic_n_draws"].tolist() == [40] * 4 and (int(fit["start"]), int(fit["end"])) == (2, 20)
        w = survival.draws_ic_of_fit(fit, "waic")
        assert survival.draws_ic_line(w) == lines[1] and survival.draws_ic_line(survival.draws_ic_of_fit(fit, "loo")) == lines[2]
        assert np.isfinite(w["elpd"]) and w["elpd"] < 0 and w["p"] > 0 and w["se"] > 0
        paths.append(str(out))
    for ic in ("waic", "loo"):
        capsys.readouterr()
        assert survival.main(["--compare"] + paths + ["--ic", ic]) == 0
        rows = capsys.readouterr().out.strip().split("\n")
        table = survival.compare_draws(fits, ic=ic)
        assert rows == survival.draws_compare_lines(table) and len(rows) == 3
        assert sorted(v["rank"] for v in table.values()) == [0, 1, 2]
        for row in rows:
            name = row.split()[0]
            assert float(row.split("elpd_diff ")[1].split()[0]) == float(f"{table[name]['elpd_diff']:.3f}")
        for v in table.values():
            assert v["dse"] >= 0 and 0.0 <= v["p_ahead"] <= 1.0 and np.isfinite([v["elpd"], v["se"], v["elpd_diff"], v["dse"]]).all()
        assert [v["elpd_diff"] for v in table.values() if v["rank"] == 0] == [0.0]
