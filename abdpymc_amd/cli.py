"""
``abdpymc-infer``: same flags and flow as the reference entry point (abd.py:885-924) --
TiterData.from_disk -> calculate_splits -> model(...) -> sample(tune, draws) -> write the posterior.

With PyMC installed the model can instead be handed to ``pm.sample`` through
:mod:`abdpymc_amd.pytensor_op`; this command uses the built-in compound sampler (NUTS + binary Gibbs) so it
runs on a box that has neither PyMC nor ArviZ.  Output: ArviZ NetCDF when ArviZ is importable, else a
``.npz`` with the same variable names (leading axes chain, draw; Deterministics with trailing gap, ind).
"""
from __future__ import annotations

import argparse
import sys
import time

import numpy as np


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser("abdpymc-infer")
    # reference flags, verbatim (abd.py:888-911)
    parser.add_argument("--tune", help="Number of tuning steps.", type=int, required=True)
    parser.add_argument("--draws", help="Number of draws.", type=int, required=True)
    parser.add_argument("--cores", help="Number of cores", type=int)
    parser.add_argument("--ititers_data", help="Path to directory for generating TiterData object.", default="cohort_data")
    parser.add_argument("--split_delta", help="Split time chunk between delta and pre-delta", action="store_true")
    parser.add_argument("--split_omicron", help="Split time chunk between omicron and delta", action="store_true")
    parser.add_argument("--ignore_pcrpos", help="Ignore PCR+ data", action="store_true")
    parser.add_argument("--netcdf", help="Path of netCDF file to save.")
    # additions (all optional)
    parser.add_argument("--chains", help="Number of chains (default: as pm.sample -- max(2, cores), cores = --cores or "
                        "min(4, CPU count)).", type=int)
    parser.add_argument("--seed", help="Random seed.", type=int, default=0)
    parser.add_argument("--device", help="HIP device ordinal.", type=int, default=-1)
    parser.add_argument("--no_deterministics", help="Do not record i / ab_n_mu / ab_s_mu per draw.", action="store_true")
    parser.add_argument("--no_discrete", help="Do not record i_raw / ab_s_waner per draw.", action="store_true")
    parser.add_argument("--thin", "--record_every", dest="thin", type=int, default=1,
                        help="Keep the per-draw (gap, ind) arrays of every K-th draw only (the 17 scalars, the statistics and the "
                        "posterior means mean_i / mean_ab_n_mu / mean_ab_s_mu cover every draw).  Default 1; a run whose arrays "
                        "exceed the host budget (ABD_RECORD_BUDGET_GB, default 8) is refused with the K that fits.")
    parser.add_argument("--dense_metric", help="Adapt a full mass matrix (PyMC's init='adapt_full') instead of a diagonal one.",
                        action="store_true")
    parser.add_argument("--waic", help="Accumulate the pointwise log-likelihood of the OD readings on the device over all draws and "
                        "report WAIC (elpd_waic, p_waic, se; per reading elpd_waic_i / p_waic_i in the output).", action="store_true")
    parser.add_argument("--log_likelihood", help="Record the pointwise log-likelihood of every OD reading at the recorded (thinned) "
                        "draws: ArviZ group log_likelihood (it_s_lik, it_n_lik), as pm.compute_log_likelihood.", action="store_true")
    parser.add_argument("--posterior_predictive", help="Record a posterior predictive replicate of every OD reading at the recorded "
                        "(thinned) draws: ArviZ groups posterior_predictive (it_s_lik, it_n_lik), as pm.sample_posterior_predictive, "
                        "and observed_data.", action="store_true")
    parser.add_argument("--ppc", help="Accumulate a posterior predictive check of the OD readings on the device over all draws and "
                        "report per antigen the readings with an extreme tail probability p = P(y_rep <= y | y) (per reading "
                        "ppc_p_it_s_lik / ppc_p_it_n_lik in the output).", action="store_true")
    parser.add_argument("--curves", help="Keep the epidemic curves of every draw (infections per gap, cumulative attack rate, "
                        "seroprevalence, mean titers; reduced over the individuals on the device, --thin does not apply) and report "
                        "the final cumulative attack rate and the peak monthly incidence with 95 %% intervals (curves_* in the "
                        "output).  An individual counts up to its last serum sample.", action="store_true")
    parser.add_argument("--sero_threshold_s", help="With --curves: S titer from which an individual counts as seropositive.",
                        type=float, default=float("inf"))
    parser.add_argument("--sero_threshold_n", help="With --curves: N titer from which an individual counts as seropositive.",
                        type=float, default=float("inf"))
    parser.add_argument("--diagnostics", help="Accumulate per cell of i / ab_n_mu / ab_s_mu, over all draws on the device, what split "
                        "R-hat and a batch-means effective sample size need (--thin does not apply) and report the largest R-hat, the "
                        "share of cells above 1.01 and the smallest ESS per variable, and the worst of the 17 scalars (diag_* and "
                        "diag_summary_* in the output).", action="store_true")
    parser.add_argument("--diag_batch", help="With --diagnostics: draws per batch of the batch-means ESS (default: the square root of "
                        "half the draws).", type=int)
    parser.add_argument("--risk", help="Keep the infection-risk-by-titer table of every draw (person-gaps at risk and infections by gap "
                        "and by bin of the previous gap's titer; reduced over the individuals on the device, --thin does not apply) "
                        "and report per antigen the protection (1 - the rate ratio stratified by gap) of the highest populated bin "
                        "against bin 0 with its 95 %% interval (risk_* in the output).  An individual counts up to its last serum "
                        "sample and, without --risk_all_infections, up to its first infection inside the window.", action="store_true")
    parser.add_argument("--risk_edges_s", help="With --risk: up to 7 ascending S titer bin edges, separated by commas.", default="")
    parser.add_argument("--risk_edges_n", help="With --risk: up to 7 ascending N titer bin edges, separated by commas.", default="")
    parser.add_argument("--risk_start", help="With --risk: the window's first gap; risk is counted from the gap after it.", type=int,
                        default=0)
    parser.add_argument("--risk_end", help="With --risk: the end of the window, one past its last gap (default: the number of gaps).",
                        type=int)
    parser.add_argument("--risk_all_infections", help="With --risk: count every infection of an individual inside the window, not "
                        "only the first.", action="store_true")
    parser.add_argument("--timelines", help="Accumulate per cell, over all draws on the device, what a per-individual timeline needs "
                        "(--thin does not apply): histograms of the S and N titers, from which the median and a 95 %% band are read, "
                        "the infection probability and the exact probability of at least one infection so far in the cell's time "
                        "chunk, and per individual the distribution of the number of infections (tl_* and tl_summary_* in the "
                        "output).  Reports the individuals more likely infected than not, the median width of the bands and the share "
                        "of bands that touch the ends of the range.", action="store_true")
    parser.add_argument("--timeline_range_s", help="With --timelines: the S titer range of the histograms, --timeline_range_s=lo,hi.", default="-4,8")
    parser.add_argument("--timeline_range_n", help="With --timelines: the N titer range of the histograms, --timeline_range_n=lo,hi.", default="-4,8")
    return parser


WAIC_KEYS = ("elpd_waic_i_it_s_lik", "elpd_waic_i_it_n_lik", "p_waic_i_it_s_lik", "p_waic_i_it_n_lik")
PPC_KEYS = ("ppc_p_it_s_lik", "ppc_p_it_n_lik")


def add_waic(res: dict) -> dict:
    """compare.waic of a gathered ``waic=True`` result: the per-reading values go into ``res`` (keys WAIC_KEYS), the totals
    are returned."""
    from . import compare

    w = compare.waic(res)
    res["elpd_waic_i_it_s_lik"], res["elpd_waic_i_it_n_lik"] = w["elpd_waic_i_s"], w["elpd_waic_i_n"]
    res["p_waic_i_it_s_lik"], res["p_waic_i_it_n_lik"] = w["p_waic_i_s"], w["p_waic_i_n"]
    return w


def add_ppc(res: dict) -> dict:
    """predictive.summary of a gathered ``ppc=True`` result: the tail probability of every reading goes into ``res`` (keys
    PPC_KEYS), the summary is returned."""
    from . import predictive

    sm = predictive.summary(res)
    res["ppc_p_it_s_lik"], res["ppc_p_it_n_lik"] = sm["it_s_lik"]["p"], sm["it_n_lik"]["p"]
    return sm


def add_curves(res: dict) -> dict:
    """curves.summary of a gathered ``curves=True`` result: its arrays go into ``res`` (``curves_summary_*``: rows lower, median,
    upper per gap), the summary is returned."""
    from . import curves

    sm = curves.summary(res)
    res.update(curves.summary_arrays(sm))
    return sm


def risk_spec_of(args, n_gaps: int):
    """The ``risk.spec`` the --risk flags ask for (``None`` without --risk); ``SystemExit`` for what ``risk.spec`` refuses."""
    if not args.risk:
        return None
    from . import risk

    try:
        edges = [[float(x) for x in text.split(",") if x.strip()] for text in (args.risk_edges_s, args.risk_edges_n)]
        return risk.spec(args.risk_start, args.risk_end, edges[0], edges[1], not args.risk_all_infections, n_gaps=n_gaps)
    except ValueError as e:
        raise SystemExit(f"--risk: {e}")


def add_risk(res: dict) -> dict:
    """risk.summary of a gathered ``risk=spec`` result.  The per-draw table is replaced in ``res`` by what a posterior file
    keeps of it: ``risk_by_bin`` (chains, draws, 2, 2, 8) the table summed over the gaps, ``risk_rate_ratio`` (chains, draws, 2,
    8) the per-draw rate ratios against bin 0, ``risk_table_sum`` (chains, 2, 2, G, 8) the table summed over the draws, and
    ``risk_summary_*``.  The summary is returned."""
    from . import risk

    sm = risk.summary(res)
    table = res.pop("risk_table")
    pd = risk.per_draw(table)
    res["risk_by_bin"], res["risk_rate_ratio"] = pd["by_bin"], pd["rate_ratio"]
    res["risk_table_sum"] = table.sum(axis=1)
    res.update(risk.summary_arrays(sm))
    return sm


def risk_line(sm: dict) -> str:
    """The CLI's one line about infection risk by titer: per antigen the highest populated bin against bin 0."""
    pct = int(round(100 * sm["prob"]))
    parts = []
    for name in ("s", "n"):
        a = sm[name]
        used = np.flatnonzero(np.nan_to_num(a["person_gaps"]["median"]) > 0)
        top = int(used[-1]) if used.size else 0
        if top == 0:
            parts.append(f"{name.upper()} no populated bin above bin 0")
            continue
        p = a["protection"]
        parts.append(f"{name.upper()} protection of bin {top} against bin 0 {100 * p['median'][top]:.1f} % ({pct} % interval "
                     f"{100 * p['lower'][top]:.1f} to {100 * p['upper'][top]:.1f}; defined in {int(p['n_defined'][top])} of "
                     f"{sm['n_draws']} draws)")
    return "risk: " + "; ".join(parts)


def add_diagnostics(res: dict, last_gap=None) -> dict:
    """diagnostics.summary of a gathered ``diagnostics=True`` result: its arrays go into ``res`` (``diag_summary_*``), the summary
    is returned."""
    from . import diagnostics

    sm = diagnostics.summary(res, last_gap)
    res.update(diagnostics.summary_arrays(sm))
    return sm


def diagnostics_line(sm: dict) -> str:
    """The CLI's one line about convergence: per variable over the followed cells, then the worst scalar."""
    parts = []
    for var in ("i", "ab_n_mu", "ab_s_mu"):
        f = sm[var].get("followed", sm[var])
        parts.append(f"{var} max R-hat {f['max_rhat']:.3f}, {100 * f['share_rhat_above_1.01']:.1f} % of {f['n_cells'] - f['n_constant']} "
                     f"non-constant followed cells above 1.01, min ESS {f['min_ess']:.0f}")
    sc = {k: v["rhat"] for k, v in sm["scalars"].items() if np.isfinite(v["rhat"])}
    worst = max(sc, key=sc.get) if sc else None
    parts.append(f"worst scalar {worst} R-hat {sc[worst]:.3f}" if worst else "no scalar with a finite R-hat")
    return "diagnostics: " + "; ".join(parts)


def timeline_ranges_of(args):
    """((lo_n, hi_n), (lo_s, hi_s)) of the --timeline_range_* flags; ``SystemExit`` for what ``timelines.check_range`` refuses."""
    from . import timelines

    out = []
    for flag, text in (("--timeline_range_n", args.timeline_range_n), ("--timeline_range_s", args.timeline_range_s)):
        try:
            lo, hi = (float(x) for x in text.split(","))
            out.append(timelines.check_range(lo, hi))
        except ValueError as e:
            raise SystemExit(f"{flag}: need lo,hi with lo < hi, got {text!r} ({e})")
    return tuple(out)


def add_timelines(res: dict, last_gap=None) -> dict:
    """timelines.summary of a gathered ``timelines=True`` result: its arrays go into ``res`` (``tl_summary_*``), the summary is
    returned.  A result gathered from several ranks carries the histograms and no pooled quantiles (``timeline_q=None``): they are
    pooled here (``timelines.merge`` / ``quantiles`` at ``DEFAULT_Q``) and the histograms are dropped from ``res``."""
    from . import timelines

    sm = timelines.summary(res, last_gap)
    if "tl_q_n" not in res:
        m = timelines.merge(res)
        q = np.array(timelines.DEFAULT_Q)
        res["tl_q"] = np.tile(q, (np.asarray(res["tl_inf"]).shape[0], 1))
        res["tl_q_n"] = timelines.quantiles(m["hist_n"], q, *m["range"][0])
        res["tl_q_s"] = timelines.quantiles(m["hist_s"], q, *m["range"][1])
        for k in timelines.HIST_KEYS:
            res.pop(k)
    res.update(timelines.summary_arrays(sm))
    return sm


def add_observed(res: dict, data) -> None:
    """The observed ODs of both antigens (no chain axis: added on the rank that writes, after any gather)."""
    res["observed_data_it_s_lik"] = np.asarray(data.s.obs[3], dtype=np.float64)
    res["observed_data_it_n_lik"] = np.asarray(data.n.obs[3], dtype=np.float64)


def write_posterior(res: dict, path: str, coords: dict) -> str:
    try:
        import arviz as az  # noqa: F401
    except ImportError:
        az = None
    if az is not None and path:
        # (UNVERIFIED-OFFLINE: ArviZ is not importable where this was written)
        dims = {"i_raw": ["gap", "ind"], "i": ["gap", "ind"], "ab_n_mu": ["gap", "ind"], "ab_s_mu": ["gap", "ind"],
                "ab_s_waner": ["ind"], "mean_i": ["chain", "gap", "ind"], "mean_ab_n_mu": ["chain", "gap", "ind"],
                "mean_ab_s_mu": ["chain", "gap", "ind"]}
        skip = ("n_grad_evals", "draw_index", "mean_i", "mean_ab_n_mu", "mean_ab_s_mu") + WAIC_KEYS
        post = {k: v for k, v in res.items()
                if not k.startswith(("stat_", "waic_", "log_likelihood_", "posterior_predictive_", "ppc_", "observed_data_", "curves_", "diag_", "risk_", "tl_"))
                and k not in skip}
        stats = {k[5:]: v for k, v in res.items() if k.startswith("stat_")}
        means = {k: res[k] for k in ("mean_i", "mean_ab_n_mu", "mean_ab_s_mu") + WAIC_KEYS + PPC_KEYS if k in res}
        # the epidemic curves: one row per draw, so they sit (and are thinned) with the statistics; what has no draw axis --
        # the number followed, the summary -- travels with the means
        for k, v in res.items():
            if k.startswith("curves_"):
                (means if k.startswith(("curves_summary_", "curves_n_followed")) else stats)[k] = v
        means.update({k: v for k, v in res.items() if k.startswith("diag_") and k != "diag_summary_scalar_names"})  # no draw axis
        means.update({k: v for k, v in res.items() if k.startswith("tl_")})  # no draw axis either
        # the risk tables: what has a draw axis sits (and is thinned) with the statistics, the rest travels with the means
        for k, v in res.items():
            if k.startswith("risk_"):
                (stats if k in ("risk_table", "risk_by_bin", "risk_rate_ratio") else means)[k] = v
        # pm.compute_log_likelihood: one variable per observed variable, its dim named as PyMC names an undimmed one
        loglik = {k[len("log_likelihood_"):]: v for k, v in res.items() if k.startswith("log_likelihood_")}
        # pm.sample_posterior_predictive: the replicates under the observed variables' names, beside the observed values
        pp = {k[len("posterior_predictive_"):]: v for k, v in res.items() if k.startswith("posterior_predictive_")}
        obs = {k[len("observed_data_"):]: v for k, v in res.items() if k.startswith("observed_data_")}
        dims.update({"it_s_lik": ["it_s_lik_dim_0"], "it_n_lik": ["it_n_lik_dim_0"],
                     "elpd_waic_i_it_s_lik": ["it_s_lik_dim_0"], "p_waic_i_it_s_lik": ["it_s_lik_dim_0"],
                     "elpd_waic_i_it_n_lik": ["it_n_lik_dim_0"], "p_waic_i_it_n_lik": ["it_n_lik_dim_0"],
                     "ppc_p_it_s_lik": ["it_s_lik_dim_0"], "ppc_p_it_n_lik": ["it_n_lik_dim_0"]})
        dims.update({k: ["gap"] for k in stats if k.startswith("curves_") and k != "curves_n_infections"})
        dims["curves_n_followed"] = ["chain", "gap"]
        if "draw_index" in res and res["draw_index"].shape[1] != next(iter(stats.values())).shape[1]:
            # --thin: an InferenceData has ONE draw axis, so the file holds the thinned draws of every variable (what
            # abdpymc-subsample-idata makes of a full one); the posterior means over ALL draws travel as constant data
            idx = res["draw_index"][0]
            n_all = next(iter(stats.values())).shape[1]
            post = {k: (v[:, idx] if v.shape[1] == n_all else v) for k, v in post.items()}
            stats = {k: v[:, idx] for k, v in stats.items()}
        idata = az.from_dict(posterior=post, sample_stats=stats, constant_data=means or None, log_likelihood=loglik or None,
                             posterior_predictive=pp or None, observed_data=obs or None, coords=coords, dims=dims)
        az.to_netcdf(idata, path)  # abd.py:924
        return path
    out = (path or "abd_posterior") + ("" if str(path or "").endswith(".npz") else ".npz")
    np.savez_compressed(out, **res, coord_gap=coords["gap"], coord_ind=coords["ind"])
    return out


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    from . import distributed
    from .data import TiterData
    from .model import model
    from .sampler import sample

    # one process per GPU under torch.distributed.run: chains are sharded, draws gathered at the end
    dist, rank, world, local = distributed.init_from_env()

    data = TiterData.from_disk(args.ititers_data)  # abd.py:913
    splits = (
        None
        if (not args.split_delta) and (not args.split_omicron)
        else data.calculate_splits(delta=args.split_delta, omicron=args.split_omicron)
    )  # abd.py:915-919
    risk_spec = risk_spec_of(args, data.n_gaps)  # (refused before anything is built)
    tl_ranges = timeline_ranges_of(args) if args.timelines else ((-4, 8), (-4, 8))
    # pm.sample(cores=...) (abd.py:922) runs chains = max(2, cores) with cores = min(4, CPU count) when not given
    import os

    cores = args.cores or min(4, os.cpu_count() or 1)
    chains = args.chains or max(2, cores)
    counts = distributed.split_counts(chains, world)
    mine, first = counts[rank], sum(counts[:rank])
    if chains < world:
        # every rank sees the same numbers and leaves together (a rank that went on alone would hang in the gather)
        if dist is not None:
            dist.destroy_process_group()
        raise SystemExit(f"{chains} chains cannot be sharded over {world} processes: fewer chains than ranks")
    device = args.device
    if world > 1 and device < 0:
        import torch

        device = local % max(1, torch.cuda.device_count())
    m = model(data, splits=splits, ignore_pcrpos=args.ignore_pcrpos, n_chains=mine, device=device)  # abd.py:921
    t0 = time.time()

    def progress(c, a, b):
        if a == b or a % max(1, b // 10) == 0:
            print(f"chain {first + c}: {a}/{b} iterations, {time.time() - t0:.1f} s", file=sys.stderr, flush=True)

    if args.thin < 1:
        raise SystemExit(f"--thin must be >= 1, got {args.thin}")
    if args.timelines and world > 1:
        # every rank hands its chains' histograms to rank 0, which pools them: refused (by every rank alike, before anything runs)
        # when what rank 0 holds after the gather -- the histograms and counters of all chains beside their recorded draws --
        # would not fit its host budget
        from . import timelines as tl_mod
        from .sampler import record_budget_bytes, record_bytes

        K = (len(data.s) + len(data.n)) if (args.log_likelihood or args.posterior_predictive) else 0
        own = tl_mod.result_bytes(chains, data.n_gaps, data.n_inds, n_q=0, hist=True)
        rest = record_bytes(chains, -(-args.draws // args.thin), data.n_gaps, data.n_inds, not args.no_deterministics, not args.no_discrete,
                            n_readings=K if args.log_likelihood else 0, n_replicates=K if args.posterior_predictive else 0)
        if own + rest > record_budget_bytes():
            if dist is not None:
                dist.destroy_process_group()
            raise SystemExit(f"--timelines over {world} processes gathers the histograms of {chains} chains on one rank: {own} bytes "
                             f"beside {rest} bytes of recorded draws, over the host budget of {record_budget_bytes()} bytes "
                             f"(ABD_RECORD_BUDGET_GB raises it; --thin, --no_deterministics, --no_discrete record less; one process "
                             f"needs no histograms on the host)")
    res = sample(m, tune=args.tune, draws=args.draws, chains=mine, seed=args.seed,
                 record_deterministics=not args.no_deterministics, record_discrete=not args.no_discrete, progress=progress,
                 chain_offset=first, dense_metric=args.dense_metric, thin=args.thin, log_likelihood=args.log_likelihood,
                 waic=args.waic, posterior_predictive=args.posterior_predictive, ppc=args.ppc, curves=args.curves,
                 sero_thresholds=(args.sero_threshold_s, args.sero_threshold_n), diagnostics=args.diagnostics,
                 diag_batch=args.diag_batch, risk=risk_spec, timelines=args.timelines, timeline_ranges=tl_ranges,
                 timeline_q=None if world > 1 else (0.025, 0.5, 0.975),  # (several ranks: rank 0 pools the histograms)
                 timelines_hist=args.timelines and world > 1)  # abd.py:922
    name = m.ctx.device_name
    m.close()
    if world > 1:
        import torch


        dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else None
        res = distributed.gather_results(res, counts, dist, dev)
    if rank == 0:
        if args.waic:
            w = add_waic(res)
            print(f"WAIC: elpd_waic {w['elpd_waic']:.3f}  p_waic {w['p_waic']:.3f}  se {w['se']:.3f}  ({w['n_readings']} readings, "
                  f"{w['n_draws']} draws; {w['n_warn']} readings with p_waic_i > 0.4)", file=sys.stderr)
        if args.ppc:
            sm = add_ppc(res)
            for name in ("it_s_lik", "it_n_lik"):
                a = sm[name]
                print(f"PPC {name}: {a['n_extreme']} of {a['n_readings']} readings ({100 * a['share_extreme']:.2f} %) with p < 0.025 "
                      f"({a['n_low']}) or p > 0.975 ({a['n_high']}); {sm['n_draws']} draws", file=sys.stderr)
        if args.curves:
            sm = add_curves(res)
            followed = np.flatnonzero(sm["n_followed"] > 0)
            if followed.size and sm["n_draws"]:
                g, inc = followed[-1], sm["incidence"]
                peak = followed[np.argmax(inc["median"][followed])]
                ar = sm["attack_rate"]
                pct = int(round(100 * sm["prob"]))
                print(f"curves: cumulative attack rate at gap {g} {100 * ar['median'][g]:.1f} % ({pct} % interval "
                      f"{100 * ar['lower'][g]:.1f}-{100 * ar['upper'][g]:.1f}; {sm['n_followed'][g]} followed); peak monthly incidence "
                      f"{100 * inc['median'][peak]:.1f} % ({100 * inc['lower'][peak]:.1f}-{100 * inc['upper'][peak]:.1f}) at gap {peak}; "
                      f"{sm['n_draws']} draws", file=sys.stderr)
        if args.risk:
            print(risk_line(add_risk(res)), file=sys.stderr)
        if args.diagnostics:
            print(diagnostics_line(add_diagnostics(res, getattr(data, "last_gap", None))), file=sys.stderr)
        if args.timelines:
            from . import timelines

            print(timelines.line(add_timelines(res, getattr(data, "last_gap", None))), file=sys.stderr)
        if args.posterior_predictive:
            add_observed(res, data)
        out = write_posterior(res, args.netcdf, data.coords)
        print(f"wrote {out}  ({chains} chains x {args.draws} draws on {world} x {name})", file=sys.stderr)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
