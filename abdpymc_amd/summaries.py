"""
The per-draw summaries of the native sampler, as the host sees them: every summary is described ONCE, by a ``Summary`` object
in its own module (``SUMMARY``), and ``sampler.sample`` / ``sample_native``, ``cli.main`` and ``cli.write_posterior`` loop over
``every()``.  A new summary is a module with such an object plus one line in ``registry()`` ("Adding a summary").

``log_likelihood`` / ``posterior_predictive`` are per-draw record rows of the sampler, not summaries: they stay in its record path.

NumPy only.
"""
from __future__ import annotations

import warnings
from typing import Dict, List, Optional

import numpy as np


def registry() -> tuple:
    """The summaries that are kept per chain, so that chains sharded over processes gather them, in the order they are planned,
    counted against the host budget, enabled, collected and reported.  (A function, not a module constant: the six modules take
    their base class from this one, whichever is imported first.)"""
    from . import compare, curves, diagnostics, predictive, risk, timelines

    return (compare.SUMMARY, predictive.SUMMARY, curves.SUMMARY, diagnostics.SUMMARY, risk.SUMMARY, timelines.SUMMARY)


def every() -> tuple:
    """``registry()`` and, behind ``compare.SUMMARY``, ``loo.SUMMARY``, which pools the draws of all chains on one device and so
    runs in one process only: what ``sample``, ``resolve`` and the command line loop over."""
    from . import loo

    reg = registry()
    return reg[:1] + (loo.SUMMARY,) + reg[1:]


class Summary:
    """What the host needs to know about one summary.  ``options``' docstring lives on the subclass: each option is documented
    there and nowhere else."""

    name = ""            # the ``sample()`` keyword that switches it on, and the CLI flag
    options: Dict[str, object] = {}  # the ``sample()`` keywords it owns -> their defaults (``name`` among them)
    prefix = ""          # every result key it returns starts with it
    draw_keys = ()       # those with a (chains, draws) axis: a NetCDF file keeps (and thins) them with the sample statistics
    derived_keys = ()    # keys ``report`` adds outside the prefix
    dims: Dict[str, list] = {}  # NetCDF dims of its keys, where they have named ones
    follow_up = False    # counts an individual up to its last serum sample: needs ``Context.set_follow_up``
    record_row: Optional[str] = None  # the per-draw record row of ``sample()`` that the host sampler refuses with it
    native_only = ""     # what ``sample(native=False)`` raises for it

    def on(self, opts) -> bool:
        return bool(opts[self.name])

    def plan(self, opts, draws: int, chains: int, G: int, N: int) -> Optional[dict]:
        """``None`` when the summary is off, else the checked request (``ValueError`` for what it refuses): the run's sizes and
        the summary's own options, to which subclasses add what they derive.  Runs before the device is touched."""
        return dict({k: opts[k] for k in self.options}, draws=int(draws), chains=int(chains), G=int(G), N=int(N)) if self.on(opts) else None

    def host_bytes(self, plan) -> int:
        """Host bytes of the arrays ``collect`` returns that count against the budget; a summary that counts some also has
        ``over_budget(plan, own, before, budget)``, the message of the refusal."""
        return 0

    def enable(self, smp, plan) -> None:
        """One call of a ``NativeSampler.enable_*`` method."""
        raise NotImplementedError

    def collect(self, smp, plan, last_gap) -> Dict[str, np.ndarray]:
        """The summary's result keys after the last draw."""
        raise NotImplementedError

    # -- the command line ---------------------------------------------------------------------------
    def add_arguments(self, parser) -> None:
        raise NotImplementedError

    def cli_options(self, args, data, chains: int, world: int) -> dict:
        """The ``sample()`` options the flags ask for (``chains``: of all ``world`` processes together); ``SystemExit`` for what
        they cannot mean."""
        return {k: getattr(args, k) for k in self.options}  # (where every option is a flag of its own name)

    def report(self, res: dict, data) -> List[str]:
        """Of a gathered result: the derived arrays go into ``res``, the lines for stderr are returned."""
        raise NotImplementedError

    # -- a posterior file ---------------------------------------------------------------------------
    def owns(self, key: str) -> bool:
        return key.startswith(self.prefix) or key in self.derived_keys

    def group(self, key: str) -> Optional[str]:
        """The ArviZ group of one of its keys (``None``: not written)."""
        return "sample_stats" if key in self.draw_keys else "constant_data"


def resolve(given: dict) -> dict:
    """Every summary option with its default, overridden by ``given``; ``TypeError`` for a keyword no summary owns."""
    opts = {k: v for s in every() for k, v in s.options.items()}
    for k in given:
        if k not in opts:
            raise TypeError(f"sample() got an unexpected keyword argument {k!r}")
    opts.update(given)
    return opts


def per_reading_result(prefix: str, names, per_chain, n_obs) -> Dict[str, np.ndarray]:
    """The keys of a per-reading accumulator (WAIC, PPC) from its chains' ``(out (3, K_s + K_n), n_draws)``: ``<prefix><name>``
    (chains, K_s + K_n) for the three rows, ``<prefix>n_draws`` (chains,) and ``<prefix>n_obs`` (chains, 2) = (K_s, K_n)."""
    res = {prefix + name: np.stack([o[j] for o, _ in per_chain]) for j, name in enumerate(names)}
    res[prefix + "n_draws"] = np.array([n for _, n in per_chain], dtype=np.int64)
    res[prefix + "n_obs"] = np.tile(np.array(n_obs, dtype=np.int64), (len(per_chain), 1))
    return res


def interval(x: np.ndarray, prob: float, count_defined: bool = False) -> Dict[str, np.ndarray]:
    """Median and equal-tailed interval over axis 0; NaN draws are ignored (a column that is NaN in every draw stays NaN) and,
    with ``count_defined``, the others are counted (``n_defined``)."""
    lo = (1.0 - prob) / 2.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # (an all-NaN column)
        q = np.nanquantile(x, [lo, 0.5, 1.0 - lo], axis=0) if x.shape[0] else np.full((3,) + x.shape[1:], np.nan)
    out = {"lower": q[0], "median": q[1], "upper": q[2]}
    if count_defined:
        out["n_defined"] = np.isfinite(x).sum(axis=0).astype(np.int64)
    return out
