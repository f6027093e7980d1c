"""
The forward simulator of a cohort on the device: infections under titer-mediated protection, S and N titers, OD readings.

Mirror of the reference's ``abdpymc.simulation`` (simulation.py:34-369) -- ``Protection``, ``Elisa``, ``Dynamics``, ``Antibody``,
``Antibodies``, ``Cohort`` with the same fields, defaults and validation rules -- so that a script ports by changing the import.
The simulation itself runs in the HIP library (``include/abd_hip.h``: ``abd_simulate`` defines it and its random streams);
the reference consumes ``np.random`` sequentially, here every draw is keyed by (seed, replicate, individual, gap) or
(seed, replicate, antigen, reading), so a replicate depends on ``(random_seed, replicate)`` only and a thousand of them are
one call (``Cohort.simulate_many``).  There is no CPU path.

Command line::

    python -m abdpymc_amd.simulation --cohort_data DIR --lam0 0.04 --seed 42 --replicate 0 --out DIR

writes a cohort directory in the reference's format (``df.csv``, ``vacs.txt``, ``pcrpos.txt``, ``t0.txt``) whose ``od`` column is
simulated, ready for ``abdpymc-infer --ititers_data DIR``, and ``truth.npz`` with the infections, the titers and the parameters.
"""
from __future__ import annotations

import argparse
import dataclasses
import math
import os
from typing import Optional, Sequence

import numpy as np

from . import _native
from .data import MEASUREMENT_N, MEASUREMENT_S, AntigenTiterData, TiterData


def _finite(obj, *names) -> None:
    for name in names:
        v = getattr(obj, name)
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
            raise ValueError(f"{name} must be a finite number, got {v!r}")
        object.__setattr__(obj, name, float(v))


def _require(ok: bool, name: str, rule: str, value) -> None:
    if not ok:
        raise ValueError(f"{name} must be {rule}, got {value!r}")


@dataclasses.dataclass(frozen=True)
class Protection:
    """Parameters of a protection curve: ``a`` the 50% protective titer, ``b`` (> 0) its slope (simulation.py:34-44)."""

    a: float = 0.0
    b: float = 1.0

    def __post_init__(self) -> None:
        _finite(self, "a", "b")
        _require(self.b > 0, "b", "> 0", self.b)

    def p_protection(self, titer):
        """Probability of protection from infection at a given titer (simulation.py:46-50)."""
        return 1 / (1 + np.exp(-self.b * (titer - self.a)))


@dataclasses.dataclass(frozen=True)
class Elisa:
    """Parameters of an ELISA titration curve: slope ``b`` (< 0), maximum response ``d`` (> 0), standard deviation ``sd`` (> 0)
    of the error on an OD reading (simulation.py:66-78)."""

    b: float = -2.2
    d: float = 1.6
    sd: float = 0.1

    def __post_init__(self) -> None:
        _finite(self, "b", "d", "sd")
        _require(self.b < 0, "b", "< 0", self.b)
        _require(self.d > 0, "d", "> 0", self.d)
        _require(self.sd > 0, "sd", "> 0", self.sd)


@dataclasses.dataclass(frozen=True)
class Dynamics:
    """How antibody titers change over time: the initial value, the permanent rise after any infection or vaccination, the
    temporary rises after an infection / a vaccination and the waning rate (simulation.py:93-115)."""

    init: float = -2.0
    perm_rise: float = 2.0
    temp_rise_i: float = 1.5
    temp_rise_v: float = 2.0
    temp_wane: float = 0.95

    def __post_init__(self) -> None:
        _finite(self, "init", "perm_rise", "temp_rise_i", "temp_rise_v", "temp_wane")
        for name in ("perm_rise", "temp_rise_i", "temp_rise_v"):
            _require(getattr(self, name) >= 0, name, ">= 0", getattr(self, name))
        _require(0.0 < self.temp_wane <= 1.0, "temp_wane", "in (0, 1] (waning parameter must be between 0-1)", self.temp_wane)


@dataclasses.dataclass(frozen=True)
class Antibody:
    """Behaviour of an antibody: protection from infection, ELISA characteristics, dynamics (simulation.py:155-164)."""

    protection: Protection = Protection()
    elisa: Elisa = Elisa()
    dynamics: Dynamics = Dynamics()

    def __post_init__(self) -> None:
        for name, cls in (("protection", Protection), ("elisa", Elisa), ("dynamics", Dynamics)):
            if not isinstance(getattr(self, name), cls):
                raise ValueError(f"{name} must be a {cls.__name__}, got {getattr(self, name)!r}")

    def as_native(self) -> dict:
        """The ten fields of ``abd_sim_antibody``."""
        p, e, d = self.protection, self.elisa, self.dynamics
        return dict(protect_a=p.a, protect_b=p.b, elisa_b=e.b, elisa_d=e.d, elisa_sd=e.sd, init=d.init, perm_rise=d.perm_rise,
                    temp_rise_i=d.temp_rise_i, temp_rise_v=d.temp_rise_v, temp_wane=d.temp_wane)


@dataclasses.dataclass(frozen=True)
class Antibodies:
    """S and N antibodies (simulation.py:167-173)."""

    s: Antibody = Antibody()
    n: Antibody = Antibody()

    def __post_init__(self) -> None:
        for name in ("s", "n"):
            if not isinstance(getattr(self, name), Antibody):
                raise ValueError(f"{name} must be an Antibody, got {getattr(self, name)!r}")

    def as_native(self) -> dict:
        return {"s": self.s.as_native(), "n": self.n.as_native()}


def check_lam0(lam0, n_gaps: int) -> np.ndarray:
    """The reference's conditions on lam0 and their messages (simulation.py:229-233)."""
    lam0 = np.asarray(lam0, dtype=np.float64)
    if lam0.ndim != 1:
        raise ValueError("lam0 should be 1D")
    if len(lam0) != n_gaps:
        raise ValueError("must have single infection rate for each time gap")
    return lam0


class Cohort:
    """
    A cohort whose infections, titers and OD readings are simulated on the device (simulation.py:282-369).

    Args:
        random_seed: key of every random stream (the reference passes it to ``np.random.seed``).
        cohort_data_path: cohort directory (``TiterData.from_disk``); or
        data: a ``TiterData``.
        antibodies: defines antibody responses.
        replicate: which replicate ``simulate_responses`` draws (each is an independent cohort under the same seed).

    Attributes:
        n_inds, n_gaps: sizes.  true: the ``TiterData`` the timing of samples, vaccinations and PCR+ results come from.
        s_titer, n_titer, infections: (n_inds, n_gaps), set by ``simulate_responses``.
    """

    def __init__(self, random_seed: int, cohort_data_path: Optional[str] = None, antibodies: Antibodies = Antibodies(),
                 data: Optional[TiterData] = None, replicate: int = 0, device: int = -1) -> None:
        if (cohort_data_path is None) == (data is None):
            raise ValueError("give exactly one of cohort_data_path and data")
        if not isinstance(antibodies, Antibodies):
            raise ValueError(f"antibodies must be an Antibodies, got {antibodies!r}")
        self.random_seed = int(random_seed)
        self.cohort_data_path = cohort_data_path
        self.antibodies = antibodies
        self.replicate = int(replicate)
        self._df = None  # the directory's reading table, read when simulate_dataset first needs it
        if cohort_data_path is not None:
            data = TiterData.from_disk(cohort_data_path)
        self.true = data
        self.n_inds, self.n_gaps = np.asarray(data.vacs).shape
        self.ctx = _native.Context(self.n_gaps, self.n_inds, data.s.obs, data.n.obs, data.vacs, data.pcrpos, device=device)
        self._od = None

    # -- lifetime (as AbdModel) -------------------------------------------------------------------
    def close(self) -> None:
        self.ctx.close()

    def __enter__(self) -> "Cohort":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    # -- the reference's methods ------------------------------------------------------------------
    def simulate_responses(self, lam0) -> None:
        """Simulate responses for all individuals: updates ``s_titer``, ``n_titer`` and ``infections`` (simulation.py:312-326;
        replicate ``self.replicate``), and draws the OD readings that ``simulate_dataset`` returns."""
        lam0 = check_lam0(lam0, self.n_gaps)
        out = self.ctx.simulate(self.antibodies.as_native(), lam0, self.random_seed, self.replicate, 1,
                                ("infections", "s_titer", "n_titer", "od_s", "od_n"))
        self.lam0 = lam0
        self.s_titer, self.n_titer = out["s_titer"][0], out["n_titer"][0]
        self.infections = out["infections"][0].astype(np.float64)
        self._od = (out["od_s"][0], out["od_n"][0])

    def _table(self):
        """The reading table of ``true``: the directory's df.csv, or one built from the arrays (S readings, then N)."""
        import pandas as pd

        if self._df is None and self.cohort_data_path is not None:
            self._df = pd.read_csv(os.path.join(str(self.cohort_data_path), "df.csv"), index_col=0)
        if self._df is not None:
            return self._df

        s, n = self.true.s, self.true.n
        return pd.DataFrame({
            "measurement": np.concatenate([np.full(len(s), MEASUREMENT_S), np.full(len(n), MEASUREMENT_N)]),
            "od": np.concatenate([s.od, n.od]),
            "elapsed_months": np.concatenate([s.idx_gap, n.idx_gap]),
            "individual_i": np.concatenate([s.idx_ind, n.idx_ind]),
            "log_dilution": np.concatenate([s.log_dilution, n.log_dilution]),
        })

    def simulate_dataset(self, df_true=None):
        """The reading table with ``od`` replaced by the simulated readings; the other columns are kept (simulation.py:355-369).
        ``df_true``: the cohort's own table (the readings are those the cohort was created with); None takes it."""
        if self._od is None:
            raise ValueError("no simulated responses yet: call simulate_responses(lam0) first")
        own = self._table()
        df = own if df_true is None else df_true
        if df is not own:
            for col in ("measurement", "elapsed_months", "individual_i", "log_dilution"):
                if len(df) != len(own) or not np.array_equal(df[col].to_numpy(), own[col].to_numpy()):
                    raise ValueError(f"df_true differs from the cohort's reading table in column {col!r}")
        df = df.copy()
        od = df["od"].to_numpy(dtype=np.float64, copy=True)
        od[(df["measurement"] == MEASUREMENT_S).to_numpy()] = self._od[0]
        od[(df["measurement"] == MEASUREMENT_N).to_numpy()] = self._od[1]
        df["od"] = od
        return df

    def to_titer_data(self) -> TiterData:
        """A ``TiterData`` carrying the simulated OD, ready for ``abdpymc_amd.model``."""
        if self._od is None:
            raise ValueError("no simulated responses yet: call simulate_responses(lam0) first")
        t = self.true
        s = AntigenTiterData("s", t.s.idx_gap, t.s.idx_ind, t.s.log_dilution, self._od[0])
        n = AntigenTiterData("n", t.n.idx_gap, t.n.idx_ind, t.n.log_dilution, self._od[1])
        new = TiterData(t.t0, s, n, t.vacs, t.pcrpos, t.n_gaps, t.n_inds, record_ids=t.record_ids)
        if hasattr(t, "ageenroll"):  # enrollment ages of a directory with individuals.csv: already in the individuals' order
            new.ageenroll = t.ageenroll
        return new

    # -- batches ----------------------------------------------------------------------------------
    def simulate_many(self, lam0, n_replicates: int, first: int = 0, outputs: Sequence[str] = _native.SIM_OUTPUTS,
                      staging_bytes: Optional[int] = None) -> dict:
        """Replicates ``first .. first + n_replicates - 1`` in one call -> dict of the batched arrays asked for
        (``Context.simulate``).  Replicate r of the batch is what ``Cohort(..., replicate=r).simulate_responses`` draws."""
        return self.ctx.simulate(self.antibodies.as_native(), check_lam0(lam0, self.n_gaps), self.random_seed, int(first),
                                 int(n_replicates), outputs, staging_bytes)

    def write(self, directory: str) -> None:
        """The simulated cohort as a cohort directory in the reference's format, and truth.npz."""
        df = self.simulate_dataset()
        os.makedirs(directory, exist_ok=True)
        df.to_csv(os.path.join(directory, "df.csv"), float_format="%.17g")
        np.savetxt(os.path.join(directory, "vacs.txt"), np.asarray(self.true.vacs), fmt="%d")
        np.savetxt(os.path.join(directory, "pcrpos.txt"), np.asarray(self.true.pcrpos), fmt="%d")
        with open(os.path.join(directory, "t0.txt"), "w") as f:
            f.write(self.true.t0 + "\n")
        par = self.antibodies.as_native()
        np.savez(os.path.join(directory, "truth.npz"), infections=self.infections.astype(np.int8), s_titer=self.s_titer,
                 n_titer=self.n_titer, od_s=self._od[0], od_n=self._od[1], lam0=self.lam0, random_seed=self.random_seed,
                 replicate=self.replicate, **{f"{ag}_{k}": v for ag in ("s", "n") for k, v in par[ag].items()})


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m abdpymc_amd.simulation", description=__doc__.split("\n\n")[0])
    p.add_argument("--cohort_data", required=True, help="cohort directory the sample timing, vaccinations and PCR+ come from")
    p.add_argument("--lam0", type=float, nargs="+", required=True, help="infection probability per gap: one value, or one per gap")
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--replicate", type=int, default=0)
    p.add_argument("--out", required=True, help="directory to write")
    p.add_argument("--device", type=int, default=-1)
    return p


def main(argv=None) -> int:
    a = build_parser().parse_args(argv)
    with Cohort(a.seed, a.cohort_data, replicate=a.replicate, device=a.device) as cohort:
        lam0 = np.full(cohort.n_gaps, a.lam0[0]) if len(a.lam0) == 1 else np.asarray(a.lam0)
        cohort.simulate_responses(lam0)
        cohort.write(a.out)
        print(f"wrote {a.out}: {cohort.n_inds} individuals x {cohort.n_gaps} gaps, {int(cohort.infections.sum())} infections")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
