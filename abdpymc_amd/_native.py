"""
ctypes binding of ``libabd_hip.so`` (C ABI: ``include/abd_hip.h``).

The HIP library is the only implementation of the hot path in this package: if it is missing or fails
to load, importing the symbols below raises -- there is no CPU fallback (the CPU restatement under
``oracle/`` is test infrastructure and is never imported from here).
"""
from __future__ import annotations

import ctypes as C
import os
import weakref
from typing import Optional, Sequence

import numpy as np

N_THETA = 17
MAX_GAPS = 512
STORE_F64, STORE_F32 = 0, 1

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ABD_HIP_LIB", os.path.join(_HERE, "libabd_hip.so"))


class AbdError(RuntimeError):
    """HIP/runtime failure inside the native library."""


class _AntigenObs(C.Structure):
    _fields_ = [
        ("n_obs", C.c_int64),
        ("idx_gap", C.POINTER(C.c_int32)),
        ("idx_ind", C.POINTER(C.c_int32)),
        ("log_dilution", C.POINTER(C.c_double)),
        ("od", C.POINTER(C.c_double)),
    ]


class _Desc(C.Structure):
    _fields_ = [
        ("n_gaps", C.c_int32),
        ("n_inds", C.c_int32),
        ("n_splits", C.c_int32),
        ("splits", C.c_int32 * 2),
        ("storage", C.c_int32),
        ("n_chain_slots", C.c_int32),
        ("device", C.c_int32),
        ("s", _AntigenObs),
        ("n", _AntigenObs),
        ("vacs", C.POINTER(C.c_int8)),
        ("pcrpos", C.POINTER(C.c_int8)),
    ]


class _SamplerOpts(C.Structure):
    _fields_ = [
        ("tune", C.c_int64),
        ("seed", C.c_uint64),
        ("target_accept", C.c_double),
        ("max_treedepth", C.c_int32),
        ("gibbs", C.c_int32),
        ("accumulate", C.c_int32),
        ("chain_offset", C.c_int32),
        ("dense_metric", C.c_int32),
        ("reserved", C.c_int32),
    ]


class _Record(C.Structure):
    _fields_ = [
        ("capacity", C.c_int64),
        ("first", C.c_int64),
        ("thin", C.c_int64),
        ("i_raw", C.POINTER(C.c_int8)),
        ("ab_s_waner", C.POINTER(C.c_int8)),
        ("i", C.POINTER(C.c_int8)),
        ("ab_n_mu", C.POINTER(C.c_double)),
        ("ab_s_mu", C.POINTER(C.c_double)),
        ("ll_s", C.POINTER(C.c_double)),
        ("ll_n", C.POINTER(C.c_double)),
        ("yrep_s", C.POINTER(C.c_double)),
        ("yrep_n", C.POINTER(C.c_double)),
    ]


class _SimAntibody(C.Structure):
    _fields_ = [(name, C.c_double) for name in ("protect_a", "protect_b", "elisa_b", "elisa_d", "elisa_sd", "init", "perm_rise",
                                                "temp_rise_i", "temp_rise_v", "temp_wane")]


class _SimParams(C.Structure):
    _fields_ = [("s", _SimAntibody), ("n", _SimAntibody)]


SIM_OUTPUTS = ("infections", "s_titer", "n_titer", "od_s", "od_n", "n_infected")  # abd_simulate's outputs, in its order

N_STATS = 11
STAT_NAMES = ("lp", "tree_depth", "n_steps", "mean_tree_accept", "step_size", "diverging", "energy", "max_energy_error",
              "gibbs_accepted", "gibbs_proposed", "t_done")

_lib = None

# every symbol include/abd_hip.h declares: name -> (restype, argtypes)
class _RiskSpec(C.Structure):  # abd_risk_spec
    _fields_ = [("start", C.c_int32), ("end", C.c_int32), ("first_only", C.c_int32), ("n_edges_s", C.c_int32),
                ("n_edges_n", C.c_int32), ("edges_s", C.c_double * 7), ("edges_n", C.c_double * 7)]


def _risk_spec(spec) -> "_RiskSpec":
    """``risk.spec``'s dict (or anything with its keys) as the ABI's struct; the library checks the values."""
    r = _RiskSpec()
    r.start, r.end, r.first_only = int(spec["start"]), int(spec["end"]), int(spec["first_only"])
    for name in ("edges_s", "edges_n"):
        e = np.atleast_1d(np.asarray(spec[name], dtype=np.float64))
        if e.ndim != 1 or e.size > 7:
            raise ValueError(f"{name}: at most 7 edges in one dimension, got shape {e.shape}")
        setattr(r, "n_" + name, int(e.size))
        getattr(r, name)[: e.size] = e.tolist()
    return r


class _SurvivalDesc(C.Structure):  # abd_survival_desc
    _fields_ = [("n_inds", C.c_int32), ("n_intervals", C.c_int32), ("n_titers", C.c_int32), ("device", C.c_int32),
                ("infected", C.c_void_p), ("exposure", C.c_void_p), ("titer", C.c_void_p * 2),
                ("ab_sd", C.c_double), ("lam0_mu_mean", C.c_double), ("lam0_mu_sd", C.c_double), ("lam0_sd_rate", C.c_double),
                ("lam0_z_sd", C.c_double)]


class _SurvivalGroupsDesc(C.Structure):  # abd_survival_groups_desc
    _fields_ = [("n_inds", C.c_int32), ("n_intervals", C.c_int32), ("n_groups", C.c_int32), ("device", C.c_int32),
                ("infected", C.c_void_p), ("exposure", C.c_void_p), ("titer", C.c_void_p), ("group", C.c_void_p),
                ("lam0_mu_mean", C.c_double), ("lam0_mu_sd", C.c_double), ("lam0_sd_rate", C.c_double), ("lam0_z_sd", C.c_double),
                ("a_mu_sd", C.c_double), ("a_sd_rate", C.c_double), ("a_z_sd", C.c_double), ("b_sd", C.c_double)]


class _SurvivalPeriodsDesc(C.Structure):  # abd_survival_periods_desc
    _fields_ = [("n_inds", C.c_int32), ("n_intervals", C.c_int32), ("n_periods", C.c_int32), ("device", C.c_int32),
                ("infected", C.c_void_p), ("exposure", C.c_void_p), ("titer", C.c_void_p), ("period", C.c_void_p),
                ("lam0_mu_mean", C.c_double), ("lam0_mu_sd", C.c_double), ("lam0_sd_rate", C.c_double), ("lam0_z_sd", C.c_double),
                ("a_mu_sd", C.c_double), ("a_sd_rate", C.c_double), ("a_z_sd", C.c_double), ("b_sd", C.c_double)]


class _SurvivalDrawsDesc(C.Structure):  # abd_survival_draws_desc
    _fields_ = [("n_datasets", C.c_int32), ("n_inds", C.c_int32), ("n_intervals", C.c_int32), ("n_titers", C.c_int32), ("device", C.c_int32),
                ("n_risk", C.c_void_p), ("event", C.c_void_p), ("titer", C.c_void_p * 2),
                ("ab_sd", C.c_double), ("lam0_mu_mean", C.c_double), ("lam0_mu_sd", C.c_double), ("lam0_sd_rate", C.c_double),
                ("lam0_z_sd", C.c_double)]


class _SurvivalDrawsGroupsDesc(C.Structure):  # abd_survival_draws_groups_desc
    _fields_ = [("n_datasets", C.c_int32), ("n_inds", C.c_int32), ("n_intervals", C.c_int32), ("n_groups", C.c_int32), ("device", C.c_int32),
                ("n_risk", C.c_void_p), ("event", C.c_void_p), ("titer", C.c_void_p), ("group", C.c_void_p),
                ("lam0_mu_mean", C.c_double), ("lam0_mu_sd", C.c_double), ("lam0_sd_rate", C.c_double), ("lam0_z_sd", C.c_double),
                ("a_mu_sd", C.c_double), ("a_sd_rate", C.c_double), ("a_z_sd", C.c_double), ("b_sd", C.c_double)]


class _SurvivalDrawsPeriodsDesc(C.Structure):  # abd_survival_draws_periods_desc
    _fields_ = [("n_datasets", C.c_int32), ("n_inds", C.c_int32), ("n_intervals", C.c_int32), ("n_periods", C.c_int32), ("device", C.c_int32),
                ("n_risk", C.c_void_p), ("event", C.c_void_p), ("titer", C.c_void_p), ("period", C.c_void_p),
                ("lam0_mu_mean", C.c_double), ("lam0_mu_sd", C.c_double), ("lam0_sd_rate", C.c_double), ("lam0_z_sd", C.c_double),
                ("a_mu_sd", C.c_double), ("a_sd_rate", C.c_double), ("a_z_sd", C.c_double), ("b_sd", C.c_double)]


SURVIVAL_MAX_GROUPS = 256  # ABD_SURVIVAL_MAX_GROUPS

# abd_gibbs_record and its ABD_GIBBS_PATH_* codes (include/abd_hip.h)
GIBBS_RECORD = np.dtype([("value", "<f8"), ("log_u", "<f8"), ("dim", "<i2"), ("gf", "<i2"), ("stop", "<i2"), ("path", "u1"),
                         ("accepted", "u1")])
GIBBS_PATHS = {"prior": 1, "early": 2, "walk": 3, "tail": 4, "wave_waner": 5, "wave_overflow": 6, "list": 7, "list_prior": 8}

_P = C.c_void_p
# array arguments (double*, int32_t*, int8_t*) are passed as plain addresses: building a typed ctypes pointer per argument
# (ndarray.ctypes.data_as) costs 1.5-3 us each, which is a third of a synchronous call on a small cohort
_D = C.c_void_p
_I32 = C.c_void_p
_I8 = C.c_void_p
SYMBOLS = {
    "abd_version": (C.c_char_p, []),
    "abd_last_error": (C.c_char_p, []),
    "abd_create": (C.c_int, [C.POINTER(_Desc), C.POINTER(_P)]),
    "abd_destroy": (C.c_int, [_P]),
    "abd_device_name": (C.c_int, [_P, C.c_char_p, C.c_int32]),
    "abd_set_discrete": (C.c_int, [_P, C.c_int32, _I8, _I8]),
    "abd_flip_discrete": (C.c_int, [_P, C.c_int32, C.c_int64]),
    "abd_get_discrete": (C.c_int, [_P, C.c_int32, _I8, _I8]),
    "abd_gibbs_sweep": (C.c_int, [_P, C.c_int32, _I32, _D, C.c_uint64, C.c_uint32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "abd_gibbs_sweep_log": (C.c_int, [_P, C.c_int32, _I32, _D, C.c_uint64, C.c_uint32, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                      _P, C.c_int64, _I32]),
    "abd_logp": (C.c_int, [_P, C.c_int32, _D, _D]),
    "abd_logp_dlogp": (C.c_int, [_P, C.c_int32, _D, _D, _D]),
    "abd_loglik_dlogp": (C.c_int, [_P, C.c_int32, _D, _D, _D]),
    "abd_logp_dlogp_batch": (C.c_int, [_P, C.c_int32, _I32, _D, _D, _D]),
    "abd_n_result_slots": (C.c_int, [_P]),
    "abd_logp_dlogp_batch_enqueue": (C.c_int, [_P, C.c_int32, C.c_int32, _I32, _D]),
    "abd_wait": (C.c_int, [_P]),
    "abd_fetch": (C.c_int, [_P, C.c_int32, _D, _D]),
    "abd_fetch_many": (C.c_int, [_P, C.c_int32, _I32, _D, _D]),
    "abd_logp_dlogp_many": (C.c_int, [_P, C.c_int32, C.c_int32, _I32, _D, _D, _D]),
    "abd_deterministics": (C.c_int, [_P, C.c_int32, _D, _I8, _D, _D]),
    "abd_curves": (C.c_int, [_P, C.c_int32, _D, C.c_double, C.c_double, _D, _D, _D]),
    "abd_set_follow_up": (C.c_int, [_P, _I32]),
    "abd_risk": (C.c_int, [_P, C.c_int32, _D, C.POINTER(_RiskSpec), _D]),
    "abd_pointwise_loglik": (C.c_int, [_P, C.c_int32, _D, _D, _D]),
    "abd_individual_loglik": (C.c_int, [_P, C.c_int32, _D, _D, _D]),
    "abd_posterior_predictive": (C.c_int, [_P, C.c_int32, _D, C.c_uint64, C.c_uint32, C.c_uint64, _D, _D, _D, _D]),
    "abd_simulate": (C.c_int, [_P, C.POINTER(_SimParams), _D, C.c_uint64, C.c_uint32, C.c_int32, _I8, _D, _D, _D, _D, _D]),
    "abd_simulate_staged": (C.c_int, [_P, C.POINTER(_SimParams), _D, C.c_uint64, C.c_uint32, C.c_int32, C.c_int64, _I8, _D, _D, _D, _D, _D]),
    "abd_sampler_create": (C.c_int, [_P, C.c_int32, _I32, _D, C.POINTER(_SamplerOpts), C.POINTER(_P)]),
    "abd_sampler_destroy": (None, [_P]),
    "abd_sampler_run": (C.c_int, [_P, C.c_int64, _D, _D]),
    "abd_sampler_run_record": (C.c_int, [_P, C.c_int64, _D, _D, C.POINTER(_Record)]),
    "abd_sampler_set_adaptation": (C.c_int, [_P, C.c_int32, _D, C.c_double]),
    "abd_sampler_means": (C.c_int, [_P, C.c_int32, _D, _D, _D, C.POINTER(C.c_int64)]),
    "abd_sampler_enable_pointwise": (C.c_int, [_P, C.c_int32]),
    "abd_sampler_pointwise_stats": (C.c_int, [_P, C.c_int32, _D, C.POINTER(C.c_int64)]),
    "abd_sampler_enable_individual_loglik": (C.c_int, [_P, C.c_int32]),
    "abd_sampler_individual_loglik_stats": (C.c_int, [_P, C.c_int32, _D, C.POINTER(C.c_int64), _D]),
    "abd_sampler_enable_predictive": (C.c_int, [_P, C.c_int32]),
    "abd_sampler_predictive_stats": (C.c_int, [_P, C.c_int32, _D, C.POINTER(C.c_int64)]),
    "abd_sampler_enable_curves": (C.c_int, [_P, C.c_int64, C.c_double, C.c_double]),
    "abd_sampler_curves": (C.c_int, [_P, C.c_int32, C.c_int64, C.c_int64, _D, _D, _D, C.POINTER(C.c_int64)]),
    "abd_sampler_enable_risk": (C.c_int, [_P, C.c_int64, C.POINTER(_RiskSpec)]),
    "abd_sampler_risk": (C.c_int, [_P, C.c_int32, C.c_int64, C.c_int64, _D, C.POINTER(C.c_int64)]),
    "abd_sampler_enable_loo": (C.c_int, [_P, C.c_int64, C.c_int32]),
    "abd_sampler_loo_rows": (C.c_int, [_P, C.c_int32, C.c_int64, C.c_int64, _D, C.POINTER(C.c_int64)]),
    "abd_sampler_loo_stats": (C.c_int, [_P, _D, _D, _D, _I32, C.POINTER(C.c_int64), _D]),
    "abd_sampler_enable_diagnostics": (C.c_int, [_P, C.c_int64, C.c_int64]),
    "abd_sampler_diagnostics": (C.c_int, [_P, C.c_int32, _D, _D, _D, _D]),
    "abd_sampler_enable_timelines": (C.c_int, [_P, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_double]),
    "abd_sampler_timelines": (C.c_int, [_P, C.c_int32, _D, _D, _D, _D, _D, C.POINTER(C.c_int64)]),
    "abd_sampler_timeline_quantiles": (C.c_int, [_P, C.c_int32, _D, _D, _D]),
    "abd_sampler_adaptation": (C.c_int, [_P, C.c_int32, _D, _D, _D]),
    "abd_sampler_enable_leapfrog_log": (C.c_int, [_P, C.c_int64]),
    "abd_sampler_leapfrog_log": (C.c_int, [_P, C.c_int32, C.c_int64, C.c_int64, _D, C.POINTER(C.c_int64)]),
    "abd_sampler_launch_shape": (C.c_int, [_P, _I32]),
    "abd_theta_prior": (C.c_int, [_P, _D, _D, _D]),
    "abd_set_individual_offset": (C.c_int, [_P, C.c_int64]),
    "abd_kernel_timing": (C.c_int, [_P, C.c_int32]),
    "abd_kernel_time": (C.c_int, [_P, _D, C.POINTER(C.c_int64), C.c_int32]),
    "abd_set_launch_config": (C.c_int, [_P, C.c_int32, C.c_int32]),
    "abd_algorithmic_bytes": (C.c_int64, [_P, C.c_int32]),
    "abd_wait_fallbacks": (C.c_int64, [_P]),
    "abd_stream_queues": (C.c_int, [_P, _I32, C.c_int32]),
    "abd_n_pipes": (C.c_int, [_P]),
    "abd_is_dense": (C.c_int, [_P]),
    "abd_survival_create": (C.c_int, [C.POINTER(_SurvivalDesc), C.POINTER(_P)]),
    "abd_survival_create_groups": (C.c_int, [C.POINTER(_SurvivalGroupsDesc), C.POINTER(_P)]),
    "abd_survival_create_periods": (C.c_int, [C.POINTER(_SurvivalPeriodsDesc), C.POINTER(_P)]),
    "abd_survival_destroy": (C.c_int, [_P]),
    "abd_survival_dim": (C.c_int32, [_P]),
    "abd_survival_logp_dlogp": (C.c_int, [_P, C.c_int32, _D, _D, _D]),
    "abd_survival_loglik_sums": (C.c_int, [_P, _D, _D]),
    "abd_survival_individual_loglik": (C.c_int, [_P, C.c_int32, _D, _D]),
    "abd_survival_waic_reset": (C.c_int, [_P]),
    "abd_survival_waic_accumulate": (C.c_int, [_P, C.c_int32, _D]),
    "abd_survival_waic_stats": (C.c_int, [_P, _D, _D, _D, C.POINTER(C.c_int64), _I32]),
    "abd_survival_loo_reserve": (C.c_int, [_P, C.c_int64]),
    "abd_survival_loo_reset": (C.c_int, [_P]),
    "abd_survival_loo_accumulate": (C.c_int, [_P, C.c_int32, _D]),
    "abd_survival_loo_append_rows": (C.c_int, [_P, C.c_int32, _D]),
    "abd_survival_loo_rows": (C.c_int, [_P, C.c_int64, C.c_int64, _D]),
    "abd_survival_loo_stats": (C.c_int, [_P, _D, _D, _D, _I32, C.POINTER(C.c_int64), _I32]),
    "abd_survival_predictive_configure": (C.c_int, [_P, C.c_int32, _P, _I32, _P, C.c_uint64]),
    "abd_survival_predictive_reset": (C.c_int, [_P]),
    "abd_survival_predictive_accumulate": (C.c_int, [_P, C.c_int32, _D, _D, _P]),
    "abd_survival_predictive_stats": (C.c_int, [_P, _D, _P, _P, C.POINTER(C.c_int64)]),
    "abd_survival_predictive_observed": (C.c_int, [_P, _D, _D, _P, _D]),
    "abd_survival_replicate": (C.c_int, [_P, C.c_int32, _D, C.c_int64, _I32]),
    "abd_survival_draws_create": (C.c_int, [C.POINTER(_SurvivalDrawsDesc), C.POINTER(_P)]),
    "abd_survival_draws_create_groups": (C.c_int, [C.POINTER(_SurvivalDrawsGroupsDesc), C.POINTER(_P)]),
    "abd_survival_draws_create_periods": (C.c_int, [C.POINTER(_SurvivalDrawsPeriodsDesc), C.POINTER(_P)]),
    "abd_survival_draws_destroy": (C.c_int, [_P]),
    "abd_survival_draws_dim": (C.c_int32, [_P]),
    "abd_survival_draws_logp_dlogp": (C.c_int, [_P, C.c_int32, _I32, _D, _D, _D]),
    "abd_survival_draws_loglik_sums": (C.c_int, [_P, C.c_int32, _D, _D]),
    "abd_survival_draws_individual_loglik": (C.c_int, [_P, C.c_int32, _I32, _D, _D]),
    "abd_survival_draws_waic_reset": (C.c_int, [_P]),
    "abd_survival_draws_waic_accumulate": (C.c_int, [_P, C.c_int32, _I32, _D]),
    "abd_survival_draws_waic_stats": (C.c_int, [_P, _D, _D, _D, _P, _I32]),  # n_draws is an array here: int64[M]
    "abd_survival_draws_loo_reserve": (C.c_int, [_P, C.c_int64]),
    "abd_survival_draws_loo_reset": (C.c_int, [_P]),
    "abd_survival_draws_loo_accumulate": (C.c_int, [_P, C.c_int32, _I32, _D]),
    "abd_survival_draws_loo_stats": (C.c_int, [_P, _D, _D, _D, _I32, _P]),
}

SURVIVAL_PREDICTIVE_BINS = 8  # ABD_SURV_PRED_BINS: bins of a binning variable (up to 7 edges)


def load():
    """Load the HIP library (once).  Raises ImportError loudly if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"abdpymc_amd: HIP library not found at {LIB_PATH}. Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950). "
            "There is no CPU fallback for the hot path."
        )
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the ABI lost a symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _err(lib) -> str:
    return lib.abd_last_error().decode("utf-8", "replace")


def _check(lib, rc: int):
    if rc == 0:
        return
    msg = _err(lib)
    if rc == -1:  # ABD_ERR_ARG -> the reference raises ValueError for the same conditions
        raise ValueError(msg)
    raise AbdError(f"[{rc}] {msg}")


def _as(arr, dtype):
    return np.ascontiguousarray(arr, dtype=dtype)


def _tptr(arr, ctype):
    """Typed ctypes pointer to an array's data (structure fields, typed out-parameters)."""
    return arr.ctypes.data_as(C.POINTER(ctype))


def _ptr(arr, ctype=None):
    """Address of a C-contiguous array's data (the array must stay referenced by the caller for the duration of the call).
    INPUT arguments only (the library reads through it): a read-only array is fine here."""
    try:
        return C.addressof(C.c_char.from_buffer(arr))  # 0.4 us; needs a writable, non-empty buffer
    except (TypeError, ValueError, BufferError):
        return arr.ctypes.data


def _theta(theta):
    """``theta`` as the (17,) float64 array one evaluation takes.  (``Context``'s timed evaluation methods check inline: a call
    costs them.)"""
    t = _as(theta, np.float64)
    if t.shape != (N_THETA,):
        raise ValueError(f"theta must have shape ({N_THETA},)")
    return t


def _out(arr, dtype, shape=None, name="output array"):
    """Address of an array the LIBRARY WRITES: it must be writeable, C-contiguous, of the exact dtype (ctypes sees only an
    address, so nothing else would catch a read-only memmap or a float32 buffer before the library writes through it)."""
    if not isinstance(arr, np.ndarray) or arr.dtype != dtype or not arr.flags.c_contiguous or not arr.flags.writeable:
        raise ValueError(f"{name} must be a writeable C-contiguous {np.dtype(dtype).name} ndarray")
    if shape is not None and arr.shape != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {arr.shape}")
    return _ptr(arr)


class Context:
    """
    Device-resident cohort + chain slots.  Mirrors what ``abd.model(data, splits, ignore_pcrpos)``
    closes over (reference abd.py:396-442).
    """

    def __init__(
        self,
        n_gaps: int,
        n_inds: int,
        s_obs,  # (idx_gap, idx_ind, log_dilution, od)
        n_obs,
        vacs,  # (N, G)
        pcrpos,  # (N, G) or None (= ignore_pcrpos)
        splits: Optional[Sequence[int]] = None,
        n_chains: int = 1,
        storage: str = "f64",
        device: int = -1,
    ):
        lib = load()
        self._lib = lib
        self._h = _P()
        self._samplers = weakref.WeakSet()  # destroyed before the context they point into
        self.n_gaps, self.n_inds, self.n_chains = int(n_gaps), int(n_inds), int(n_chains)
        d = _Desc()
        d.n_gaps, d.n_inds = self.n_gaps, self.n_inds
        splits = tuple(splits or ())
        if len(splits) > 2:
            raise NotImplementedError("only implemented 1-3 time chunks (0-2 splits)")
        d.n_splits = len(splits)
        for k, s in enumerate(splits):
            d.splits[k] = int(s)
        d.storage = {"f64": STORE_F64, "f32": STORE_F32}[storage]
        d.n_chain_slots = self.n_chains
        d.device = device
        keep = []

        def obs(o):
            g, j, x, y = o
            g, j = _as(g, np.int32), _as(j, np.int32)
            x, y = _as(x, np.float64), _as(y, np.float64)
            if not (g.shape == j.shape == x.shape == y.shape and g.ndim == 1):
                raise ValueError("observation arrays must be 1-D and of equal length")
            keep.extend([g, j, x, y])
            a = _AntigenObs()
            a.n_obs = g.size
            a.idx_gap, a.idx_ind = _tptr(g, C.c_int32), _tptr(j, C.c_int32)
            a.log_dilution, a.od = _tptr(x, C.c_double), _tptr(y, C.c_double)
            return a

        d.s, d.n = obs(s_obs), obs(n_obs)
        self.n_obs_s, self.n_obs_n = int(d.s.n_obs), int(d.n.n_obs)  # readings of it_s_lik / it_n_lik
        vacs = np.asarray(vacs)
        if vacs.shape != (self.n_inds, self.n_gaps):
            raise ValueError(f"vacs shape {vacs.shape} != (n_inds, n_gaps) = {(self.n_inds, self.n_gaps)}")
        v8 = _as(vacs, np.int8)
        if not np.array_equal(v8, vacs):
            raise ValueError("vacs must be 0/1")
        keep.append(v8)
        d.vacs = _tptr(v8, C.c_int8)
        if pcrpos is not None:
            pcrpos = np.asarray(pcrpos)
            if vacs.shape != pcrpos.shape:
                raise ValueError("vacs and pcrpos are different shapes")  # abd.py:196-197
            p8 = _as(pcrpos, np.int8)
            if not np.array_equal(p8, pcrpos):
                raise ValueError("pcrpos must be 0/1")
            keep.append(p8)
            d.pcrpos = _tptr(p8, C.c_int8)
        _check(lib, lib.abd_create(C.byref(d), C.byref(self._h)))
        self.n_result_slots = lib.abd_n_result_slots(self._h)
        # one counter per chain slot, bumped by everything that rewrites the slot's device-side discrete state
        # (set_discrete, flip_discrete, gibbs_sweep, the native sampler): host mirrors of that state (DiscreteMirror)
        # are only trusted while the counter stands where they left it
        self._generation = [0] * self.n_chains

    # -- lifetime ---------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            for smp in list(self._samplers):
                smp.close()
            self._lib.abd_destroy(self._h)
            self._h = _P()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- info -------------------------------------------------------------------------------
    @property
    def device_name(self) -> str:
        buf = C.create_string_buffer(256)
        _check(self._lib, self._lib.abd_device_name(self._h, buf, 256))
        return buf.value.decode()

    @property
    def is_dense(self) -> bool:
        return bool(self._lib.abd_is_dense(self._h))

    @property
    def n_pipes(self) -> int:
        """HIP streams that stream-ordered dense launches rotate over."""
        return int(self._lib.abd_n_pipes(self._h))

    @property
    def wait_fallbacks(self) -> int:
        """Synchronous calls that had to fall back from the polled completion tag to a stream synchronise (expect 0)."""
        return int(self._lib.abd_wait_fallbacks(self._h))

    def stream_queues(self):
        """Hardware queue of each of the context's 8 HIP streams (streams with the same number serialise their kernels)."""
        q = (C.c_int32 * 8)()
        _check(self._lib, self._lib.abd_stream_queues(self._h, q, 8))
        return list(q)

    def algorithmic_bytes(self, n_chains: int) -> int:
        return int(self._lib.abd_algorithmic_bytes(self._h, n_chains))

    # -- discrete state -----------------------------------------------------------------------
    def generation(self, chain: int) -> int:
        """Changes every time the slot's device-side (i_raw, ab_s_waner) is rewritten by anyone."""
        return self._generation[int(chain)]

    def _bump(self, chains):
        for c in np.atleast_1d(chains):
            self._generation[int(c)] += 1

    def set_discrete(self, chain: int, i_raw, waner):
        i_raw, waner = np.asarray(i_raw), np.asarray(waner)
        if i_raw.shape != (self.n_gaps, self.n_inds):
            raise ValueError(f"i_raw shape {i_raw.shape} != (n_gaps, n_inds) = {(self.n_gaps, self.n_inds)}")
        if waner.shape != (self.n_inds,):
            raise ValueError(f"ab_s_waner shape {waner.shape} != ({self.n_inds},)")
        i8, w8 = _as(i_raw, np.int8), _as(waner, np.int8)
        if not (np.array_equal(i8, i_raw) and np.array_equal(w8, waner)):
            raise ValueError("i_raw / ab_s_waner must be 0/1")
        _check(self._lib, self._lib.abd_set_discrete(self._h, chain, _ptr(i8, C.c_int8), _ptr(w8, C.c_int8)))
        self._bump(chain)

    def flip_discrete(self, chain: int, flat: int):
        _check(self._lib, self._lib.abd_flip_discrete(self._h, chain, int(flat)))
        self._bump(chain)

    def get_discrete(self, chain: int):
        i = np.empty((self.n_gaps, self.n_inds), dtype=np.int8)
        w = np.empty(self.n_inds, dtype=np.int8)
        _check(self._lib, self._lib.abd_get_discrete(self._h, chain, _ptr(i, C.c_int8), _ptr(w, C.c_int8)))
        return i, w

    def gibbs_sweep(self, chains, theta, seed: int, sweep: int, log: bool = False):
        """One binary Gibbs-Metropolis sweep of each chain's [i_raw, ab_s_waner] in place -> (accepted, proposed).
        ``log=True`` (tests; the same decisions from a logging instantiation of the kernel) -> (accepted, proposed, records,
        n_records): ``records`` a GIBBS_RECORD array (chains, n_inds, n_gaps + 1) -- what the kernel decided each proposal
        of an individual with, in the individual's order, ``abd_gibbs_record`` of include/abd_hip.h -- of which the first
        ``n_records[chain, individual]`` are filled."""
        ch = _as(np.atleast_1d(chains), np.int32)
        t = _as(np.atleast_2d(theta), np.float64)
        if t.shape != (ch.size, N_THETA):
            raise ValueError(f"theta must have shape ({ch.size}, {N_THETA})")
        acc = np.zeros(ch.size, dtype=np.int64)
        prop = np.zeros(ch.size, dtype=np.int64)
        self._bump(ch)
        head = (self._h, ch.size, _ptr(ch, C.c_int32), _ptr(t, C.c_double), C.c_uint64(seed & (2**64 - 1)),
                C.c_uint32(sweep & 0xFFFFFFFF), _tptr(acc, C.c_int64), _tptr(prop, C.c_int64))
        if not log:
            _check(self._lib, self._lib.abd_gibbs_sweep(*head))
            return acc, prop
        rec = np.zeros((ch.size, self.n_inds, self.n_gaps + 1), dtype=GIBBS_RECORD)
        n_rec = np.zeros((ch.size, self.n_inds), dtype=np.int32)
        _check(self._lib, self._lib.abd_gibbs_sweep_log(*head, _out(rec, GIBBS_RECORD), self.n_inds * (self.n_gaps + 1),
                                                        _out(n_rec, np.int32)))
        return acc, prop, rec, n_rec

    # -- evaluations ------------------------------------------------------------------------
    def logp(self, chain: int, theta) -> float:
        t = _as(theta, np.float64)
        if t.shape != (N_THETA,):
            raise ValueError(f"theta must have shape ({N_THETA},)")
        out = C.c_double()
        _check(self._lib, self._lib.abd_logp(self._h, chain, _ptr(t, C.c_double), C.byref(out)))
        return out.value

    def logp_dlogp(self, chain: int, theta):
        t = _as(theta, np.float64)
        if t.shape != (N_THETA,):
            raise ValueError(f"theta must have shape ({N_THETA},)")
        out = C.c_double()
        g = np.empty(N_THETA)
        _check(self._lib, self._lib.abd_logp_dlogp(self._h, chain, _ptr(t, C.c_double), C.byref(out), _ptr(g, C.c_double)))
        return out.value, g

    def loglik_dlogp(self, chain: int, theta):
        """Data term only (the two observed Normals) and its gradient w.r.t. theta."""
        t = _as(theta, np.float64)
        if t.shape != (N_THETA,):
            raise ValueError(f"theta must have shape ({N_THETA},)")
        out = C.c_double()
        g = np.empty(N_THETA)
        _check(self._lib, self._lib.abd_loglik_dlogp(self._h, chain, _ptr(t, C.c_double), C.byref(out), _ptr(g, C.c_double)))
        return out.value, g

    def logp_dlogp_batch(self, chains, theta):
        ch = _as(chains, np.int32)
        t = _as(theta, np.float64)
        if t.shape != (ch.size, N_THETA):
            raise ValueError(f"theta must have shape ({ch.size}, {N_THETA})")
        lp = np.empty(ch.size)
        g = np.empty((ch.size, N_THETA))
        _check(
            self._lib,
            self._lib.abd_logp_dlogp_batch(
                self._h, ch.size, _ptr(ch, C.c_int32), _ptr(t, C.c_double), _ptr(lp, C.c_double), _ptr(g, C.c_double)
            ),
        )
        return lp, g

    def enqueue(self, slot: int, chains, theta):
        ch = _as(chains, np.int32)
        t = _as(theta, np.float64)
        if t.shape != (ch.size, N_THETA):
            raise ValueError(f"theta must have shape ({ch.size}, {N_THETA})")
        _check(
            self._lib,
            self._lib.abd_logp_dlogp_batch_enqueue(self._h, slot, ch.size, _ptr(ch, C.c_int32), _ptr(t, C.c_double)),
        )

    def wait(self):
        _check(self._lib, self._lib.abd_wait(self._h))

    def fetch(self, slot: int, n: int):
        lp = np.empty(n)
        g = np.empty((n, N_THETA))
        _check(self._lib, self._lib.abd_fetch(self._h, slot, _ptr(lp, C.c_double), _ptr(g, C.c_double)))
        return lp, g

    def fetch_many(self, slots, n_per_slot: int, out_lp=None, out_g=None):
        """fetch() for several slots at once -> (len(slots), n_per_slot) logp and (len(slots), n_per_slot, 17) grad;
        ``out_lp`` / ``out_g``: C-contiguous float64 arrays of those shapes to write into instead of new ones."""
        sl = _as(slots, np.int32)
        lp = np.empty((sl.size, n_per_slot)) if out_lp is None else out_lp
        g = np.empty((sl.size, n_per_slot, N_THETA)) if out_g is None else out_g
        _check(self._lib, self._lib.abd_fetch_many(self._h, sl.size, _ptr(sl, C.c_int32),
                                                   _out(lp, np.float64, (sl.size, n_per_slot), "out_lp"),
                                                   _out(g, np.float64, (sl.size, n_per_slot, N_THETA), "out_g")))
        return lp, g

    def logp_dlogp_many(self, chains, thetas, out_lp=None, out_g=None):
        """``thetas`` (K, n, 17): K independent evaluations of the same n chains, stream-ordered inside the library
        (enqueue all, wait once, fetch) -> logp (K, n), grad (K, n, 17); ``out_lp`` / ``out_g`` to write into."""
        ch = _as(chains, np.int32)
        t = _as(thetas, np.float64)
        if t.ndim != 3 or t.shape[1:] != (ch.size, N_THETA):
            raise ValueError(f"thetas must have shape (K, {ch.size}, {N_THETA})")
        K = t.shape[0]
        lp = np.empty((K, ch.size)) if out_lp is None else out_lp
        g = np.empty((K, ch.size, N_THETA)) if out_g is None else out_g
        _check(self._lib, self._lib.abd_logp_dlogp_many(self._h, K, ch.size, _ptr(ch, C.c_int32), _ptr(t, C.c_double),
                                                        _out(lp, np.float64, (K, ch.size), "out_lp"),
                                                        _out(g, np.float64, (K, ch.size, N_THETA), "out_g")))
        return lp, g

    def deterministics(self, chain: int, theta):
        t = _as(theta, np.float64)
        G, N = self.n_gaps, self.n_inds
        i = np.empty((G, N), dtype=np.int8)
        mun = np.empty((G, N))
        mus = np.empty((G, N))
        _check(
            self._lib,
            self._lib.abd_deterministics(
                self._h, chain, _ptr(t, C.c_double), _ptr(i, C.c_int8), _ptr(mun, C.c_double), _ptr(mus, C.c_double)
            ),
        )
        return i, mun, mus

    def set_follow_up(self, last_gap=None):
        """End of follow-up per individual for the curves: ``last_gap`` is (N,) with -1 <= v < G (-1: never followed);
        ``None``: everyone to the last gap.  ``ValueError`` for a value outside."""
        if last_gap is None:
            _check(self._lib, self._lib.abd_set_follow_up(self._h, None))
            return
        lg = np.asarray(last_gap)
        if lg.shape != (self.n_inds,) or not np.issubdtype(lg.dtype, np.integer):
            raise ValueError(f"last_gap must be an integer array of shape ({self.n_inds},)")
        if lg.size and (lg.min() < -1 or lg.max() >= self.n_gaps):  # (before the cast to int32 could wrap a value round)
            raise ValueError(f"last_gap outside [-1, {self.n_gaps})")
        lg = _as(lg, np.int32)
        _check(self._lib, self._lib.abd_set_follow_up(self._h, _ptr(lg, C.c_int32)))

    def curves(self, chain: int, theta, thr_s: float = np.inf, thr_n: float = np.inf):
        """The epidemic curves of (theta, the chain slot's discrete state), reduced over the individuals on the device ->
        {"counts": (4, G) int64 -- infected, ever_infected, seropos_s, seropos_n --, "n_infections": (8,) int64,
        "titer_sums": (2, G) -- ab_s_mu, ab_n_mu}: ``curves.from_deterministics`` of ``deterministics(chain, theta)`` under
        the context's follow-up (``set_follow_up``)."""
        t = _theta(theta)
        G = self.n_gaps
        counts, n_inf, sums = np.empty((4, G), np.int64), np.empty(8, np.int64), np.empty((2, G))
        _check(self._lib, self._lib.abd_curves(self._h, int(chain), _ptr(t, C.c_double), float(thr_s), float(thr_n),
                                               _out(counts, np.int64), _out(n_inf, np.int64), _out(sums, np.float64)))
        return {"counts": counts, "n_infections": n_inf, "titer_sums": sums}

    def risk(self, chain: int, theta, spec):
        """The infection-risk-by-titer table of (theta, the chain slot's discrete state), reduced over the individuals on the
        device -> (2, 2, G, 8) int64, antigen (S, N) x (at risk, events) x gap x bin: ``risk.from_deterministics`` of
        ``deterministics(chain, theta)`` under the context's follow-up (``set_follow_up``) and ``spec`` (``risk.spec``)."""
        t = _theta(theta)
        sp = _risk_spec(spec)
        table = np.empty((2, 2, self.n_gaps, 8), np.int64)
        _check(self._lib, self._lib.abd_risk(self._h, int(chain), _ptr(t, C.c_double), C.byref(sp), _out(table, np.int64)))
        return table

    def pointwise_loglik(self, chain: int, theta):
        """Log-density of every OD reading at (theta, the chain slot's discrete state) -> (ll_s, ll_n), each in the order the
        readings were given (what ``pm.compute_log_likelihood`` records per draw for ``it_s_lik`` / ``it_n_lik``)."""
        t = _theta(theta)
        ll_s, ll_n = np.empty(self.n_obs_s), np.empty(self.n_obs_n)
        _check(self._lib, self._lib.abd_pointwise_loglik(self._h, int(chain), _ptr(t, C.c_double), _ptr(ll_s, C.c_double),
                                                         _ptr(ll_n, C.c_double)))
        return ll_s, ll_n

    def individual_loglik(self, chain: int, theta):
        """Per individual, the sum of ``pointwise_loglik`` over its S readings and over its N readings at (theta, the chain
        slot's discrete state) -> (ll_s, ll_n), each (n_inds,); 0 where the individual has no reading of that antigen.  Summed
        on the device in a fixed order: the same state gives the same bits."""
        t = _theta(theta)
        ll_s, ll_n = np.empty(self.n_inds), np.empty(self.n_inds)
        _check(self._lib, self._lib.abd_individual_loglik(self._h, int(chain), _ptr(t, C.c_double), _ptr(ll_s, C.c_double),
                                                          _ptr(ll_n, C.c_double)))
        return ll_s, ll_n

    def posterior_predictive(self, chain: int, theta, seed: int = 0, stream: int = 0, draw: int = 0, mean: bool = False):
        """Posterior predictive replicate of every OD reading at (theta, the chain slot's discrete state) -> (yrep_s, yrep_n),
        each in the order the readings were given; ``mean=True`` adds the noise-free means (m_s, m_n).  The normals are keyed
        by (seed, stream, draw) and the reading (abd_hip.h: abd_posterior_predictive): the native sampler's recorded replicate
        of chain c at iteration t is ``posterior_predictive(.., seed, chain_offset + c, t)``."""
        t = _theta(theta)
        y_s, y_n = np.empty(self.n_obs_s), np.empty(self.n_obs_n)
        m_s, m_n = (np.empty(self.n_obs_s), np.empty(self.n_obs_n)) if mean else (None, None)
        _check(self._lib, self._lib.abd_posterior_predictive(
            self._h, int(chain), _ptr(t, C.c_double), C.c_uint64(int(seed) & (2**64 - 1)), C.c_uint32(int(stream) & 0xFFFFFFFF),
            C.c_uint64(int(draw) & (2**64 - 1)), _ptr(y_s, C.c_double), _ptr(y_n, C.c_double),
            None if m_s is None else _ptr(m_s, C.c_double), None if m_n is None else _ptr(m_n, C.c_double)))
        return (y_s, y_n, m_s, m_n) if mean else (y_s, y_n)

    def simulate(self, params, lam0, seed: int = 0, first_replicate: int = 0, n_replicates: int = 1, outputs=SIM_OUTPUTS,
                 staging_bytes: Optional[int] = None):
        """Replicates ``first_replicate .. first_replicate + n_replicates - 1`` of the forward simulation of this cohort
        (abd_hip.h: abd_simulate) at ``lam0`` (n_gaps infection probabilities).  ``params``: {"s": {...}, "n": {...}} with the
        ten fields of ``abd_sim_antibody`` each.  -> dict of the ``outputs`` asked for (any of ``SIM_OUTPUTS``):
        infections (R, n_inds, n_gaps) int8, s_titer / n_titer (R, n_inds, n_gaps), od_s / od_n (R, n_obs) in the order the
        readings were given, n_infected (R, n_gaps) int64.  A replicate depends on (seed, its number) only.
        ``staging_bytes``: device memory one chunk of replicates may occupy in this call (None: the library's default)."""
        lam = _as(lam0, np.float64)
        if lam.ndim != 1:
            raise ValueError("lam0 should be 1D")
        if lam.shape[0] != self.n_gaps:
            raise ValueError("must have single infection rate for each time gap")
        outputs = tuple(outputs)
        unknown = [o for o in outputs if o not in SIM_OUTPUTS]
        if unknown:
            raise ValueError(f"unknown outputs {unknown}: choose from {SIM_OUTPUTS}")
        p = _SimParams()
        for ag in ("s", "n"):
            for name, _ in _SimAntibody._fields_:
                setattr(getattr(p, ag), name, float(params[ag][name]))
        R = int(n_replicates)
        if R < 1:
            raise ValueError(f"n_replicates must be >= 1, got {R}")
        if not (0 <= int(first_replicate) and int(first_replicate) + R <= 2 ** 32):
            raise ValueError(f"first_replicate + n_replicates = {int(first_replicate) + R} exceeds 2^32")
        G, N = self.n_gaps, self.n_inds
        shapes = {"infections": ((R, N, G), np.int8), "s_titer": ((R, N, G), np.float64), "n_titer": ((R, N, G), np.float64),
                  "od_s": ((R, self.n_obs_s), np.float64), "od_n": ((R, self.n_obs_n), np.float64),
                  "n_infected": ((R, G), np.int64)}
        out = {name: np.zeros(*shapes[name]) for name in SIM_OUTPUTS if name in outputs}
        ptrs = [_ptr(out[name]) if name in out and out[name].size else None for name in SIM_OUTPUTS]
        _check(self._lib, self._lib.abd_simulate_staged(self._h, C.byref(p), _ptr(lam), C.c_uint64(int(seed) & (2 ** 64 - 1)),
                                                        C.c_uint32(int(first_replicate)), R, int(staging_bytes or 0), *ptrs))
        return out

    def theta_prior(self, theta):
        """The theta-only part of the joint logp (continuous priors + Jacobians) and its gradient."""
        t = _theta(theta)
        out = C.c_double()
        g = np.empty(N_THETA)
        _check(self._lib, self._lib.abd_theta_prior(self._h, _ptr(t, C.c_double), C.byref(out), _ptr(g, C.c_double)))
        return out.value, g

    def set_individual_offset(self, first_individual: int):
        _check(self._lib, self._lib.abd_set_individual_offset(self._h, int(first_individual)))

    def sampler(self, chains, theta0, tune: int, seed: int = 0, target_accept: float = 0.8, max_treedepth: int = 10,
                gibbs: bool = True, accumulate: bool = False, chain_offset: int = 0,
                dense_metric: bool = False, pointwise: bool = False, predictive: bool = False, curves: int = 0,
                sero_thresholds=None, diagnostics=None, risk: int = 0, risk_spec=None, timelines=None) -> "NativeSampler":
        """The compound step [NUTS; Gibbs sweep] for several chains, driven inside the library: the chains advance as
        independent units on their own HIP streams (abd_hip.h: abd_sampler_create).  The summary keywords map onto
        ``NativeSampler``'s ``enable_*`` methods, which say what each keeps: ``pointwise`` / ``predictive``: on or off;
        ``curves`` / ``risk``: the draws per chain to keep (0: off), with ``sero_thresholds`` / ``risk_spec``; ``diagnostics`` = (D,
        L) and ``timelines`` = (D, (lo_n, hi_n), (lo_s, hi_s)) for D planned draws (``None``: off)."""
        if int(curves) < 0:
            raise ValueError(f"curves must be a number of draws >= 0, got {curves}")
        if int(risk) < 0:
            raise ValueError(f"risk must be a number of draws >= 0, got {risk}")
        if int(risk) and risk_spec is None:
            raise ValueError("risk needs a risk_spec (risk.spec)")
        smp = NativeSampler(self, chains, theta0, tune=tune, seed=seed, target_accept=target_accept, max_treedepth=max_treedepth,
                            gibbs=gibbs, accumulate=accumulate, chain_offset=chain_offset, dense_metric=dense_metric)
        if pointwise:
            smp.enable_pointwise()
        if predictive:
            smp.enable_predictive()
        if int(curves):
            smp.enable_curves(curves, sero_thresholds)
        if diagnostics is not None:
            smp.enable_diagnostics(*diagnostics)
        if int(risk):
            smp.enable_risk(risk, risk_spec)
        if timelines is not None:
            smp.enable_timelines(*timelines)
        return smp

    # -- measurement --------------------------------------------------------------------------
    def kernel_timing(self, mode):
        """0/False off; 1/True HIP events per launch, launches serialised (isolated kernel); 2 per window of
        stream-ordered launches in their real launch shape."""
        _check(self._lib, self._lib.abd_kernel_timing(self._h, int(mode)))

    def set_launch_config(self, blocks: int = 0, chains_per_wave: int = 0):
        _check(self._lib, self._lib.abd_set_launch_config(self._h, int(blocks), int(chains_per_wave)))

    def kernel_time(self, reset: bool = True):
        ms = C.c_double()
        n = C.c_int64()
        _check(self._lib, self._lib.abd_kernel_time(self._h, C.byref(ms), C.byref(n), int(reset)))
        return ms.value, n.value


class DiscreteMirror:
    """
    Host mirror of ONE chain slot's device-side ``(i_raw, ab_s_waner)``, for callers that are handed the whole
    discrete state on every call (``Model.compile_logp()``'s point function under BinaryGibbsMetropolis, a PyTensor
    ``Op.perform``): ``update`` uploads only what changed -- nothing, a few ``abd_flip_discrete`` calls, or the whole
    panel.  The mirror is trusted only while the slot's generation counter (``Context.generation``) stands where
    this mirror left it: anything else that rewrites the slot (another callable's ``set_discrete``, a device Gibbs
    sweep, the native sampler) bumps the counter and the next ``update`` re-uploads.
    """

    MAX_FLIPS = 8

    def __init__(self, ctx: "Context", chain: int = 0):
        self.ctx, self.chain = ctx, int(chain)
        self._state = None
        self._gen = None
        self.uploads = self.flips = self.hits = 0  # what update() did so far (tests, profiling)

    def invalidate(self):
        self._state = None

    def adopt(self, i_raw, waner):
        """The device holds exactly this state now (e.g. it was just read back after a device sweep): remember it under
        the slot's current generation without uploading anything."""
        i_raw, waner = np.asarray(i_raw), np.asarray(waner)
        self._state = (i_raw.copy(), waner.copy(), i_raw, waner)
        self._gen = self.ctx.generation(self.chain)

    def update(self, i_raw, waner):
        ctx, c = self.ctx, self.chain
        i_raw, waner = np.asarray(i_raw), np.asarray(waner)
        prev = self._state
        if prev is not None and self._gen == ctx.generation(c) and prev[0].shape == i_raw.shape and prev[1].shape == waner.shape:
            if i_raw is prev[2] and waner is prev[3] and not (i_raw.flags.writeable or waner.flags.writeable):
                self.hits += 1  # the very same read-only arrays: nothing can have changed
                return
            di = np.flatnonzero(i_raw.ravel() != prev[0].ravel())
            dw = np.flatnonzero(waner != prev[1])
            if di.size + dw.size == 0:
                self.hits += 1
                return
            if di.size + dw.size <= self.MAX_FLIPS:
                for f in di:
                    ctx.flip_discrete(c, int(f))
                for f in dw:
                    ctx.flip_discrete(c, int(i_raw.size + f))
                self.flips += int(di.size + dw.size)
                self._state = (i_raw.copy(), waner.copy(), i_raw, waner)
                self._gen = ctx.generation(c)
                return
        ctx.set_discrete(c, i_raw, waner)
        self.uploads += 1
        self._state = (i_raw.copy(), waner.copy(), i_raw, waner)
        self._gen = ctx.generation(c)


class NativeSampler:
    """``abd_sampler_*``: what ``pm.sample`` runs for this model (abd.py:921-922): independent chains, one evaluation launch
    per leapfrog of a unit of 1-4 chains, leapfrog trains (abd_hip.h)."""

    def __init__(self, ctx: Context, chains, theta0, tune, seed=0, target_accept=0.8, max_treedepth=10, gibbs=True,
                 accumulate=False, chain_offset=0, dense_metric=False):
        self._ctx = ctx  # keeps the context alive
        self._lib = ctx._lib
        self._h = _P()
        ch = _as(np.atleast_1d(chains), np.int32)
        t0 = _as(np.atleast_2d(theta0), np.float64)
        if t0.shape != (ch.size, N_THETA):
            raise ValueError(f"theta0 must have shape ({ch.size}, {N_THETA})")
        self.n = int(ch.size)
        self.n_obs = (ctx.n_obs_s, ctx.n_obs_n)  # readings of it_s_lik / it_n_lik
        self._chains = ch.copy()
        o = _SamplerOpts()
        o.tune, o.seed = int(tune), int(seed) & (2**64 - 1)
        o.target_accept, o.max_treedepth = float(target_accept), int(max_treedepth)
        o.gibbs, o.accumulate = int(bool(gibbs)), int(bool(accumulate))
        o.chain_offset = int(chain_offset)
        o.dense_metric = int(bool(dense_metric))
        _check(self._lib, self._lib.abd_sampler_create(ctx._h, self.n, _ptr(ch, C.c_int32), _ptr(t0, C.c_double), C.byref(o),
                                                       C.byref(self._h)))
        ctx._samplers.add(self)

    # -- the per-draw summaries: switched on before the first draw, read out by the method named -----------------------------
    def enable_pointwise(self):
        """Accumulate the pointwise log-likelihood statistics of every draw on the device (``pointwise_stats``)."""
        _check(self._lib, self._lib.abd_sampler_enable_pointwise(self._h, 1))

    def enable_individual_loglik(self):
        """Accumulate the statistics of every individual's joint log-likelihood over every draw on the device
        (``individual_loglik_stats``)."""
        _check(self._lib, self._lib.abd_sampler_enable_individual_loglik(self._h, 1))

    def enable_predictive(self):
        """Accumulate the posterior predictive check statistics of every draw on the device (``predictive_stats``)."""
        _check(self._lib, self._lib.abd_sampler_enable_predictive(self._h, 1))

    def enable_curves(self, draws: int, sero_thresholds=None):
        """Keep the epidemic curves of ``draws`` draws per chain on the device (``curves``), seropositive at ``sero_thresholds`` =
        (thr_s, thr_n) on the titer scale (``None``: off)."""
        thr_s, thr_n = (np.inf, np.inf) if sero_thresholds is None else sero_thresholds
        _check(self._lib, self._lib.abd_sampler_enable_curves(self._h, int(draws), float(thr_s), float(thr_n)))

    def enable_diagnostics(self, planned: int, batch: int):
        """Accumulate per cell what split R-hat and a batch-means ESS need over the ``planned`` draws, in batches of ``batch``
        (``diagnostics``)."""
        _check(self._lib, self._lib.abd_sampler_enable_diagnostics(self._h, int(planned), int(batch)))

    def enable_risk(self, draws: int, spec):
        """Keep the infection-risk-by-titer table of ``draws`` draws per chain on the device, counted under ``spec`` (``risk.spec``;
        ``risk``)."""
        sp = _risk_spec(spec)
        _check(self._lib, self._lib.abd_sampler_enable_risk(self._h, int(draws), C.byref(sp)))

    def enable_timelines(self, planned: int, range_n, range_s):
        """Accumulate per cell the titer histograms over ``range_n`` = (lo_n, hi_n) and ``range_s`` and the infection timing counters
        over the ``planned`` draws (``timelines`` / ``timeline_quantiles``)."""
        (lo_n, hi_n), (lo_s, hi_s) = range_n, range_s
        _check(self._lib, self._lib.abd_sampler_enable_timelines(self._h, int(planned), float(lo_n), float(hi_n), float(lo_s),
                                                                 float(hi_s)))

    def enable_loo(self, draws: int, thin: int = 1):
        """Keep every individual's joint log-likelihood T_j of draws 0, ``thin``, 2 ``thin``, ... of the ``draws`` per chain on the
        device for PSIS-LOO by individual (``loo_rows`` / ``loo_stats``); ``draws`` = 0 releases."""
        _check(self._lib, self._lib.abd_sampler_enable_loo(self._h, int(draws), int(thin)))

    def run(self, n_iter: int):
        """Advance all chains by n_iter iterations -> theta (n, n_iter, 17), stats {name: (n, n_iter)}."""
        return self.run_record(n_iter, 0)

    def run_record(self, n_iter: int, first: int, i_raw=None, ab_s_waner=None, i=None, ab_n_mu=None, ab_s_mu=None, thin: int = 1,
                   ll_s=None, ll_n=None, yrep_s=None, yrep_n=None):
        """
        run() that also writes every iteration's discrete state / Deterministics of every chain into the given
        C-contiguous arrays of shape (n, capacity, G, N) (int8 for i_raw and i, float64 for the two mu) and
        (n, capacity, N) int8 for ab_s_waner, at draws first .. first + n_iter - 1; ``ll_s`` / ``ll_n`` (n, capacity, K)
        float64 receive the pointwise log-likelihood of the readings (``Context.pointwise_loglik``), ``yrep_s`` / ``yrep_n`` their
        posterior predictive replicates (``Context.posterior_predictive`` keyed by the sampler's seed, the chain's global id and
        the iteration).  thin = K > 1: only iterations
        0, K, 2K, ... of the call are written, at draws first, first + 1, ... (ceil(n_iter / K) of them).
        """
        if thin < 1:
            raise ValueError(f"thin must be >= 1, got {thin}")
        G, N = self._ctx.n_gaps, self._ctx.n_inds
        rec = _Record()
        cap = None
        for name, arr, dt, tail in (("i_raw", i_raw, np.int8, (G, N)), ("ab_s_waner", ab_s_waner, np.int8, (N,)),
                                    ("i", i, np.int8, (G, N)), ("ab_n_mu", ab_n_mu, np.float64, (G, N)),
                                    ("ab_s_mu", ab_s_mu, np.float64, (G, N)),
                                    ("ll_s", ll_s, np.float64, (self._ctx.n_obs_s,)),
                                    ("ll_n", ll_n, np.float64, (self._ctx.n_obs_n,)),
                                    ("yrep_s", yrep_s, np.float64, (self._ctx.n_obs_s,)),
                                    ("yrep_n", yrep_n, np.float64, (self._ctx.n_obs_n,))):
            if arr is None:
                continue
            if arr.dtype != dt or not arr.flags.c_contiguous or not arr.flags.writeable or arr.shape[0] != self.n or arr.shape[2:] != tail:
                raise ValueError(f"{name}: need a writeable C-contiguous {np.dtype(dt).name} array of shape (n, capacity) + {tail}")
            if cap is not None and arr.shape[1] != cap:
                raise ValueError("record arrays differ in capacity")
            cap = arr.shape[1]
            setattr(rec, name, _tptr(arr, C.c_int8 if dt == np.int8 else C.c_double))
        rec.capacity, rec.first, rec.thin = int(cap or 0), int(first), int(thin)
        theta = np.empty((self.n, n_iter, N_THETA))
        stats = np.empty((self.n, n_iter, N_STATS))
        self._ctx._bump(self._chains)  # the sweeps rewrite the chains' discrete state
        _check(self._lib, self._lib.abd_sampler_run_record(self._h, int(n_iter), _ptr(theta, C.c_double), _ptr(stats, C.c_double),
                                                           None if cap is None else C.byref(rec)))  # (no array: abd_sampler_run)
        return theta, {name: stats[:, :, k].copy() for k, name in enumerate(STAT_NAMES)}

    def means(self, k: int):
        """Posterior means of i, ab_n_mu, ab_s_mu of the k-th chain over the accumulated draws, and their count."""
        G, N = self._ctx.n_gaps, self._ctx.n_inds
        out = [np.empty((G, N)) for _ in range(3)]
        n = C.c_int64()
        _check(self._lib, self._lib.abd_sampler_means(self._h, int(k), *[_ptr(o, C.c_double) for o in out], C.byref(n)))
        return out[0], out[1], out[2], n.value

    def _reading_stats(self, fn, k: int):
        out = np.empty((3, self._ctx.n_obs_s + self._ctx.n_obs_n))
        n = C.c_int64()
        _check(self._lib, fn(self._h, int(k), _ptr(out, C.c_double), C.byref(n)))
        return out, n.value

    def pointwise_stats(self, k: int):
        """Pointwise log-likelihood statistics of the k-th chain over its draws -> (out, n_draws): out is (3, K_s + K_n), S
        readings then N in the caller's order; rows log sum exp(ll), mean(ll), sum of squared deviations (compare.merge)."""
        return self._reading_stats(self._lib.abd_sampler_pointwise_stats, k)

    def individual_loglik_stats(self, k: int):
        """Statistics of every individual's joint log-likelihood T_j (``Context.individual_loglik``: ll_s + ll_n) of the k-th
        chain over its draws -> (out, n_draws, n_readings): out is (3, n_inds), rows as ``pointwise_stats``; n_readings
        (n_inds,) int64, the individual's readings of both antigens."""
        N = self._ctx.n_inds
        out, n_readings = np.empty((3, N)), np.empty(N, np.int64)
        n = C.c_int64()
        _check(self._lib, self._lib.abd_sampler_individual_loglik_stats(self._h, int(k), _ptr(out, C.c_double), C.byref(n),
                                                                        _out(n_readings, np.int64)))
        return out, n.value, n_readings

    def predictive_stats(self, k: int):
        """Posterior predictive check statistics of the k-th chain over its draws -> (out, n_draws): out is (3, K_s + K_n), S
        readings then N in the caller's order; rows mean and sum of squared deviations of the predictive mean, mean tail
        probability P(y_rep <= y) (predictive.merge)."""
        return self._reading_stats(self._lib.abd_sampler_predictive_stats, k)

    def _kept_draws(self, fn, k: int, *tails):
        """What a summary kept of every draw of the k-th chain so far: ``fn`` is asked for their number d, then for draws [0, d)
        into one new array of shape (d,) + tail per (tail, dtype) of ``tails``."""
        n = C.c_int64()
        _check(self._lib, fn(self._h, int(k), 0, 0, *[None] * len(tails), C.byref(n)))
        out = [np.empty((n.value,) + tail, dt) for tail, dt in tails]
        if n.value:
            _check(self._lib, fn(self._h, int(k), 0, n.value, *[_out(o, o.dtype) for o in out], None))
        return out

    def curves(self, k: int):
        """The epidemic curves of every draw of the k-th chain so far (``Context.curves`` per draw) -> {"counts": (draws, 4, G)
        int64, "n_infections": (draws, 8) int64, "titer_sums": (draws, 2, G)}."""
        G = self._ctx.n_gaps
        counts, n_inf, sums = self._kept_draws(self._lib.abd_sampler_curves, k, ((4, G), np.int64), ((8,), np.int64), ((2, G), np.float64))
        return {"counts": counts, "n_infections": n_inf, "titer_sums": sums}

    def diagnostics(self, k: int):
        """The convergence accumulators of the k-th chain over its draws so far (abd_hip.h: abd_sampler_diagnostics) ->
        {"i_counts": (4, G, N) int64 -- c_h0, c_h1, sum_cb, sum_cb2 --, "ab_n_mu", "ab_s_mu": (6, G, N) -- mean_h0, M2_h0,
        mean_h1, M2_h1, bm_mean, bm_M2 --, "info": (4,) int64 -- draws in half 0, in half 1, batches closed, L}:
        ``diagnostics.from_draws`` of the chain's draws."""
        G, N = self._ctx.n_gaps, self._ctx.n_inds
        cnt, mun, mus, info = np.empty((4, G, N), np.int64), np.empty((6, G, N)), np.empty((6, G, N)), np.empty(4, np.int64)
        _check(self._lib, self._lib.abd_sampler_diagnostics(self._h, int(k), _out(cnt, np.int64), _out(mun, np.float64),
                                                            _out(mus, np.float64), _out(info, np.int64)))
        return {"i_counts": cnt, "ab_n_mu": mun, "ab_s_mu": mus, "info": info}

    def timelines(self, k: int, hist: bool = False):
        """The timeline counters of the k-th chain over its draws so far (abd_hip.h: abd_sampler_timelines) -> {"inf", "cum":
        (G, N) int64, "ninf": (N, 8) int64, "n_draws": int} and, with ``hist``, {"hist_n", "hist_s": (G, N, 64) uint16}:
        ``timelines.from_draws`` of the chain's draws."""
        G, N = self._ctx.n_gaps, self._ctx.n_inds
        inf, cum, ninf = np.empty((G, N), np.int64), np.empty((G, N), np.int64), np.empty((N, 8), np.int64)
        hn, hs = (np.empty((G, N, 64), np.uint16), np.empty((G, N, 64), np.uint16)) if hist else (None, None)
        n = C.c_int64()
        _check(self._lib, self._lib.abd_sampler_timelines(self._h, int(k), None if hn is None else _out(hn, np.uint16),
                                                          None if hs is None else _out(hs, np.uint16), _out(inf, np.int64),
                                                          _out(cum, np.int64), _out(ninf, np.int64), C.byref(n)))
        out = {"inf": inf, "cum": cum, "ninf": ninf, "n_draws": n.value}
        if hist:
            out["hist_n"], out["hist_s"] = hn, hs
        return out

    def timeline_quantiles(self, q):
        """Quantiles ``q`` (1 to 8 numbers in [0, 1]) of the two titers per cell from the histograms pooled over the sampler's chains,
        computed on the device (abd_hip.h: abd_sampler_timeline_quantiles) -> (q_n, q_s), each (len(q), G, N)."""
        G, N = self._ctx.n_gaps, self._ctx.n_inds
        qa = _as(np.atleast_1d(q), np.float64)
        if qa.ndim != 1:
            raise ValueError(f"q must be one-dimensional, got shape {qa.shape}")
        nq = int(qa.size)
        out_n, out_s = np.empty((max(nq, 1), G, N)), np.empty((max(nq, 1), G, N))
        _check(self._lib, self._lib.abd_sampler_timeline_quantiles(self._h, nq, _ptr(qa, C.c_double), _out(out_n, np.float64),
                                                                   _out(out_s, np.float64)))
        return out_n[:nq], out_s[:nq]

    def risk(self, k: int):
        """The infection-risk-by-titer table of every draw of the k-th chain so far (``Context.risk`` per draw) -> (draws, 2, 2, G,
        8) int64."""
        return self._kept_draws(self._lib.abd_sampler_risk, k, ((2, 2, self._ctx.n_gaps, 8), np.int64))[0]

    def loo_rows(self, k: int, first: int = 0, count=None):
        """Kept rows [first, first + count) of the k-th chain's part of the LOO matrix (``count`` None: all it holds from ``first``)
        -> (count, n_inds): T_j = ll_s + ll_n of ``Context.individual_loglik`` at those draws."""
        if count is None:
            n = C.c_int64()
            _check(self._lib, self._lib.abd_sampler_loo_rows(self._h, int(k), 0, 0, None, C.byref(n)))
            count = max(0, n.value - int(first))
        out = np.empty((int(count), self._ctx.n_inds))
        _check(self._lib, self._lib.abd_sampler_loo_rows(self._h, int(k), int(first), int(count), _ptr(out, C.c_double), None))
        return out

    def loo_stats(self):
        """PSIS-LOO by individual over the kept draws of all chains of a finished run, smoothed on the device -> {"elpd_loo",
        "pareto_k", "lppd": (n_inds,), "n_tail": (n_inds,) int32, "n_readings": (n_inds,) int64, "n_draws": int}."""
        N = self._ctx.n_inds
        elpd, k, lppd = np.empty(N), np.empty(N), np.empty(N)
        tail, n_readings = np.empty(N, np.int32), np.empty(N, np.int64)
        n = C.c_int64()
        _check(self._lib, self._lib.abd_sampler_loo_stats(self._h, _ptr(elpd, C.c_double), _ptr(k, C.c_double), _ptr(lppd, C.c_double),
                                                          _ptr(tail, C.c_int32), C.byref(n), _out(n_readings, np.int64)))
        return {"elpd_loo": elpd, "pareto_k": k, "lppd": lppd, "n_tail": tail, "n_readings": n_readings, "n_draws": n.value}

    def adaptation(self, k: int):
        """(diagonal of M^-1, step size) of the k-th chain."""
        inv_mass = np.empty(N_THETA)
        eps = C.c_double()
        _check(self._lib, self._lib.abd_sampler_adaptation(self._h, int(k), _ptr(inv_mass, C.c_double), C.byref(eps), None))
        return inv_mass, eps.value

    def set_adaptation(self, k: int, inv_mass=None, step_size: float = 0.0):
        """Install a diagonal M^-1 and / or a step size for the k-th chain (between two runs)."""
        im = None if inv_mass is None else np.ascontiguousarray(inv_mass, dtype=np.float64)
        if im is not None and im.shape != (N_THETA,):
            raise ValueError(f"inv_mass must have {N_THETA} entries")
        _check(self._lib, self._lib.abd_sampler_set_adaptation(self._h, int(k), None if im is None else _ptr(im, C.c_double), float(step_size)))

    def metric(self, k: int) -> np.ndarray:
        """Full M^-1 (17 x 17) of the k-th chain."""
        m = np.empty((N_THETA, N_THETA))
        _check(self._lib, self._lib.abd_sampler_adaptation(self._h, int(k), None, None, _ptr(m, C.c_double)))
        return m

    # -- a test and debug facility: every evaluation the chains consume, and the launch shape they are evaluated with ----------
    LEAPFROG_COLS = 58
    _leapfrog_capacity = 0
    TRAIN_KINDS = ("none", "lists", "dense")

    def enable_leapfrog_log(self, rows_per_chain: int):
        """Log every evaluation a chain's NUTS state consumes, up to ``rows_per_chain`` rows per chain (0: off); before the first
        run (abd_hip.h: abd_sampler_enable_leapfrog_log)."""
        _check(self._lib, self._lib.abd_sampler_enable_leapfrog_log(self._h, int(rows_per_chain)))
        self._leapfrog_capacity = int(rows_per_chain)

    def leapfrog_log(self, k: int):
        """The k-th chain's log so far -> (rows, n_total): one record per kept row with the fields ``kind`` (0 the start point, 1
        a transition's start point evaluated again after a sweep, 2 a leaf), ``iteration``, ``depth``, ``n_leaf``, ``dir``,
        ``eps``, ``lp`` and ``q``, ``p_half``, ``g`` (17 each); n_total counts the rows beyond the capacity too."""
        n = C.c_int64()
        _check(self._lib, self._lib.abd_sampler_leapfrog_log(self._h, int(k), 0, 0, None, C.byref(n)))
        have = min(n.value, self._leapfrog_capacity)
        rows = np.empty((have, self.LEAPFROG_COLS))
        if have:
            _check(self._lib, self._lib.abd_sampler_leapfrog_log(self._h, int(k), 0, have, _ptr(rows, C.c_double), None))
        dt = np.dtype([("kind", "f8"), ("iteration", "f8"), ("depth", "f8"), ("n_leaf", "f8"), ("dir", "f8"), ("eps", "f8"),
                       ("lp", "f8"), ("q", "f8", (N_THETA,)), ("p_half", "f8", (N_THETA,)), ("g", "f8", (N_THETA,))])
        return rows.view(dt).reshape(have), n.value

    def launch_shape(self):
        """{"unit": chains per unit, "trains": "none" / "lists" / "dense", "workgroups": workgroups with a range of a unit's leapfrog
        launch as the kernel sees it, "threads": host threads} (abd_hip.h: abd_sampler_launch_shape)."""
        out = np.zeros(4, np.int32)
        _check(self._lib, self._lib.abd_sampler_launch_shape(self._h, _ptr(out, C.c_int32)))
        return {"unit": int(out[0]), "trains": self.TRAIN_KINDS[int(out[1])], "workgroups": int(out[2]), "threads": int(out[3])}

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.abd_sampler_destroy(self._h)
            self._h = _P()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _SurvivalHandle:
    """What the handles of the survival models share: the library, the handle ``_h`` (destroyed by the library's ``_destroy``) and
    the check of the points of a call."""

    _destroy = None  # the name of the library's destroy function

    def __init__(self):
        self._lib = load()
        self._h = _P()

    def _created(self, rc: int, dim_fn: str, n_sums: int):
        """after the library's creator: its refusal raised, else ``dim`` read and ``n_sums`` kept"""
        _check(self._lib, rc)
        self.dim = int(getattr(self._lib, dim_fn)(self._h))
        self.n_sums = n_sums

    def _points(self, theta):
        t = _as(theta, np.float64)
        t = t.reshape(1, -1) if t.ndim == 1 else t
        if t.ndim != 2 or t.shape[1] != self.dim:
            raise ValueError(f"theta must have shape ({self.dim},) or (n, {self.dim}), got {t.shape}")
        return t

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            getattr(self._lib, self._destroy)(self._h)
            self._h = _P()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Survival(_SurvivalHandle):
    """One survival model's data resident on the device (abd_hip.h: ``abd_survival``): ``infected``, ``exposure`` (N, T) and one or
    two titer arrays (N, T); ``priors`` = (ab_sd, lam0_mu_mean, lam0_mu_sd, lam0_sd_rate, lam0_z_sd).  The library checks the cells."""

    _destroy = "abd_survival_destroy"

    def __init__(self, infected, exposure, titers, priors, device: int = -1):
        super().__init__()
        y, e, *xs = self._planes(infected, exposure, titers, "titers")
        if len(xs) not in (1, 2):
            raise ValueError(f"one or two titer arrays, got {len(xs)}")
        d = _SurvivalDesc()
        d.n_inds, d.n_intervals, d.n_titers, d.device = y.shape[0], y.shape[1], len(xs), device
        d.infected, d.exposure = y.ctypes.data, e.ctypes.data
        for k, x in enumerate(xs):
            d.titer[k] = x.ctypes.data
        d.ab_sd, d.lam0_mu_mean, d.lam0_mu_sd, d.lam0_sd_rate, d.lam0_z_sd = (float(v) for v in priors)
        self._created(self._lib.abd_survival_create(C.byref(d), C.byref(self._h)), "abd_survival_dim", y.shape[1] + 2 + len(xs))

    def _planes(self, infected, exposure, titers, what: str):
        """infected, exposure and the titers as float64 arrays of one shape (N, T); ``n_inds``, ``n_intervals``, ``n_titers``"""
        y, e = _as(infected, np.float64), _as(exposure, np.float64)
        xs = [_as(x, np.float64) for x in titers]
        if y.ndim != 2 or e.shape != y.shape or any(x.shape != y.shape for x in xs):
            raise ValueError(f"infected, exposure and the {what} must share a shape (N, T)")
        self.n_inds, self.n_intervals, self.n_titers = y.shape[0], y.shape[1], len(xs)
        return [y, e] + xs

    def logp_dlogp(self, theta):
        """``theta`` (D,) -> (logp, grad (D,)); (n, D) -> (logp (n,), grad (n, D))."""
        t = _as(theta, np.float64)
        one = t.ndim == 1
        t2 = t.reshape(1, -1) if one else t
        if t2.ndim != 2 or t2.shape[1] != self.dim:
            raise ValueError(f"theta must have shape ({self.dim},) or (n, {self.dim}), got {t.shape}")
        lp, g = np.empty(t2.shape[0]), np.empty(t2.shape)
        _check(self._lib, self._lib.abd_survival_logp_dlogp(self._h, t2.shape[0], _ptr(t2), _ptr(lp), _ptr(g)))
        return (float(lp[0]), g[0]) if one else (lp, g)

    def loglik_sums(self, theta):
        """The raw device sums at one point: S_t (T), L, W_0, W_k (K); of a grouped handle S_t (T), L, W_x, W0_g (Gr); of a handle
        by period S_t (T), L, W_x, W0_t (T)."""
        t = _as(theta, np.float64)
        if t.shape != (self.dim,):
            raise ValueError(f"theta must have shape ({self.dim},)")
        out = np.empty(self.n_sums)
        _check(self._lib, self._lib.abd_survival_loglik_sums(self._h, _ptr(t), _ptr(out)))
        return out

    def individual_loglik(self, theta):
        """``theta`` (n, D) (or (D,)) -> (n, N): every individual's Poisson log-likelihood over its intervals at every point, in
        the caller's order of individuals; exactly 0 for an individual without a followed cell."""
        t = self._points(theta)
        out = np.empty((t.shape[0], self.n_inds))
        _check(self._lib, self._lib.abd_survival_individual_loglik(self._h, t.shape[0], _ptr(t), _ptr(out)))
        return out

    def waic_reset(self):
        _check(self._lib, self._lib.abd_survival_waic_reset(self._h))

    def waic_accumulate(self, theta):
        """Folds the draws ``theta`` (n, D), in order, into the running statistics of ``individual_loglik`` kept on the device."""
        t = self._points(theta)
        _check(self._lib, self._lib.abd_survival_waic_accumulate(self._h, t.shape[0], _ptr(t)))

    def waic_stats(self):
        """((lse, mean, m2, n_draws), n_cells): ``compare``'s statistics of all draws folded, each (N,), and every individual's
        number of followed cells (N,) int64."""
        N = self.n_inds
        lse, mean, m2, cells = np.empty(N), np.empty(N), np.empty(N), np.empty(N, np.int32)
        n = C.c_int64()
        _check(self._lib, self._lib.abd_survival_waic_stats(self._h, _ptr(lse), _ptr(mean), _ptr(m2), C.byref(n), _ptr(cells, C.c_int32)))
        return (lse, mean, m2, int(n.value)), cells.astype(np.int64)

    LOO_MAX_DRAWS = 16384  # ABD_SURVIVAL_LOO_MAX_DRAWS

    def loo_reserve(self, capacity: int):
        """Room on the device for ``capacity`` draws of the per-individual log-likelihood (PSIS-LOO); 0 releases it."""
        _check(self._lib, self._lib.abd_survival_loo_reserve(self._h, int(capacity)))

    def loo_reset(self):
        _check(self._lib, self._lib.abd_survival_loo_reset(self._h))

    def loo_accumulate(self, theta):
        """Evaluates the draws ``theta`` (n, D) and stores their rows, in order, in the matrix ``loo_reserve`` made room for."""
        t = self._points(theta)
        _check(self._lib, self._lib.abd_survival_loo_accumulate(self._h, t.shape[0], _ptr(t)))

    def loo_append_rows(self, ll):
        """Stores the host rows ``ll`` (n, N), in the caller's order of individuals, in the place of evaluated ones."""
        r = _as(ll, np.float64)
        if r.ndim != 2 or r.shape[1] != self.n_inds:
            raise ValueError(f"ll must have shape (n, {self.n_inds}), got {r.shape}")
        _check(self._lib, self._lib.abd_survival_loo_append_rows(self._h, r.shape[0], _ptr(r)))

    def loo_rows(self, first: int, count: int):
        """(count, N): the stored draws ``first .. first + count - 1``."""
        out = np.empty((max(int(count), 0), self.n_inds))
        _check(self._lib, self._lib.abd_survival_loo_rows(self._h, int(first), int(count), _ptr(out)))
        return out

    def loo_stats(self):
        """(elpd_loo, pareto_k, lppd (N,), n_tail (N,) int64, n_draws, n_cells (N,) int64) of the draws held."""
        N = self.n_inds
        elpd, k, lppd = np.empty(N), np.empty(N), np.empty(N)
        tail, cells = np.empty(N, np.int32), np.empty(N, np.int32)
        n = C.c_int64()
        _check(self._lib, self._lib.abd_survival_loo_stats(self._h, _ptr(elpd), _ptr(k), _ptr(lppd), _ptr(tail, C.c_int32), C.byref(n),
                                                           _ptr(cells, C.c_int32)))
        return elpd, k, lppd, tail.astype(np.int64), int(n.value), cells.astype(np.int64)

    def predictive_configure(self, titers, edges, seed: int = 0):
        """The binning variables of the posterior predictive checks: one or two titer arrays (N, T) with their edges (each up to 7,
        finite, strictly ascending).  The library checks them, computes the constants and sets the draw counter to 0."""
        xs = [_as(x, np.float64) for x in titers]
        es = [_as(np.asarray(e, dtype=np.float64).reshape(-1), np.float64) for e in edges]
        if len(xs) != len(es):
            raise ValueError(f"{len(xs)} binning variables with {len(es)} sets of edges")
        if any(x.shape != (self.n_inds, self.n_intervals) for x in xs):
            raise ValueError(f"a binning variable must have shape ({self.n_inds}, {self.n_intervals})")
        n = len(xs)
        tp = (C.c_void_p * max(n, 1))(*[x.ctypes.data for x in xs])
        ep = (C.c_void_p * max(n, 1))(*[e.ctypes.data if e.size else None for e in es])
        ne = np.array([e.size for e in es] or [0], dtype=np.int32)
        _check(self._lib, self._lib.abd_survival_predictive_configure(self._h, n, C.addressof(tp), _ptr(ne), C.addressof(ep),
                                                                      int(seed) & 0xFFFFFFFFFFFFFFFF))
        self.n_predictive_vars = n

    def predictive_reset(self):
        _check(self._lib, self._lib.abd_survival_predictive_reset(self._h))

    def predictive_accumulate(self, theta):
        """Folds the draws ``theta`` (n, D) in order; returns (expected (n, n_var, 8) float64, replicate (n, n_var, 8) int64): per draw
        the expected and the replicated infections of every bin of every binning variable."""
        t = self._points(theta)
        nv = getattr(self, "n_predictive_vars", 0) or 1  # before predictive_configure the library refuses the call
        exp_, rep = np.zeros((t.shape[0], nv, SURVIVAL_PREDICTIVE_BINS)), np.zeros((t.shape[0], nv, SURVIVAL_PREDICTIVE_BINS), np.int64)
        _check(self._lib, self._lib.abd_survival_predictive_accumulate(self._h, t.shape[0], _ptr(t), _ptr(exp_), _ptr(rep)))
        return exp_, rep

    def predictive_stats(self):
        """(sum_e, sum_r, n_pos, n_draws): per individual (N,) over the draws folded, the sums of E_j and of R_j and the number of
        draws with R_j >= 1."""
        N = self.n_inds
        sum_e, sum_r, n_pos = np.empty(N), np.empty(N, np.int64), np.empty(N, np.int64)
        n = C.c_int64()
        _check(self._lib, self._lib.abd_survival_predictive_stats(self._h, _ptr(sum_e), _ptr(sum_r), _ptr(n_pos), C.byref(n)))
        return sum_e, sum_r, n_pos, int(n.value)

    def predictive_observed(self):
        """(observed (n_var, 8), person_time (n_var, 8), n_cells (n_var, 8) int64, observed_ind (N,)): the constants of the data."""
        nv = getattr(self, "n_predictive_vars", 0) or 1
        obs, pt = np.zeros((nv, SURVIVAL_PREDICTIVE_BINS)), np.zeros((nv, SURVIVAL_PREDICTIVE_BINS))
        cells, ind = np.zeros((nv, SURVIVAL_PREDICTIVE_BINS), np.int64), np.zeros(self.n_inds)
        _check(self._lib, self._lib.abd_survival_predictive_observed(self._h, _ptr(obs), _ptr(pt), _ptr(cells), _ptr(ind)))
        return obs, pt, cells, ind

    def replicate(self, theta, draw0: int = 0):
        """``theta`` (n, D) -> (n, N, T) int32: the per-cell replicates of the draws ``draw0 .. draw0 + n - 1``, in the caller's order;
        what ``predictive_accumulate`` draws for those indices.  Folds nothing."""
        t = self._points(theta)
        out = np.zeros((t.shape[0], self.n_inds, self.n_intervals), np.int32)
        _check(self._lib, self._lib.abd_survival_replicate(self._h, t.shape[0], _ptr(t), int(draw0), _ptr(out)))
        return out


class SurvivalGroups(Survival):
    """The survival model by group resident on the device (abd_hip.h: ``abd_survival_create_groups``): ``infected``, ``exposure``,
    ``titer`` (N, T), ``group`` (N,) indices in [0, ``n_groups``), ``priors`` = (lam0_mu_mean, lam0_mu_sd, lam0_sd_rate, lam0_z_sd,
    a_mu_sd, a_sd_rate, a_z_sd, b_sd).  The library checks the labels and the cells; the evaluations are ``Survival``'s."""

    def __init__(self, infected, exposure, titer, group, n_groups: int, priors, device: int = -1):
        _SurvivalHandle.__init__(self)
        y, e, x = self._planes(infected, exposure, [titer], "titer")
        g = _as(group, np.int32)
        if g.shape != (y.shape[0],):
            raise ValueError(f"group must have shape ({y.shape[0]},), got {g.shape}")
        d = _SurvivalGroupsDesc()
        d.n_inds, d.n_intervals, d.n_groups, d.device = y.shape[0], y.shape[1], int(n_groups), device
        d.infected, d.exposure, d.titer, d.group = y.ctypes.data, e.ctypes.data, x.ctypes.data, g.ctypes.data
        (d.lam0_mu_mean, d.lam0_mu_sd, d.lam0_sd_rate, d.lam0_z_sd, d.a_mu_sd, d.a_sd_rate, d.a_z_sd,
         d.b_sd) = (float(v) for v in priors)
        self.n_groups = int(n_groups)
        self._created(self._lib.abd_survival_create_groups(C.byref(d), C.byref(self._h)), "abd_survival_dim", y.shape[1] + 2 + int(n_groups))


class SurvivalPeriods(Survival):
    """The survival model by period resident on the device (abd_hip.h: ``abd_survival_create_periods``): ``infected``, ``exposure``,
    ``titer`` (N, T), ``period`` (T,) indices in [0, ``n_periods``), ``priors`` = (lam0_mu_mean, lam0_mu_sd, lam0_sd_rate, lam0_z_sd,
    a_mu_sd, a_sd_rate, a_z_sd, b_sd).  The library checks the labels and the cells; the evaluations are ``Survival``'s."""

    def __init__(self, infected, exposure, titer, period, n_periods: int, priors, device: int = -1):
        _SurvivalHandle.__init__(self)
        y, e, x = self._planes(infected, exposure, [titer], "titer")
        p = _as(period, np.int32)
        if p.shape != (y.shape[1],):
            raise ValueError(f"period must have shape ({y.shape[1]},), got {p.shape}")
        d = _SurvivalPeriodsDesc()
        d.n_inds, d.n_intervals, d.n_periods, d.device = y.shape[0], y.shape[1], int(n_periods), device
        d.infected, d.exposure, d.titer, d.period = y.ctypes.data, e.ctypes.data, x.ctypes.data, p.ctypes.data
        (d.lam0_mu_mean, d.lam0_mu_sd, d.lam0_sd_rate, d.lam0_z_sd, d.a_mu_sd, d.a_sd_rate, d.a_z_sd,
         d.b_sd) = (float(v) for v in priors)
        self.n_periods = int(n_periods)
        self._created(self._lib.abd_survival_create_periods(C.byref(d), C.byref(self._h)), "abd_survival_dim", 2 * y.shape[1] + 2)


class SurvivalDraws(_SurvivalHandle):
    """An ensemble of per-draw datasets resident on the device (abd_hip.h: ``abd_survival_draws``): ``n_risk``, ``event`` (M, N) int32
    and one or two titer arrays (M, T, N); ``priors`` as ``Survival``'s.  Every point names its dataset.  The library checks the
    datasets.  A handle of its own kind: its per-individual, WAIC and PSIS-LOO calls work per dataset (abd_hip.h:
    ``abd_survival_draws_individual_loglik`` ...); it has no predictive calls."""

    _destroy = "abd_survival_draws_destroy"

    def __init__(self, n_risk, event, titers, priors, device: int = -1):
        super().__init__()
        nr, ev, *xs = self._datasets(n_risk, event, titers)
        if len(xs) not in (1, 2):
            raise ValueError(f"one or two titer arrays, got {len(xs)}")
        d = _SurvivalDrawsDesc()
        d.n_datasets, d.n_inds, d.n_intervals, d.n_titers, d.device = nr.shape[0], nr.shape[1], xs[0].shape[1], len(xs), device
        d.n_risk, d.event = nr.ctypes.data, ev.ctypes.data
        for k, x in enumerate(xs):
            d.titer[k] = x.ctypes.data
        d.ab_sd, d.lam0_mu_mean, d.lam0_mu_sd, d.lam0_sd_rate, d.lam0_z_sd = (float(v) for v in priors)
        self._created(self._lib.abd_survival_draws_create(C.byref(d), C.byref(self._h)), "abd_survival_draws_dim", self.n_intervals + 2 + len(xs))

    def _datasets(self, n_risk, event, titers):
        """n_risk, event as int32 arrays of one shape (M, N) and the titers as float64 arrays of one shape (M, T, N); ``n_datasets``,
        ``n_inds``, ``n_intervals``, ``n_titers``"""
        nr, ev = _as(n_risk, np.int32), _as(event, np.int32)
        xs = [_as(x, np.float64) for x in titers]
        if nr.ndim != 2 or ev.shape != nr.shape:
            raise ValueError("n_risk and event must share a shape (M, N)")
        if not xs:
            raise ValueError("one or two titer arrays, got 0")
        if any(x.ndim != 3 or (x.shape[0], x.shape[2]) != nr.shape or x.shape != xs[0].shape for x in xs):
            raise ValueError(f"the titers must share a shape (M, T, N) with (M, N) = {nr.shape}")
        self.n_datasets, self.n_inds, self.n_intervals, self.n_titers = nr.shape[0], nr.shape[1], xs[0].shape[1], len(xs)
        return [nr, ev] + xs

    def logp_dlogp(self, dataset, theta):
        """``dataset`` an index and ``theta`` (D,) -> (logp, grad (D,)); ``dataset`` (n,) and ``theta`` (n, D) -> (logp (n,), grad (n, D))."""
        t = _as(theta, np.float64)
        one = t.ndim == 1
        t2 = t.reshape(1, -1) if one else t
        ds = _as(dataset, np.int32).reshape(-1)
        if t2.ndim != 2 or t2.shape[1] != self.dim or ds.shape != (t2.shape[0],):
            raise ValueError(f"theta must have shape ({self.dim},) or (n, {self.dim}) with one dataset index per point, got {t.shape} and {ds.shape}")
        lp, g = np.empty(t2.shape[0]), np.empty(t2.shape)
        _check(self._lib, self._lib.abd_survival_draws_logp_dlogp(self._h, t2.shape[0], _ptr(ds), _ptr(t2), _ptr(lp), _ptr(g)))
        return (float(lp[0]), g[0]) if one else (lp, g)

    def loglik_sums(self, dataset: int, theta):
        """The raw device sums of one point on one dataset: S_t (T), L, W_0, W_k (K); of a grouped ensemble S_t (T), L, W_x, W0_g (Gr);
        of an ensemble by period S_t (T), L, W_x, W0_t (T)."""
        t = _as(theta, np.float64)
        if t.shape != (self.dim,):
            raise ValueError(f"theta must have shape ({self.dim},)")
        out = np.empty(self.n_sums)
        _check(self._lib, self._lib.abd_survival_draws_loglik_sums(self._h, int(dataset), _ptr(t), _ptr(out)))
        return out

    def _rows(self, dataset, theta):
        """(dataset (n,) int32, theta (n, D)): one dataset index per point; a single index goes with every point."""
        t = self._points(theta)
        ds = _as(dataset, np.int32).reshape(-1)
        if ds.size == 1 and t.shape[0] != 1:
            ds = np.full(t.shape[0], ds[0], dtype=np.int32)
        if ds.shape != (t.shape[0],):
            raise ValueError(f"one dataset index per point (or one for all): {ds.shape[0]} for {t.shape[0]} points")
        return ds, t

    def draws_individual_loglik(self, dataset, theta):
        """``dataset`` (n,) (or one index) and ``theta`` (n, D) (or (D,)) -> (n, N): every individual's log-likelihood over its
        intervals at risk in the point's dataset, in the caller's order of individuals; exactly 0 for one never at risk."""
        ds, t = self._rows(dataset, theta)
        out = np.empty((t.shape[0], self.n_inds))
        _check(self._lib, self._lib.abd_survival_draws_individual_loglik(self._h, t.shape[0], _ptr(ds), _ptr(t), _ptr(out)))
        return out

    def draws_waic_reset(self):
        _check(self._lib, self._lib.abd_survival_draws_waic_reset(self._h))

    def draws_waic_accumulate(self, dataset, theta):
        """Folds the draws ``theta`` (n, D), in order, each into the running statistics of its own dataset."""
        ds, t = self._rows(dataset, theta)
        _check(self._lib, self._lib.abd_survival_draws_waic_accumulate(self._h, t.shape[0], _ptr(ds), _ptr(t)))

    def draws_waic_stats(self):
        """(lse, mean, m2 (M, N), n_draws (M,) int64, n_cells (M, N) int64): ``compare``'s statistics per dataset; NaN and 0 draws
        for a dataset nothing was folded into."""
        M, N = self.n_datasets, self.n_inds
        lse, mean, m2, cells = np.empty((M, N)), np.empty((M, N)), np.empty((M, N)), np.empty((M, N), np.int32)
        n = np.zeros(M, np.int64)
        _check(self._lib, self._lib.abd_survival_draws_waic_stats(self._h, _ptr(lse), _ptr(mean), _ptr(m2), _ptr(n), _ptr(cells)))
        return lse, mean, m2, n, cells.astype(np.int64)

    LOO_MAX_DRAWS = 16384  # ABD_SURVIVAL_LOO_MAX_DRAWS, per dataset

    def draws_loo_reserve(self, capacity: int):
        """Room on the device for ``capacity`` draws of the per-individual log-likelihood of every dataset; 0 releases it."""
        _check(self._lib, self._lib.abd_survival_draws_loo_reserve(self._h, int(capacity)))

    def draws_loo_reset(self):
        _check(self._lib, self._lib.abd_survival_draws_loo_reset(self._h))

    def draws_loo_accumulate(self, dataset, theta):
        """Evaluates the draws ``theta`` (n, D) and stores every row as the next draw of its dataset."""
        ds, t = self._rows(dataset, theta)
        _check(self._lib, self._lib.abd_survival_draws_loo_accumulate(self._h, t.shape[0], _ptr(ds), _ptr(t)))

    def draws_loo_stats(self):
        """(elpd_loo, pareto_k, lppd (M, N), n_tail (M, N) int64, n_draws (M,) int64) of the draws every dataset holds."""
        M, N = self.n_datasets, self.n_inds
        elpd, k, lppd, tail = np.empty((M, N)), np.empty((M, N)), np.empty((M, N)), np.empty((M, N), np.int32)
        n = np.zeros(M, np.int64)
        _check(self._lib, self._lib.abd_survival_draws_loo_stats(self._h, _ptr(elpd), _ptr(k), _ptr(lppd), _ptr(tail), _ptr(n)))
        return elpd, k, lppd, tail.astype(np.int64), n


class SurvivalDrawsGroups(SurvivalDraws):
    """The survival model by group over an ensemble of per-draw datasets (abd_hip.h: ``abd_survival_draws_create_groups``): ``n_risk``,
    ``event`` (M, N) int32, ``titer`` (M, T, N), ``group`` (N,) indices in [0, ``n_groups``) shared by all datasets, ``priors`` as
    ``SurvivalGroups``'.  The library checks the labels and the datasets; the evaluations are ``SurvivalDraws``'."""

    def __init__(self, n_risk, event, titer, group, n_groups: int, priors, device: int = -1):
        _SurvivalHandle.__init__(self)
        nr, ev, x = self._datasets(n_risk, event, [titer])
        g = _as(group, np.int32)
        if g.shape != (nr.shape[1],):
            raise ValueError(f"group must have shape ({nr.shape[1]},), got {g.shape}")
        d = _SurvivalDrawsGroupsDesc()
        d.n_datasets, d.n_inds, d.n_intervals, d.n_groups, d.device = nr.shape[0], nr.shape[1], x.shape[1], int(n_groups), device
        d.n_risk, d.event, d.titer, d.group = nr.ctypes.data, ev.ctypes.data, x.ctypes.data, g.ctypes.data
        (d.lam0_mu_mean, d.lam0_mu_sd, d.lam0_sd_rate, d.lam0_z_sd, d.a_mu_sd, d.a_sd_rate, d.a_z_sd,
         d.b_sd) = (float(v) for v in priors)
        self.n_groups = int(n_groups)
        self._created(self._lib.abd_survival_draws_create_groups(C.byref(d), C.byref(self._h)), "abd_survival_draws_dim",
                      self.n_intervals + 2 + int(n_groups))


class SurvivalDrawsPeriods(SurvivalDraws):
    """The survival model by period over an ensemble of per-draw datasets (abd_hip.h: ``abd_survival_draws_create_periods``):
    ``n_risk``, ``event`` (M, N) int32, ``titer`` (M, T, N), ``period`` (T,) indices in [0, ``n_periods``), ``priors`` as
    ``SurvivalPeriods``'.  The library checks the labels and the datasets; the evaluations are ``SurvivalDraws``'."""

    def __init__(self, n_risk, event, titer, period, n_periods: int, priors, device: int = -1):
        _SurvivalHandle.__init__(self)
        nr, ev, x = self._datasets(n_risk, event, [titer])
        p = _as(period, np.int32)
        if p.shape != (x.shape[1],):
            raise ValueError(f"period must have shape ({x.shape[1]},), got {p.shape}")
        d = _SurvivalDrawsPeriodsDesc()
        d.n_datasets, d.n_inds, d.n_intervals, d.n_periods, d.device = nr.shape[0], nr.shape[1], x.shape[1], int(n_periods), device
        d.n_risk, d.event, d.titer, d.period = nr.ctypes.data, ev.ctypes.data, x.ctypes.data, p.ctypes.data
        (d.lam0_mu_mean, d.lam0_mu_sd, d.lam0_sd_rate, d.lam0_z_sd, d.a_mu_sd, d.a_sd_rate, d.a_z_sd,
         d.b_sd) = (float(v) for v in priors)
        self.n_periods = int(n_periods)
        self._created(self._lib.abd_survival_draws_create_periods(C.byref(d), C.byref(self._h)), "abd_survival_draws_dim", 2 * self.n_intervals + 2)
