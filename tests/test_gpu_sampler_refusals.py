"""
What the native sampler answers to a bad request, as (exception type, full message): an index outside the sampler's chains, a
read-out of something that is not on, a draw window past the end, an enable call after the first run, a run past the planned
draws, and the enable functions' own argument checks -- under each of the three ways a sampler runs (observation-list trains,
dense trains, result rows with units of two chains on both cohorts).  The strings are the library's as of the commit before the
summaries' host side moved into `abd_sampler_summaries.hip`; a refactor of that code leaves every one of them, and which of
several simultaneous faults is reported, as it is.  Through `NativeSampler` where it forwards, through the library's symbols
where the wrapper would check first or fixes an argument.
"""
import contextlib
import ctypes
import os

import numpy as np
import pytest

from abdpymc_amd import risk
from abdpymc_amd._native import AbdError

from tests.test_gpu_summaries_together import _model

pytestmark = pytest.mark.gpu
N_CHAINS, TUNE, N_ITER = 2, 1, 3  # two draws per chain
# mode -> (cohort, environment at creation, launch_shape()["trains"], ["unit"])
MODES = {
    "list_trains": ("test", {}, "lists", 1),
    "dense_trains": ("dense", {}, "dense", 1),
    "rows_lists": ("test", {"ABD_SAMPLER_TRAINS": "0", "ABD_SAMPLER_UNIT": "2"}, "none", 2),
    "rows_dense": ("dense", {"ABD_SAMPLER_TRAINS": "0", "ABD_SAMPLER_UNIT": "2"}, "none", 2),
}
STATE = "[-3] "  # ABD_ERR_STATE as _native._check words it; ABD_ERR_ARG is a ValueError with the bare message
OUTSIDE = "k=%d outside [0, 2)"


@contextlib.contextmanager
def _env(**kw):
    names = ("ABD_SAMPLER_TRAINS", "ABD_SAMPLER_UNIT", "ABD_SAMPLER_THREADS")
    old = {k: os.environ.pop(k, None) for k in names}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k in names:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


class _Case:
    def __init__(self, mode, golden_dir):
        which, self.env, self.trains, self.unit = MODES[mode]
        self.m = _model(which, golden_dir)
        self.ctx = self.m.ctx
        pt = self.m.initial_point()
        self.q0 = np.empty((N_CHAINS, 17))
        for c in range(N_CHAINS):
            self.ctx.set_discrete(c, pt["i_raw"].astype(np.int8), pt["ab_s_waner"].astype(np.int8))
            self.q0[c] = self.m.ravel(pt) + np.random.default_rng([7, c]).uniform(-1, 1, size=17)
        self.spec = risk.spec(0, self.m.n_gaps, 0.5 * np.arange(1, 8), 0.25 * np.arange(1, 8), 1)
        self.fresh = self.sampler()  # nothing enabled, never run
        self.ran = self.sampler()    # curves, risk and the leapfrog log on; three iterations
        self.ran.enable_curves(2)
        self.ran.enable_risk(2, self.spec)
        self.ran.enable_leapfrog_log(4)  # (the start point and at least one row per iteration: the log is full)
        self.ran.run(N_ITER)

    def sampler(self, **kw):
        with _env(**self.env):
            return self.ctx.sampler(np.arange(N_CHAINS), self.q0, tune=TUNE, seed=7, **kw)


@pytest.fixture(scope="module", params=list(MODES))
def case(request, golden_dir):
    c = _Case(request.param, golden_dir)
    yield c
    c.m.close()


def _refused(kind, text, call, *args):
    with pytest.raises(kind) as e:
        call(*args)
    assert type(e.value) is kind and str(e.value) == text, (str(e.value), text)


def _direct(smp, name, *args):
    """abd_sampler_<name>(handle, *args) on the loaded library, its return code raised as NativeSampler raises it"""
    from abdpymc_amd._native import _check

    _check(smp._lib, getattr(smp._lib, "abd_sampler_" + name)(smp._h, *args))


def test_the_case_runs_the_mode_it_names(case):
    for smp in (case.fresh, case.ran):
        shape = smp.launch_shape()
        assert (shape["trains"], shape["unit"]) == (case.trains, case.unit), shape


@pytest.mark.parametrize("k", [-1, N_CHAINS])
def test_a_chain_index_outside_the_sampler(case, k):
    s = case.fresh  # (nothing is enabled either: the index is what is reported)
    text = OUTSIDE % k
    for call in (s.means, s.pointwise_stats, s.predictive_stats, s.individual_loglik_stats, s.curves, s.diagnostics, s.timelines, s.risk,
                 s.leapfrog_log, s.adaptation, s.set_adaptation, s.metric):
        _refused(ValueError, text, call, k)
    _refused(ValueError, text, _direct, s, "curves", k, 0, 1, None, None, None, None)
    _refused(ValueError, text, _direct, s, "risk", k, 0, 1, None, None)
    _refused(ValueError, text, _direct, s, "leapfrog_log", k, 0, 1, None, None)


def test_a_read_out_of_something_not_enabled(case):
    s = case.fresh
    for call, text in ((s.means, "the sampler was created without accumulate"),
                       (s.pointwise_stats, "pointwise accumulation is not enabled (abd_sampler_enable_pointwise)"),
                       (s.predictive_stats, "predictive accumulation is not enabled (abd_sampler_enable_predictive)"),
                       (s.individual_loglik_stats, "individual_loglik accumulation is not enabled (abd_sampler_enable_individual_loglik)"),
                       (s.curves, "curves are not enabled (abd_sampler_enable_curves)"),
                       (s.diagnostics, "diagnostics are not enabled (abd_sampler_enable_diagnostics)"),
                       (s.timelines, "timelines are not enabled (abd_sampler_enable_timelines)"),
                       (s.risk, "risk is not enabled (abd_sampler_enable_risk)"),
                       (s.leapfrog_log, "the leapfrog log is not enabled (abd_sampler_enable_leapfrog_log)")):
        _refused(AbdError, STATE + text, call, 0)
    _refused(AbdError, STATE + "timelines are not enabled (abd_sampler_enable_timelines)", s.timeline_quantiles, [0.5])
    # a window that would be refused too: "not enabled" comes first
    _refused(AbdError, STATE + "curves are not enabled (abd_sampler_enable_curves)", _direct, s, "curves", 0, 0, 9, None, None, None, None)
    _refused(AbdError, STATE + "risk is not enabled (abd_sampler_enable_risk)", _direct, s, "risk", 0, 0, 9, None, None)


def test_a_draw_window_one_past_the_end(case):
    s = case.ran
    n = ctypes.c_int64(-1)
    _refused(ValueError, "curves: draws [0, 3) are beyond the 2 the chain has", _direct, s, "curves", 1, 0, 3, None, None, None, None)
    _refused(ValueError, "curves: draws [2, 3) are beyond the 2 the chain has", _direct, s, "curves", 0, 2, 1, None, None, None,
             ctypes.byref(n))
    assert n.value == 2  # (the count is handed out before the window is refused)
    _refused(ValueError, "curves: draws [-1, 0) are beyond the 2 the chain has", _direct, s, "curves", 0, -1, 1, None, None, None, None)
    _refused(ValueError, "risk: draws [0, 3) are beyond the 2 the chain has", _direct, s, "risk", 1, 0, 3, None, None)
    _refused(ValueError, "risk: draws [1, 3) are beyond the 2 the chain has", _direct, s, "risk", 0, 1, 2, None, None)
    _refused(ValueError, "leapfrog log: rows [0, 5) are beyond the 4 the chain holds", _direct, s, "leapfrog_log", 1, 0, 5, None, None)
    _refused(ValueError, "leapfrog log: rows [4, 5) are beyond the 4 the chain holds", _direct, s, "leapfrog_log", 0, 4, 1, None, None)
    _refused(ValueError, "rows is NULL", _direct, s, "leapfrog_log", 0, 0, 4, None, None)
    assert s.curves(0)["counts"].shape[0] == 2 and s.risk(1).shape[0] == 2 and len(s.leapfrog_log(0)[0]) == 4


def test_every_enable_after_the_first_run(case):
    s = case.ran
    after = " must be enabled before the first abd_sampler_run call"
    for call, args, what in ((s.enable_pointwise, (), "pointwise accumulation"),
                             (s.enable_predictive, (), "predictive accumulation"),
                             (s.enable_individual_loglik, (), "individual_loglik accumulation"),
                             (s.enable_curves, (2,), "curves"),
                             (s.enable_curves, (0,), "curves"),
                             (s.enable_diagnostics, (2, 1), "diagnostics"),
                             (s.enable_timelines, (2, (-3, 7), (-2, 6)), "timelines"),
                             (s.enable_risk, (2, case.spec), "risk"),
                             (s.enable_leapfrog_log, (4,), "the leapfrog log"),
                             (s.enable_leapfrog_log, (0,), "the leapfrog log")):
        _refused(AbdError, STATE + what + after, call, *args)
    # the arguments are looked at first
    _refused(ValueError, "capacity=-1 is negative", s.enable_curves, -1)
    _refused(ValueError, "diagnostics: planned_draws=1 is neither 0 nor >= 2", s.enable_diagnostics, 1, 1)


def test_a_run_past_the_planned_draws(case):
    s = case.sampler()  # a refused run is no run: one sampler serves all four
    for on, off, text in ((lambda: s.enable_curves(2), lambda: s.enable_curves(0), "curves: draws up to 3 do not fit capacity 2"),
                          (lambda: s.enable_diagnostics(2, 1), lambda: s.enable_diagnostics(0, 1), "diagnostics: draws up to 3 pass the planned 2"),
                          (lambda: s.enable_risk(2, case.spec), lambda: s.enable_risk(0, case.spec), "risk: draws up to 3 do not fit capacity 2"),
                          (lambda: s.enable_timelines(2, (-3, 7), (-2, 6)), lambda: s.enable_timelines(0, (-3, 7), (-2, 6)),
                           "timelines: draws up to 3 pass the planned 2")):
        on()
        _refused(AbdError, STATE + text, s.run, 4)
        off()
    # with all four on, the first of the run's own order is reported
    s.enable_timelines(2, (-3, 7), (-2, 6)), s.enable_risk(3, case.spec), s.enable_diagnostics(2, 1), s.enable_curves(3)
    _refused(AbdError, STATE + "diagnostics: draws up to 3 pass the planned 2", s.run, 4)
    _refused(ValueError, "n_iter=-1 is negative", _direct, s, "run", -1, None, None)
    s.close()


def test_the_enable_functions_check_their_arguments(case):
    s = case.fresh
    _refused(ValueError, "capacity=-1 is negative", s.enable_curves, -1)
    _refused(ValueError, "capacity=-1 is negative", s.enable_risk, -1, case.spec)
    _refused(ValueError, "capacity=-1 is negative", s.enable_leapfrog_log, -1)
    _refused(ValueError, "diagnostics: planned_draws=-1 is neither 0 nor >= 2", s.enable_diagnostics, -1, 1)
    _refused(ValueError, "diagnostics: planned_draws=1 is neither 0 nor >= 2", s.enable_diagnostics, 1, 1)
    _refused(ValueError, "diagnostics: batch_len=0 is below 1", s.enable_diagnostics, 4, 0)
    _refused(ValueError, "timelines: planned_draws=-1 outside [0, 65535] (16-bit counters)", s.enable_timelines, -1, (-3, 7), (-2, 6))
    _refused(ValueError, "timelines: planned_draws=65536 outside [0, 65535] (16-bit counters)", s.enable_timelines, 65536, (-3, 7), (-2, 6))
    _refused(ValueError, "timelines: the range [7, -3) of ab_n_mu is not finite and ascending", s.enable_timelines, 4, (7, -3), (-2, 6))
    _refused(ValueError, "timelines: the range [-2, inf) of ab_s_mu is not finite and ascending", s.enable_timelines, 4, (-3, 7), (-2, np.inf))
    _refused(ValueError, "timelines: the range [nan, 7) of ab_n_mu is not finite and ascending", s.enable_timelines, 4, (np.nan, 7), (-2, 6))
    q = np.array([1.5, 0.5])
    _refused(ValueError, "timelines: n_q=0 outside [1, 8]", _direct, s, "timeline_quantiles", 0, q.ctypes.data, None, None)
    _refused(ValueError, "timelines: n_q=9 outside [1, 8]", _direct, s, "timeline_quantiles", 9, q.ctypes.data, None, None)
    _refused(ValueError, "timelines: q is NULL", _direct, s, "timeline_quantiles", 1, None, None, None)
    _refused(ValueError, "timelines: q[0]=1.5 outside [0, 1]", s.timeline_quantiles, q)  # (before "not enabled")
    _refused(ValueError, "timelines: q[1]=1.5 outside [0, 1]", s.timeline_quantiles, q[::-1].copy())
    # nothing was switched on by a refused call
    _refused(AbdError, STATE + "timelines are not enabled (abd_sampler_enable_timelines)", s.timelines, 0)
    _refused(AbdError, STATE + "diagnostics are not enabled (abd_sampler_enable_diagnostics)", s.diagnostics, 0)


def test_set_adaptation(case):
    s = case.fresh
    im = np.ones(17)
    im[3] = 0.0
    _refused(ValueError, "inv_mass[3]=0 is not a positive finite number", s.set_adaptation, 0, im)
    im[3] = np.inf
    _refused(ValueError, "inv_mass[3]=inf is not a positive finite number", s.set_adaptation, 1, im)
    _refused(ValueError, "step_size is not finite", s.set_adaptation, 0, None, np.inf)
    # A chain runs a dense metric once its first window of more than 17 tuning draws has closed: the one sampler here with a tuning
    # phase of 20 and 19 iterations (a dense metric rules the trains out: result rows, whatever the case's mode)
    with _env(**case.env):
        d = case.ctx.sampler(np.arange(N_CHAINS), case.q0, tune=20, seed=7, dense_metric=True)
    assert d.launch_shape()["trains"] == "none"
    _refused(ValueError, "inv_mass[3]=inf is not a positive finite number", d.set_adaptation, 1, im)  # (still diagonal)
    d.run(19)
    assert np.count_nonzero(d.metric(1)) > 17
    _refused(AbdError, STATE + "chain 1 runs a dense metric", d.set_adaptation, 1, np.ones(17))
    _refused(ValueError, OUTSIDE % 2, d.set_adaptation, 2, im)
    d.close()
