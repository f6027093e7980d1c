"""
The host NUTS bit for bit against recorded chains (abdpymc_amd.sampler: Nuts, WindowedAdaptation, sample_chain; abdpymc_amd.survival:
_chain, _chain_gen, sample_draws): ``record`` below runs every caller of the one tree builder and the one adaptation loop on
closed-form targets, and ``tests/golden/host_nuts_golden.npz`` holds what it returned when the tree builder and the adaptation loop
still existed in several copies (``tests/golden/NOTICE_host_nuts.md``).  The targets use + - * / only, so the only libm calls are
the sampler's own.
"""
import os
import types

import numpy as np
import pytest

from abdpymc_amd import sampler, survival
from abdpymc_amd.model import THETA_NAMES

DIM = 5
SCALES = np.array([0.25, 0.5, 1.0, 2.0, 4.0])  # unequal: the metric adaptation has something to find
CENTRE = np.array([1.0, -2.0, 0.5, 3.0, -1.0])
WALL = 0.3  # of the walled target: logp = -inf where q[0] > WALL, close to the start and to the mode
STATS = ("lp", "tree_depth", "mean_tree_accept", "step_size", "n_steps", "diverging")
SEEDS = (0, 1, 2)
TUNE, DRAWS = 150, 100


def gaussian(scales=SCALES, centre=CENTRE):
    w = 1.0 / (scales * scales)

    def fn(q):
        d = q - centre
        return -0.5 * float(np.sum(w * d * d)), -(w * d)

    return fn


def walled(q):
    if q[0] > WALL:
        return -np.inf, np.zeros_like(q)
    return -0.5 * float(np.sum(q * q)), -q


def _put(out, prefix, chain):
    draws, stats = chain
    out[prefix + "_draws"] = draws
    for name in STATS:
        out[f"{prefix}_stat_{name}"] = stats[name]


def drive_by_hand(gen, fn):
    """a generator of points against ``fn``, written out: the protocol ``sample_draws`` speaks to its chains"""
    q = next(gen)
    while True:
        try:
            q = gen.send(fn(q))
        except StopIteration as fin:
            return fin.value


class _DiscreteTarget:
    """What ``sample_chain`` asks of a context, without ``gibbs_sweep`` (the host sweep runs): a Gaussian in the 17 value variables
    whose centre and height depend on the G N + N bits."""

    def __init__(self, G, N):
        self.bits = np.zeros(G * N + N, dtype=np.int8)
        self.u = 0.05 * (1.0 + np.arange(G * N + N))
        self.w = 1.0 / (0.5 + 0.125 * np.arange(len(THETA_NAMES)))
        self.n_logp = 0

    def set_discrete(self, chain, i_raw, waner):
        self.bits = np.concatenate([np.asarray(i_raw).ravel(), np.asarray(waner).ravel()]).astype(np.int8)

    def flip_discrete(self, chain, idx):
        self.bits[idx] ^= 1

    def logp_dlogp(self, chain, q):
        d = q - float(np.sum(self.u * self.bits))
        return -0.5 * float(np.sum(self.w * d * d)) - 0.3 * float(np.sum(self.bits)), -(self.w * d)

    def logp(self, chain, q):
        self.n_logp += 1
        return self.logp_dlogp(chain, q)[0]


def discrete_model(G=2, N=3):
    pt = {name: 0.1 * k - 0.5 for k, name in enumerate(THETA_NAMES)}
    pt["i_raw"], pt["ab_s_waner"] = np.zeros((G, N), dtype=np.int8), np.zeros(N, dtype=np.int8)
    return types.SimpleNamespace(ctx=_DiscreteTarget(G, N), n_gaps=G, n_inds=N, initial_point=lambda: dict(pt),
                                 ravel=lambda p: np.array([float(p[n]) for n in THETA_NAMES]))


def draws_model():
    """three datasets for ``sample_draws``: the Gaussian at three sets of scales"""
    fns = [gaussian(SCALES * f, CENTRE + m) for m, f in enumerate((1.0, 0.5, 2.0))]
    model = types.SimpleNamespace(dim=DIM, K=1, n_datasets=3, names=tuple(f"x{k}" for k in range(DIM)), constrain=lambda q: {},
                                  initial_point=lambda: np.zeros(DIM))

    def evaluator(datasets, q):
        out = [fns[int(m)](row) for m, row in zip(datasets, q)]
        return np.array([o[0] for o in out]), np.stack([o[1] for o in out])

    return model, evaluator


def record(sampler, survival):
    """Every array the fixture holds, from the given modules."""
    out = {}
    fn = gaussian()
    for s in SEEDS:
        _put(out, f"gauss_chain_s{s}", survival._chain(fn, DIM, TUNE, DRAWS, np.random.default_rng([11, s]), 0.8, None))
        _put(out, f"gauss_gen_s{s}", drive_by_hand(survival._chain_gen(DIM, TUNE, DRAWS, np.random.default_rng([11, s]), 0.8, None), fn))
        _put(out, f"wall_chain_s{s}", survival._chain(walled, DIM, TUNE, DRAWS, np.random.default_rng([12, s]), 0.9, np.full(DIM, -1.0)))
    _put(out, "gauss_fixed", survival._chain(fn, DIM, 5, 40, np.random.default_rng(13), q0=CENTRE, adapt=False, step_size=0.05))
    model, evaluator = draws_model()
    fit = survival.sample_draws(model, tune=TUNE, draws=DRAWS, chains_per_dataset=1, seed=14, evaluator=evaluator)
    for name in model.names + tuple("stat_" + k for k in STATS) + ("dataset", "n_evaluations", "n_calls"):
        out["draws_" + name] = np.asarray(fit[name])
    # the kernel alone: the depth cap, and the step size search beside the wall
    rng = np.random.default_rng(15)
    nuts = sampler.Nuts(fn, DIM, rng, max_treedepth=3)
    q = CENTRE + rng.uniform(-1, 1, size=DIM)
    lp, g = fn(q)
    nuts.eps = nuts.find_reasonable_eps(q, lp, g)
    nuts.da = sampler.DualAveraging(nuts.eps)
    rows = []
    for it in range(80):
        if it == 40:
            nuts.eps = 0.02  # trees that only the cap ends
        q, lp, g, st = nuts.step(q, lp, g, adapt=it < 40)
        rows.append(np.concatenate([q, [lp, st["tree_depth"], st["mean_tree_accept"], st["step_size"], st["n_steps"], st["diverging"]]]))
    out["capped_rows"], out["capped_n_grad"], out["capped_eps"] = np.array(rows), np.array(nuts.n_grad), np.array(nuts.eps)
    eps = []
    for s in range(8):
        near = sampler.Nuts(walled, DIM, np.random.default_rng(1600 + s))  # momenta towards the wall and away from it
        q = np.zeros(DIM)
        q[0] = WALL - 0.02
        eps.append(near.find_reasonable_eps(q, *walled(q)))
    out["wall_eps"] = np.array(eps)
    # the compound chain on the host sweep
    for c in (0, 1):
        m = discrete_model()
        res = sampler.sample_chain(m, c, TUNE, 40, seed=17, record_deterministics=False)
        out[f"compound_c{c}_q"] = np.stack([res[name] for name in THETA_NAMES], axis=-1)
        for name in ("i_raw", "ab_s_waner", "n_grad_evals") + tuple(k for k in sorted(res) if k.startswith("stat_")):
            out[f"compound_c{c}_{name}"] = np.asarray(res[name])
        out[f"compound_c{c}_n_logp"] = np.array(m.ctx.n_logp)
    return out


@pytest.fixture(scope="module")
def golden(golden_dir):
    with np.load(os.path.join(golden_dir, "host_nuts_golden.npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def now():
    return record(sampler, survival)


def _same(golden, now, prefix):
    keys = [k for k in golden if k.startswith(prefix)]
    assert keys and sorted(keys) == sorted(k for k in now if k.startswith(prefix))
    for k in keys:
        assert now[k].dtype == golden[k].dtype, k
        np.testing.assert_array_equal(now[k], golden[k], err_msg=k)


def test_every_recorded_array_is_computed(golden, now):
    assert sorted(golden) == sorted(now)


def test_chain_on_the_gaussian(golden, now):
    _same(golden, now, "gauss_chain_")
    for s in SEEDS:  # the adaptation found the scales: real trees, a metric far from the unit one
        assert golden[f"gauss_chain_s{s}_stat_tree_depth"].max() >= 3
        assert golden[f"gauss_chain_s{s}_draws"].shape == (DRAWS, DIM)
        assert len(np.unique(golden[f"gauss_chain_s{s}_stat_step_size"])) == 1  # da.final() holds through the draws


def test_generator_driven_by_hand_is_the_chain(golden, now):
    _same(golden, now, "gauss_gen_")
    for s in SEEDS:
        for name in ("draws",) + tuple("stat_" + k for k in STATS):
            np.testing.assert_array_equal(golden[f"gauss_gen_s{s}_{name}"], golden[f"gauss_chain_s{s}_{name}"])


def test_sample_draws_on_three_datasets(golden, now):
    _same(golden, now, "draws_")
    assert golden["draws_dataset"].tolist() == [0, 1, 2] and int(golden["draws_n_calls"]) < int(golden["draws_n_evaluations"])


def test_walled_target_takes_the_non_finite_branches(golden, now):
    _same(golden, now, "wall_")
    div = np.concatenate([golden[f"wall_chain_s{s}_stat_diverging"] for s in SEEDS]) != 0
    depth = np.concatenate([golden[f"wall_chain_s{s}_stat_tree_depth"] for s in SEEDS])
    steps = np.concatenate([golden[f"wall_chain_s{s}_stat_n_steps"] for s in SEEDS])
    assert div.sum() >= 1                          # a last subtree whose every leaf lay behind the wall
    assert (steps < 2.0 ** (depth - 1)).sum() >= 1  # a subtree that s1 = False cut before its 2^(j-1) leaves
    assert (steps[div] < 2.0 ** (depth[div] - 1)).any() or (depth[div] == 1).any()
    for s in SEEDS:
        assert (golden[f"wall_chain_s{s}_draws"][:, 0] <= WALL).all()
    assert (golden["wall_eps"] < 0.1).any() and (golden["wall_eps"] >= 0.1).any()  # the search halves where the first step crosses


def test_depth_cap_ends_trees(golden, now):
    _same(golden, now, "capped_")
    depth, n_steps = golden["capped_rows"][:, DIM + 1], golden["capped_rows"][:, DIM + 4]
    assert (depth[40:] == 3).all() and (n_steps[40:] == 4).all() and depth.max() == 3


def test_fixed_step_size_without_adaptation(golden, now):
    _same(golden, now, "gauss_fixed_")
    assert (golden["gauss_fixed_stat_step_size"] == 0.05).all()


def test_compound_chain_on_the_host_sweep(golden, now):
    _same(golden, now, "compound_")
    for c in (0, 1):
        assert golden[f"compound_c{c}_q"].shape == (40, len(THETA_NAMES)) and golden[f"compound_c{c}_i_raw"].shape == (40, 2, 3)
        assert 0 < golden[f"compound_c{c}_i_raw"].mean() < 1 and int(golden[f"compound_c{c}_n_logp"]) > 0  # the bits move
        assert len(np.unique(golden[f"compound_c{c}_stat_step_size"])) == 1
