"""
What a call of abd_logp_dlogp_many on a dense cohort launched, read back through the public ABI, and Python restatements of the two
rules that decide it (abd_fuse_plan.hpp: fuse_steps / fuse_plan; abd_eval.hip: dense_blocks).  TEST INFRASTRUCTURE ONLY.

After logp_dlogp_many a step that rode behind the first step of its launch leaves its result slot empty (its rows lie inside the
first step's block): ctx.fetch raises "result slot ... is empty".  The first step of every launch stays fetchable and returns the
call's own bits.  Walking the slots 0 .. K-1 therefore recovers the first step and the step count of every launch -- on a context
with more chain slots than the call has chains (observed_plan says why).
"""
import functools

import numpy as np
import pytest

S_MAX = 4  # abd_fuse_plan.hpp: kFuseMaxSteps
MIN_LAUNCHES_PER_PIPE = 4  # kFuseMinLaunchesPerPipe
MAX_ROWS = 16  # abd_types.hpp: ABD_MAX_BATCH
WAVES_PER_BLOCK = 4  # ABD_WAVES_PER_BLOCK
MIN_ROWS = 4  # abd_host.hpp: kMinRows
BLOCKS_PER_CU = 4  # abd_context.hip: dbpc


def fuse_steps(K, n, pipes):
    if n < 1 or n > MAX_ROWS:
        return 1
    for s in range(max(1, min(S_MAX, MAX_ROWS // n)), 1, -1):
        if K >= MIN_LAUNCHES_PER_PIPE * s * max(1, pipes):
            return s
    return 1


def fuse_plan(K, n, pipes, ring):
    """[(first step, steps)] of the call's launches in order; none crosses a window of `ring` result slots"""
    S = fuse_steps(K, n, pipes)
    return [(k, min(S, min(K, w0 + ring) - k)) for w0 in range(0, K, ring) for k in range(w0, min(K, w0 + ring), S)]


def k_fused(ctx):
    """fused launches on every pipe, a remainder, and the call's last launch shaped for an empty chip"""
    return 4 * S_MAX * ctx.n_pipes + 3


def pick_cpw(n):
    return 4 if n % 4 == 0 else (2 if n % 2 == 0 else 1)


def dense_blocks(n_cu, n_pipes, n_inds, n_gaps, cpw, grid_rows, steps, shared=True):
    """workgroups per grid row of a dense launch of `steps` steps (dense_blocks with blocks_max >= 16 n_cu, which never binds);
    shared: the launch is one of n_pipes in rotation (the call's last launch and every launch of a one-pipe context are not)"""
    nsub = WAVES_PER_BLOCK // cpw
    rows = -(-n_inds // 64) * n_gaps
    cap = max(1, rows // (MIN_ROWS * nsub))
    whole = n_cu * BLOCKS_PER_CU
    pipe_blocks = min(whole, n_cu * max(1, BLOCKS_PER_CU // n_pipes))
    want = max(1, pipe_blocks // max(1, steps)) if shared and n_pipes > 1 else max(n_cu, whole // max(1, grid_rows))
    return max(1, min(want, cap))


def observed_plan(ctx, K, n, lp, g=None):
    """[(first step, steps)] from the result slots the call left behind; the fetchable ones must hold the call's own bits"""
    assert K <= ctx.n_result_slots
    # a launch's block has n rows per step and a slot has ctx.n_chains: with n == ctx.n_chains a step that rode behind lands
    # exactly on its own slot's rows and stays fetchable, and the slots tell nothing.  The context needs a spare chain slot.
    assert n < ctx.n_chains, (n, ctx.n_chains)
    firsts = []
    for k in range(K):
        try:
            lp_k, g_k = ctx.fetch(k, n)
        except RuntimeError as e:
            assert f"result slot {k} is empty" in str(e), e
            continue
        assert lp_k.tobytes() == np.ascontiguousarray(lp[k]).tobytes(), f"slot {k}: logp differs from the call's"
        if g is not None:
            assert g_k.tobytes() == np.ascontiguousarray(g[k]).tobytes(), f"slot {k}: gradient differs from the call's"
        firsts.append(k)
    assert firsts and firsts[0] == 0, firsts
    return [(a, b - a) for a, b in zip(firsts, firsts[1:] + [K])]


def assert_fused(ctx, K, n, S, lp, g=None):
    """the call ran the launches abd_fuse_plan.hpp plans for (K, n, ctx.n_pipes): the largest carries S steps, and a shorter
    remainder launch ends the call (K = 16 pipes + 3 leaves one for S = 2 and 4 always, for S = 3 unless 3 divides pipes)"""
    pipes = ctx.n_pipes
    plan = observed_plan(ctx, K, n, lp, g)
    assert plan == fuse_plan(K, n, pipes, ctx.n_result_slots), (K, n, pipes, plan)
    assert max(steps for _, steps in plan) == S == fuse_steps(K, n, pipes), (K, n, pipes, S, plan)
    assert S > 1, "the call did not fuse"
    if K % S:
        assert plan[-1][1] == K % S < S, plan
    else:
        assert S == 3 and pipes % 3 == 0, (K, S, pipes)
    return plan


@functools.lru_cache(maxsize=None)
def _n_cu():
    import torch  # (the import and the first query take seconds: once per process)

    return torch.cuda.get_device_properties(0).multi_processor_count


def fused_smaller_than_single_or_skip(ctx, n_inds, n_gaps, n, S, may_skip):
    """(fused grid, single-step grid) of a launch in rotation, from the machine's CU count and the context's pipes; fused < single
    asserted -- or, where the machine's numbers make it false and the case may, skipped with the two numbers"""
    n_cu = _n_cu()
    cpw = pick_cpw(n)
    single = dense_blocks(n_cu, ctx.n_pipes, n_inds, n_gaps, cpw, n // cpw, 1)
    fused = dense_blocks(n_cu, ctx.n_pipes, n_inds, n_gaps, cpw, S * n // cpw, S)
    if not fused < single:
        msg = f"{n_cu} CUs, {ctx.n_pipes} pipes: a launch of {S} steps x {n} chains gets {fused} workgroups per row, a single step {single}"
        if may_skip:
            pytest.skip(msg)
        pytest.fail(msg)
    return fused, single
