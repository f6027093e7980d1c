"""--timelines over several ranks on CPU: two gloo ranks push their chains' timelines.from_draws results, uint16 histograms
included, through distributed.gather_results, and rank 0 pools them as the CLI does (cli.add_timelines), against the answer of
one process that holds all chains."""
import os
import socket

import numpy as np

from abdpymc_amd import timelines as tl

RANGES = ((-3.0, 3.0), (-2.0, 4.0))
SPLITS = (2,)
LAST = np.array([5, 3, -1, 0, 5])


def _draws():
    rng = np.random.default_rng(4)
    i = (rng.random((3, 9, 6, 5)) < 0.2).astype(np.int8)
    return i, rng.normal(0, 3, i.shape), rng.normal(1, 3, i.shape)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q):
    import torch.distributed as dist

    from abdpymc_amd import cli
    from abdpymc_amd.distributed import gather_results, split_counts

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    counts = split_counts(3, world)  # uneven shards: 2 chains and 1
    a, b = sum(counts[:rank]), sum(counts[:rank + 1])
    i, n, s = _draws()
    mine = tl.from_draws(i[a:b], n[a:b], s[a:b], RANGES, splits=SPLITS, last_gap=LAST)
    mine["tl_hist_n"][0, 0, 0, 0] += 40000  # (a count above 2^15: the histograms travel as a signed type and must come back whole)
    assert mine["tl_hist_n"].dtype == np.uint16
    merged = gather_results(mine, counts, dist)
    out = None
    if rank == 0:
        assert merged["tl_hist_n"].dtype == np.uint16 and merged["tl_hist_n"].shape == (3, 6, 5, 64)
        assert merged["tl_inf"].dtype == np.int64 and merged["tl_range"].dtype == np.float64
        hists = {k: merged[k].copy() for k in tl.HIST_KEYS}
        sm = cli.add_timelines(merged, LAST)
        out = (hists, merged, sm["cum_p"], tl.line(sm))
    else:
        assert merged is None
    dist.barrier()
    dist.destroy_process_group()
    q.put((rank, out))


def test_two_ranks_gather_histograms_and_rank_0_pools_them():
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert got[1] is None
    hists, res, cum_p, line = got[0]
    i, n, s = _draws()
    whole = tl.from_draws(i, n, s, RANGES, splits=SPLITS, last_gap=LAST)
    whole["tl_hist_n"][0, 0, 0, 0] += 40000  # rank 0's first chain ...
    whole["tl_hist_n"][2, 0, 0, 0] += 40000  # ... and rank 1's
    for k in tl.HIST_KEYS:
        np.testing.assert_array_equal(hists[k], whole[k], err_msg=k)
    for k in ("tl_inf", "tl_cum", "tl_ninf", "tl_info", "tl_range"):
        np.testing.assert_array_equal(res[k], whole[k], err_msg=k)
    assert not any(k in res for k in tl.HIST_KEYS) and set(tl.RESULT_KEYS) <= set(res)
    pooled = tl.merge(whole)
    np.testing.assert_array_equal(res["tl_q_n"], tl.quantiles(pooled["hist_n"], tl.DEFAULT_Q, *RANGES[0]))
    np.testing.assert_array_equal(res["tl_q_s"], tl.quantiles(pooled["hist_s"], tl.DEFAULT_Q, *RANGES[1]))
    assert res["tl_q"].tolist() == [list(tl.DEFAULT_Q)] * 3
    np.testing.assert_array_equal(cum_p, pooled["cum"] / 27)
    np.testing.assert_array_equal(res["tl_summary_ab_s_mu"], res["tl_q_s"])
    assert line.startswith("timelines: ") and "27 draws" in line
