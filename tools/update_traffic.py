#!/usr/bin/env python3
"""Rewrite the counter-derived numbers of profiles/traffic.json from the PMC summaries of one tools/profile_round.sh run:
usage: tools/update_traffic.py profiles/r03 PREFIX [STEPS]   (PREFIX = the run's file prefix, e.g. "d_")
Reads PREFIX{c3,c5,c2}_pmc_sq.txt / _pmc_fetch_size.txt / _pmc_write_size_l2.txt (tools/pmc_summary.py output: one block
per (kernel, grid)) and PREFIXkernel_sources_sha256.txt; keeps the notes and the algorithmic byte counts.
With STEPS > 1 the summaries come from passes over `tools/sweep.py --many K`, whose launches carry STEPS steps each
(abd_fuse_plan.hpp; a launch that shares the chip has as many workgroups as a single step's had): only `pipe_grid` of the
configs whose files are there is rewritten: the vector instructions divided by STEPS -- per step, which is what bench.py sets
against its device time per step --, the bytes as the launch moves them (its steps walk the same panel rows, so the bytes do
not divide: per step they would be fewer than one evaluation has to read) -- and the full-grid entries (one single-step launch alone on the chip), the other
configs and kernel_sources_sha256 are kept."""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
d, pre = sys.argv[1], sys.argv[2]
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 1
path = os.path.join(ROOT, "profiles", "traffic.json")
t = json.load(open(path))


def blocks(fn):
    """{workgroups: {counter: mean}} of the dense kernel's blocks in a pmc_summary file"""
    out, cur = {}, None
    for line in open(os.path.join(ROOT, d, fn)):
        m = re.search(r"abd_dense_kernel.*= (\d+) workgroups", line)
        if m:
            cur = out.setdefault(int(m.group(1)), {})
            continue
        if line.startswith("void ") or line.startswith("abd_"):
            cur = None
            continue
        m = re.match(r"\s+(\w+)\s+n=\s*\d+\s+mean=([0-9.e+]+)", line)
        if m and cur is not None:
            cur[m.group(1)] = float(m.group(2))
    return out


def hbm(f, w):
    return int(round(f * 1024 * 2 + w * 1024))


rel = os.path.relpath(os.path.join(ROOT, d), ROOT)
for cfg in ("c3", "c5", "c2"):
    if steps > 1:
        if not os.path.exists(os.path.join(ROOT, d, f"{pre}{cfg}_pmc_sq.txt")) or "pipe_grid" not in t[cfg]:
            continue
        sq, fe, wr = blocks(f"{pre}{cfg}_pmc_sq.txt"), blocks(f"{pre}{cfg}_pmc_fetch_size.txt"), blocks(f"{pre}{cfg}_pmc_write_size_l2.txt")
        pipe = sorted(sq)[0]
        f, w, v = fe[pipe]["FETCH_SIZE"], wr[pipe]["WRITE_SIZE"], sq[pipe]["SQ_INSTS_VALU"] / steps
        t[cfg]["pipe_grid"].update(
            workgroups=pipe, steps_per_launch=steps, fetch_size_kib_raw=f, write_size_kib_raw=w,
            hbm_bytes_per_launch=hbm(f, w), valu_insts_per_launch=int(v),
            valu_source=f"{rel}/{pre}{cfg}_pmc_sq.txt (SQ_INSTS_VALU / {steps}, {pipe} workgroups carrying {steps} steps)",
            note=f"a stream-ordered launch that carries {steps} consecutive steps of abd_logp_dlogp_many ({pipe} workgroups, {pipe // steps} ranges per "
                 f"chain and step, four launches sharing the chip): vector instructions per STEP (the launch's / {steps}); bytes per LAUNCH -- "
                 f"its {steps} steps walk the same panel rows, so one pass over the panels serves them all")
        print(cfg, "pipe grid", pipe, "per step of", steps, int(v), t[cfg]["pipe_grid"]["hbm_bytes_per_launch"])
        continue
    sq, fe, wr = blocks(f"{pre}{cfg}_pmc_sq.txt"), blocks(f"{pre}{cfg}_pmc_fetch_size.txt"), blocks(f"{pre}{cfg}_pmc_write_size_l2.txt")
    grids = sorted(sq)
    full, pipe = grids[-1], grids[0]
    e = t[cfg]
    e.update(fetch_size_kib_raw=fe[full]["FETCH_SIZE"], write_size_kib_raw=wr[full]["WRITE_SIZE"],
             hbm_bytes_per_launch=hbm(fe[full]["FETCH_SIZE"], wr[full]["WRITE_SIZE"]),
             valu_insts_per_launch=int(sq[full]["SQ_INSTS_VALU"]),
             valu_source=f"{rel}/{pre}{cfg}_pmc_sq.txt (SQ_INSTS_VALU, {full} workgroups)")
    if "pipe_grid" in e and pipe != full:
        e["pipe_grid"].update(workgroups=pipe, fetch_size_kib_raw=fe[pipe]["FETCH_SIZE"], write_size_kib_raw=wr[pipe]["WRITE_SIZE"],
                              hbm_bytes_per_launch=hbm(fe[pipe]["FETCH_SIZE"], wr[pipe]["WRITE_SIZE"]),
                              valu_insts_per_launch=int(sq[pipe]["SQ_INSTS_VALU"]),
                              valu_source=f"{rel}/{pre}{cfg}_pmc_sq.txt (SQ_INSTS_VALU, {pipe} workgroups)")
    print(cfg, "full grid", full, int(sq[full]["SQ_INSTS_VALU"]), e["hbm_bytes_per_launch"], "pipe grid", pipe, int(sq[pipe]["SQ_INSTS_VALU"]))
if steps > 1:  # the other entries were not collected again: their sources' sha256 (and with it bench.py's `stale`) stays
    json.dump(t, open(path, "w"), indent=1)
    sys.exit(0)
t["kernel_sources_sha256"] = open(os.path.join(ROOT, d, f"{pre}kernel_sources_sha256.txt")).read().strip()
t["_about"] = re.sub(r"profiles/r\d+/\w_\*_pmc_\*\.txt", f"{rel}/{pre}*_pmc_*.txt", t["_about"])
json.dump(t, open(path, "w"), indent=1)
print("kernel_sources_sha256", t["kernel_sources_sha256"])
