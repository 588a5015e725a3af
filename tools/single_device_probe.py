"""Cost of evaluations on a context whose only read set is single-end, with its windows aligned and its read-major table
built on the host (today's route) or on the device (Context.set_single_device): one JSON line per run.

One run is one leg -- the library is chosen when the process starts, so the legs of a comparison are separate runs, alternated
by the job that starts them:

  p  another build of the library, named by GAML_HIP_LIB (the parent commit's development build), as it is
  f  this tree with the context's switch off (the default) -- must equal p within the spread of the rounds
  o  this tree with Context.set_single_device(True): windows aligned in device batches, the record pool mirrored, the table
     rebuilt by the kernels of gaml_amd/csrc/single_tables.hip.h

Workloads:
  cfg1     BASELINE config 1: a 50 kbp graph, 10,000 single-end reads of 100 bases
  cfg1big  a single-end set of cfg3's size: 833,333 reads of 100 bases on synth.WORKLOADS["cfg3"]'s graph

Reported: the cold first call (the start assembly of synth.sa_sequence: every window new); the annealing pattern of
synth.sa_sequence, one blocking call per edited path set -- median and p90 over all calls and the median over the calls that
aligned new windows; batches of 8 candidates one edit away from the current assembly with set_single_onepass on, microseconds
per path set. The last value of the sequence is printed in hex: the legs must agree on its bits.

Usage: python tools/single_device_probe.py --leg o --workload cfg1big [--iters 80] [--batches 8] [--tag NAME]
       GAML_HIP_LIB=build_ab/libgaml_hip_parent.so python tools/single_device_probe.py --leg p --workload cfg1
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

os.environ.setdefault("GAML_HIP_FLAVOUR", "dev")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gaml_amd import api, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", required=True, choices=["p", "f", "o"])
    ap.add_argument("--workload", default="cfg1", choices=["cfg1", "cfg1big"])
    ap.add_argument("--iters", type=int, default=80)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    if a.leg == "p" and not os.environ.get("GAML_HIP_LIB"):
        sys.exit("leg p scores with another build of the library: name it in GAML_HIP_LIB")
    if a.workload == "cfg1":
        seed, n_reads = 101, 10_000
        genome = synth.make_genome(50_000, seed)
        g = synth.make_graph(genome, synth.cut_lengths(50_000, seed))
    else:
        wl = synth.WORKLOADS["cfg3"]
        seed, n_reads = wl.seed, wl.n_pairs
        genome, g = wl.build()
    ctx = api.Context(device=a.device)
    ctx.set_graph(*g.packed())
    rs = ctx.add_single(api.single_cfg(), *synth.pack_reads(synth.make_single_reads(genome, n_reads, 100, 0.01, seed + 1)))
    if a.leg == "o":
        ctx.set_single_device(True)
    start, seq = synth.sa_sequence(g, a.iters, seed=seed % 1000, threshold=500)

    t0 = time.perf_counter()
    ctx.calc_prob(start)
    cold_us = (time.perf_counter() - t0) * 1e6
    us, new = [], []
    for paths in seq:
        before = ctx.window_count(rs, 0)
        fp = api.FlatPaths(paths)
        t0 = time.perf_counter()
        value = ctx.score(fp)
        us.append((time.perf_counter() - t0) * 1e6)
        new.append(ctx.window_count(rs, 0) > before)
    us, new = np.array(us), np.array(new)

    ctx.set_single_onepass(True)
    rng = np.random.default_rng(seed % 1000)
    cur, per_set = seq[-1], []
    for _ in range(a.batches):
        b = api.BatchPaths([synth.sa_move(rng, cur, g) for _ in range(8)])
        t0 = time.perf_counter()
        ctx.calc_prob_batch(b)
        per_set.append((time.perf_counter() - t0) * 1e6 / 8)

    res = {"tag": a.tag, "leg": a.leg, "lib": os.environ.get("GAML_HIP_LIB", ""), "version": api.version(), "workload": a.workload, "reads": n_reads,
           "paths": len(start), "iters": a.iters, "cold_first_call_us": round(cold_us, 1),
           "sa_median_us": round(float(np.median(us)), 2), "sa_p90_us": round(float(np.percentile(us, 90)), 2),
           "sa_new_window_calls": int(new.sum()), "sa_new_window_median_us": round(float(np.median(us[new])), 2) if new.any() else None,
           "batch_us_per_set_median": round(float(np.median(per_set)), 2), "batch_us_per_set": [round(x, 2) for x in per_set],
           "windows": ctx.window_count(rs, 0), "aligner": ctx.aligner_stats(), "last_value": float(value).hex()}
    if hasattr(api.lib(), "gaml_hip_single_device_stats"):
        res["single_device"] = ctx.get_single_device()
        res["single_device_stats"] = ctx.single_device_stats(rs)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
