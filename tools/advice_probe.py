"""Cost of the advice move's alignment side (ExtendPathsAdv moves.cc:948-986) on a BASELINE workload: one JSON line.

  build           gaml_hip_advice_build (wall, ms): over a cache that holds the start state's windows already -- GAML's
                  order of calls: every long node's window came with the first CalcProb, nothing is left to align
                  (build_ms_warm_cache) -- and on a fresh context, where it aligns those windows itself (build_ms_cold_cache)
  query           gaml_hip_advice_candidates over `--walks` walks of an annealing-like set: contigs of the genome walk,
                  forward and reversed, some with gaps, some joined out of order (uncached windows); first pass (cold:
                  registers + aligns what is missing) and a second pass over the same walks (warm), median / p90 us
  host            the same queries on a host-only context (one core): the CPU figure the device is compared with

Usage: python tools/advice_probe.py --workload cfg3j [--walks 1000] [--host-walks 200]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gaml_amd import api, synth  # noqa: E402

THRESHOLD = 500


def walks(g, n, seed):
    rng = np.random.default_rng(seed)
    walk = synth.genome_walk(g)
    out = []
    for k in range(n):
        a = int(rng.integers(0, len(walk) - 4))
        p = list(walk[a:a + int(rng.integers(2, 30))])
        if k % 4 == 1 and len(p) > 3:
            c = int(rng.integers(1, len(p) - 1))
            p[c] = -max(1, g.node_len(p[c]))
        if k % 5 == 2:
            c = int(rng.integers(0, len(walk) - 3))
            p = p + list(walk[c:c + 3])
        if k % 2 == 1:
            p = [x ^ 1 if x >= 0 else x for x in reversed(p)]
        out.append(p)
    return out


def run(ctx, rs, ws, g, seed):
    rng = np.random.default_rng(seed)
    t, sizes = [], []
    for p in ws:
        reach = rng.integers(0, g.n_nodes, 64).tolist()
        only_out, allow_gaps = bool(rng.random() < 0.8), bool(rng.random() < 0.2)
        t0 = time.perf_counter()
        c = ctx.advice_candidates(rs, p, reach, only_out, allow_gaps)
        t.append((time.perf_counter() - t0) * 1e6)
        sizes.append(len(c))
    return np.array(t), sizes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg3j", choices=sorted(synth.WORKLOADS))
    ap.add_argument("--walks", type=int, default=1000)
    ap.add_argument("--host-walks", type=int, default=200)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    wl = synth.WORKLOADS[a.workload]
    genome, g = wl.build()
    pr = synth.make_paired_reads(genome, wl.n_pairs, wl.read_len, wl.insert_mean, wl.insert_std, wl.err, wl.seed)
    r1, r2 = synth.pack_reads(pr.mate1), synth.pack_reads(pr.mate2)
    start = [[x] for x in synth.genome_walk(g) if g.node_len(x) > THRESHOLD]  # the reference's start state (gaml.cc:1002-1005)
    ws = walks(g, a.walks, 7)
    res = {"workload": a.workload, "pairs": wl.n_pairs, "walks": a.walks, "threshold": THRESHOLD}

    ctx = api.Context(device=a.device)
    ctx.set_graph(*g.packed())
    rs = ctx.add_paired(api.paired_cfg(wl.insert_mean, wl.insert_std), *r1, *r2)
    ctx.calc_prob(start)
    t0 = time.perf_counter()
    ctx.advice_build(rs, THRESHOLD)
    res["build_ms_warm_cache"] = round((time.perf_counter() - t0) * 1e3, 3)
    res["index_entries"] = int(len(ctx.advice_index(rs)[1]))
    cold, sizes = run(ctx, rs, ws, g, 1)
    warm, _ = run(ctx, rs, ws, g, 1)
    res["query_cold_us_median"], res["query_cold_us_p90"] = round(float(np.median(cold)), 1), round(float(np.percentile(cold, 90)), 1)
    res["query_warm_us_median"], res["query_warm_us_p90"] = round(float(np.median(warm)), 1), round(float(np.percentile(warm, 90)), 1)
    res["candidates_median"] = float(np.median(sizes))

    fresh = api.Context(device=a.device)
    fresh.set_graph(*g.packed())
    frs = fresh.add_paired(api.paired_cfg(wl.insert_mean, wl.insert_std), *r1, *r2)
    t0 = time.perf_counter()
    fresh.advice_build(frs, THRESHOLD)
    res["build_ms_cold_cache"] = round((time.perf_counter() - t0) * 1e3, 1)
    fresh.close()

    host = api.Context(device=-1)
    host.set_graph(*g.packed())
    hrs = host.add_paired(api.paired_cfg(wl.insert_mean, wl.insert_std), *r1, *r2)
    t0 = time.perf_counter()
    host.advice_build(hrs, THRESHOLD)
    res["host_build_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    hw = ws[:a.host_walks]
    run(host, hrs, hw, g, 1)  # registers + aligns on the host: not what is compared
    hwarm, _ = run(host, hrs, hw, g, 1)
    res["host_query_warm_us_median"] = round(float(np.median(hwarm)), 1)
    res["speedup_warm_median"] = round(float(np.median(hwarm) / np.median(warm[:len(hw)])), 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
