"""Cost of a batched evaluation on contexts with a single-end read set: one JSON line per run.

One run is one leg -- the library is chosen when the process starts, so the legs of a comparison are separate runs, alternated
by the job that starts them:

  p  another build of the library, named by GAML_HIP_LIB (the parent commit's development build), as it is
  f  this tree with the context's switch off (the default): a single-end set keeps the whole context on the sequential path --
     must equal p within the spread of the rounds
  o  this tree with Context.set_single_onepass(True): per chunk of 8 path sets one pass per read set
     (single_score_multi_kernel beside paired_score_multi_kernel)

Workloads:
  cfg1    BASELINE config 1: a 50 kbp graph, 10,000 single-end reads of 100 bases, nothing else
  cfg2s   synth.WORKLOADS["cfg2"]'s pairs plus 10,000 single-end reads of 100 bases over the same graph (weight 0.25)

A start assembly (synth.sa_sequence); batches of 8 candidates one edit away from the current assembly, and batches of 8
unrelated path sets (the walk cut into contigs of 3..10 nodes). Everything is scored once and folded into the record tables
before anything is timed. Reported: per kind of batch the microseconds per path set (median over the batches of a pass, then
median and range over the passes) and the microseconds per gaml_hip_fix_gap_length search on the same context (gaps in
contigs of 8 nodes, as tools/gap_probe.py places them).

Usage: python tools/single_batch_probe.py --leg o --workload cfg2s [--batches 12] [--passes 5] [--sites 24] [--tag NAME]
       GAML_HIP_LIB=build_ab/libgaml_hip_parent.so python tools/single_batch_probe.py --leg p --workload cfg1
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

N_SINGLE, SINGLE_LEN = 10_000, 100


def timed_pass(ctx, batches):
    """microseconds per path set of every batch, one call each"""
    out = []
    for b in batches:
        t0 = time.perf_counter()
        ctx.calc_prob_batch(b)
        out.append((time.perf_counter() - t0) * 1e6 / b.n_sets)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", required=True, choices=["p", "f", "o"])
    ap.add_argument("--workload", default="cfg2s", choices=["cfg1", "cfg2s"])
    ap.add_argument("--batches", type=int, default=12)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--sites", type=int, default=24)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    if a.leg == "p" and not os.environ.get("GAML_HIP_LIB"):
        sys.exit("leg p scores with another build of the library: name it in GAML_HIP_LIB")
    ctx = api.Context(device=a.device)
    if a.workload == "cfg1":
        seed, pairs = 101, 0
        genome = synth.make_genome(50_000, seed)
        g = synth.make_graph(genome, synth.cut_lengths(50_000, seed))
        ctx.set_graph(*g.packed())
    else:
        wl = synth.WORKLOADS["cfg2"]
        seed, pairs = wl.seed, wl.n_pairs
        genome, g = wl.build()
        ctx.set_graph(*g.packed())
        pr = synth.make_paired_reads(genome, wl.n_pairs, wl.read_len, wl.insert_mean, wl.insert_std, wl.err, wl.seed)
        ctx.add_paired(api.paired_cfg(wl.insert_mean, wl.insert_std, weight=1.0), *synth.pack_reads(pr.mate1), *synth.pack_reads(pr.mate2))
    walk = synth.genome_walk(g)
    rs = ctx.add_single(api.single_cfg(weight=0.25 if pairs else 1.0), *synth.pack_reads(synth.make_single_reads(genome, N_SINGLE, SINGLE_LEN, 0.01, seed + 1)))
    if a.leg == "o":
        ctx.set_single_onepass(True)

    _, seq = synth.sa_sequence(g, 60, seed=seed % 1000, threshold=500)
    base = seq[-1]
    rng = np.random.default_rng(seed % 1000)
    cand_sets, cur = [], base
    for _ in range(a.batches):
        cands = [synth.sa_move(rng, cur, g) for _ in range(8)]
        cand_sets.append(cands)
        if rng.random() < 0.6:
            cur = cands[int(rng.integers(0, 8))]
    other_sets = []
    for k in range(a.batches):
        other_sets.append([[walk[i:i + c] for i in range((k + c) % c, len(walk), c)] for c in range(3, 11)])
    cand_b = [api.BatchPaths(s) for s in cand_sets]
    other_b = [api.BatchPaths(s) for s in other_sets]

    # gap sites: contigs of 8 nodes, one inner node replaced by a gap that starts at the node's length, a third of it or twice it + 5
    contigs = [walk[k:k + 8] for k in range(0, len(walk), 8)]
    inner = [k for k, p in enumerate(contigs) if len(p) >= 5]
    sites = []
    for j in range(a.sites):
        pid = int(inner[int(rng.integers(0, len(inner)))])
        pos = int(rng.integers(2, len(contigs[pid]) - 2))
        true = g.node_len(contigs[pid][pos])
        ps = [list(p) for p in contigs]
        ps[pid][pos] = -(true, max(1, true // 3), 2 * true + 5)[j % 3]
        sites.append((api.FlatPaths(ps), pid, pos))

    # every window scored once, the record tables folded, one untimed pass of everything
    for b in cand_b + other_b:
        ctx.calc_prob_batch(b)
    for fp, pid, pos in sites:
        ctx.fix_gap_length(fp, pid, pos, trace_cap=256)
    ctx.compact_tables()
    ctx.calc_prob(base)
    timed_pass(ctx, cand_b + other_b)
    for fp, pid, pos in sites[:3]:
        ctx.fix_gap_length(fp, pid, pos, trace_cap=256)

    cand_med, other_med, gap_med, lengths = [], [], [], []
    for _ in range(a.passes):
        ctx.calc_prob(base)
        cand_med.append(float(np.median(timed_pass(ctx, cand_b))))
        other_med.append(float(np.median(timed_pass(ctx, other_b))))
        us = []
        for fp, pid, pos in sites:
            t0 = time.perf_counter()
            length, trace = ctx.fix_gap_length(fp, pid, pos, trace_cap=256)
            us.append((time.perf_counter() - t0) * 1e6)
            lengths.append(length)
        gap_med.append(float(np.median(us)))
    values = [v for v, _, _ in ctx.calc_prob_batch(cand_b[0])]  # (the legs must agree on these bits)

    def summary(v):
        return {"median_us": round(float(np.median(v)), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2), "per_pass_us": [round(x, 2) for x in v]}

    res = {"tag": a.tag, "leg": a.leg, "lib": os.environ.get("GAML_HIP_LIB", ""), "version": api.version(), "workload": a.workload, "pairs": pairs,
           "single_reads": N_SINGLE, "paths": len(base), "batches": a.batches, "passes": a.passes,
           "candidates_us_per_set": summary(cand_med), "unrelated_us_per_set": summary(other_med), "gap_search_us": summary(gap_med),
           "gap_length_sum": int(np.sum(lengths)), "gap_stats": ctx.gap_stats(), "first_batch_values": [float(v).hex() for v in values]}
    if hasattr(api.lib(), "gaml_hip_single_stats"):
        res["single_stats"] = ctx.single_stats(rs)
        res["single_onepass"] = ctx.single_onepass()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
