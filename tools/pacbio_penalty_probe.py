"""Cost of a batched evaluation on BASELINE config 4 (paired + PacBio reads over one graph) when the PacBio set carries a
coverage penalty: one JSON line per run.

One run is one leg -- the library and the context's switch are chosen when the process starts, so the legs of a comparison
are separate runs, alternated by the job that starts them:

  p  another build of the library, named by GAML_HIP_LIB (the parent commit's development build), as it is: a penalised
     PacBio set keeps the whole context on one launch per read set and path set
  f  this tree with the switch off (the default): must equal p
  o  this tree with Context.set_pacbio_penalty_onepass(True): per chunk of 8 path sets one pass per read set, the chunk's
     new paths swept one contig per block behind the PacBio dispatch (pacbio_path_sweep_kernel)

Workload: the one of tools/mixed_batch_probe.py -- synth.WORKLOADS["cfg2"] pairs plus make_pacbio_records(g, walk, 2000, 5000,
0.15, seed) at weight 0.5 -- with penalty_constant = 0.0001 on the PacBio set and penalty_step = --penalty-step (default 400:
the run reports the start assembly's bad_bases, which must not be 0 for the sweep to have anything to find); a start assembly
of a few hundred paths (synth.sa_sequence); batches of 8 candidates one edit away from the current assembly, batches of 8
unrelated path sets (the walk cut into contigs of 3..10 nodes), gap-length searches on contigs of 8 nodes. Everything is
scored once and folded into the record tables before anything is timed. Reported: microseconds per candidate, per unrelated
path set and per gaml_hip_fix_gap_length search (median over the batches of a pass, then median and range over the passes),
and the counters of gaml_hip_pacbio_penalty_stats where the library has them.

Usage: python tools/pacbio_penalty_probe.py --leg o [--batches 12] [--passes 5] [--sites 24] [--tag NAME]
       GAML_HIP_LIB=build_ab/libgaml_hip_parent.so python tools/pacbio_penalty_probe.py --leg p
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
    ap.add_argument("--workload", default="cfg2", choices=sorted(synth.WORKLOADS))
    ap.add_argument("--batches", type=int, default=12)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--sites", type=int, default=24)
    ap.add_argument("--pacbio-reads", type=int, default=2000)
    ap.add_argument("--pacbio-len", type=int, default=5000)
    ap.add_argument("--penalty-step", type=float, default=400.0)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    if a.leg == "p" and not os.environ.get("GAML_HIP_LIB"):
        sys.exit("leg p scores with another build of the library: name it in GAML_HIP_LIB")
    wl = synth.WORKLOADS[a.workload]
    genome, g = wl.build()
    walk = synth.genome_walk(g)
    pr = synth.make_paired_reads(genome, wl.n_pairs, wl.read_len, wl.insert_mean, wl.insert_std, wl.err, wl.seed)
    pb = synth.make_pacbio_records(g, walk, a.pacbio_reads, a.pacbio_len, 0.15, wl.seed)
    ctx = api.Context(device=a.device)
    ctx.set_graph(*g.packed())
    ctx.add_paired(api.paired_cfg(wl.insert_mean, wl.insert_std, weight=1.0), *synth.pack_reads(pr.mate1), *synth.pack_reads(pr.mate2))
    rs = ctx.add_pacbio(api.single_cfg(mismatch_prob=0.15, weight=0.5, min_prob_per_base=-1.1, penalty_constant=0.0001, penalty_step=a.penalty_step), pb.lens)
    for wk, rec, lp in zip(pb.walks, pb.recs, pb.logps):
        ctx.put_pacbio_records(rs, wk, rec, lp)
    if a.leg == "o":
        ctx.set_pacbio_penalty_onepass(True)

    start, seq = synth.sa_sequence(g, 60, seed=wl.seed % 1000, threshold=500)
    base = seq[-1]
    rng = np.random.default_rng(wl.seed % 1000)
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
    base_bad = ctx.bad_bases(rs)
    timed_pass(ctx, cand_b + other_b)
    for fp, pid, pos in sites[:3]:
        ctx.fix_gap_length(fp, pid, pos, trace_cap=256)

    before = ctx.table_stats(0)
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
    after = ctx.table_stats(0)

    def summary(v):
        return {"median_us": round(float(np.median(v)), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2), "per_pass_us": [round(x, 2) for x in v]}

    res = {"tag": a.tag, "leg": a.leg, "lib": os.environ.get("GAML_HIP_LIB", ""), "version": api.version(), "workload": a.workload, "pairs": wl.n_pairs,
           "pacbio_reads": a.pacbio_reads, "pacbio_subwalks": len(pb.walks), "pacbio_records": int(sum(len(r) for r in pb.recs)),
           "penalty_step": a.penalty_step, "start_assembly_bad_bases": int(base_bad),
           "paths": len(base), "batches": a.batches, "passes": a.passes,
           "candidates_us_per_set": summary(cand_med), "unrelated_us_per_set": summary(other_med), "gap_search_us": summary(gap_med),
           "gap_length_sum": int(np.sum(lengths)), "gap_stats": ctx.gap_stats(),
           "chunks_patched": after["batches_patched"] - before["batches_patched"], "chunks_full": after["batches_full"] - before["batches_full"]}
    if hasattr(api.lib(), "gaml_hip_pacbio_stats"):
        res["pacbio_stats"] = ctx.pacbio_stats(rs)
    if hasattr(api.lib(), "gaml_hip_pacbio_penalty_stats"):
        res["pacbio_penalty_onepass"] = ctx.get_pacbio_penalty_onepass()
        res["pacbio_penalty_stats"] = ctx.pacbio_penalty_stats(rs)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
