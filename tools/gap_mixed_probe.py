"""Cost of a gap-length search on contexts that hold a PacBio or a single-end read set: one JSON line per run.

One run is one leg -- the library is chosen when the process starts, so the legs of a comparison are separate runs, alternated
by the job that starts them:

  p  another build of the library, named by GAML_HIP_LIB (the parent commit's development build), as it is
  f  this tree with the context's switch off (the default): the search runs on the gap profile's fallback, one batch per step
     -- must equal p within the spread of the rounds
  o  this tree with Context.set_gap_mixed_device(True): up to 8 lengths per device pass, the single-end tables and the PacBio
     count columns of every length derived on the device (gap_mixed.hip.h)

Workloads:
  cfg4    BASELINE config 4: synth.WORKLOADS["cfg2"]'s pairs plus make_pacbio_records(g, walk, 2000, 5000, 0.15, seed) at weight 0.5
  cfg2s   cfg2's pairs plus 10,000 single-end reads of 100 bases over the same graph (weight 0.25)
  cfg1    BASELINE config 1: a 50 kbp graph, 10,000 single-end reads of 100 bases, nothing else

Gap sites as tools/gap_probe.py places them: the walk as contigs of 8 nodes, one inner node replaced by a gap that starts at
the node's length, a third of it or twice it + 5. Every search runs once and the record tables are folded before anything
is timed. Reported: microseconds per search (median and p90 over sites x passes, median per pass), evaluations, lengths
scored and passes (device passes, or the fallback's batches = profile calls) per search, microseconds per pass, and
gaml_hip_last_phases of the last search's last pass. `trace_bits` are the first sites' traces: the legs must agree on them.

Usage: python tools/gap_mixed_probe.py --leg o --workload cfg4 [--passes 5] [--sites 24] [--tag NAME]
       GAML_HIP_LIB=build_ab/libgaml_hip_parent.so python tools/gap_mixed_probe.py --leg p --workload cfg1
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", required=True, choices=["p", "f", "o"])
    ap.add_argument("--workload", default="cfg4", choices=["cfg4", "cfg2s", "cfg1"])
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--sites", type=int, default=24)
    ap.add_argument("--pacbio-reads", type=int, default=2000)
    ap.add_argument("--pacbio-len", type=int, default=5000)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    if a.leg == "p" and not os.environ.get("GAML_HIP_LIB"):
        sys.exit("leg p scores with another build of the library: name it in GAML_HIP_LIB")
    ctx = api.Context(device=a.device)
    pairs = 0
    if a.workload == "cfg1":
        seed = 101
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
    if a.workload == "cfg4":
        pb = synth.make_pacbio_records(g, walk, a.pacbio_reads, a.pacbio_len, 0.15, seed)
        rs = ctx.add_pacbio(api.single_cfg(mismatch_prob=0.15, weight=0.5), pb.lens)
        for wk, rec, lp in zip(pb.walks, pb.recs, pb.logps):
            ctx.put_pacbio_records(rs, wk, rec, lp)
    else:
        rs = ctx.add_single(api.single_cfg(weight=0.25 if pairs else 1.0), *synth.pack_reads(synth.make_single_reads(genome, N_SINGLE, SINGLE_LEN, 0.01, seed + 1)))
    if a.leg == "o":
        ctx.set_gap_mixed_device(True)

    rng = np.random.default_rng(seed % 1000)
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

    # every window scored once -- by blocking calls, the same on every leg: a gap's length names no window of its own, and the
    # legs' searches evaluate different numbers of path sets, which would fold the records into the tables in another order
    # (same values to the last bit or two, not the same bits) --, the record tables folded, one untimed round of searches
    for fp, pid, pos in sites:
        ctx.calc_prob(fp)
    ctx.compact_tables()
    ctx.calc_prob(contigs)
    for fp, pid, pos in sites:
        ctx.fix_gap_length(fp, pid, pos, trace_cap=256)

    def steps(st):  # device passes, or the fallback's batches (one per profile call)
        return st["device_passes"] if st["device_lengths"] else st["calls"]

    all_us, per_pass, evals, lens_scored, n_steps, lengths, bits = [], [], [], [], [], [], []
    for p in range(a.passes):
        ctx.calc_prob(contigs)
        us = []
        for k, (fp, pid, pos) in enumerate(sites):
            s0 = ctx.gap_stats()
            t0 = time.perf_counter()
            length, trace = ctx.fix_gap_length(fp, pid, pos, trace_cap=256)
            us.append((time.perf_counter() - t0) * 1e6)
            s1 = ctx.gap_stats()
            d = {key: s1[key] - s0[key] for key in s1}
            evals.append(len(trace))
            lens_scored.append(d["device_lengths"] + d["fallback_lengths"])
            n_steps.append(steps(d))
            lengths.append(length)
            if p == 0 and k < 4:
                bits.append([[l, float(v).hex()] for l, v in trace])
        all_us += us
        per_pass.append(float(np.median(us)))
    phases = [round(float(x), 2) for x in ctx.last_phases()]

    res = {"tag": a.tag, "leg": a.leg, "lib": os.environ.get("GAML_HIP_LIB", ""), "version": api.version(), "workload": a.workload, "pairs": pairs,
           "paths": len(contigs), "sites": a.sites, "passes": a.passes,
           "gap_search_us": {"median_us": round(float(np.median(all_us)), 2), "p90_us": round(float(np.percentile(all_us, 90)), 2),
                             "min_pass_median_us": round(min(per_pass), 2), "max_pass_median_us": round(max(per_pass), 2), "per_pass_median_us": [round(x, 2) for x in per_pass]},
           "evaluations_per_search": round(float(np.mean(evals)), 2), "lengths_scored_per_search": round(float(np.mean(lens_scored)), 2),
           "steps_per_search": round(float(np.mean(n_steps)), 2), "us_per_step": round(float(np.sum(all_us) / max(1, np.sum(n_steps))), 2),
           "last_phases_us": phases, "gap_length_sum": int(np.sum(lengths)), "gap_stats": ctx.gap_stats(), "trace_bits": bits}
    if a.workload == "cfg4" and hasattr(api.lib(), "gaml_hip_pacbio_stats"):
        res["pacbio_stats"] = ctx.pacbio_stats(rs)
    if a.workload != "cfg4" and hasattr(api.lib(), "gaml_hip_single_stats"):
        res["single_stats"] = ctx.single_stats(rs)
    res["gap_mixed_device"] = ctx.gap_mixed_device()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
