"""Cost of one gap-length search (FixGapLength moves.cc:694-800) on a BASELINE workload, three ways: one JSON line.

  a  the search restated in Python (tests/gap_oracle.py) driving blocking gaml_hip_calc_prob calls through ctypes, one per
     evaluation, on a prebuilt flat path set whose gap entry is rewritten in place (what a caller could do before
     gaml_hip_fix_gap_length existed)
  b  gaml_hip_fix_gap_length on a context with Knob.GAP_FALLBACK: the fallback route, one batch call per step of the search
  c  gaml_hip_fix_gap_length on the device route: passes of up to 8 lengths, tables derived on the device

With --penalty the read set carries the example configuration's coverage penalty (tools/penalty_probe.py: KW), and two more
ways tell the routes of such a set apart:

  f  gaml_hip_fix_gap_length with the context's gap_penalty_device flag off: the fallback a penalised context takes by
     default (what every library before the flag does: run this way alone under GAML_HIP_LIB=<older build> for that leg)
  p  the same with the flag on: the device route, every length's coverage layout derived on the device

The path set is the genome walk cut into contigs of `--contig` nodes; a site replaces one inner node of a contig by a gap
whose starting length is the node's length, a third of it, or twice it + 5 (in turn). One search per site and way,
the ways alternated site by site, the whole round `--reps` times: per way and round the median and p90 per search; the
figure to compare is c's median against the spread of a's medians over the rounds. Every way must find the same length.

Usage: python tools/gap_probe.py --workload cfg3j [--sites 200] [--reps 5] [--ways abc]
       python tools/gap_probe.py --workload cfg3j --penalty --ways fp [--tag NAME]
       rocprofv3 --kernel-trace --stats -d DIR -- python tools/gap_probe.py --workload cfg3j --ways c --reps 1
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

os.environ.setdefault("GAML_HIP_FLAVOUR", "dev")  # way b sets a knob: the development build
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from gaml_amd import api, synth  # noqa: E402
import gap_oracle as go  # noqa: E402


def make_sites(g, n_sites, contig, seed):
    walk = synth.genome_walk(g)
    paths = [walk[k:k + contig] for k in range(0, len(walk), contig)]
    rng = np.random.default_rng(seed)
    inner = [k for k, p in enumerate(paths) if len(p) >= 5]
    sites = []
    for j in range(n_sites):
        pid = int(inner[int(rng.integers(0, len(inner)))])
        pos = int(rng.integers(2, len(paths[pid]) - 2))
        true = g.node_len(paths[pid][pos])
        start = (true, max(1, true // 3), 2 * true + 5)[j % 3]
        sites.append((pid, pos, start))
    return paths, sites


class Way:
    def __init__(self, name, ctx):
        self.name, self.ctx, self.us, self.evals, self.passes, self.lengths = name, ctx, [], [], [], []

    def search(self, fp, at, pid, pos, start):
        ctx = self.ctx
        fp.flat[at] = -start
        p0 = ctx.gap_stats()["device_passes"]
        t0 = time.perf_counter()
        if self.name == "a":
            def ev(length):
                fp.flat[at] = -length
                return ctx.score(fp)
            s = go.Search(ev, start)
            length, n = s.length, len(s.trace)
        else:
            length, trace = ctx.fix_gap_length(fp, pid, pos, trace_cap=256)
            n = len(trace)
        self.us.append((time.perf_counter() - t0) * 1e6)
        self.evals.append(n)
        self.passes.append(ctx.gap_stats()["device_passes"] - p0)
        self.lengths.append(length)
        return length


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg3j", choices=sorted(synth.WORKLOADS))
    ap.add_argument("--sites", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--contig", type=int, default=8)
    ap.add_argument("--ways", default="abc")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--penalty", action="store_true", help="the example configuration's coverage penalty on the read set")
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    kw = dict(penalty_constant=0.00013, penalty_step=3000.0, min_prob_start=-80.0) if a.penalty else {}  # (tools/penalty_probe.py: KW)
    wl = synth.WORKLOADS[a.workload]
    genome, g = wl.build()
    pr = synth.make_paired_reads(genome, wl.n_pairs, wl.read_len, wl.insert_mean, wl.insert_std, wl.err, wl.seed)
    r1, r2 = synth.pack_reads(pr.mate1), synth.pack_reads(pr.mate2)
    paths, sites = make_sites(g, a.sites, a.contig, 7)
    offs = np.zeros(len(paths) + 1, np.int64)
    offs[1:] = np.cumsum([len(p) for p in paths])

    ways = []
    for name in a.ways:
        ctx = api.Context(device=a.device)
        ctx.set_graph(*g.packed())
        ctx.add_paired(api.paired_cfg(wl.insert_mean, wl.insert_std, **kw), *r1, *r2)
        if name == "b":
            ctx.debug_set_knob(api.Knob.GAP_FALLBACK, 1)
        if name == "p" or (name == "c" and a.penalty):
            ctx.set_gap_penalty_device(True)
        ways.append(Way(name, ctx))
    # one flat path set per site (the node at the site replaced by the gap), built before anything is timed
    fps = []
    for pid, pos, start in sites:
        ps = [list(p) for p in paths]
        ps[pid][pos] = -start
        fps.append((api.FlatPaths(ps), int(offs[pid]) + pos))
    # every window the sites name, then the record tables folded once: no alignment and no table build inside a timed search
    for w in ways:
        for fp, at in fps:
            w.ctx.score(fp)
        w.ctx.compact_tables()
        w.ctx.score(fps[0][0])
        for (pid, pos, start), (fp, at) in list(zip(sites, fps))[:3]:
            w.search(fp, at, pid, pos, start)
        w.us, w.evals, w.passes, w.lengths = [], [], [], []

    res = {"tag": a.tag, "lib": os.environ.get("GAML_HIP_LIB", ""), "penalty": kw, "workload": a.workload, "pairs": wl.n_pairs, "paths": len(paths), "nodes": int(offs[-1]), "sites": a.sites, "reps": a.reps, "ways": {}}
    rounds = {w.name: [] for w in ways}
    for rep in range(a.reps):
        for w in ways:
            w.us = []
        for j, ((pid, pos, start), (fp, at)) in enumerate(zip(sites, fps)):
            got = [ways[(j + k) % len(ways)].search(fp, at, pid, pos, start) for k in range(len(ways))]
            assert len(set(got)) == 1, (pid, pos, start, got)
        for w in ways:
            rounds[w.name].append((float(np.median(w.us)), float(np.percentile(w.us, 90))))
    for w in ways:
        med = [m for m, _ in rounds[w.name]]
        res["ways"][w.name] = {
            "median_us_per_round": [round(m, 1) for m in med],
            "p90_us_per_round": [round(p, 1) for _, p in rounds[w.name]],
            "median_us": round(float(np.median(med)), 1),
            "median_spread_us": round(max(med) - min(med), 1),
            "evaluations_per_search": round(float(np.mean(w.evals)), 2),
            "device_passes_per_search": round(float(np.mean(w.passes)), 2),
            "gap_stats": w.ctx.gap_stats(),
        }
    res["final_length_median"] = float(np.median(ways[0].lengths))
    res["searches_that_move"] = int(sum(1 for n in ways[0].evals[:a.sites] if n > 3))
    if "f" in res["ways"] and "p" in res["ways"]:
        F, P = res["ways"]["f"], res["ways"]["p"]
        res["p_below_f_by_us"] = round(F["median_us"] - P["median_us"], 1)
        res["p_below_f_by_more_than_the_rounds_differ"] = bool(F["median_us"] - P["median_us"] > max(F["median_spread_us"], P["median_spread_us"]))
    if "a" in res["ways"] and "c" in res["ways"]:
        A, Cw = res["ways"]["a"], res["ways"]["c"]
        res["c_below_a_by_us"] = round(A["median_us"] - Cw["median_us"], 1)
        res["claim_holds"] = bool(A["median_us"] - Cw["median_us"] > A["median_spread_us"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
