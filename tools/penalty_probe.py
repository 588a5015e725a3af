"""Cost of blocking evaluations of a read set WITH a coverage penalty (the reference's jumping library, example.cfg:20-29, on
cfg3j as bench.py's `jumping` block sets it up): one JSON line.

  a  1,000 single-edit annealing steps (synth.sa_sequence from the start state) in a context of its own: per call the
     median, p90 and max, and the median of gaml_hip_last_phases -- the calls that share most paths with their predecessor
  b  the 8 rotating unrelated path sets of bench.py (every call a whole-set call), 400 calls
  c  200 gaml_hip_fix_gap_length searches at the sites tools/gap_probe.py uses (a penalised set: the fallback route, one
     blocking call per evaluation; its steps of 2-3 lengths are batches -- or, with --gap-penalty-device, the device route:
     passes of up to 8 lengths, every length's coverage layout derived on the device)
  d  gaml_hip_calc_prob_batch: 200 batches of 8 single-edit candidates of the current assembly (synth.sa_move, 60 % of the
     batches adopt one candidate), 100 batches of the 8 unrelated path sets of part b, and 100 batches each of the first
     2, 3 and 4 candidates (the sizes of the gap fallback's steps): per batch and per candidate the median, p90 and max

The library under test is whatever GAML_HIP_LIB / GAML_HIP_FLAVOUR select: run it alternately on two builds (for example a
tools/build_variant.sh build of another commit), several rounds, and compare the medians of the rounds' medians against
their spread between rounds.

Usage: python tools/penalty_probe.py [--parts abcd] [--steps 1000] [--searches 200] [--tag NAME]
       rocprofv3 --kernel-trace --stats -d DIR -- python tools/penalty_probe.py --parts a
"""
from __future__ import annotations

import argparse
import gc
import json
import os
import sys
import time

import numpy as np

os.environ.setdefault("GAML_HIP_FLAVOUR", "dev")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from gaml_amd import api, synth  # noqa: E402
import gap_probe  # noqa: E402

KW = dict(penalty_constant=0.00013, penalty_step=3000.0, min_prob_start=-80.0)
PHASES = ("planning", "tables", "align", "write", "sync_tables", "launch", "bytes", "wait")


def stats(us):
    us = np.asarray(us)
    return {"median_us": round(float(np.median(us)), 2), "p90_us": round(float(np.percentile(us, 90)), 2), "max_us": round(float(us.max()), 1)}


def timed(ctx, fps, phases=None):
    us = []
    for fp in fps:
        t0 = time.perf_counter()
        ctx.score(fp)
        us.append((time.perf_counter() - t0) * 1e6)
        if phases is not None:
            phases.append(ctx.last_phases())
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--searches", type=int, default=200)
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--tag", default="")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--gap-penalty-device", action="store_true", help="part c on the gap profile's device route (Context.set_gap_penalty_device)")
    a = ap.parse_args()
    wl = synth.WORKLOADS["cfg3j"]
    genome, g = wl.build()
    pr = synth.make_paired_reads(genome, wl.n_pairs, wl.read_len, wl.insert_mean, wl.insert_std, wl.err, wl.seed)
    r1, r2 = synth.pack_reads(pr.mate1), synth.pack_reads(pr.mate2)

    def make():
        c = api.Context(device=a.device)
        c.set_graph(*g.packed())
        c.add_paired(api.paired_cfg(wl.insert_mean, wl.insert_std, **KW), *r1, *r2)
        if a.gap_penalty_device:
            c.set_gap_penalty_device(True)
        return c

    res = {"tag": a.tag, "lib": os.environ.get("GAML_HIP_LIB", ""), "version": api.version(), "workload": wl.name, "pairs": wl.n_pairs, "config": KW,
           "gap_penalty_device": bool(a.gap_penalty_device)}
    gc.disable()
    if "a" in a.parts:
        start, seq = synth.sa_sequence(g, a.steps)
        fps = [api.FlatPaths(s) for s in seq]
        ctx = make()
        ctx.calc_prob(start)           # every window of the start state aligned, tables built
        ctx.compact_tables()
        ctx.calc_prob(start)
        ph = []
        us = timed(ctx, fps, ph)
        ph = np.array(ph)
        tabs, info = ctx.debug_table_occurrences(0)
        res["a"] = dict(stats(us), steps=len(us), paths=len(start), incremental_calls=info["incremental_calls"], whole_set_calls=info["full_calls"],
                        phases_median={k: round(float(v), 2) for k, v in zip(PHASES, np.median(ph, axis=0))},
                        quiet_median_us=round(float(np.median([u for u, p in zip(us, ph) if p[2] < 1.0])), 2),  # calls that aligned no new window
                        value=ctx.score(fps[-1]), bad_bases=ctx.bad_bases(0), static_pairs=ctx.table_stats(0)["static_index_pairs"])
        ctx.close()
    if "b" in a.parts or "c" in a.parts or "d" in a.parts:
        ctx = make()
    if "b" in a.parts:
        walk = synth.genome_walk(g)
        n = len(walk)
        variants = [[list(walk)]]
        for i in range(1, 8):  # bench.py path_variants
            cut = (n * i) // 8
            cut -= cut % 2
            cut = max(1, min(n - 1, cut))
            variants.append([list(walk[:cut]), list(walk[cut:])])
        fps = [api.FlatPaths(v) for v in variants]
        for v in variants:
            ctx.calc_prob(v)
        ctx.compact_tables()
        timed(ctx, fps * 2)
        ph = []
        us = timed(ctx, [fps[i % 8] for i in range(400)], ph)
        res["b"] = dict(stats(us), calls=len(us), phases_median={k: round(float(v), 2) for k, v in zip(PHASES, np.median(np.array(ph), axis=0))},
                        value=ctx.score(fps[0]), bad_bases=ctx.bad_bases(0))
    if "c" in a.parts:
        paths, sites = gap_probe.make_sites(g, a.searches, 8, 7)
        fps = []
        for pid, pos, start in sites:
            ps = [list(p) for p in paths]
            ps[pid][pos] = -start
            fps.append(api.FlatPaths(ps))
        for fp in fps:
            ctx.score(fp)
        ctx.compact_tables()
        ctx.score(fps[0])
        for (pid, pos, start), fp in list(zip(sites, fps))[:3]:
            ctx.fix_gap_length(fp, pid, pos, trace_cap=256)
        us, evals, lengths = [], [], []
        for (pid, pos, start), fp in zip(sites, fps):
            t0 = time.perf_counter()
            length, trace = ctx.fix_gap_length(fp, pid, pos, trace_cap=256)
            us.append((time.perf_counter() - t0) * 1e6)
            evals.append(len(trace))
            lengths.append(length)
        res["c"] = dict(stats(us), searches=len(us), evaluations_per_search=round(float(np.mean(evals)), 2),
                        us_per_evaluation=round(float(np.median(np.array(us) / np.maximum(1, evals))), 2),
                        lengths_sum=int(np.sum(lengths)), gap_stats=ctx.gap_stats())
    if "d" in a.parts:
        start, seq = synth.sa_sequence(g, 60)
        base = seq[-1]
        rng = np.random.default_rng(7)
        batches, current = [], base
        for _ in range(a.batches):
            cands = [synth.sa_move(rng, current, g) for _ in range(8)]
            batches.append(cands)
            if rng.random() < 0.6:
                current = cands[int(rng.integers(0, 8))]
        walk = synth.genome_walk(g)
        n = len(walk)
        variants = [[list(walk)]]
        for i in range(1, 8):  # bench.py path_variants
            cut = (n * i) // 8
            cut -= cut % 2
            cut = max(1, min(n - 1, cut))
            variants.append([list(walk[:cut]), list(walk[cut:])])
        ctx.calc_prob(base)
        for cands in batches:          # every window the candidates touch aligned
            ctx.calc_prob_batch(cands)
        ctx.calc_prob_batch(variants)
        ctx.compact_tables()
        ctx.calc_prob(base)

        def run(lists):
            bps = [api.BatchPaths(b) for b in lists]
            us = []
            for bp in bps:
                t0 = time.perf_counter()
                ctx.calc_prob_batch(bp)
                us.append((time.perf_counter() - t0) * 1e6)
            k = len(lists[0])
            per = stats(np.asarray(us) / k)
            return dict(stats(us), batches=len(us), sets=k, per_set_median_us=per["median_us"], per_set_p90_us=per["p90_us"], per_set_max_us=per["max_us"])

        before = ctx.table_stats(0)
        d = {"candidates": run(batches)}
        ctx.calc_prob(variants[0])
        run([variants] * 3)
        d["unrelated"] = run([variants] * (a.batches // 2))
        for k in (2, 3, 4):
            ctx.calc_prob(base)
            d["candidates_%d" % k] = run([b[:k] for b in batches[: a.batches // 2]])
        after = ctx.table_stats(0)
        d["batches_patched"] = after["batches_patched"] - before["batches_patched"]
        d["batches_full"] = after["batches_full"] - before["batches_full"]
        last = ctx.calc_prob_batch(batches[-1])
        d["value"], d["bad_bases"] = last[-1][0], ctx.bad_bases(0)
        res["d"] = d
    print(json.dumps(res))


if __name__ == "__main__":
    main()
