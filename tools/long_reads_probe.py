"""The 2x300 workload (synth.WORKLOADS["cfg2x300"]: reads above 254 bases, the aligner's wide kernels): the cold first call
with the device aligner and with the host aligner (ALIGNER_ROUTE = HOST), the small batches along the annealing pattern, the aligner's
stages -- one JSON line.  python tools/long_reads_probe.py [--iters N] [--no-host]"""
import argparse, json, os, sys, time
os.environ.setdefault("GAML_HIP_FLAVOUR", "dev")  # tools look inside the library: the development build
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gaml_amd import synth, api

ap = argparse.ArgumentParser()
ap.add_argument("--workload", default="cfg2x300")
ap.add_argument("--iters", type=int, default=400, help="annealing moves after the cold call")
ap.add_argument("--no-host", action="store_true", help="skip the host-aligner context (kernel traces: device work only)")
args = ap.parse_args()

wl = synth.WORKLOADS[args.workload]
genome = synth.make_genome(wl.genome_len, wl.seed)
g = synth.make_graph(genome, synth.cut_lengths(wl.genome_len, wl.seed))
pr = synth.make_paired_reads(genome, wl.n_pairs, wl.read_len, wl.insert_mean, wl.insert_std, wl.err, wl.seed)
reads = (*synth.pack_reads(pr.mate1), *synth.pack_reads(pr.mate2))
start, seq = synth.sa_sequence(g, args.iters)
flat = [api.FlatPaths(p) for p in seq]


def cold(aligner_route):
    ctx = api.Context(device=0)
    ctx.set_graph(*g.packed())
    ctx.add_paired(api.paired_cfg(wl.insert_mean, wl.insert_std), *reads)
    ctx.debug_set_knob(api.Knob.ALIGNER_ROUTE, aligner_route)
    t = time.perf_counter(); value = ctx.calc_prob(start)[0]; dt = time.perf_counter() - t
    return ctx, value, dt


out = {"workload": wl.name, "library": api.version(), "read_len": wl.read_len, "paths_cold": len(start)}
warm, _, _ = cold(0); warm.close()  # (the first context of a process also pays for the runtime's start)
ctx, v_dev, t_dev = cold(0)
st, sg = ctx.aligner_stats(), ctx.aligner_stages()
out["cold_device"] = {"call_ms": round(t_dev * 1e3, 2), "aligner_ms": round(st["us"] / 1e3, 2), "windows": st["windows"], "candidates": st["candidates"],
                      "stages_us": {k: round(float(v), 1) for k, v in sg.items() if k != "batches"}, "batches": sg["batches"]}
per, new_w, al_us = [], [], []
w_prev, us_prev = st["windows"], st["us"]
for f in flat:
    t = time.perf_counter(); ctx.score(f); per.append((time.perf_counter() - t) * 1e6)
    s = ctx.aligner_stats()
    new_w.append(s["windows"] - w_prev); al_us.append(s["us"] - us_prev); w_prev, us_prev = s["windows"], s["us"]
per, new_w, al_us = np.array(per), np.array(new_w), np.array(al_us)
al = new_w > 0
sg2 = ctx.aligner_stages()
out["small_batches"] = {"calls": int(len(per)), "aligning_calls": int(al.sum()), "windows": int(new_w.sum()),
                        "aligner_us_per_batch_median": round(float(np.median(al_us[al])), 1) if al.any() else None,
                        "aligner_us_per_batch_p90": round(float(np.percentile(al_us[al], 90)), 1) if al.any() else None,
                        "aligning_call_us_median": round(float(np.median(per[al])), 1) if al.any() else None,
                        "other_call_us_median": round(float(np.median(per[~al])), 1) if (~al).any() else None,
                        "batches": sg2["batches"] - sg["batches"]}
out["stages_us_total"] = {k: round(float(v), 1) for k, v in sg2.items() if k != "batches"}
v_end = ctx.calc_prob(seq[-1])[0] if seq else v_dev
ctx.close()
if not args.no_host:
    host, v_host, t_host = cold(api.AlignerRoute.HOST)
    hs = host.aligner_stats()
    per_h = []
    for f in flat:
        t = time.perf_counter(); host.score(f); per_h.append((time.perf_counter() - t) * 1e6)
    per_h = np.array(per_h)
    out["cold_host"] = {"call_ms": round(t_host * 1e3, 2), "device_windows": hs["windows"], "same_value": bool(v_host == v_dev)}
    out["small_batches"]["host_aligner_aligning_call_us_median"] = round(float(np.median(per_h[al])), 1) if al.any() else None
    out["same_value_at_the_end"] = bool((host.calc_prob(seq[-1])[0] if seq else v_host) == v_end)
    out["cold_speedup"] = round(t_host / t_dev, 2)
    host.close()
print(json.dumps(out))
