"""Where one blocking CalcProb goes (cfg3 by default), per upload route (UPLOAD_ROUTE: 0 = host writes device memory through
the BAR, MEMCPY = staging + hipMemcpyAsync, COPY_KERNEL = staging + copy kernel) and occurrence-table route (NO_OCC_DEVICE: 0 =
whole-set calls build them on the device, 1 = on the host): medians of gaml_hip_debug_profile over 400 steps.
  python tools/phase_profile.py [cfg3|cfg2] [batch]"""
import os, sys, time
os.environ.setdefault("GAML_HIP_FLAVOUR", "dev")  # tools look inside the library: the development build
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gaml_amd import synth, api
import bench
wl = synth.WORKLOADS[sys.argv[1] if len(sys.argv) > 1 else "cfg3"]
genome = synth.make_genome(wl.genome_len, wl.seed)
g = synth.make_graph(genome, synth.cut_lengths(wl.genome_len, wl.seed))
pr = synth.make_paired_reads(genome, wl.n_pairs, wl.read_len, wl.insert_mean, wl.insert_std, wl.err, wl.seed)
ctx = api.Context(device=0)
ctx.set_graph(*g.packed())
rs = ctx.add_paired(api.paired_cfg(300.0, 30.0), *synth.pack_reads(pr.mate1), *synth.pack_reads(pr.mate2))
vp = bench.path_variants(synth.genome_walk(g))
variants = [api.FlatPaths(v) for v in vp]
[ctx.score(v) for v in variants]; ctx.compact_tables(); ctx.score(variants[0])
names = ["pass1", "tables_host", "-", "pack/write", "table_sync", "launch", "bytes", "wait"]
K, U = api.Knob, api.UploadRoute
# NO_OCC_DEVICE: whole-set calls build their occurrence tables on the host (no device route)
for knob, value in ((K.UPLOAD_ROUTE, 0), (K.UPLOAD_ROUTE, U.COPY_KERNEL), (K.UPLOAD_ROUTE, U.MEMCPY), (K.UPLOAD_ROUTE, 0),
                    (K.NO_OCC_DEVICE, 1), (K.NO_OCC_DEVICE, 0), (K.NO_OCC_DEVICE, 1), (K.NO_OCC_DEVICE, 0)):
    ctx.debug_set_knob(knob, value)
    for i in range(50): ctx.score(variants[i % 8])
    prof, ts = [], []
    for i in range(400):
        t = time.perf_counter(); ctx.score(variants[i % 8]); ts.append((time.perf_counter() - t) * 1e6); prof.append(ctx.debug_profile())
    med = np.median(np.array(prof), axis=0)
    print(f"{knob.name}={int(value)}: step median {np.median(ts):.1f} us p90 {np.percentile(ts, 90):.1f} | " + ", ".join(f"{n} {v:.1f}" for n, v in zip(names, med) if n != "-"))
    ctx.debug_set_knob(knob, 0)
print("routes:", ctx.debug_occ_route(rs) if hasattr(ctx, "debug_occ_route") else "n/a")
if len(sys.argv) > 2:
    bp = api.BatchPaths(vp)
    for route in (0, api.BatchRoute.SEQUENTIAL, 0):
        ctx.debug_set_knob(K.BATCH_ROUTE, route)
        for _ in range(5): ctx.calc_prob_batch(bp)
        t = time.perf_counter()
        for _ in range(50): ctx.calc_prob_batch(bp)
        dt = (time.perf_counter() - t) / 50
        print(f"batch of 8, BATCH_ROUTE={int(route)} ({'one pass' if route == 0 else 'sequential'}): {dt * 1e6:.1f} us per call, {dt * 1e6 / 8:.1f} us per set")
    ctx.set_event_timing(1); ctx.kernel_stats(reset=True)
    ctx.debug_set_knob(K.BATCH_ROUTE, 0)
    for _ in range(20): ctx.calc_prob_batch(bp)
    print("multi kernel:", ctx.kernel_stats(reset=True))
