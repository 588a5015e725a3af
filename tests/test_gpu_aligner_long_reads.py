"""GPU window aligner on reads of 255 to 510 bases (the wide instantiation of the span and extension kernels) against the
library's host aligner and the oracle: identical Aligment records for every window, equal values, and the aligner's
counters show that the device did the work (reference AlignSubpathInternal graph.cc:839-899). The host aligner itself is
pinned against the oracle at these lengths by tests/test_long_reads_host.py."""
import time

import numpy as np
import pytest

from gaml_amd import synth
from long_reads_cases import long_read_case

pytestmark = pytest.mark.gpu


def _pack_ragged(reads):
    offs = np.zeros(len(reads) + 1, np.int64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    return np.ascontiguousarray(np.concatenate(reads) if reads else np.zeros(0, np.uint8)), offs


def _ctx(api, gb, go, reads, aligner_route, mean, sd):
    ctx = api.Context(device=0)
    ctx.debug_set_knob(api.Knob.ALIGNER_ROUTE, aligner_route)
    ctx.set_graph(gb, go)
    ctx.add_paired(api.paired_cfg(mean, sd), *reads)
    return ctx


def _oracle(gb, go, reads, mean, sd):
    import oracle_py as op
    orc = op.Oracle()
    orc.set_graph(gb, go)
    orc.add_paired(*reads, 0.01, op.paired_cfg(mean, sd))
    return orc


def _all_windows(ctx, mate):
    return [tuple(ctx.debug_window_walk(0, mate, w)) for w in range(ctx.window_count(0, mate))]


def _device_equals_host_and_oracle(gb, go, reads, sets, mean, sd):
    """A device-aligner context and its host-aligner twin (AlignerRoute.HOST) over `sets`: equal values and floored counts, the
    likelihood within 1e-9 of the oracle's, the device counted its windows, every window of both mates identical to the
    host aligner's, every fifth window of mate 1 identical to the oracle's. Returns the device context."""
    from gaml_amd import api
    gpu, cpu = _ctx(api, gb, go, reads, 0, mean, sd), _ctx(api, gb, go, reads, api.AlignerRoute.HOST, mean, sd)
    orc = _oracle(gb, go, reads, mean, sd)
    for paths in sets:
        a, b = gpu.calc_prob(paths), cpu.calc_prob(paths)
        assert a[0] == b[0] and a[1].tolist() == b[1].tolist()
        want = orc.calc_prob(paths, fresh=True)[0]
        assert abs(a[0] - want) <= 1e-9 * abs(want), (a[0], want)
    st = gpu.aligner_stats()
    print("device aligner:", st)
    assert st["windows"] > 0 and st["candidates"] > 0
    assert cpu.aligner_stats()["windows"] == 0 and cpu.aligner_stats()["candidates"] == 0
    n_records = 0
    for mate in (0, 1):
        wa, wb = _all_windows(gpu, mate), _all_windows(cpu, mate)
        assert wa == wb
        for key in wa:
            ra, rb = gpu.window_records(0, mate, list(key)), cpu.window_records(0, mate, list(key))
            assert ra.shape == rb.shape and (ra == rb).all(), key
            n_records += len(ra)
    assert n_records > 0
    for key in _all_windows(gpu, 0)[::5]:
        orc.align_window(0, 0, list(key))
        assert (orc.window_records(0, 0, list(key)) == gpu.window_records(0, 0, list(key))).all(), key
    return gpu


@pytest.mark.parametrize("L", [255, 300, 400, 510])
def test_gpu_records_equal_host_aligner_and_oracle_on_long_reads(L):
    g, pr, sets = long_read_case(L)
    reads = (*synth.pack_reads(pr.mate1), *synth.pack_reads(pr.mate2))
    _device_equals_host_and_oracle(*g.packed(), reads, sets, 2.2 * L, 0.2 * L)


def test_mixed_mates_narrow_and_wide():
    """Mate 1 of 150 bases, mate 2 of 300: the general route runs the narrow kernels for mate 1 and the wide ones for mate 2;
    the small batches of the annealing walk run both mates in the wide paired pipeline."""
    from gaml_amd import api
    g, pr, sets = long_read_case(300)
    reads = (*synth.pack_reads(np.ascontiguousarray(pr.mate1[:, :150])), *synth.pack_reads(pr.mate2))
    gb, go = g.packed()
    _device_equals_host_and_oracle(gb, go, reads, sets, 660.0, 60.0)
    gpu, cpu = _ctx(api, gb, go, reads, 0, 660.0, 60.0), _ctx(api, gb, go, reads, api.AlignerRoute.HOST, 660.0, 60.0)
    start, seq = synth.sa_sequence(g, 60, seed=3, threshold=400)
    for ps in [start] + seq:
        a, b = gpu.calc_prob(ps), cpu.calc_prob(ps)
        assert a[0] == b[0] and a[1].tolist() == b[1].tolist()
    assert gpu.aligner_stats()["windows"] > 0 and cpu.aligner_stats()["windows"] == 0
    for mate in (0, 1):
        wa = _all_windows(gpu, mate)
        assert wa == _all_windows(cpu, mate)
        for key in wa:
            assert gpu.window_records(0, mate, list(key)).tobytes() == cpu.window_records(0, mate, list(key)).tobytes(), key


def test_ragged_lengths_across_254():
    """Mate 1 with ragged lengths 200..330 (the index is built for the LAST read's length, graph.cc:1286; the span chunking
    follows it, the choice of kernels follows the longest read), mate 2 of 150 bases."""
    L = 330
    g, pr, sets = long_read_case(L)
    rng = np.random.default_rng(5)
    m1 = [pr.mate1[i, : int(rng.integers(200, 331))].copy() for i in range(len(pr.mate1))]
    assert min(len(r) for r in m1) < 254 < max(len(r) for r in m1)
    reads = (*_pack_ragged(m1), *synth.pack_reads(np.ascontiguousarray(pr.mate2[:, :150])))
    _device_equals_host_and_oracle(*g.packed(), reads, sets, 2.2 * L, 0.2 * L)


def test_three_routes_agree_at_300_bases():
    """The paired small-batch pipeline (wide: both mates in one kernel), one small pipeline per mate (AlignerRoute.PER_MATE) and the
    general route (AlignerRoute.GENERAL) along an annealing-style walk: bit-equal values and records, equal window counts."""
    from gaml_amd import api
    G, n, seed, L = 120_000, 6000, 77, 300
    genome = synth.plant_repeats(synth.make_genome(G, seed), 2, 700, seed)
    g = synth.make_graph(genome, synth.cut_lengths(G, seed, long_rng=(600, 4000), short_rng=(25, 330)))
    pr = synth.make_paired_reads(genome, n, L, 660.0, 66.0, 0.01, seed)
    gb, go = g.packed()
    reads = (*synth.pack_reads(pr.mate1), *synth.pack_reads(pr.mate2))
    fast, per_mate, general = (_ctx(api, gb, go, reads, k, 660.0, 66.0) for k in (0, api.AlignerRoute.PER_MATE, api.AlignerRoute.GENERAL))
    start, seq = synth.sa_sequence(g, 120, seed=3, threshold=400)
    for ps in [start] + seq:
        a, b, c = fast.calc_prob(ps), general.calc_prob(ps), per_mate.calc_prob(ps)
        assert a[0] == b[0] == c[0] and a[1].tolist() == b[1].tolist() == c[1].tolist()
    assert fast.aligner_stats()["windows"] == general.aligner_stats()["windows"] == per_mate.aligner_stats()["windows"] > 0
    for mate in (0, 1):
        wa = _all_windows(fast, mate)
        assert wa == _all_windows(general, mate) == _all_windows(per_mate, mate)
        for key in wa:
            rec = fast.window_records(0, mate, list(key)).tobytes()
            assert rec == general.window_records(0, mate, list(key)).tobytes() == per_mate.window_records(0, mate, list(key)).tobytes()


def test_the_cap_holds_at_510():
    """One read of 511 bases in either mate: the host aligner serves the whole set, with the same values."""
    from gaml_amd import api
    g, pr, sets = long_read_case(300)
    longer = synth.make_paired_reads(synth.make_genome(90_000, 81 + 300), 1, 511, 1200.0, 20.0, 0.005, 9)
    m1, m2 = [r for r in pr.mate1], [r for r in pr.mate2]
    m1[17], m2[17] = longer.mate1[0], longer.mate2[0]
    reads = (*_pack_ragged(m1), *_pack_ragged(m2))
    gb, go = g.packed()
    gpu, cpu = _ctx(api, gb, go, reads, 0, 660.0, 60.0), _ctx(api, gb, go, reads, api.AlignerRoute.HOST, 660.0, 60.0)
    for paths in sets:
        a, b = gpu.calc_prob(paths), cpu.calc_prob(paths)
        assert a[0] == b[0] and a[1].tolist() == b[1].tolist()
    assert gpu.aligner_stats()["windows"] == 0 and cpu.aligner_stats()["windows"] == 0


def test_device_aligner_is_faster_than_host_at_2x300():
    """The cold first evaluation of the 2 x 300 workload: the relation tests/test_gpu_aligner.py asserts at cfg2."""
    from gaml_amd import api
    wl = synth.WORKLOADS["cfg2x300"]
    genome = synth.make_genome(wl.genome_len, wl.seed)
    g = synth.make_graph(genome, synth.cut_lengths(wl.genome_len, wl.seed))
    pr = synth.make_paired_reads(genome, wl.n_pairs, wl.read_len, wl.insert_mean, wl.insert_std, wl.err, wl.seed)
    gb, go = g.packed()
    reads = (*synth.pack_reads(pr.mate1), *synth.pack_reads(pr.mate2))
    walk = synth.genome_walk(g)
    out = {}
    for name, route in (("gpu", 0), ("cpu", api.AlignerRoute.HOST)):
        ctx = _ctx(api, gb, go, reads, route, wl.insert_mean, wl.insert_std)
        t0 = time.time()
        out[name] = (ctx.calc_prob([walk]), time.time() - t0, ctx)
    assert out["gpu"][0][0] == out["cpu"][0][0] and out["gpu"][0][1].tolist() == out["cpu"][0][1].tolist()
    assert out["gpu"][2].aligner_stats()["windows"] > 0 and out["cpu"][2].aligner_stats()["windows"] == 0
    print(f"cold CalcProb 2x300: gpu aligner {out['gpu'][1]:.3f} s ({out['gpu'][2].aligner_stats()}), host aligner {out['cpu'][1]:.3f} s")
    assert out["gpu"][1] < out["cpu"][1]
