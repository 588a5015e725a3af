"""Single-end sets on the device route (Context.set_single_device, gaml_amd/csrc/single_device.hip.h): windows aligned in
device batches, the host's record pool mirrored, the read-major table rebuilt by the kernels of single_tables.hip.h. The
table is checked entry by entry against build_read_major (debug_single_table_check) on the hand-made records of
tests/single_table_cases.py; values, floored counts, per-read values and window records are those of a twin context with
the switch off, bit for bit and record for record."""
import numpy as np
import pytest

import single_table_cases as stc
from aligner_hard_cases import hard_case
from gaml_amd import synth

pytestmark = pytest.mark.gpu

# what tests/test_gpu_other_sets.py::test_single_end_parity holds single calls of a single-end set to, against the oracle
ORACLE_VALUE, ORACLE_READ = 1e-12, 4e-16


def _single_ctx(g, reads, on, onepass=False, cfg_kw=None):
    from gaml_amd import api
    c = api.Context(device=0)
    c.set_single_device(on)
    c.set_single_onepass(onepass)
    c.set_graph(*g.packed())
    rs = c.add_single(api.single_cfg(**(cfg_kw or {})), *reads)
    return c, rs


def _aligment(r):
    from gaml_amd import api
    out = np.zeros(len(r), api.ALIGMENT)
    out["position"], out["edit_dist"], out["read_id"], out["orientation"] = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
    return out


def _same_call(a, b):
    return a[0] == b[0] and a[1].tolist() == b[1].tolist() and a[2] == b[2]


@pytest.mark.parametrize("case", stc.cases(), ids=repr)
def test_table_build_on_hand_made_records(case):
    g, walk = stc.graph()
    reads = synth.pack_reads(stc.reads(case.n_reads))
    (a, rs), (b, _), (off, _) = _single_ctx(g, reads, True), _single_ctx(g, reads, True), _single_ctx(g, reads, False)
    builds, last_records, fed = 0, None, 0
    for step in case.steps:
        for c in (a, b, off):
            if step[0] == "put":
                c.put_window_records(rs, 0, [walk[step[1]]], _aligment(step[2]))
            elif step[0] == "align":
                c.align_window(rs, 0, [walk[step[1]]])
        if step[0] == "put":
            fed += len(step[2])
        if step[0] != "score":
            continue
        paths, counts = [[walk[x]] for x in step[1]], step[2]
        before = a.single_device_stats(rs)
        got = [c.calc_prob(paths) for c in (a, b, off)]
        st, chk = a.single_device_stats(rs), a.debug_single_table_check(rs)
        print(case, step[1], counts, st, chk, repr(got[0][0]))
        assert a.single_stats(rs)["records"] == counts["records"]
        assert chk["compared"] == case.n_reads + counts["extras"] and (chk["first"], chk["extra"], chk["sizes"]) == (0, 0, 0), chk
        builds += last_records is None or counts["records"] != last_records  # one build per change of the active windows
        last_records = counts["records"]
        assert st["device_builds"] == builds and st["host_builds"] == 0, st
        assert st["mirrored_records"] >= fed and (st["mirrored_records"] == before["mirrored_records"] or before["device_builds"] < builds)
        assert _same_call(got[0], got[1]) and _same_call(got[0], got[2])
        pa, pb, po = a.read_probs(rs), b.read_probs(rs), off.read_probs(rs)
        assert pa.tobytes() == pb.tobytes() and pa.tobytes() == po.tobytes()
        assert b.debug_single_table_check(rs)["first"] == 0 and off.single_device_stats(rs)["device_builds"] == 0
    assert builds >= 1


@pytest.fixture(scope="module")
def cfg1():
    genome = synth.make_genome(50_000, 101)
    g = synth.make_graph(genome, synth.cut_lengths(50_000, 101))
    return genome, g, synth.pack_reads(synth.make_single_reads(genome, 2000, 100, 0.01, 102))


def test_same_bits_with_the_switch_on_and_off_and_the_oracle(cfg1):
    import oracle_py as op
    genome, g, reads = cfg1
    (on, rs), (off, _) = _single_ctx(g, reads, True), _single_ctx(g, reads, False)
    orc = op.Oracle()
    orc.set_graph(*g.packed())
    ors = orc.add_single(*reads, 0.01, op.single_cfg())
    start, seq = synth.sa_sequence(g, 14, seed=101, threshold=500)
    grew = 0
    for k, paths in enumerate([start] + seq):
        before = on.window_count(rs, 0)
        a, b = on.calc_prob(paths), off.calc_prob(paths)
        want, wprobs, o3 = orc.single_detail(ors, paths)
        grew += on.window_count(rs, 0) > before
        print(k, repr(a[0]), repr(b[0]), repr(want), a[1].tolist(), a[2], on.single_device_stats(rs))
        assert _same_call(a, b), k
        assert on.read_probs(rs).tobytes() == off.read_probs(rs).tobytes()
        assert on.window_count(rs, 0) == off.window_count(rs, 0)
        chk = on.debug_single_table_check(rs)
        assert (chk["first"], chk["extra"], chk["sizes"]) == (0, 0, 0), (k, chk)
        assert a[1].tolist() == [[int(o3[0]), 2000]] and a[2] == int(o3[1])
        np.testing.assert_allclose(on.read_probs(rs), wprobs, rtol=ORACLE_READ, atol=0)
        assert abs(a[0] - want) <= ORACLE_VALUE * abs(want)
    assert grew >= 3  # (the sequence adds windows step by step)
    st = on.single_device_stats(rs)
    assert st["aligned_windows"] == on.window_count(rs, 0) == on.aligner_stats()["windows"] and st["host_builds"] == 0
    assert off.single_device_stats(rs)["device_builds"] == 0 and off.aligner_stats()["windows"] == 0


def test_batches_and_the_gap_search_with_the_switch_on_and_off(cfg1):
    genome, g, reads = cfg1
    ways = [(dev, onepass) for dev in (True, False) for onepass in (True, False)]
    ctxs = [_single_ctx(g, reads, dev, onepass) for dev, onepass in ways]
    start, seq = synth.sa_sequence(g, 18, seed=5, threshold=500)
    walk = synth.genome_walk(g)
    gap_paths = [walk[:4] + [-150] + walk[5:9], walk[9:14]]
    vals = []
    for (c, rs), way in zip(ctxs, ways):
        got = c.calc_prob_batch(seq[:9]) + c.calc_prob_batch(seq[9:])  # a chunk of 8 and a leftover set; then a chunk of 8 and one more
        length, trace = c.fix_gap_length(gap_paths, 0, 4)
        print(way, [repr(v) for v, _, _ in got[:3]], length, len(trace), c.single_device_stats(rs), c.single_stats(rs))
        vals.append(([(v, z.tolist(), tl) for v, z, tl in got], length, [(l, v) for l, v in trace], c.read_probs(rs).tobytes()))
        if way[0]:
            chk = c.debug_single_table_check(rs)
            assert (chk["first"], chk["extra"], chk["sizes"]) == (0, 0, 0), (way, chk)
            assert c.single_device_stats(rs)["host_builds"] == 0 and c.single_device_stats(rs)["device_builds"] > 0
        assert (c.single_stats(rs)["multi_launches"] > 0) == way[1]
    for way, v in zip(ways[1:], vals[1:]):
        assert v == vals[0], way


@pytest.mark.parametrize("L", [16, 100, 254, 255, 510])
def test_device_aligned_windows_hold_the_host_aligner_records(L):
    """Single-end sets cut from the aligner's hard cases (mate 1 of tests/aligner_hard_cases.py: tandem repeats in and
    across nodes, a two-letter stretch, 30 % of the reads with an inserted or deleted base)."""
    g, packed, indel, regions, sets = hard_case(L, n_uniform=1200, n_dense=400 if L <= 31 else 120)
    reads = packed[:2]
    (on, rs), (off, _) = _single_ctx(g, reads, True), _single_ctx(g, reads, False)
    assert indel[0].any() and len(regions) == 8
    for paths in sets:
        a, b = on.calc_prob(paths), off.calc_prob(paths)
        assert _same_call(a, b), (L, a, b)
        assert on.read_probs(rs).tobytes() == off.read_probs(rs).tobytes()
    n = on.window_count(rs, 0)
    assert n == off.window_count(rs, 0) > 20
    records = 0
    for wid in range(n):
        w = on.debug_window_walk(rs, 0, wid)
        assert off.debug_window_walk(rs, 0, wid) == w
        ra, rb = on.window_records(rs, 0, w), off.window_records(rs, 0, w)
        assert np.array_equal(ra, rb), (L, w)
        records += len(ra)
    st, routes = on.single_device_stats(rs), on.debug_aligner_routes()
    print(L, "windows", n, "records", records, st, on.aligner_stats(), routes)
    assert records > 500
    assert on.aligner_stats()["windows"] == st["aligned_windows"] == n > 0 and routes["flushed"] == 0
    assert off.aligner_stats()["windows"] == 0
    if L == 16:  # a batch of more than 100,000 seed candidates: its hits are ordered on the device before the host files them
        assert on.aligner_stats()["candidates"] > 100_000
    chk = on.debug_single_table_check(rs)
    assert (chk["first"], chk["extra"], chk["sizes"]) == (0, 0, 0), chk


def test_reads_the_device_aligner_does_not_cover_stay_on_the_host_aligner():
    """600 bases: past the device aligner's 510. The host aligner files the windows; the table is still built on the device."""
    genome = synth.make_genome(30_000, 61)
    g = synth.make_graph(genome, synth.cut_lengths(30_000, 61, long_rng=(900, 2500)))
    reads = synth.pack_reads(synth.make_single_reads(genome, 1500, 600, 0.002, 62))  # (few errors: the aligner accepts 3 + 3)
    (on, rs), (off, _) = _single_ctx(g, reads, True), _single_ctx(g, reads, False)
    walk = synth.genome_walk(g)
    for paths in ([walk[:8]], [walk[:8], walk[8:]], [walk]):
        assert _same_call(on.calc_prob(paths), off.calc_prob(paths))
        assert on.read_probs(rs).tobytes() == off.read_probs(rs).tobytes()
        chk = on.debug_single_table_check(rs)
        assert (chk["first"], chk["extra"], chk["sizes"]) == (0, 0, 0), chk
    st = on.single_device_stats(rs)
    print(st, on.single_stats(rs), on.aligner_stats())
    assert st["aligned_windows"] == 0 and on.aligner_stats()["windows"] == 0
    assert st["device_builds"] >= 2 and st["host_builds"] == 0 and st["mirrored_records"] > 0
    assert (on.read_probs(rs) > 0).any()


def test_beside_a_paired_set_and_across_flips_of_the_switch(cfg1):
    """2,000 pairs + 1,000 single-end reads: the context equals its switch-off twin; a third context flips the switch between
    calls (off, on, off, on, ...) and equals both, its table rebuilt on the other route after every flip."""
    from gaml_amd import api
    genome, g, _ = cfg1
    pr = synth.make_paired_reads(genome, 2000, 100, 300.0, 30.0, 0.01, 103)
    sr = synth.pack_reads(synth.make_single_reads(genome, 1000, 100, 0.01, 104))
    ctxs = []
    for on in (True, False, False):
        c = api.Context(device=0)
        c.set_single_device(on)
        c.set_graph(*g.packed())
        c.add_paired(api.paired_cfg(300.0, 30.0, weight=1.0), *synth.pack_reads(pr.mate1), *synth.pack_reads(pr.mate2))
        ctxs.append((c, c.add_single(api.single_cfg(weight=0.25), *sr)))
    (on, rs), (off, _), (flip, _) = ctxs
    start, seq = synth.sa_sequence(g, 9, seed=11, threshold=500)
    calls = [start] + seq + [seq[-1]]  # (the last set twice: a flip without new windows rebuilds all the same)
    for k, paths in enumerate(calls):
        flip.set_single_device(k % 2 == 1)
        before = flip.single_device_stats(rs)
        a, b, f = on.calc_prob(paths), off.calc_prob(paths), flip.calc_prob(paths)
        st = flip.single_device_stats(rs)
        print(k, repr(a[0]), repr(b[0]), repr(f[0]), st)
        assert a[1].tolist() == b[1].tolist() == f[1].tolist() and a[2] == b[2] == f[2]
        assert a[0] == b[0] == f[0], k  # (the paired set's tables are built the same way on all three)
        pa = on.read_probs(rs).tobytes()
        assert pa == off.read_probs(rs).tobytes() and pa == flip.read_probs(rs).tobytes()
        chk = flip.debug_single_table_check(rs)
        assert (chk["first"], chk["extra"], chk["sizes"]) == (0, 0, 0), (k, chk)
        if k:  # the table came from the other route: this call builds it anew
            grown = (st["device_builds"] - before["device_builds"], st["host_builds"] - before["host_builds"])
            assert grown == ((1, 0) if k % 2 == 1 else (0, 1)), (k, grown)
    assert on.single_device_stats(rs)["host_builds"] == 0 and off.single_device_stats(rs)["device_builds"] == 0


def test_a_repeated_path_set_aligns_uploads_and_builds_nothing(cfg1):
    genome, g, reads = cfg1
    on, rs = _single_ctx(g, reads, True)
    walk = synth.genome_walk(g)
    for paths in ([walk[:10]], [walk[:10], walk[10:]]):
        first = on.calc_prob(paths)
        st, aln = on.single_device_stats(rs), on.aligner_stats()
        assert st["aligned_windows"] > 0 and st["mirrored_records"] > 0 and st["device_builds"] > 0
        again = on.calc_prob(paths)
        assert _same_call(first, again)
        assert on.single_device_stats(rs) == st and on.aligner_stats()["windows"] == aln["windows"]
    assert st["device_builds"] == 2
