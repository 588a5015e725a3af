"""gaml_hip_calc_prob_batch over contexts with single-end sets and the context's switch on (Context.set_single_onepass): a
chunk of up to 8 path sets is scored in one pass per read set -- single_score_multi_kernel beside the paired and the PacBio
multi-set kernels -- and gives the bits, the floored counts and the per-read values of as many single calls; with the switch
off (the default) nothing moves. Inputs: tests/single_batch_cases.py (checked on the oracle by
tests/test_single_batch_cases_host.py)."""
import numpy as np
import pytest

import gap_oracle as go
import single_batch_cases as sc
from gaml_amd import synth

pytestmark = pytest.mark.gpu

COLD_PAIRED = 1e-13  # a cold paired batch fills the delta lists in another order: last bits of the sum (tests/test_gpu_batch.py)


@pytest.fixture(scope="module")
def fx():
    return sc.Fixture()


def _compare(got, want, exact):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        print(f"set {k}: {a[0]!r} / {b[0]!r}, zeros {a[1].tolist()} / {b[1].tolist()}, total length {a[2]} / {b[2]}")
    for k, (a, b) in enumerate(zip(got, want)):
        assert a[1].tolist() == b[1].tolist() and a[2] == b[2], (k, a[1].tolist(), b[1].tolist(), a[2], b[2])
        if exact:
            assert a[0] == b[0], (k, a[0], b[0])
        else:
            assert abs(a[0] - b[0]) <= COLD_PAIRED * abs(b[0]), (k, a[0], b[0])


def _same_read_probs(many, one, h, exact):
    assert np.array_equal(many.read_probs(h["single"]), one.read_probs(h["single"]))  # single-end: always the same bits
    if h["pacbio"] is not None:
        assert np.array_equal(many.read_probs(h["pacbio"]), one.read_probs(h["pacbio"]))
    if h["paired"] is not None:
        a, b = many.read_probs(h["paired"]), one.read_probs(h["paired"])
        assert np.array_equal(a, b) if exact else np.allclose(a, b, rtol=COLD_PAIRED, atol=0)


def _warm(ctxs, sets, base):
    """every window of `sets` aligned and folded into the record tables: the same device state on every context"""
    for c in ctxs:
        for s in sets:
            c.calc_prob(s)
        c.compact_tables()
        c.calc_prob(base)


def _counters(c, h):
    """chunks on the one-pass routes: (single-end, paired, PacBio)"""
    st = c.table_stats(h["paired"]) if h["paired"] is not None else None
    return (c.single_stats(h["single"])["multi_launches"], st["batches_patched"] + st["batches_full"] if st else 0,
            c.pacbio_stats(h["pacbio"])["multi_launches"] if h["pacbio"] is not None else 0)


@pytest.mark.parametrize("layout", sc.LAYOUTS)
def test_batch_equals_single_calls_bit_for_bit(fx, layout):
    (many, h), (one, _) = fx.layout(layout, onepass=True), fx.layout(layout)
    assert many.single_onepass() and not one.single_onepass()
    families = ((fx.candidates(), sc.FLOORED_CANDIDATES), (fx.unrelated(), sc.FLOORED_UNRELATED))  # 8 sets: one chunk; 9: a chunk and a leftover set
    for rnd in ("cold", "warm"):  # cold: the batch is the context's first call, windows are registered mid-chunk
        exact = rnd == "warm" or h["paired"] is None
        if rnd == "warm" and h["paired"] is not None:
            _warm([many, one], fx.candidates() + fx.unrelated(), fx.base())
        for sets, floored in families:
            print(layout, rnd, len(sets), "sets")
            got = many.calc_prob_batch(sets)
            _compare(got, [one.calc_prob(s) for s in sets], exact)
            if rnd == "cold":  # the oracle's counts are those of a cache that holds no window of a later call (single-end sets come first in `zeros`)
                assert [int(g[1][0][0]) for g in got] == floored
            _same_read_probs(many, one, h, exact)
            assert many.bad_bases(h["single"]) == 0
    assert many.single_stats(h["single"])["multi_launches"] == 4 and one.single_stats(h["single"])["multi_launches"] == 0


def test_the_route_follows_the_switch(fx):
    """Switch on: the counters of all three read sets grow by the number of chunks. Switch off (the default),
    BatchRoute.SEQUENTIAL with the switch on, single calls: none moves. All four give the same values."""
    from gaml_amd import api
    layout = "paired+pacbio+single"
    ways = ["on", "off", "sequential", "single calls"]
    ctxs = [fx.layout(layout, onepass=w in ("on", "sequential")) for w in ways]
    ctxs[2][0].debug_set_knob(api.Knob.BATCH_ROUTE, api.BatchRoute.SEQUENTIAL)
    cands, other = fx.candidates(), fx.unrelated()
    _warm([c for c, _ in ctxs], cands + other, fx.base())
    vals = []
    for way, (c, h) in zip(ways, ctxs):
        before = _counters(c, h)
        got = [c.calc_prob(s) for s in cands + other] if way == "single calls" else c.calc_prob_batch(cands) + c.calc_prob_batch(other)
        grown = tuple(a - b for a, b in zip(_counters(c, h), before))
        print(way, "chunks on the one-pass routes (single-end, paired, PacBio):", grown)
        assert grown == ((2, 2, 2) if way == "on" else (0, 0, 0)), (way, grown)
        vals.append([(v, z.tolist(), tl) for v, z, tl in got])
    for way, v in zip(ways[1:], vals[1:]):
        assert v == vals[0], way
    for c, h in ctxs[1:]:
        assert np.array_equal(c.read_probs(h["single"]), ctxs[0][0].read_probs(ctxs[0][1]["single"]))


def test_against_the_oracle(fx):
    """The single-end set alone, on contexts whose window cache holds what the calls before registered and nothing else (the
    oracle scores every set on a fresh cache; these two families in this order give the same counts): floored counts are the
    recorded ones, values and per-read values agree with the oracle within what tests/test_gpu_other_sets.py holds single
    calls of a single-end set to."""
    c, h = fx.layout("single", onepass=True)
    o, ors = fx.oracle_single()
    for name, sets, floored in (("candidates", fx.candidates(), sc.FLOORED_CANDIDATES), ("unrelated", fx.unrelated(), sc.FLOORED_UNRELATED)):
        got = c.calc_prob_batch(sets)
        assert [int(g[1][0][0]) for g in got] == floored
        for k, (g, s) in enumerate(zip(got, sets)):
            want, wz, wtl = o.calc_prob(s, fresh=True)
            print(name, k, repr(g[0]), repr(want))
            assert g[1].tolist() == wz.tolist() and g[2] == wtl, (name, k)
            assert abs(g[0] - want) <= 1e-12 * abs(want), (name, k, g[0], want)
        if name == "candidates":  # per-read values: those of the chunk's last set
            _, wprobs, o3 = o.single_detail(ors, sets[-1])
            assert int(o3[0]) == floored[-1] and (wprobs > 0).any()
            np.testing.assert_allclose(c.read_probs(h["single"]), wprobs, rtol=4e-16, atol=0)
    assert c.single_stats(h["single"])["multi_launches"] == 2
    # a chunk that ends with [w[3:9]] * 3: every window of that path has an occurrence list
    c, h = fx.layout("single", onepass=True)
    sets = fx.unrelated()[:6]
    got = c.calc_prob_batch(sets)
    assert [int(g[1][0][0]) for g in got] == sc.FLOORED_UNRELATED[:6]
    _, wprobs, o3 = o.single_detail(ors, sets[-1])
    assert int(o3[0]) == sc.FLOORED_UNRELATED[5] and (wprobs > 0).any()
    np.testing.assert_allclose(c.read_probs(h["single"]), wprobs, rtol=4e-16, atol=0)
    assert c.single_stats(h["single"])["multi_launches"] == 1


@pytest.mark.parametrize("route", ["default", "FULL_TABLES"])
def test_a_chunk_handed_over_counts_once(fx, route):
    """A route that hands its chunk on after the single-end launch (cold, the first chunk's tables cannot be built from
    patches; a chunk with candidate 4, whose second path changes the occurrence lists; FULL_TABLES skips the patch route):
    the route that takes over scores the sets again. Values of single calls, every chunk counted once."""
    from gaml_amd import api
    (many, h), (one, _) = fx.layout("paired+single", onepass=True), fx.layout("paired+single")
    if route != "default":
        many.debug_set_knob(api.Knob.BATCH_ROUTE, api.BatchRoute[route])
    for sets in (fx.candidates(), fx.unrelated(), fx.candidates()):
        before = _counters(many, h)
        got = many.calc_prob_batch(sets)
        _compare(got, [one.calc_prob(s) for s in sets], exact=False)
        grown = tuple(a - b for a, b in zip(_counters(many, h), before))
        print(route, len(sets), "sets:", grown, many.table_stats(h["paired"]))
        assert grown == (1, 1, 0), grown
        _same_read_probs(many, one, h, exact=False)
    st = many.table_stats(h["paired"])
    assert st["batches_full"] >= 1  # (a chunk the patch route handed over, or never took)
    assert route == "default" or st["batches_patched"] == 0


@pytest.mark.parametrize("n_reads, read_len", [(1, 100), (257, 100), (4200, 50)])
def test_single_multi_kernel_shapes(n_reads, read_len):
    """Single-end-only contexts: 1 read; 257 reads (two blocks, a ragged last wave); 4,200 reads (17 blocks: more than the
    finisher's 16 ticket groups). Five small path sets, one empty, one holding a path three times. The batch equals the
    single calls bit for bit; the per-read values left behind are the last set's, after a batch of 5 and after a batch of 2."""
    from gaml_amd import api
    genome = synth.make_genome(40_000, 53)
    g = synth.make_graph(genome, synth.cut_lengths(40_000, 53, long_rng=(900, 2500)))
    walk = synth.genome_walk(g)
    reads = synth.pack_reads(synth.make_single_reads(genome, n_reads, read_len, 0.01, 57))
    ctxs = []
    for onepass in (True, False):
        c = api.Context(device=0)
        c.set_graph(*g.packed())
        rs = c.add_single(api.single_cfg(), *reads)
        c.set_single_onepass(onepass)
        ctxs.append((c, rs))
    (many, rs), (one, _) = ctxs
    sets = [[walk[:12], walk[3:7]], [walk], [walk[1:6]] * 3, [], [walk[:2]]]
    for batch in (sets, sets[:2]):
        got = many.calc_prob_batch(batch)
        want = [one.calc_prob(s) for s in batch]
        for k, (a, b) in enumerate(zip(got, want)):
            print(n_reads, k, repr(a[0]), repr(b[0]), a[1].tolist(), b[1].tolist())
            assert a[0] == b[0] and a[1].tolist() == b[1].tolist() and a[2] == b[2], (k, a, b)
            assert a[1].tolist()[0][1] == n_reads
        assert got[1][1][0][0] < n_reads or n_reads == 1  # (the whole walk: reads score)
        assert np.array_equal(many.read_probs(rs), one.read_probs(rs))
    assert many.single_stats(rs)["multi_launches"] == 2 and one.single_stats(rs)["multi_launches"] == 0


def test_gap_search_runs_on_the_one_pass_fallback(fx):
    """fix_gap_length on the paired + single layout with the switch on: the device route does not serve it (gap_stats:
    fallback lengths only), the fallback's batches take the one-pass route. Length and trace are those of the reference's
    search driven by blocking calls (tests/gap_oracle.py), cold and warm."""
    (dev, h), (twin, _) = fx.layout("paired+single", onepass=True), fx.layout("paired+single")
    paths = fx.candidates()[5]
    path_id = 1
    gap_pos = paths[path_id].index(-120)
    for rnd in ("cold", "warm"):
        before = _counters(dev, h)
        length, trace = dev.fix_gap_length(paths, path_id, gap_pos)
        want = go.Search(lambda l: twin.calc_prob(go.with_length(paths, path_id, gap_pos, l))[0], 120)
        after = _counters(dev, h)
        st = dev.gap_stats()
        print(rnd, "length", length, "evaluations", len(trace), "chunks", after, before, st)
        assert length == want.length and [l for l, _ in trace] == [l for l, _ in want.trace]
        for (l, v), (_, wv) in zip(trace, want.trace):
            print(l, repr(v), repr(wv))
        if rnd == "warm":
            assert [v for _, v in trace] == [v for _, v in want.trace]
        else:
            assert all(abs(v - wv) <= COLD_PAIRED * abs(wv) for (_, v), (_, wv) in zip(trace, want.trace))
        assert st["device_lengths"] == 0 and st["device_passes"] == 0 and st["fallback_lengths"] > 0, st
        assert after[0] > before[0] and after[1] - before[1] == after[0] - before[0], (before, after)
        for c in (dev, twin):
            c.compact_tables()
            c.calc_prob(paths)
