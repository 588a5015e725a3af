"""gaml_hip_calc_prob_batch over contexts with PacBio sets (BASELINE config 4: paired + PacBio): a chunk of up to 8 path
sets is scored in one pass per read set -- pacbio_score_multi_kernel beside paired_score_multi_kernel -- and gives the bits,
the floored counts, the per-read values and the bookkeeping of as many single calls; the gap-length search's fallback runs
on top of it. Inputs: tests/pacbio_batch_cases.py (checked on the oracle by tests/test_pacbio_batch_cases_host.py)."""
import numpy as np
import pytest

import gap_oracle as go
import pacbio_batch_cases as pc
from gaml_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fa():
    return pc.FixtureA()


@pytest.fixture(scope="module")
def oracle_values(fa):
    """the oracle's (value, zeros, total length) of every set of both families, computed once"""
    o = fa.oracle()
    return {name: [o.calc_prob(s, fresh=True) for s in sets] for name, sets in (("candidates", fa.candidates()), ("unrelated", fa.unrelated()))}


def _equal(got, want):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        print(f"set {k}: {a[0]!r} / {b[0]!r}, zeros {a[1].tolist()} / {b[1].tolist()}, total length {a[2]} / {b[2]}")
    for k, (a, b) in enumerate(zip(got, want)):
        assert a[0] == b[0], (k, a[0], b[0])
        assert a[1].tolist() == b[1].tolist() and a[2] == b[2], (k, a[1].tolist(), b[1].tolist(), a[2], b[2])


def _chunks(c, paired, pacbio):
    st = c.table_stats(paired)
    return st["batches_patched"] + st["batches_full"], c.pacbio_stats(pacbio)["multi_launches"]


def _warm(ctxs, sets, base):
    """every window of `sets` aligned and folded into the record tables: the same device state on every context"""
    for c in ctxs:
        for s in sets:
            c.calc_prob(s)
        c.compact_tables()
        c.calc_prob(base)


def test_batch_equals_single_calls_bit_for_bit(fa):
    (many, paired, pacbio), (one, _, _) = fa.context(), fa.context()
    for sets in (fa.candidates(), fa.unrelated()):  # 8 sets: one chunk; 9 sets: a chunk of 8 and a leftover set
        for rnd in ("cold", "warm"):
            print(rnd, len(sets), "sets")
            _equal(many.calc_prob_batch(sets), [one.calc_prob(s) for s in sets])
            assert np.array_equal(many.read_probs(pacbio), one.read_probs(pacbio))  # the last set's
            assert np.array_equal(many.read_probs(paired), one.read_probs(paired))
            assert many.bad_bases(pacbio) == 0 and one.bad_bases(pacbio) == 0
    assert many.pacbio_stats(pacbio)["multi_launches"] == 4


def test_the_one_pass_route_was_taken(fa):
    """The route counters of both read sets grow by the number of chunks; with BatchRoute.SEQUENTIAL neither moves. Every
    route gives the same bits: device-built tables, whole tables per set, no capture, one launch per set, single calls."""
    from gaml_amd import api
    cands, other = fa.candidates(), fa.unrelated()
    R = api.BatchRoute
    routes = [0, R.FULL_TABLES, R.NO_CAPTURE, R.SEQUENTIAL, None]  # None: single calls
    assert sorted(int(r) for r in routes[1:4]) == sorted(int(r) for r in R)
    ctxs = [fa.context() for _ in routes]
    for route, (c, _, _) in zip(routes, ctxs):
        if route:
            c.debug_set_knob(api.Knob.BATCH_ROUTE, route)
    # a chunk the patch route can follow to its end: every set one cut, one dropped path or one shortened path away from the
    # assembly (a path that occurs twice -- candidate 4 -- changes the occurrence lists: that chunk is handed over)
    base = fa.base()
    plain = [base[:i] + [base[i][:3], base[i][3:]] + base[i + 1:] for i in range(6)] + [cands[6], cands[7]]
    _warm([c for c, _, _ in ctxs], cands + other + plain, base)
    vals = []
    for route, (c, paired, pacbio) in zip(routes, ctxs):
        before = _chunks(c, paired, pacbio)
        if route is None:
            got = [c.calc_prob(s) for s in cands + other + [base] + plain]
        else:
            got = c.calc_prob_batch(cands) + c.calc_prob_batch(other) + [c.calc_prob(base)] + c.calc_prob_batch(plain)
        after = _chunks(c, paired, pacbio)
        grown = (after[0] - before[0], after[1] - before[1])
        print(route, "chunks on the one-pass route (paired, PacBio):", grown)
        assert grown == ((0, 0) if route in (R.SEQUENTIAL, None) else (3, 3)), (route, before, after)
        vals.append([(v, z.tolist(), tl) for v, z, tl in got])
    for route, v in zip(routes[1:], vals[1:]):
        assert v == vals[0], route
    st = ctxs[0][0].table_stats(ctxs[0][1])
    print(st)
    assert st["batches_patched"] >= 1 and st["batches_full"] >= 1, st
    assert ctxs[1][0].table_stats(ctxs[1][1])["batches_patched"] == 0


@pytest.mark.parametrize("route", ["default", "FULL_TABLES", "SEQUENTIAL"])
def test_misses_count_every_set_once(fa, route):
    """Sub-walk lookups that find nothing: a batch adds what single calls of its sets add -- also when a route hands its
    chunk over after the PacBio launch (cold, the first chunk's tables cannot be built from patches: the full-tables route
    takes it; FULL_TABLES and SEQUENTIAL force the other hand-overs)."""
    from gaml_amd import api
    (many, paired, pacbio), (one, _, opb) = fa.context(), fa.context()
    if route != "default":
        many.debug_set_knob(api.Knob.BATCH_ROUTE, api.BatchRoute[route])
    assert many.pacbio_stats(pacbio)["misses"] == 0
    for sets in (fa.candidates(), fa.unrelated(), fa.candidates()):
        b0, s0 = many.pacbio_stats(pacbio)["misses"], one.pacbio_stats(opb)["misses"]
        got = many.calc_prob_batch(sets)
        want = [one.calc_prob(s) for s in sets]
        b1, s1 = many.pacbio_stats(pacbio)["misses"], one.pacbio_stats(opb)["misses"]
        print(route, len(sets), "sets: misses", b1 - b0, "/", s1 - s0, many.table_stats(paired))
        assert s1 - s0 > 0 and b1 - b0 == s1 - s0
        assert [g[1].tolist() for g in got] == [w[1].tolist() for w in want]
    if route == "default":
        assert many.table_stats(paired)["batches_full"] >= 1  # (a chunk the patch route handed over)


def test_against_the_oracle(fa, oracle_values):
    c, paired, pacbio = fa.context()
    for name, sets, floored in (("candidates", fa.candidates(), pc.FLOORED_CANDIDATES), ("unrelated", fa.unrelated(), pc.FLOORED_UNRELATED)):
        got = c.calc_prob_batch(sets)
        assert [int(g[1][-1][0]) for g in got] == floored
        for k, (g, w) in enumerate(zip(got, oracle_values[name])):
            print(name, k, repr(g[0]), repr(w[0]), abs(g[0] - w[0]) / abs(w[0]))
            assert g[1].tolist() == w[1].tolist() and g[2] == w[2], (name, k)
            assert abs(g[0] - w[0]) <= 1e-9 * abs(w[0]), (name, k, g[0], w[0])
    assert c.pacbio_stats(pacbio)["multi_launches"] == 2


def test_pacbio_only_context_with_many_records_per_read():
    """Three reads, up to 200 records per sub-walk: the lanes of a wave stride over a read's records, every set folds its
    own counts (0, 1, 2, 3 occurrences). No paired set: the PacBio launch is all a chunk does."""
    from gaml_amd import api
    import oracle_py as op
    genome = synth.make_genome(40_000, 53)
    g = synth.make_graph(genome, synth.cut_lengths(40_000, 53, long_rng=(900, 2500)))
    gb, gofs = g.packed()
    walk = synth.genome_walk(g)[:6]
    rng = np.random.default_rng(5)
    lens = np.array([1500, 1500, 1800], np.int32)
    ctxs = []
    for _ in range(2):
        c = api.Context(device=0)
        c.set_graph(gb, gofs)
        ctxs.append((c, c.add_pacbio(api.single_cfg(mismatch_prob=0.15, min_prob_per_base=-2.0), lens)))
    orc = op.Oracle()
    orc.set_graph(gb, gofs)
    ors = orc.add_pacbio(lens, 0.15, op.single_cfg(min_prob_per_base=-2.0))
    for sub in synth.all_subwalks_for_pacbio(g, walk, int(lens.max())):
        k = int(rng.integers(0, 200))
        rec = np.stack([rng.integers(0, 500, k), rng.integers(1500, 2000, k), rng.integers(0, 2, k)], axis=1).astype(np.int32)
        lp = rng.uniform(-2400, -1700, k)
        for c, rs in ctxs:
            c.put_pacbio_records(rs, sub, rec, lp)
        orc.pacbio_put(ors, sub, rec, lp)
    (many, rs), (one, _) = ctxs
    sets = [[walk, walk[1:4]], [walk], [walk[1:4]] * 3, [], [walk[:2]]]
    for batch in (sets, sets[:2]):  # the per-read values left behind: those of [walk[:2]], then those of [walk]
        got = many.calc_prob_batch(batch)
        _equal(got, [one.calc_prob(s) for s in batch])
        for s, b in zip(batch, got):
            want, wlp, o3 = orc.pacbio_detail(ors, s)
            assert b[1].tolist() == [[int(o3[0]), 3]] and b[2] == int(o3[1])
            assert abs(b[0] - want) <= 1e-12 * abs(want), (s, b[0], want)
        lp = many.read_probs(rs)
        fin = np.isfinite(wlp)  # (of the batch's last set)
        assert (np.isfinite(lp) == fin).all() and not fin[2]
        np.testing.assert_allclose(lp[fin], wlp[fin], rtol=1e-12)
        assert np.array_equal(lp, one.read_probs(rs))
    assert many.pacbio_stats(rs)["multi_launches"] == 2 and one.pacbio_stats(rs)["multi_launches"] == 0


def test_the_cache_grows_between_batches(fa):
    """More records under a cached sub-walk and a sub-walk nobody had filed yet: the next batch's count table has a row
    more and the record arrays are uploaded again."""
    (many, paired, pacbio), (one, _, _) = fa.context(), fa.context()
    sets = fa.unrelated()
    _equal(many.calc_prob_batch(sets), [one.calc_prob(s) for s in sets])
    new = [fa.walk[4] ^ 1]  # a node of the twin walk: every PacBio read of that set was floored so far
    assert not any(list(w) == new for w in fa.pb.walks)
    rec_new = np.array([[0, 1500, r] for r in range(12)], np.int32)
    lp_new = np.linspace(-1400.0, -2100.0, 12)
    rec_old = np.array([[10, 1900, r] for r in (3, 3, 77, 149)], np.int32)
    lp_old = np.array([-1500.0, -1650.0, -1300.0, -2500.0])
    before = many.pacbio_stats(pacbio)
    for c in (many, one):
        c.put_pacbio_records(pacbio, new, rec_new, lp_new)
        c.put_pacbio_records(pacbio, list(fa.pb.walks[0]), rec_old, lp_old)
    after = many.pacbio_stats(pacbio)
    assert after["subwalks"] == before["subwalks"] + 1 and after["records"] == before["records"] + 16
    got = many.calc_prob_batch(sets)
    _equal(got, [one.calc_prob(s) for s in sets])
    assert int(got[3][1][-1][0]) == pc.FLOORED_UNRELATED[3] - 12  # the twin walk: twelve reads have an alignment now
    assert np.array_equal(many.read_probs(pacbio), one.read_probs(pacbio))
    assert many.pacbio_stats(pacbio)["multi_launches"] == 2


@pytest.mark.parametrize("kind", ["pacbio penalty", "single-end set"])
def test_contexts_that_stay_sequential(fa, kind):
    kw = dict(pacbio_penalty=0.0001) if kind == "pacbio penalty" else dict(single=True)
    (many, paired, pacbio), (one, _, _) = fa.context(**kw), fa.context(**kw)
    for sets in (fa.candidates(), fa.unrelated()):
        _equal(many.calc_prob_batch(sets), [one.calc_prob(s) for s in sets])
        assert many.bad_bases(pacbio) == one.bad_bases(pacbio)
    assert _chunks(many, paired, pacbio) == (0, 0)


def test_gap_search_runs_on_the_one_pass_fallback(fa):
    """fix_gap_length on a mixed context: the device route does not serve it (gap_stats: fallback lengths only), the
    fallback's batches take the one-pass route. Length and trace are those of the reference's search driven by blocking
    calls (tests/gap_oracle.py) -- once cold, then with every window folded into the record tables: bit for bit."""
    (dev, paired, pacbio), (twin, _, _) = fa.context(), fa.context()
    paths = fa.candidates()[5]
    path_id = 1
    gap_pos = paths[path_id].index(-120)
    cur = 120
    for rnd in ("cold", "warm"):
        before = _chunks(dev, paired, pacbio)
        length, trace = dev.fix_gap_length(paths, path_id, gap_pos)
        want = go.Search(lambda l: twin.calc_prob(go.with_length(paths, path_id, gap_pos, l))[0], cur)
        after = _chunks(dev, paired, pacbio)
        st = dev.gap_stats()
        print(rnd, "length", length, "evaluations", len(trace), "chunks", after[0] - before[0], st)
        assert length == want.length and [l for l, _ in trace] == [l for l, _ in want.trace]
        for (l, v), (_, wv) in zip(trace, want.trace):
            print(l, repr(v), repr(wv))
        if rnd == "warm":
            assert [v for _, v in trace] == [v for _, v in want.trace]
        else:
            assert all(abs(v - wv) <= 1e-13 * abs(wv) for (_, v), (_, wv) in zip(trace, want.trace))
        assert st["device_lengths"] == 0 and st["device_passes"] == 0 and st["fallback_lengths"] > 0, st
        assert after[0] > before[0] and after[1] - before[1] == after[0] - before[0], (before, after)
        for c in (dev, twin):
            c.compact_tables()
            c.calc_prob(paths)
