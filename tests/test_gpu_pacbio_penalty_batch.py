"""gaml_hip_calc_prob_batch over contexts whose PacBio set carries a coverage penalty, with the context's switch on
(gaml_hip_set_pacbio_penalty_onepass): the chunk takes the one-pass routes, sweeps every distinct path it has no bad_bases for
once -- one contig per block (pacbio_path_sweep_kernel), contigs above the block's capacity through the general chain -- and
a set's bad_bases is the sum over its paths. Values, floored counts, per-read values, bad_bases and the bookkeeping are those
of as many single calls, bit for bit. Inputs: tests/pacbio_penalty_batch_cases.py (checked on the oracle by
tests/test_pacbio_penalty_cases_host.py)."""
import numpy as np
import pytest

import gap_oracle as go
import pacbio_penalty_batch_cases as pp

pytestmark = pytest.mark.gpu

ZERO = {"chunks": 0, "block_contigs": 0, "chain_contigs": 0, "memo_paths": 0}


@pytest.fixture(scope="module")
def fp():
    return pp.FixtureP()


@pytest.fixture(scope="module")
def fc():
    return pp.FixtureC()


@pytest.fixture(scope="module")
def crafted(fc):
    """per step of fixture C, computed once: the oracle's (value, bad_bases) per set and a twin context's single calls"""
    out = {}
    for step in pp.STEPS_C:
        o, ors = fc.oracle(step)
        want = []
        for s in fc.sets():
            v, _, o3 = o.pacbio_detail(ors, s)
            want.append((v, int(o3[2])))
        one, rs = fc.context(step)
        single = []
        for s in fc.sets():
            single.append(one.calc_prob(s) + (one.bad_bases(rs),))
        one.close()
        out[step] = (want, single)
    return out


def _equal(got, want):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        print(f"set {k}: {a[0]!r} / {b[0]!r}, zeros {a[1].tolist()} / {b[1].tolist()}, total length {a[2]} / {b[2]}")
    for k, (a, b) in enumerate(zip(got, want)):
        assert a[0] == b[0], (k, a[0], b[0])
        assert a[1].tolist() == b[1].tolist() and a[2] == b[2], (k, a[1].tolist(), b[1].tolist(), a[2], b[2])


def _singles(c, pacbio, sets, paired=None):
    """single calls of `sets`: their results, the PacBio set's bad_bases after each (and the paired set's)"""
    res, bad, pbad = [], [], []
    for s in sets:
        res.append(c.calc_prob(s))
        bad.append(c.bad_bases(pacbio))
        if paired is not None:
            pbad.append(c.bad_bases(paired))
    return res, bad, pbad


def _paired_chunks(c, paired):
    st = c.table_stats(paired)
    return st["batches_patched"] + st["batches_full"]


def _delta(after, before):
    return {k: after[k] - before[k] for k in after}


def test_switch_on_equals_single_calls_bit_for_bit(fp):
    from gaml_amd import api
    many, paired, pacbio = fp.context(onepass=True)
    one = fp.context()[0]
    seq = fp.context(onepass=True)[0]
    seq.debug_set_knob(api.Knob.BATCH_ROUTE, api.BatchRoute.SEQUENTIAL)
    off = fp.context(onepass=False)[0]
    assert many.get_pacbio_penalty_onepass() and not one.get_pacbio_penalty_onepass() and not off.get_pacbio_penalty_onepass()
    chunks = 0
    for sets, table in ((fp.candidates(), pp.BAD_CANDIDATES), (fp.unrelated(), pp.BAD_UNRELATED)):  # one chunk of 8; a chunk of 8 and a leftover set
        for rnd in ("cold", "warm"):
            print(rnd, len(sets), "sets")
            want, wbad, _ = _singles(one, pacbio, sets)
            got = many.calc_prob_batch(sets)
            chunks += 1
            _equal(got, want)
            assert wbad == table
            assert many.debug_pacbio_batch_bad_bases(pacbio) == wbad and many.bad_bases(pacbio) == wbad[-1] == one.bad_bases(pacbio)
            assert many.bad_bases(paired) == one.bad_bases(paired) == 0
            assert np.array_equal(many.read_probs(pacbio), one.read_probs(pacbio))  # the last set's
            assert np.array_equal(many.read_probs(paired), one.read_probs(paired))
            assert many.pacbio_stats(pacbio)["multi_launches"] == chunks == many.pacbio_penalty_stats(pacbio)["chunks"] == _paired_chunks(many, paired)
            assert many.pacbio_stats(pacbio)["misses"] == one.pacbio_stats(pacbio)["misses"]
            for c in (seq, off):  # one launch per set, and the switch off: nothing is counted, the same bits
                _equal(c.calc_prob_batch(sets), want)
                assert c.debug_pacbio_batch_bad_bases(pacbio) == wbad and c.bad_bases(pacbio) == wbad[-1]
                assert np.array_equal(c.read_probs(pacbio), one.read_probs(pacbio))
                assert c.pacbio_stats(pacbio)["multi_launches"] == 0 and c.pacbio_penalty_stats(pacbio) == ZERO and _paired_chunks(c, paired) == 0
    st = many.pacbio_penalty_stats(pacbio)
    print(st)
    assert st["chunks"] == 4 and st["chain_contigs"] == 0 and st["block_contigs"] > 0 and st["memo_paths"] > 0


def test_against_the_oracle(fp):
    for with_paired in (True, False):
        c, paired, pacbio = fp.context(paired=with_paired, onepass=True)
        o, ors = fp.oracle(paired=with_paired)
        for name, sets, bad, floored in (("candidates", fp.candidates(), pp.BAD_CANDIDATES, pp.FLOORED_CANDIDATES),
                                         ("unrelated", fp.unrelated(), pp.BAD_UNRELATED, pp.FLOORED_UNRELATED)):
            got = c.calc_prob_batch(sets)
            assert [int(g[1][-1][0]) for g in got] == floored
            assert c.debug_pacbio_batch_bad_bases(pacbio) == bad
            for k, (g, s) in enumerate(zip(got, sets)):
                w = o.calc_prob(s, fresh=True)
                rel = abs(g[0] - w[0]) / abs(w[0])
                print("paired + PacBio" if with_paired else "PacBio only", name, k, repr(g[0]), repr(w[0]), rel)
                assert g[1].tolist() == w[1].tolist() and g[2] == w[2], (name, k)
                assert rel <= 1e-12, (name, k, g[0], w[0])
        assert c.pacbio_penalty_stats(pacbio)["chunks"] == 2


def test_the_memo_serves_a_repeated_batch_and_follows_the_record_cache(fp):
    many, paired, pacbio = fp.context(onepass=True)
    one = fp.context()[0]
    sets = fp.candidates()
    n_distinct = len(pp.distinct_paths(sets))
    first = many.calc_prob_batch(sets)
    st1 = many.pacbio_penalty_stats(pacbio)
    assert st1 == {"chunks": 1, "block_contigs": n_distinct, "chain_contigs": 0, "memo_paths": 0}
    again = many.calc_prob_batch(sets)
    st2 = many.pacbio_penalty_stats(pacbio)
    assert st2 == {"chunks": 2, "block_contigs": n_distinct, "chain_contigs": 0, "memo_paths": n_distinct}  # nothing swept
    assert [a[0] for a in again] == [a[0] for a in first] and many.debug_pacbio_batch_bad_bases(pacbio) == pp.BAD_CANDIDATES
    # a record under a cached sub-walk: the record cache has changed, every value is swept again
    wk = list(fp.pb.walks[0])
    rec = np.array([[3000, 4800, 7]], np.int32)
    lp = np.array([-2100.0])
    for c in (many, one):
        c.put_pacbio_records(pacbio, wk, rec, lp)
    got = many.calc_prob_batch(sets)
    want, wbad, _ = _singles(one, pacbio, sets)
    _equal(got, want)
    assert many.debug_pacbio_batch_bad_bases(pacbio) == wbad
    print(wbad)
    st3 = many.pacbio_penalty_stats(pacbio)
    assert st3 == {"chunks": 3, "block_contigs": 2 * n_distinct, "chain_contigs": 0, "memo_paths": n_distinct}


def test_each_distinct_path_is_swept_once(fp):
    many, paired, pacbio = fp.context(onepass=True)
    sets = fp.candidates()
    listed, distinct = sum(len(s) for s in sets), len(pp.distinct_paths(sets))
    assert distinct < listed
    many.calc_prob_batch(sets)
    st = many.pacbio_penalty_stats(pacbio)
    print(listed, "paths listed,", distinct, "distinct:", st)
    assert st["block_contigs"] + st["chain_contigs"] == distinct and st["memo_paths"] == 0
    assert many.debug_pacbio_batch_bad_bases(pacbio) == pp.BAD_CANDIDATES


@pytest.mark.parametrize("route", ["default", "FULL_TABLES", "SEQUENTIAL"])
def test_hand_overs_count_every_set_once(fp, route):
    """A route that hands its chunk on after the PacBio launch (cold, the first chunk's tables cannot be built from patches:
    the full-tables route takes it; FULL_TABLES and SEQUENTIAL force the other hand-overs) has launched the sweeps twice:
    misses, bad_bases and the counters are those of one pass."""
    from gaml_amd import api
    many, paired, pacbio = fp.context(onepass=True)
    one = fp.context()[0]
    if route != "default":
        many.debug_set_knob(api.Knob.BATCH_ROUTE, api.BatchRoute[route])
    known = set()
    for sets in (fp.candidates(), fp.unrelated(), fp.candidates()):
        m0, s0, p0 = many.pacbio_stats(pacbio)["misses"], one.pacbio_stats(pacbio)["misses"], many.pacbio_penalty_stats(pacbio)
        got = many.calc_prob_batch(sets)
        want, wbad, _ = _singles(one, pacbio, sets)
        m1, s1, p1 = many.pacbio_stats(pacbio)["misses"], one.pacbio_stats(pacbio)["misses"], many.pacbio_penalty_stats(pacbio)
        print(route, len(sets), "sets: misses", m1 - m0, "/", s1 - s0, _delta(p1, p0), many.table_stats(paired))
        assert s1 - s0 > 0 and m1 - m0 == s1 - s0
        assert [g[1].tolist() for g in got] == [w[1].tolist() for w in want]
        assert many.debug_pacbio_batch_bad_bases(pacbio) == wbad
        if route == "SEQUENTIAL":
            assert _delta(p1, p0) == ZERO
        else:
            chunk = set(pp.distinct_paths(sets[:8]))  # (a ninth set is a single call)
            assert _delta(p1, p0) == {"chunks": 1, "block_contigs": len(chunk - known), "chain_contigs": 0, "memo_paths": len(chunk & known)}
            known |= chunk
    if route == "default":
        assert many.table_stats(paired)["batches_full"] >= 1  # (a chunk the patch route handed over)


@pytest.mark.parametrize("kind", ["pacbio only", "both penalised"])
def test_other_contexts(fp, kind):
    from gaml_amd import api
    kw = dict(paired=False) if kind == "pacbio only" else dict(paired_penalty=True)
    many, paired, pacbio = fp.context(onepass=True, **kw)
    one = fp.context(**kw)[0]
    seq = fp.context(onepass=True, **kw)[0]
    seq.debug_set_knob(api.Knob.BATCH_ROUTE, api.BatchRoute.SEQUENTIAL)
    for sets, table in ((fp.candidates(), pp.BAD_CANDIDATES), (fp.unrelated(), pp.BAD_UNRELATED)):
        want, wbad, wpbad = _singles(one, pacbio, sets, paired)
        _equal(many.calc_prob_batch(sets), want)
        _equal(seq.calc_prob_batch(sets), want)
        assert wbad == table
        assert many.debug_pacbio_batch_bad_bases(pacbio) == seq.debug_pacbio_batch_bad_bases(pacbio) == wbad
        assert np.array_equal(many.read_probs(pacbio), one.read_probs(pacbio))
        if paired is not None:
            print(kind, "paired bad_bases", wpbad)
            assert many.debug_batch_bad_bases(paired) == seq.debug_batch_bad_bases(paired) == wpbad
            assert np.array_equal(many.read_probs(paired), one.read_probs(paired))
    assert many.pacbio_penalty_stats(pacbio)["chunks"] == 2 and seq.pacbio_penalty_stats(pacbio) == ZERO
    if paired is not None:
        assert _paired_chunks(many, paired) == 2 and _paired_chunks(seq, paired) == 0


CAPS_C = {"above": pp.LARGEST_C + 1, "exact": pp.LARGEST_C, "one below": pp.LARGEST_C - 1, "one": 1}


@pytest.mark.parametrize("cap", list(CAPS_C))
@pytest.mark.parametrize("step", pp.STEPS_C)
def test_crafted_intervals_on_both_sweep_routes(fc, crafted, step, cap):
    """Nested, identical and touching intervals, records below GetMinReadProb, a gap, a path listed three times, the empty
    set: the capacity knob sends the contigs to the block-per-contig kernel, to the general chain, or the largest one alone
    to the chain."""
    want, single = crafted[step]
    sets = fc.sets()
    many, rs = fc.context(step, onepass=True, cap=CAPS_C[cap])
    got = many.calc_prob_batch(sets)
    bad = many.debug_pacbio_batch_bad_bases(rs)
    st = many.pacbio_penalty_stats(rs)
    print(step, cap, bad, st)
    assert bad == [w[1] for w in want] == pp.BAD_C[step]       # the oracle's
    assert bad == [s[3] for s in single]                        # a single call's
    _equal(got, [s[:3] for s in single])
    for k, (g, w) in enumerate(zip(got, want)):
        assert abs(g[0] - w[0]) <= 1e-12 * abs(w[0]), (k, g[0], w[0])
    counts = {tuple(p): n for s, ns in zip(sets, pp.COUNTS_C) for p, n in zip(s, ns)}
    block = sum(1 for n in counts.values() if n <= CAPS_C[cap])
    assert len(counts) == 24
    assert st == {"chunks": 1, "block_contigs": block, "chain_contigs": len(counts) - block, "memo_paths": 0}
    assert block == {"above": 24, "exact": 24, "one below": 23, "one": 0}[cap]
    many.close()


def test_gap_search_runs_on_the_one_pass_fallback(fp):
    """fix_gap_length on candidate 5's 120-base gap with the switch on: the fallback's batches take the one-pass route on
    both read sets (a new gap length is a new path: one contig swept per length)."""
    dev, paired, pacbio = fp.context(onepass=True)
    twin = fp.context()[0]
    paths = fp.candidates()[5]
    path_id = 1
    gap_pos = paths[path_id].index(-120)
    cur = 120
    for rnd in ("cold", "warm"):
        before = (_paired_chunks(dev, paired), dev.pacbio_stats(pacbio)["multi_launches"], dev.pacbio_penalty_stats(pacbio))
        length, trace = dev.fix_gap_length(paths, path_id, gap_pos)
        want = go.Search(lambda l: twin.calc_prob(go.with_length(paths, path_id, gap_pos, l))[0], cur)
        after = (_paired_chunks(dev, paired), dev.pacbio_stats(pacbio)["multi_launches"], dev.pacbio_penalty_stats(pacbio))
        st = dev.gap_stats()
        print(rnd, "length", length, "evaluations", len(trace), "chunks", after[0] - before[0], st, _delta(after[2], before[2]))
        assert length == want.length and [l for l, _ in trace] == [l for l, _ in want.trace]
        for (l, v), (_, wv) in zip(trace, want.trace):
            print(l, repr(v), repr(wv))
        if rnd == "warm":
            assert [v for _, v in trace] == [v for _, v in want.trace]
        else:
            assert all(abs(v - wv) <= 1e-13 * abs(wv) for (_, v), (_, wv) in zip(trace, want.trace))
        assert st["device_lengths"] == 0 and st["device_passes"] == 0 and st["fallback_lengths"] > 0, st
        assert after[0] > before[0] and after[1] - before[1] == after[0] - before[0] == after[2]["chunks"] - before[2]["chunks"], (before, after)
        for c in (dev, twin):
            c.compact_tables()
            c.calc_prob(paths)


def test_a_multi_device_context_keeps_the_flag(fp):
    """Its batches go other ways (the shards' sweeps wait for each other's intervals): the flag is kept, the values are the
    twin's -- sums over shards, so to 1e-12 -- with its zeros, lengths and bad_bases."""
    from gaml_amd import api
    one, paired, pacbio = fp.context()
    multi = api.Context(devices=[0, 0])
    multi.set_graph(*fp.g.packed())
    multi.add_paired(api.paired_cfg(300.0, 30.0, weight=1.0), *fp.paired_args)
    mpb = multi.add_pacbio(api.single_cfg(mismatch_prob=0.15, penalty_step=pp.STEP_P, **pp.PACBIO_KW_P), fp.pb.lens)
    for wk, rec, lp in zip(fp.pb.walks, fp.pb.recs, fp.pb.logps):
        multi.put_pacbio_records(mpb, wk, rec, lp)
    assert not multi.get_pacbio_penalty_onepass()
    multi.set_pacbio_penalty_onepass(True)
    assert multi.get_pacbio_penalty_onepass()
    sets = fp.candidates()
    got = multi.calc_prob_batch(sets)
    want, wbad, _ = _singles(one, pacbio, sets)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g[1].tolist() == w[1].tolist() and g[2] == w[2], k
        assert abs(g[0] - w[0]) <= 1e-12 * abs(w[0]), (k, g[0], w[0])
    assert multi.bad_bases(mpb) == wbad[-1]
    assert multi.pacbio_penalty_stats(mpb) == ZERO
    multi.close()
