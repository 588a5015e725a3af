"""gaml_hip_calc_prob_batch over read sets with a coverage penalty: one pass over the records per chunk of up to 8 path sets.

Every path set of a launch marks coverage into a bitmap of its own (paired_score_multi_kernel's COV instantiation), one
dispatch sweeps them all (coverage_sweep_multi_kernel) and one hands the per-set bad_bases to the host. Checked here: the
batch takes the one-pass routes (tables from patches / whole tables), and on both, cold and warm, for pairs of one length
combination, of three (thresholds in LDS) and of 198 (more than the kernel keeps there), it returns the values, floored
counts, total lengths and bad_bases of single calls and of the oracle -- for candidates of one assembly, for unrelated
sets, and for a batch with an empty assembly, repeated windows (GEN instantiation) and a gap. The sets of a batch differ
in their coverage marks (test_inputs_exercise_the_penalty): a kernel that mixed the sets' bitmaps up would not pass."""
import functools

import numpy as np
import pytest

from gaml_amd import synth

G, SEED, N_PAIRS, PENALTY = 150_000, 17, 2_500, 0.0002
VARIANTS = ("one", "few", "many")
# the oracle's bad_bases (variant `one`; second library: 1,500 pairs, insert 400 +- 40, penalty 0.0005)
WANT_ONE = {"cands": [6405, 6267, 6722, 6073, 5467, 5804, 6073, 6073], "unrel": [5723, 5956, 6073, 7233, 5723, 6569, 6073, 5723],
            "mixed": [0, 9983, 0, 5723, 5723]}
WANT_LIB2 = {"cands": [3098, 2941, 2579, 2579, 2579, 2102, 2579, 2579], "unrel": [1905, 2579, 3107, 4634, 1905, 3851, 2579, 2534],
             "mixed": [0, 5384, 0, 1905, 1905]}


def _pack(reads):
    offs = np.zeros(len(reads) + 1, np.int64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    return np.concatenate([np.asarray(r, np.uint8) for r in reads]), offs


@functools.lru_cache(maxsize=None)
def _graph():
    genome = synth.plant_repeats(synth.make_genome(G, SEED), 3, 800, SEED)
    g = synth.make_graph(genome, synth.cut_lengths(G, SEED, long_rng=(600, 4000), short_rng=(25, 330)))
    start, seq = synth.sa_sequence(g, 120, seed=5, threshold=400)
    base = seq[59]
    assert len(base) == 48

    def A(k):
        return [p for i, p in enumerate(base) if i not in (3 * k, 3 * k + 5)] + [base[3 * k] + base[3 * k + 5]]

    def B(k):
        return [p for i, p in enumerate(base) if i != 5 * k]

    walk = synth.genome_walk(g)
    cut = len(walk) // 2
    gap = None
    for ps in ([start] + seq)[40:]:  # the first set with a gap inside a path
        for i, p in enumerate(ps):
            for q, x in enumerate(p):
                if gap is None and x < 0 and 0 < q < len(p) - 1:
                    gap = (ps, i, q)
    assert gap is not None
    fam = {"cands": [A(2), A(4), A(7), A(3), B(2), B(3), B(0), base],
           "unrel": [seq[k] for k in (3, 40, 77, 119, 10, 99, 58, 31)],
           "mixed": [[], [walk[:cut] + walk[cut - 3:cut] + walk[cut:]], [walk[:3]], gap[0], seq[3]]}
    return genome, g, base, fam, gap


@functools.lru_cache(maxsize=None)
def _reads(variant):
    genome = _graph()[0]
    pr = synth.make_paired_reads(genome, N_PAIRS, 100, 240.0, 24.0, 0.01, SEED)
    m1, m2 = list(pr.mate1), list(pr.mate2)
    if variant == "few":
        for i in range(0, N_PAIRS, 4):
            m1[i] = m1[i][:90]
        for i in range(1, N_PAIRS, 6):
            m2[i] = m2[i][:95]
    elif variant == "many":  # the trimming of test_gpu_penalty_route._case(True)
        rng = np.random.default_rng(3)
        for i in range(0, N_PAIRS, 3):
            m1[i] = m1[i][: int(rng.integers(70, 100))]
        for i in range(1, N_PAIRS, 5):
            m2[i] = m2[i][: int(rng.integers(80, 100))]
    else:
        assert variant == "one"
    return (*_pack(m1), *_pack(m2))


@functools.lru_cache(maxsize=None)
def _reads2():
    pr = synth.make_paired_reads(_graph()[0], 1_500, 100, 400.0, 40.0, 0.01, SEED + 1)
    return (*_pack(list(pr.mate1)), *_pack(list(pr.mate2)))


@functools.lru_cache(maxsize=None)
def _oracle(variant, two=False):
    """family -> per path set (value, floored counts, total_len, [bad_bases per read set], [per-read probabilities per read
    set]); computed once, never changed"""
    import oracle_py as op
    g, fam = _graph()[1], _graph()[3]
    orc = op.Oracle()
    orc.set_graph(*g.packed())
    rs = [orc.add_paired(*_reads(variant), 0.01, op.paired_cfg(240.0, 24.0, penalty_constant=PENALTY))]
    if two:
        rs.append(orc.add_paired(*_reads2(), 0.01, op.paired_cfg(400.0, 40.0, penalty_constant=0.0005, weight=0.5)))
    out = {}
    for name, sets in fam.items():
        rows = []
        for ps in sets:
            v, z, tl = orc.calc_prob(ps, fresh=True)
            pb = [orc.paired_probs(r) for r in rs]
            rows.append((v, z.tolist(), tl, [int(b) for _, b in pb], [p.copy() for p, _ in pb]))
        out[name] = rows
    return out


def _ctx(variant, two=None, batch_route=None):
    """two: None one library; True a second, penalised one beside it; False a second one without penalty; batch_route: the
    name of an api.BatchRoute"""
    from gaml_amd import api
    c = api.Context(device=0)
    if batch_route:
        c.debug_set_knob(api.Knob.BATCH_ROUTE, api.BatchRoute[batch_route])
    c.set_graph(*_graph()[1].packed())
    c.add_paired(api.paired_cfg(240.0, 24.0, penalty_constant=PENALTY), *_reads(variant))
    if two is not None:
        c.add_paired(api.paired_cfg(400.0, 40.0, penalty_constant=0.0005 if two else 0.0, weight=0.5), *_reads2())
    return c


def _call(c, ps):
    v, z, tl = c.calc_prob(ps)
    return v, z.tolist(), tl, [c.bad_bases(r) for r in range(c.num_readsets())]


def _batch(c, sets):
    got = c.calc_prob_batch(sets)
    bads = [c.debug_batch_bad_bases(r) for r in range(c.num_readsets())]
    assert all(len(b) == len(sets) for b in bads)
    return [(b[0], b[1].tolist(), b[2], [bads[r][k] for r in range(len(bads))]) for k, b in enumerate(got)]


def test_inputs_exercise_the_penalty():
    """what the batches are chosen for: the sets of a batch differ in their uncovered bases"""
    for variant in VARIANTS:
        o = _oracle(variant)
        for name in ("cands", "unrel"):
            bads = [r[3][0] for r in o[name]]
            print(variant, name, bads)
            assert len(bads) == 8 and all(b > 0 for b in bads) and len(set(bads)) >= 4, (variant, name, bads)
        print(variant, "mixed", [r[3][0] for r in o["mixed"]])
    for name, want in WANT_ONE.items():
        assert [r[3][0] for r in _oracle("one")[name]] == want, name
    o2 = _oracle("one", True)
    for name, want in WANT_LIB2.items():
        assert [r[3][0] for r in o2[name]] == WANT_ONE[name] and [r[3][1] for r in o2[name]] == want, name
        assert len({r[0] for r in o2[name]}) == len(want), name  # every value of a batch differs from the others


@pytest.mark.gpu
def test_batch_takes_the_one_pass_routes():
    base, fam = _graph()[2], _graph()[3]
    c = _ctx("one")
    c.calc_prob(base)
    c.calc_prob_batch(fam["cands"])
    c.calc_prob_batch(fam["cands"])
    c.calc_prob_batch(fam["unrel"])
    st = c.table_stats(0)
    print(st)
    assert st["batches_patched"] + st["batches_full"] == 3 and st["batches_patched"] >= 1, st
    c.kernel_stats(reset=True)
    c.calc_prob_batch(fam["cands"])
    launches = c.kernel_stats()["launches"]
    print("scoring launches of one 8-set batch:", launches)
    assert 1 <= launches <= 2  # (one read set: the two halves of the batch)
    s = _ctx("one", batch_route="SEQUENTIAL")  # the sequential path: one call per path set
    s.calc_prob(base)
    s.calc_prob_batch(fam["cands"])
    s.calc_prob_batch(fam["unrel"])
    st = s.table_stats(0)
    assert st["batches_patched"] == 0 and st["batches_full"] == 0, st


def _same(got, want, tol, what):
    """counts, total_len and bad_bases exactly; the value within tol relative (0: bit for bit)"""
    assert len(got) == len(want), what
    for k, (a, b) in enumerate(zip(got, want)):
        assert a[1:] == b[1:], (what, k, a, b)
        if tol == 0:
            assert a[0] == b[0], (what, k, a, b)
        else:
            assert abs(a[0] - b[0]) <= tol * abs(b[0]), (what, k, a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_batch_equals_single_calls(variant):
    """1e-13 relative between two contexts with different call sequences (the bound of test_gpu_batch.py for the same
    situation: the contexts' delta lists fill and their tables are rebuilt at different calls, so the sum of 2,500 logs is
    taken in another order); bit for bit on one context."""
    fam = _graph()[3]
    order = [("cands", fam["cands"]), ("unrel", fam["unrel"]), ("mixed", fam["mixed"]), ("eleven", fam["cands"] + fam["unrel"][:3])]
    many_ctx, one_ctx = _ctx(variant), _ctx(variant)
    chunks = []
    for phase in ("cold", "warm"):
        for name, sets in order:
            want = [_call(one_ctx, s) for s in sets]
            _same(_batch(many_ctx, sets), want, 1e-13, (phase, name))
        st = many_ctx.table_stats(0)
        chunks.append((st["batches_patched"], st["batches_full"]))
        if phase == "cold":
            one_ctx.compact_tables()
            many_ctx.compact_tables()
    print(variant, "chunks patched / full after the cold and the warm phase", chunks)
    # warm: every chunk (1 + 1 + 1 + 2) takes a one-pass route, some of them from patches
    assert sum(chunks[1]) - sum(chunks[0]) == 5 and chunks[1][0] > chunks[0][0], chunks
    # one context, the same device state on both sides: every route gives the single calls' bits
    from gaml_amd.api import BatchRoute, Knob
    for route in (0, BatchRoute.FULL_TABLES, BatchRoute.NO_CAPTURE, BatchRoute.SEQUENTIAL):
        many_ctx.debug_set_knob(Knob.BATCH_ROUTE, route)
        for name, sets in order[:3]:
            got = _batch(many_ctx, sets)
            _same(got, [_call(many_ctx, s) for s in sets], 0, ("BATCH_ROUTE", route, name))
    many_ctx.debug_set_knob(Knob.BATCH_ROUTE, 0)
    # what a batch leaves behind is the last set's
    got = _batch(many_ctx, fam["cands"])
    assert many_ctx.bad_bases(0) == got[-1][3][0]
    want = _call(one_ctx, fam["cands"][-1])
    assert want[3] == got[-1][3]
    assert np.array_equal(many_ctx.read_probs(0), one_ctx.read_probs(0))
    # a blocking call right after a batch: the resident copy and the coverage layout are usable again
    a, b = _call(many_ctx, fam["unrel"][2]), _call(one_ctx, fam["unrel"][2])
    _same([a], [b], 1e-13, "blocking call after a batch")
    assert np.array_equal(many_ctx.read_probs(0), one_ctx.read_probs(0))


def _against_oracle(c, o, families):
    for name in families:
        sets = _graph()[3][name]
        got = _batch(c, sets)
        for k, (a, w) in enumerate(zip(got, o[name])):
            assert a[1:] == (w[1], w[2], w[3]), (name, k, a, w[:4])
            assert a[0] == w[0] or abs(a[0] - w[0]) <= 1e-9 * abs(w[0]), (name, k, a[0], w[0])
        for r in range(c.num_readsets()):
            np.testing.assert_allclose(c.read_probs(r), o[name][-1][4][r], rtol=4e-16, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["one", "many"])
def test_batch_against_the_oracle(variant):
    """tolerances of test_gpu_penalty_route.py; one base of bad_bases moves the value by 2e-4 on |v| ~ 78: 2.6e-6 relative"""
    c = _ctx(variant)
    _against_oracle(c, _oracle(variant), ("cands", "unrel", "mixed"))
    st = c.table_stats(0)
    assert st["batches_patched"] + st["batches_full"] == 3, st


@pytest.mark.gpu
@pytest.mark.parametrize("second_penalised", [True, False])
def test_two_libraries(second_penalised):
    base, fam = _graph()[2], _graph()[3]
    many_ctx, one_ctx = _ctx("one", second_penalised), _ctx("one", second_penalised)
    for c in (many_ctx, one_ctx):
        c.calc_prob(base)
    for phase in ("cold", "warm"):
        for name in ("cands", "unrel"):
            want = [_call(one_ctx, s) for s in fam[name]]
            got = _batch(many_ctx, fam[name])
            if not second_penalised:
                assert all(g[3][1] == 0 for g in got)
            _same(got, want, 1e-13 if phase == "cold" else 0, (phase, name))
        if phase == "cold":  # the same device state on both sides: everything folded into the record tables
            for c in (many_ctx, one_ctx):
                c.compact_tables()
                c.calc_prob(base)
    for r in (0, 1):
        st = many_ctx.table_stats(r)
        assert st["batches_patched"] + st["batches_full"] == 4, (r, st)
    if second_penalised:
        _against_oracle(_ctx("one", True), _oracle("one", True), ("cands", "unrel", "mixed"))


@pytest.mark.gpu
def test_gap_search_through_the_fallback():
    gap_set, gap_path, gap_pos = _graph()[4]
    twin = [y ^ 1 for y in reversed(gap_set[(gap_path + 1) % len(gap_set)]) if y >= 0]
    full = gap_set + [twin]
    dev, seq_ctx = _ctx("one"), _ctx("one", batch_route="SEQUENTIAL")
    res = []
    for c in (dev, seq_ctx):  # identical call sequences
        c.calc_prob(full)
        c.compact_tables()
        c.calc_prob(full)
        before = c.table_stats(0)
        length, trace = c.fix_gap_length(full, gap_path, gap_pos)
        st, after = c.gap_stats(), c.table_stats(0)
        assert st["device_lengths"] == 0 and st["fallback_lengths"] > 0, st
        res.append((length, trace, after["batches_patched"] + after["batches_full"] - before["batches_patched"] - before["batches_full"]))
    print(res[0][0], len(res[0][1]), res[0][2])
    assert res[0][0] == res[1][0] and res[0][1] == res[1][1]
    assert res[0][2] > 0 and res[1][2] == 0  # the fallback's multi-length steps took the one-pass route
