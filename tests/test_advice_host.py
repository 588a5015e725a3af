"""The advice move of a paired set on host-only contexts (device = -1; -1,-1): gaml_hip_advice_build / _index /
_candidates against the reference's BuildAdviceIndex and the candidate loop of ExtendPathsAdv (moves.cc:948-986),
restated over the oracle's window cache (tests/advice_oracle.py)."""
import numpy as np
import pytest

from advice_oracle import make_case, oracle_candidates, oracle_index, query_paths

THRESHOLD = 500


@pytest.fixture(scope="module")
def case(built):
    return make_case()


def _contexts(case, devices=None):
    from gaml_amd import api
    import oracle_py as op
    g, (b1, o1), (b2, o2) = case
    gb, go = g.packed()
    ctx = api.Context(device=-1) if devices is None else api.Context(devices=devices)
    ctx.set_graph(gb, go)
    rs = ctx.add_paired(api.paired_cfg(1500.0, 150.0), b1, o1, b2, o2)
    orc = op.Oracle()
    orc.set_graph(gb, go)
    ors = orc.add_paired(b1, o1, b2, o2, 0.01, op.paired_cfg(1500.0, 150.0))
    return ctx, rs, orc, ors


def _library_keys(ctx, rs, mate):
    return {tuple(ctx.debug_window_walk(rs, mate, w)) for w in range(ctx.window_count(rs, mate))}


def _check_index(ctx, rs, advice, advice1):
    offs, nodes, orient1 = ctx.advice_index(rs)
    assert len(offs) == len(advice) + 1
    for r in range(len(advice)):
        got = nodes[offs[r]:offs[r + 1]].tolist()
        assert got == advice[r], r
        assert [v for v, f in zip(got, orient1[offs[r]:offs[r + 1]]) if f] == advice1[r], r


def _run_queries(ctx, rs, orc, ors, g, advice1, n_pairs):
    node_len = [g.node_len(i) for i in range(g.n_nodes)]
    rng = np.random.default_rng(11)
    got_all = []
    for path in query_paths(g):
        last = path[-1]
        reaches = [[], sorted(set(int(x) for x in rng.integers(0, g.n_nodes, g.n_nodes // 3))), list(range(g.n_nodes))]
        for reach in reaches:
            for only_out in (True, False):
                for allow_gaps in (False, True):
                    got = ctx.advice_candidates(rs, path, reach, only_out, allow_gaps)
                    want = oracle_candidates(orc, ors, node_len, path, advice1, reach, only_out, allow_gaps, n_pairs)
                    assert got.tolist() == want, (path, len(reach), only_out, allow_gaps, last)
                    got_all.append(got)
    return got_all


def test_index_and_candidates_match_the_oracle(case):
    g = case[0]
    ctx, rs, orc, ors = _contexts(case)
    n_pairs = ctx.readset_reads(rs)
    node_len = [g.node_len(i) for i in range(g.n_nodes)]
    ctx.advice_build(rs, THRESHOLD)
    advice, advice1 = oracle_index(orc, ors, node_len, THRESHOLD, n_pairs)
    assert sum(len(a) for a in advice1) > 100 and any(len(a) > 1 for a in advice)
    _check_index(ctx, rs, advice, advice1)
    lists = _run_queries(ctx, rs, orc, ors, g, advice1, n_pairs)
    assert sum(len(x) for x in lists) > 0 and any(len(x) == 0 for x in lists)
    for mate in (0, 1):  # the windows the build and the queries registered: the reference's
        assert _library_keys(ctx, rs, mate) == set(orc.window_keys(ors, mate)), mate


def test_build_rules(case):
    from gaml_amd import api
    g, (b1, o1), (b2, o2) = case
    ctx = api.Context(device=-1)
    ctx.set_graph(*g.packed())
    single = ctx.add_single(api.single_cfg(), b1, o1)
    rs = ctx.add_paired(api.paired_cfg(1500.0, 150.0), b1, o1, b2, o2)
    walk = synth_walk(g)[:4]
    with pytest.raises(api.GamlHipError) as e:
        ctx.advice_candidates(rs, walk)
    assert e.value.code == api.ESTATE  # query before the build
    with pytest.raises(api.GamlHipError) as e:
        ctx.advice_index(rs)
    assert e.value.code == api.ESTATE
    with pytest.raises(api.GamlHipError) as e:
        ctx.advice_build(single, THRESHOLD)
    assert e.value.code == api.EINVAL  # not a paired set
    ctx.advice_build(rs, THRESHOLD)
    first = ctx.advice_index(rs)
    wins = ctx.window_count(rs, 1)
    ctx.advice_build(rs, 100)  # graph.cc:324: a second build does nothing
    again = ctx.advice_index(rs)
    assert ctx.window_count(rs, 1) == wins
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    with pytest.raises(api.GamlHipError) as e:
        ctx.advice_candidates(rs, [0, g.n_nodes])
    assert e.value.code == api.EINVAL
    n, head = ctx.advice_candidates(rs, synth_walk(g)[:8], allow_gaps=True, only_out=False, cap=2)
    full = ctx.advice_candidates(rs, synth_walk(g)[:8], allow_gaps=True, only_out=False)
    assert n == len(full) and head.tolist() == full[:2].tolist()
    ranked = api.Context(device=-1, rank=0, world=2)  # rank-per-process contexts are not served
    ranked.set_graph(*g.packed())
    r2 = ranked.add_paired(api.paired_cfg(1500.0, 150.0), b1, o1, b2, o2)
    with pytest.raises(api.GamlHipError) as e:
        ranked.advice_build(r2, THRESHOLD)
    assert e.value.code == api.ESTATE


def synth_walk(g):
    from gaml_amd import synth
    return synth.genome_walk(g)


def test_two_host_shards_match_one(case):
    g = case[0]
    one, rs1, _, _ = _contexts(case)
    two, rs2, _, _ = _contexts(case, devices=[-1, -1])
    one.advice_build(rs1, THRESHOLD)
    two.advice_build(rs2, THRESHOLD)
    for a, b in zip(one.advice_index(rs1), two.advice_index(rs2)):
        assert np.array_equal(a, b)
    reach = list(range(0, g.n_nodes, 3))
    for path in query_paths(g, n=6, seed=9):
        for flags in ((True, False), (False, True), (True, True)):
            a = one.advice_candidates(rs1, path, reach, *flags)
            b = two.advice_candidates(rs2, path, reach, *flags)
            assert a.tolist() == b.tolist()


def test_first_slot_takes_the_last_orientation_at_its_position(built):
    """A pair whose first slot is rewritten by a later record of the opposite strand at the same absolute position
    (graph.cc:708-723) drops out; the others stay (tests/advice_oracle.py: overwrite_case)."""
    from advice_oracle import overwrite_case
    from gaml_amd import api
    ctx, rs, a, b, v = overwrite_case(lambda: api.Context(device=-1))
    ctx.advice_build(rs, 500)
    offs, nodes, orient1 = ctx.advice_index(rs)
    assert offs.tolist() == [0, 1, 2, 3, 4] and nodes.tolist() == [v] * 4 and orient1.all()
    assert ctx.advice_candidates(rs, [a, b], [], only_out=True, allow_gaps=True).tolist() == [v, v, v]  # pairs 1, 2, 3
    assert ctx.advice_candidates(rs, [b], [v], only_out=True, allow_gaps=False).tolist() == [v]       # pair 3 alone
