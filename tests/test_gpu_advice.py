"""The advice move of a paired set on the device (advice.hip.h): index and candidate lists against the host-only context
and the oracle restatement of the reference (tests/advice_oracle.py), on one device and on two in-process shards;
repeats, short outputs, and the scores around it."""
import numpy as np
import pytest

from advice_oracle import make_case, oracle_candidates, oracle_index, query_paths
from gaml_amd import synth

pytestmark = pytest.mark.gpu

THRESHOLD = 500


def _ctx(g, r1, r2, device=0, devices=None, cfg=(1500.0, 150.0)):
    from gaml_amd import api
    ctx = api.Context(device=device) if devices is None else api.Context(devices=devices)
    ctx.set_graph(*g.packed())
    rs = ctx.add_paired(api.paired_cfg(*cfg), *r1, *r2)
    return ctx, rs


def _oracle(g, r1, r2, cfg=(1500.0, 150.0)):
    import oracle_py as op
    orc = op.Oracle()
    orc.set_graph(*g.packed())
    return orc, orc.add_paired(*r1, *r2, 0.01, op.paired_cfg(*cfg))


def _same_index(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def _flag_sets():
    return [(o, a) for o in (True, False) for a in (False, True)]


@pytest.fixture(scope="module")
def case(built):
    g, r1, r2 = make_case()
    return g, r1, r2


def test_device_matches_host_and_oracle(case):
    g, r1, r2 = case
    dev, rs = _ctx(g, r1, r2)
    host, hrs = _ctx(g, r1, r2, device=-1)
    orc, ors = _oracle(g, r1, r2)
    n = dev.readset_reads(rs)
    node_len = [g.node_len(i) for i in range(g.n_nodes)]
    dev.advice_build(rs, THRESHOLD)
    host.advice_build(hrs, THRESHOLD)
    _, advice1 = oracle_index(orc, ors, node_len, THRESHOLD, n)
    idx = dev.advice_index(rs)
    _same_index(idx, host.advice_index(hrs))
    rng = np.random.default_rng(5)
    total = 0
    for path in query_paths(g):
        for reach in ([], sorted(set(rng.integers(0, g.n_nodes, g.n_nodes // 3).tolist())), list(range(g.n_nodes))):
            for only_out, allow_gaps in _flag_sets():
                got = dev.advice_candidates(rs, path, reach, only_out, allow_gaps)
                want = oracle_candidates(orc, ors, node_len, path, advice1, reach, only_out, allow_gaps, n)
                assert got.tolist() == want
                assert host.advice_candidates(hrs, path, reach, only_out, allow_gaps).tolist() == want
                again = dev.advice_candidates(rs, path, reach, only_out, allow_gaps)  # a repeat: the same list
                assert np.array_equal(got, again)
                total += len(got)
                if len(got) > 3:  # cap below the count: the true count and a correct prefix
                    k, head = dev.advice_candidates(rs, path, reach, only_out, allow_gaps, cap=3)
                    assert k == len(got) and head.tolist() == got[:3].tolist()
    assert total > 0
    for mate in (0, 1):
        keys = {tuple(dev.debug_window_walk(rs, mate, w)) for w in range(dev.window_count(rs, mate))}
        assert keys == set(orc.window_keys(ors, mate))


def test_two_device_shards_match_one(case):
    g, r1, r2 = case
    one, rs1 = _ctx(g, r1, r2)
    two, rs2 = _ctx(g, r1, r2, devices=[0, 0])
    one.advice_build(rs1, THRESHOLD)
    two.advice_build(rs2, THRESHOLD)
    _same_index(one.advice_index(rs1), two.advice_index(rs2))
    reach = list(range(0, g.n_nodes, 3))
    for path in query_paths(g, n=8, seed=9):
        for only_out, allow_gaps in _flag_sets():
            a = one.advice_candidates(rs1, path, reach, only_out, allow_gaps)
            b = two.advice_candidates(rs2, path, reach, only_out, allow_gaps)
            assert a.tolist() == b.tolist()


def test_jumping_library_at_1mbp():
    """1 Mbp, 60 000 jumping pairs (insert 3700 +- 350, like test_gpu_properties.py): device = host-only = oracle."""
    G, seed = 1_000_000, 41
    genome = synth.make_genome(G, seed)
    g = synth.make_graph(genome, synth.cut_lengths(G, seed))
    pr = synth.make_paired_reads(genome, 60_000, 150, 3700.0, 350.0, 0.01, seed)
    r1, r2 = synth.pack_reads(pr.mate1), synth.pack_reads(pr.mate2)
    cfg = (3700.0, 350.0)
    dev, rs = _ctx(g, r1, r2, cfg=cfg)
    host, hrs = _ctx(g, r1, r2, device=-1, cfg=cfg)
    two, rs2 = _ctx(g, r1, r2, devices=[0, 0], cfg=cfg)
    orc, ors = _oracle(g, r1, r2, cfg=cfg)
    node_len = [g.node_len(i) for i in range(g.n_nodes)]
    walk = synth.genome_walk(g)
    for c in (dev, two, orc):  # a scored path set first: its windows are in the caches (host-only: index only)
        c.calc_prob([walk])
    for c, r in ((dev, rs), (host, hrs), (two, rs2)):
        c.advice_build(r, THRESHOLD)
    _, advice1 = oracle_index(orc, ors, node_len, THRESHOLD, 60_000)
    idx = dev.advice_index(rs)
    _same_index(idx, host.advice_index(hrs))
    _same_index(idx, two.advice_index(rs2))
    assert len(idx[1]) > 60_000
    for path in query_paths(g, n=6, seed=21):
        reach = walk[:: 2]
        for only_out, allow_gaps in ((True, False), (False, True)):
            got = dev.advice_candidates(rs, path, reach, only_out, allow_gaps)
            want = oracle_candidates(orc, ors, node_len, path, advice1, reach, only_out, allow_gaps, 60_000)
            assert got.tolist() == want
            assert two.advice_candidates(rs2, path, reach, only_out, allow_gaps).tolist() == want


def test_interleaved_with_calc_prob(case):
    """~200 calls, calc_prob and advice queries interleaved, against the oracle: the windows the queries register score
    like any other window."""
    g, r1, r2 = case
    dev, rs = _ctx(g, r1, r2)
    orc, ors = _oracle(g, r1, r2)
    n = dev.readset_reads(rs)
    node_len = [g.node_len(i) for i in range(g.n_nodes)]
    start, seq = synth.sa_sequence(g, 120, seed=13, threshold=THRESHOLD)
    dev.advice_build(rs, THRESHOLD)
    _, advice1 = oracle_index(orc, ors, node_len, THRESHOLD, n)
    rng = np.random.default_rng(17)
    calls = 0
    for k, paths in enumerate([start] + seq):
        got = dev.calc_prob(paths)
        want, wz, wtl = orc.calc_prob(paths, fresh=True)
        assert got[2] == wtl and got[1].tolist() == wz.tolist()
        assert abs(got[0] - want) <= 1e-9 * abs(want), (k, got[0], want)
        calls += 1
        if k % 3 == 0:
            p = paths[int(rng.integers(0, len(paths)))]
            if rng.random() < 0.5:
                p = [x ^ 1 if x >= 0 else x for x in reversed(p)]
            only_out, allow_gaps = bool(rng.random() < 0.8), bool(rng.random() < 0.2)
            reach = sorted(set(rng.integers(0, g.n_nodes, 40).tolist()))
            a = dev.advice_candidates(rs, p, reach, only_out, allow_gaps)
            assert a.tolist() == oracle_candidates(orc, ors, node_len, p, advice1, reach, only_out, allow_gaps, n)
            calls += 1
    assert calls >= 150
    for mate in (0, 1):
        keys = {tuple(dev.debug_window_walk(rs, mate, w)) for w in range(dev.window_count(rs, mate))}
        assert keys == set(orc.window_keys(ors, mate))


def test_scores_unchanged_by_the_index(case):
    """calc_prob of a fixed path set is bit-equal before the build, after it and after queries that register nothing new."""
    g, r1, r2 = case
    dev, rs = _ctx(g, r1, r2)
    walk = synth.genome_walk(g)
    paths = [walk]
    dev.calc_prob(paths)
    before = dev.calc_prob(paths)
    wins = (dev.window_count(rs, 0), dev.window_count(rs, 1))
    dev.advice_build(rs, THRESHOLD)
    assert (dev.window_count(rs, 0), dev.window_count(rs, 1)) == wins  # every long node's window came with the path set
    after_build = dev.calc_prob(paths)
    for flags in _flag_sets():
        dev.advice_candidates(rs, walk, walk[::3], *flags)
    assert (dev.window_count(rs, 0), dev.window_count(rs, 1)) == wins
    after_queries = dev.calc_prob(paths)
    for x in (after_build, after_queries):
        assert x[0] == before[0] and x[1].tolist() == before[1].tolist() and x[2] == before[2]


def test_overwrite_rule_and_serial_wrap_on_the_device(built):
    """The first slot ends with the orientation of the LAST record at its absolute position (tests/advice_oracle.py:
    overwrite_case), on the device; then past the wrap of the 16-bit call serial (65,535 queries) two alternating walks
    with different qualifying pairs keep their own answers -- stale per-pair words never count."""
    from advice_oracle import overwrite_case
    from gaml_amd import api
    ctx, rs, a, b, v = overwrite_case(lambda: api.Context(device=0))
    ctx.advice_build(rs, 500)
    offs, nodes, orient1 = ctx.advice_index(rs)
    assert offs.tolist() == [0, 1, 2, 3, 4] and nodes.tolist() == [v] * 4 and orient1.all()
    ab = np.array([a, b], np.int32)
    bb = np.array([b], np.int32)
    for k in range(66_000):
        if k % 2 == 0:
            got = ctx.advice_candidates(rs, ab, (), only_out=True, allow_gaps=True)
            assert got.tolist() == [v, v, v], k  # pairs 1, 2, 3 (pair 0 was rewritten to reverse)
        else:
            got = ctx.advice_candidates(rs, bb, (), only_out=True, allow_gaps=True)
            assert got.tolist() == [v], k  # pair 3 alone
