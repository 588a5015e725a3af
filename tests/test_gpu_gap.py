"""gaml_hip_gap_profile and gaml_hip_fix_gap_length on the GPU: a profile gives what the batch call, single calls and the
oracle give for the same path sets, on the device route (tables of every length derived on the device from the resident
ones) and on the fallback; the search follows the reference's FixGapLength (tests/gap_oracle.py) evaluation for
evaluation; neither leaves anything behind that a later call could see; the adapter's FixGapLength gives the same
lengths."""
import os
import re
import subprocess

import numpy as np
import pytest

import gap_oracle as go
from gaml_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "mock_ref", "_build", "gap_driver")


def _pack(reads):
    offs = np.zeros(len(reads) + 1, np.int64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    return np.concatenate([np.asarray(r, np.uint8) for r in reads]), offs


def _twin(path):
    return [x ^ 1 if x >= 0 else x for x in reversed(path)]


class Case:
    def __init__(self, g, m1, m2):
        self.g, self.m1, self.m2 = g, list(m1), list(m2)
        self.walk = synth.genome_walk(g)

    def make(self, single=None, penalty=0.0, devices=None, gap_fallback=False):
        from gaml_amd import api
        c = api.Context(device=0) if devices is None else api.Context(devices=devices)
        c.set_graph(*self.g.packed())
        c.add_paired(api.paired_cfg(go.INSERT_MEAN, go.INSERT_STD, penalty_constant=penalty), *_pack(self.m1), *_pack(self.m2))
        if single is not None:
            c.add_single(api.single_cfg(), *synth.pack_reads(single))
        if gap_fallback:
            c.debug_set_knob(api.Knob.GAP_FALLBACK, 1)
        return c

    def oracle(self):
        import oracle_py as op
        o = op.Oracle()
        o.set_graph(*self.g.packed())
        o.add_paired(*_pack(self.m1), *_pack(self.m2), 0.01, op.paired_cfg(go.INSERT_MEAN, go.INSERT_STD))
        return o


@pytest.fixture(scope="module")
def plain():
    g, pr, walk = go.make_inputs()
    return Case(g, pr.mate1, pr.mate2)


@pytest.fixture(scope="module")
def repeats():
    genome = synth.plant_repeats(synth.make_genome(go.GENOME, go.SEED), 2, 700, go.SEED)
    g = synth.make_graph(genome, synth.cut_lengths(go.GENOME, go.SEED, long_rng=(900, 4000)))
    pr = synth.make_paired_reads(genome, 24000, 100, go.INSERT_MEAN, go.INSERT_STD, 0.01, go.SEED)
    return Case(g, pr.mate1, pr.mate2)


@pytest.fixture(scope="module")
def mixed():
    g, pr, walk = go.make_inputs()
    m1, m2 = list(pr.mate1), list(pr.mate2)
    rng = np.random.default_rng(3)  # trimmed reads: several (L1, L2) combinations -> the length-code tables
    for i in range(0, len(m1), 3):
        m1[i] = m1[i][: int(rng.integers(70, 100))]
    for i in range(1, len(m2), 5):
        m2[i] = m2[i][: int(rng.integers(80, 100))]
    return Case(g, m1, m2)


def _same(got, want, rel):
    bit_equal = 0
    for k, (a, b) in enumerate(zip(got, want)):
        assert a[2] == b[2], (k, a[2], b[2])
        assert a[1].tolist() == b[1].tolist(), (k, a[1].tolist(), b[1].tolist())
        assert abs(a[0] - b[0]) <= rel * abs(b[0]), (k, a[0], b[0])
        bit_equal += a[0] == b[0]
    assert len(got) == len(want)
    return bit_equal


def _profile_cases(walk):
    w = walk
    base = go.gap_set(w, 5, 100)
    rng = np.random.default_rng(17)
    nineteen = [int(x) for x in rng.permutation(np.arange(40, 160, 6))[:19]]
    two_gaps = [w[:5] + [-40] + w[6:10] + [-70] + w[11:], w[3:9]]
    ends = [[-30] + w[2:12] + [-50] + w[13:14], w[20:26]]  # a leading gap, and a trailing contig of one node
    with_twin = [w[:7] + [-90] + w[8:], _twin(w[:7] + [-90] + w[8:])]
    again = [w[:8] + [-60] + w[5:8] + w[9:], w[3:9]]  # nodes 5..7 in front of the gap and behind it: list entries of ONE path on both sides
    return {
        "one length": (base, 0, 5, [100]),
        "eight lengths": (base, 0, 5, [100, 67, 1, 99, 101, 200, 33, 150]),
        "nine lengths": (base, 0, 5, [100, 67, 1, 99, 101, 200, 33, 150, 68]),
        "nineteen lengths": (base, 0, 5, nineteen),
        "repeated lengths": (base, 0, 5, [50, 50, 60, 50, 60, 60, 50, 61, 61, 50]),
        "far from the first": (base, 0, 5, [100, 1, 5000, 40000, 3, 1000000]),
        "first is the shortest": (base, 0, 5, [1, 2, 900]),
        "leading gap": (ends, 0, 0, [30, 1, 31, 400]),
        "gap before a one-node contig": (ends, 0, 11, [50, 49, 600, 2]),
        "two gaps, the first varied": (two_gaps, 0, 5, [40, 41, 39, 80, 160, 7]),
        "two gaps, the second varied": (two_gaps, 0, 10, [70, 140, 35, 71]),
        "second path edited": ([w[3:9], w[:7] + [-90] + w[8:]], 1, 7, [90, 45, 180]),
        "twin in the set": (with_twin, 0, 7, [90, 75, 76, 74, 300]),
        "twin edited": (with_twin, 1, len(w) - 8, [90, 75, 150]),
        "stretch on both sides": (again, 0, 8, [60, 61, 59, 120, 240, 1]),
    }


def _check_profile(case, paths, path_id, gap_pos, lens):
    dev, one, many = case.make(), case.make(), case.make()
    sets = [go.with_length(paths, path_id, gap_pos, l) for l in lens]
    got = dev.gap_profile(paths, path_id, gap_pos, lens)
    st = dev.gap_stats()
    assert st["device_lengths"] == len(lens) and st["fallback_lengths"] == 0, st
    assert st["device_passes"] == (len(lens) + 7) // 8, st
    eq_b = _same(got, many.calc_prob_batch(sets), 1e-13)
    eq_s = _same(got, [one.calc_prob(s) for s in sets], 1e-13)
    print(f"{len(lens)} lengths: {eq_b} bit-equal to the batch call, {eq_s} to single calls")
    for mate in (0, 1):
        assert dev.window_count(0, mate) == one.window_count(0, mate)
    # warm, and with another first length: the same values again
    again = dev.gap_profile(paths, path_id, gap_pos, lens[::-1])
    assert [a[0] for a in again] == [a[0] for a in got][::-1]
    return got


@pytest.mark.parametrize("name", ["one length", "eight lengths", "nine lengths", "nineteen lengths", "repeated lengths", "far from the first",
                                  "first is the shortest", "leading gap", "gap before a one-node contig", "two gaps, the first varied",
                                  "two gaps, the second varied", "second path edited", "twin in the set", "twin edited", "stretch on both sides"])
def test_profile_equals_batch_and_single_calls(plain, name):
    _check_profile(plain, *_profile_cases(plain.walk)[name])


@pytest.mark.parametrize("name", ["eight lengths", "twin in the set", "stretch on both sides", "two gaps, the first varied"])
def test_profile_on_a_genome_with_repeats(repeats, name):
    """plant_repeats: reads with several alignments (the record classes beyond the compact one); with the stretch on both
    sides of the gap, windows that occur several times in the path set (list entries) as well."""
    paths, path_id, gap_pos, lens = _profile_cases(repeats.walk)[name]
    dev = repeats.make()
    dev.calc_prob(paths)
    classes = dev.pair_classes(0)
    assert sum(classes[1:]) > 0, classes
    if name == "stretch on both sides":
        wids = dev.debug_table_occurrences(0, 0)[0][:, 0].tolist()
        assert len(wids) > len(set(wids))
    _check_profile(repeats, paths, path_id, gap_pos, lens)


@pytest.mark.parametrize("name", ["nine lengths", "twin in the set"])
def test_profile_with_mixed_read_lengths(mixed, name):
    _check_profile(mixed, *_profile_cases(mixed.walk)[name])


@pytest.mark.parametrize("name", ["nine lengths", "far from the first", "leading gap", "two gaps, the second varied", "twin in the set", "stretch on both sides"])
def test_profile_against_the_oracle(plain, name):
    paths, path_id, gap_pos, lens = _profile_cases(plain.walk)[name]
    o = plain.oracle()
    got = plain.make().gap_profile(paths, path_id, gap_pos, lens)
    want = [o.calc_prob(go.with_length(paths, path_id, gap_pos, l)) for l in lens]
    _same(got, want, 1e-9)


def test_profile_against_the_oracle_with_repeats(repeats):
    paths, path_id, gap_pos, lens = _profile_cases(repeats.walk)["stretch on both sides"]
    o = repeats.oracle()
    got = repeats.make().gap_profile(paths, path_id, gap_pos, lens)
    _same(got, [o.calc_prob(go.with_length(paths, path_id, gap_pos, l)) for l in lens], 1e-9)


def test_routes(plain):
    """A context of paired sets scores every length on the device route; a single-end set beside the paired one, a
    coverage penalty, Knob.GAP_FALLBACK and a multi-device context report the fallback. Same values whatever the route."""
    paths, path_id, gap_pos, lens = _profile_cases(plain.walk)["nine lengths"]
    sets = [go.with_length(paths, path_id, gap_pos, l) for l in lens]
    dev = plain.make()
    ref = dev.gap_profile(paths, path_id, gap_pos, lens)
    assert dev.gap_stats() == {"calls": 1, "device_lengths": 9, "fallback_lengths": 0, "device_passes": 2}

    def fallback(c, want, rel):
        got = c.gap_profile(paths, path_id, gap_pos, lens)
        st = c.gap_stats()
        assert st["device_lengths"] == 0 and st["device_passes"] == 0 and st["fallback_lengths"] == len(lens), st
        _same(got, want, rel)
        length, trace = c.fix_gap_length(paths, path_id, gap_pos)  # the search on this route: what it asks for, nothing ahead
        st2 = c.gap_stats()
        assert st2["device_lengths"] == 0 and st2["fallback_lengths"] - st["fallback_lengths"] == len(set(l for l, _ in trace)), (st, st2)
        return length, trace

    want_len, want_trace = dev.fix_gap_length(paths, path_id, gap_pos)
    got = fallback(plain.make(gap_fallback=True), ref, 1e-13)
    assert got[0] == want_len and [l for l, _ in got[1]] == [l for l, _ in want_trace]
    got = fallback(plain.make(devices=[0, 0]), ref, 1e-13)
    assert got[0] == want_len and [l for l, _ in got[1]] == [l for l, _ in want_trace]
    genome = synth.make_genome(go.GENOME, go.SEED)
    sr = synth.make_single_reads(genome, 2000, 100, 0.01, go.SEED)
    fallback(plain.make(single=sr), [plain.make(single=sr).calc_prob(s) for s in sets], 1e-13)
    fallback(plain.make(penalty=0.0005), [plain.make(penalty=0.0005).calc_prob(s) for s in sets], 1e-13)


def _search_cases(case):
    out = []
    for i in go.GAP_SITES:
        for start in go.start_lengths(case.g.node_len(case.walk[i])):
            out.append((go.gap_set(case.walk, i, start), 0, i))
    w = case.walk
    out.append(([w[:5] + [-1] + w[5:], w[3:9]], 0, 5))   # no base missing: a gap of 1 that should stay (cur == 1)
    out.append(([w[:5] + [-2] + w[5:], w[3:9]], 0, 5))
    return out


def test_search_follows_the_reference(plain):
    """Length and trace equal the restatement's over the oracle and over a twin context's calc_prob, for every checked
    input (no comparison there is closer than 1e-10, tests/test_gap_host.py: no case is left out); the trace's values
    are the profile's; a search of 20+ evaluations takes fewer device passes than evaluations."""
    o = plain.oracle()
    dev, twin = plain.make(), plain.make()
    states, doublings, span2 = set(), 0, 0
    # every window the cases name, then the record tables folded once: nothing rebuilds them between a search and the
    # profile its values are compared with bit for bit (a rebuild changes the order of the final sum)
    for paths, path_id, gap_pos in _search_cases(plain):
        dev.calc_prob(paths)
    dev.compact_tables()
    dev.calc_prob(_search_cases(plain)[0][0])
    for paths, path_id, gap_pos in _search_cases(plain):
        cur = -paths[path_id][gap_pos]
        want = go.oracle_search(o, paths, path_id, gap_pos)
        before = dev.gap_stats()
        length, trace = dev.fix_gap_length(paths, path_id, gap_pos)
        after = dev.gap_stats()
        passes = after["device_passes"] - before["device_passes"]
        print(f"gap at {gap_pos}, start {cur}: -> {length}, state {want.state}, {len(trace)} evaluations, {passes} device passes, "
              f"{after['device_lengths'] - before['device_lengths']} lengths scored")
        assert length == want.length, (gap_pos, cur)
        assert [l for l, _ in trace] == [l for l, _ in want.trace], (gap_pos, cur)
        for (l, v), (_, wv) in zip(trace, want.trace):
            assert abs(v - wv) <= 1e-9 * abs(wv), (gap_pos, cur, l)
        mine = go.Search(lambda l: twin.calc_prob(go.with_length(paths, path_id, gap_pos, l))[0], cur)
        assert mine.length == length and [l for l, _ in mine.trace] == [l for l, _ in trace]
        for (l, v), (_, tv) in zip(trace, mine.trace):
            assert abs(v - tv) <= 1e-13 * abs(tv), (gap_pos, cur, l)
        assert after["fallback_lengths"] == 0
        lens = sorted(set(l for l, _ in trace))
        prof = dict(zip(lens, (p[0] for p in dev.gap_profile(paths, path_id, gap_pos, lens))))
        assert all(prof[l] == v for l, v in trace), (gap_pos, cur)
        if len(trace) >= 20:
            assert passes < len(trace), (passes, len(trace))
        states.add((want.state, cur == 1))
        ls = [l for l, _ in want.trace]
        if want.state == 1:
            k = 2 if cur == 1 else 3
            n = 0
            while k + n < len(ls) and ls[k + n] == (2 * cur) << n:
                n += 1
            doublings = max(doublings, n)
        span2 += any(a == b for a, b in zip(ls, ls[1:]))
    # what the cases cover: stay with cur > 1 and with cur == 1, up, down, a bound that doubles more than once, a span-2 end
    assert {(0, False), (0, True), (1, True), (1, False), (2, False)} <= states, states
    assert doublings >= 2 and span2 >= 1


def test_nothing_is_left_behind(plain):
    """After a profile and a search the window cache is what one-by-one evaluations leave, and the next calls -- an
    unrelated path set, then an incremental edit of it -- give the twin's values."""
    paths, path_id, gap_pos, lens = _profile_cases(plain.walk)["nineteen lengths"]
    dev, twin = plain.make(), plain.make()
    dev.gap_profile(paths, path_id, gap_pos, lens)
    for l in lens:
        twin.calc_prob(go.with_length(paths, path_id, gap_pos, l))
    length, trace = dev.fix_gap_length(paths, path_id, gap_pos)
    for l, _ in trace:
        twin.calc_prob(go.with_length(paths, path_id, gap_pos, l))
    for mate in (0, 1):
        assert dev.window_count(0, mate) == twin.window_count(0, mate)
    w = plain.walk
    other = [w[10:40], _twin(w[45:70]), w[70:]]
    edited = [w[10:40], _twin(w[45:70]), w[70:90] + w[91:]]
    back = go.with_length(paths, path_id, gap_pos, length)
    _same([dev.calc_prob(s) for s in (other, edited, back, paths)], [twin.calc_prob(s) for s in (other, edited, back, paths)], 1e-13)
    # and straight after a profile: an incremental edit of the profiled set itself
    dev.gap_profile(paths, path_id, gap_pos, lens[:3])
    twin.calc_prob(go.with_length(paths, path_id, gap_pos, lens[0]))
    near = [paths[0][:-1], paths[1]]
    _same([dev.calc_prob(near)], [twin.calc_prob(near)], 1e-13)
    for mate in (0, 1):
        assert dev.window_count(0, mate) == twin.window_count(0, mate)


@pytest.mark.parametrize("devices", ["", "0,0"])
def test_adapter_gives_the_library_lengths(tmp_path, plain, devices):
    """ProbCalculator::FixGapLength, as the moves.cc patch of INTEGRATION.md §8 calls it, on FASTQ / LastGraph files."""
    from gaml_amd import api
    assert os.path.exists(DRIVER)
    d = str(tmp_path)
    synth.write_lastgraph(os.path.join(d, "LastGraph"), plain.g)
    f1, f2 = os.path.join(d, "a_1.fastq"), os.path.join(d, "a_2.fastq")
    synth.write_fastq(f1, np.asarray(plain.m1), "p", 1)
    synth.write_fastq(f2, np.asarray(plain.m2), "p", 2)
    jobs = [(5, 7), (5, 311), (7, 111), (9, 58), (9, 900)]
    env = dict(os.environ)
    env.pop("GAML_HIP_DEVICES", None)
    if devices:
        env["GAML_HIP_DEVICES"] = devices
    out = subprocess.run([DRIVER, os.path.join(d, "LastGraph"), f1, f2, str(go.INSERT_MEAN), str(go.INSERT_STD)] + [str(x) for j in jobs for x in j],
                         capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr
    rows = [(int(a), int(b), int(c)) for a, b, c in re.findall(r"gap (\d+) (\d+) -> (\d+)", out.stdout)]
    assert [r[:2] for r in rows] == jobs, out.stdout[:2000]
    ctx = api.Context(device=0)
    ctx.load_graph(os.path.join(d, "LastGraph"))
    ctx.add_paired_fastq(api.paired_cfg(go.INSERT_MEAN, go.INSERT_STD), f1, f2)
    walk = list(range(0, plain.g.n_nodes, 2))
    for site, start, got in rows:
        length, _ = ctx.fix_gap_length(go.gap_set(walk, site, start), 0, site)
        assert got == length, (site, start)
