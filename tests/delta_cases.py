"""Inputs shared by the tests of the device delta-list maintenance (tests/test_delta_cases_host.py,
tests/test_gpu_delta_lists.py): three read sets and, per scenario, a sequence of path sets -- the first builds the record
tables, every later one activates a chosen group of windows -- together with the launch the maintenance has to choose for
that group by default and with DELTA_ONE_BLOCK (gaml_amd/csrc/paired_tables.hip.h paired_delta_apply). Deterministic; numpy only."""
from functools import lru_cache

import numpy as np

from gaml_amd import synth

READ_LEN, INSERT = 100, (240.0, 24.0)
LONG = 500  # a node longer than this is a "long node" (the pieces alternate 600-4,000 and 25-330 bases)

# name -> (genome length, pairs, seed, planted repeat copies)
FIXTURES = {"small": (60_000, 3_000, 5, 0), "medium": (120_000, 24_000, 7, 5), "large": (300_000, 120_000, 11, 0)}
# the long nodes (index among the long nodes) that hold a copy of the medium fixture's repeat
REPEAT_NODES = (4, 8, 18, 31, 34, 39)


def delta_cap(n_pairs):
    """Pairs the delta store has room for (paired_reserve_delta); a call whose records would take the lists past
    delta_cap - 2,048 rebuilds the tables instead of extending the lists."""
    return max(4096, n_pairs // 2) + 8192


def hard_limit(n_pairs):
    return delta_cap(n_pairs) - 2048


@lru_cache(maxsize=None)
def fixture(name):
    """(graph, paired reads, long nodes in walk order) of one of FIXTURES."""
    G, n, seed, repeats = FIXTURES[name]
    genome = synth.make_genome(G, seed)
    if repeats:
        genome = synth.plant_repeats(genome, repeats, 800, seed)
    g = synth.make_graph(genome, synth.cut_lengths(G, seed, long_rng=(600, 4000), short_rng=(25, 330)))
    pr = synth.make_paired_reads(genome, n, READ_LEN, INSERT[0], INSERT[1], 0.01, seed)
    longs = [x for x in synth.genome_walk(g) if g.node_len(x) > LONG]
    return g, pr, longs


def packed_reads(pr):
    return (*synth.pack_reads(pr.mate1), *synth.pack_reads(pr.mate2))


def _solo(nodes):
    return [[x] for x in nodes]


# What a step's activation has to come to, and what paired_delta_apply then launches: (records lo, records hi, windows lo,
# windows hi, route by default, route with DELTA_ONE_BLOCK). A route is a dict of the counters gaml_hip_debug_delta_routes
# returns that the step must add ("one", "two", "four", "eight": one-block launches by records per thread; "multi_block",
# "multi_block_wlist", "windows_cut"); a counter it does not name must not move. A tuple as a value: (at least, at most).
class Scenario:
    def __init__(self, name, fix, steps, expect):
        self.name, self.fixture, self.steps, self.expect = name, fix, steps, expect

    def __repr__(self):
        return self.name


def _medium_add(first, last):
    """tables from the long nodes k >= 10 as single paths, then the long nodes first .. last as well"""
    _, _, longs = fixture("medium")
    return [_solo(longs[10:]), _solo(longs[first:last + 1]) + _solo(longs[10:])]


def pieces_steps():
    """Tables from the medium fixture's genome walk and its twin walk -- reads around the short nodes then have 3 to 4
    records on a mate, some 5,800 pairs: enough for the record tables' class of that size to exist (below 1,024 such
    pairs they are scored with the longer lists) -- then the forward walk cut behind every short node: each piece ends in
    a window the whole walk did not have, and the reads across those ends gain a record."""
    g, _, _ = fixture("medium")
    walk = synth.genome_walk(g)
    rev = [x ^ 1 for x in reversed(walk)]
    pieces, cur = [], []
    for x in walk:
        cur.append(x)
        if g.node_len(x) <= LONG:
            pieces.append(cur)
            cur = []
    if cur:
        pieces.append(cur)
    return [[walk, rev], pieces + [rev]]


def spill_steps():
    """The medium fixture's repeat: tables without the long nodes 4, 8 and 18, then these three one call each -- the reads
    of the repeat go from 3 records per mate to 4, 5 and 6 -- then the twins of all six long nodes with a copy as well (the
    reversed walks: the lists of those reads double)."""
    _, _, longs = fixture("medium")
    held_back = REPEAT_NODES[:3]
    cur = [x for k, x in enumerate(longs) if k not in held_back]
    steps = [_solo(cur)]
    for k in held_back:
        cur = cur + [longs[k]]
        steps.append(_solo(cur))
    steps.append(_solo(cur) + [[longs[k] ^ 1] for k in reversed(REPEAT_NODES)])
    return steps


# records the steps of spill_steps activate: what each launch needs, (at least, at most)
SPILL_RECORDS = ((2049, 3000), (1025, 2048), (1025, 2048), (8193, 16384))
# ... and the launches those make: by default / with DELTA_ONE_BLOCK (see scenarios())
SPILL_ROUTES = (({"four": 1}, {"four": 1}), ({"two": 1}, {"two": 1}), ({"two": 1}, {"two": 1}), ({"multi_block": 1}, {"launches": 2, "windows_cut": 1}))


def sa_walk_steps(iters=40):
    """a short annealing walk from the spill scenario's last set: pairs already on the lists are touched again and again"""
    g, _, _ = fixture("medium")
    rng = np.random.default_rng(23)
    cur, out = spill_steps()[-1], []
    for _ in range(iters):
        new = synth.sa_move(rng, cur, g)
        out.append(new)
        if rng.random() < 0.6:
            cur = new
    return out


@lru_cache(maxsize=None)
def scenarios():
    g_s, _, longs_s = fixture("small")
    _, _, longs_l = fixture("large")
    walk_s = synth.genome_walk(g_s)
    at = walk_s.index(longs_s[0])
    joined = [walk_s[at:walk_s.index(longs_s[1]) + 1]] + _solo(longs_s[2:])  # the first two long nodes and what lies between them
    multi = {"multi_block": 1}
    return [
        Scenario("small-junction-walk", "small", [_solo(longs_s), joined, [walk_s], [walk_s, [x ^ 1 for x in reversed(walk_s)]]],
                 [(1, 128, 1, 64, {"one": 1, "min_block": (64, 128)}, {"one": 1, "min_block": (64, 128)}),
                  (1025, 2048, 1, 64, {"two": 1}, {"two": 1}),
                  (3001, 8192, 65, 128, {"multi_block": 1, "multi_block_wlist": 1}, {"launches": (2, 9)})]),
        Scenario("medium-0", "medium", _medium_add(0, 0), [(513, 1024, 1, 64, {"one": 1, "min_block": 1024}, {"one": 1, "min_block": 1024})]),
        Scenario("medium-0-1", "medium", _medium_add(0, 1), [(1025, 2048, 1, 64, {"two": 1}, {"two": 1})]),
        Scenario("medium-0-3", "medium", _medium_add(0, 3), [(2049, 3000, 1, 64, {"four": 1}, {"four": 1})]),
        Scenario("medium-1-4", "medium", _medium_add(1, 4), [(3001, 4096, 1, 64, multi, {"four": 1})]),
        Scenario("medium-0-4", "medium", _medium_add(0, 4), [(4097, 8192, 1, 64, multi, {"eight": 1})]),
        Scenario("medium-0-9", "medium", _medium_add(0, 9), [(8193, 16384, 1, 64, multi, {"launches": 2, "windows_cut": 1})]),
        Scenario("medium-pieces", "medium", pieces_steps(), [(3001, 8192, 65, 192, {"multi_block": 1, "multi_block_wlist": 1}, {"launches": (3, 9)})]),
        Scenario("large-0-31", "large", [_solo(longs_l[32:]), _solo(longs_l)],
                 [(49153, 2 * 49152, 1, 64, {"multi_block": 2, "windows_cut": 1}, {"launches": 7})]),
    ]


def scenario(name):
    return next(s for s in scenarios() if s.name == name)


def measure(ctx, rs, steps):
    """On a context that need not have a device: per step after the first, (records, windows, pairs) -- the records and
    the number of the windows the step activates (both mates, windows without records left out), from the occurrence lists
    of gaml_hip_debug_prepare, and the pairs the earlier steps after the first had touched (no fewer than the lists hold
    when the step begins: a call rebuilds the tables when pairs on the lists + its records pass hard_limit) -- and per
    step, per mate, the records per read over every window in use so far."""
    seen = [set(), set()]
    out, per_read = [], []
    n = ctx.readset_reads(rs)
    counts = [np.zeros(n, np.int64), np.zeros(n, np.int64)]
    touched = np.zeros(n, bool)
    for k, paths in enumerate(steps):
        ctx.debug_prepare(paths)
        records = windows = 0
        before = int(touched.sum())
        for mate in (0, 1):
            used = set(int(w) for w in ctx.debug_occurrences(rs, mate)[:, 0])
            for w in sorted(used - seen[mate]):
                recs = ctx.window_records(rs, mate, ctx.debug_window_walk(rs, mate, w))
                if recs is None or len(recs) == 0:
                    continue
                records += len(recs)
                windows += 1
                counts[mate] += np.bincount(recs[:, 2], minlength=n)
                if k > 0:
                    touched[recs[:, 2]] = True
            seen[mate] |= used
        out.append((records, windows, before))
        per_read.append([c.copy() for c in counts])
    return out[1:], per_read
