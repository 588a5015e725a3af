"""Inputs of the gap-profile tests over read sets with a coverage penalty (tests/test_gap_penalty_cases_host.py keeps them
honest on the CPU, tests/test_gpu_gap_penalty.py runs them on the device route).

The graph and libraries are those of tests/test_gpu_penalty_batch.py. Library B (1,500 pairs, insert 400 +- 40, penalty
0.0005) is the one whose pairs straddle a short node: with the node at walk position 81 (63 bases) or 105 (129 bases)
replaced by a gap, B's bad_bases is positive and depends on the gap's length (a scan of all 55 short-node sites found
these two). Library A's 40-base inner distance never straddles one: its bad_bases is the same at every length.

A profile varies ONE gap. The issue's "twin in the set" case, [e(L), twin(e(L))], varies two; it is pinned as stated for
the oracle (TWIN_BOTH_WANT), and the profile runs [e(L), twin(e(63))]: the twin keeps the node's own length, every window
still occurs twice (GEN instantiation, list entries)."""
import functools

import numpy as np

from gaml_amd import synth

G, SEED = 150_000, 17
PENALTY_A, PENALTY_B = 0.0002, 0.0005
SITE81_LENS = [63, 1, 62, 64, 96, 163, 213, 263, 313, 363, 463, 1000, 40000]      # thirteen lengths: two passes; lens[0] is the base
SITE105_LENS = [129, 1, 128, 130, 162, 229, 279, 329, 379, 429, 529, 1000, 40000]
SHORT_LENS = [63, 1, 62, 64, 96, 263, 1000]  # (1, 63, 263, 1000 are the pinned ones; 62, 64, 96: d != 0 with and without a change of the region's size)

# Start lengths of the searches the GPU test follows. Of 1, 7, 63 and 900 at both sites these compare no two values closer
# than 1e-9 relative over the oracle; dropped: site 81 from 63 and 900 (closest comparison 1.5e-10), site 105 from 7 and 900
# (2.2e-10) and from 63 (8.8e-10). tests/test_gap_penalty_cases_host.py checks both lists.
SEARCH_STARTS = {"site 81, edited first": (1, 7), "site 105, edited first": (1,)}
SEARCH_DROPPED = {"site 81, edited first": (63, 900), "site 105, edited first": (7, 63, 900)}
SEARCH_ENDS = {"site 81, edited first": 15, "site 105, edited first": 134}


def pack(reads):
    offs = np.zeros(len(reads) + 1, np.int64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    return np.concatenate([np.asarray(r, np.uint8) for r in reads]), offs


def twin(path):
    return [x ^ 1 if x >= 0 else x for x in reversed(path)]


@functools.lru_cache(maxsize=None)
def graph():
    genome = synth.plant_repeats(synth.make_genome(G, SEED), 3, 800, SEED)
    g = synth.make_graph(genome, synth.cut_lengths(G, SEED, long_rng=(600, 4000), short_rng=(25, 330)))
    return genome, g, synth.genome_walk(g)


@functools.lru_cache(maxsize=None)
def reads_b(trimmed=False):
    pr = synth.make_paired_reads(graph()[0], 1_500, 100, 400.0, 40.0, 0.01, SEED + 1)
    m1, m2 = list(pr.mate1), list(pr.mate2)
    if trimmed:  # several length codes: the trimming of test_gpu_penalty_batch._reads("many")
        rng = np.random.default_rng(3)
        for i in range(0, len(m1), 3):
            m1[i] = m1[i][: int(rng.integers(70, 100))]
        for i in range(1, len(m2), 5):
            m2[i] = m2[i][: int(rng.integers(80, 100))]
    return (*pack(m1), *pack(m2))


@functools.lru_cache(maxsize=None)
def reads_a():
    pr = synth.make_paired_reads(graph()[0], 2_500, 100, 240.0, 24.0, 0.01, SEED)
    return (*pack(list(pr.mate1)), *pack(list(pr.mate2)))


def edited81(length):
    w = graph()[2]
    return w[69:81] + [-length] + w[82:93]


def cases():
    """name -> (paths with the base length in the gap, path_id, gap_pos, lens); lens[0] is the base length"""
    w = graph()[2]
    e = edited81(63)
    two_gaps = w[69:75] + [-graph()[1].node_len(w[75])] + w[76:81] + [-63] + w[82:93]
    return {
        "site 81, edited first": ([e, w[93:99]], 0, 12, SITE81_LENS),
        "site 81, edited in the middle": ([w[30:36], e, w[93:99]], 1, 12, SITE81_LENS),
        "site 105, edited first": ([w[93:105] + [-129] + w[106:111], w[:6]], 0, 12, SITE105_LENS),
        "two gaps, the second varied": ([two_gaps, w[93:99]], 0, 12, SHORT_LENS),
        "twin in the set": ([e, twin(e)], 0, 12, SHORT_LENS),
        # of our own
        "edited last": ([w[30:36], w[93:99], e], 2, 12, SHORT_LENS),
        "leading gap": ([[-63] + w[82:93], w[69:81], w[93:99]], 0, 0, SHORT_LENS),
        "two gaps, the first varied": ([w[69:81] + [-63] + w[82:93] + [-129] + w[106:111], w[:6]], 0, 12, SHORT_LENS),
    }


# the oracle's bad_bases of library B alone (fresh=True), per case and length
WANT = {
    "site 81, edited first": {**{l: 1770 for l in (1, 62, 63, 64, 96, 163, 213, 263, 313, 363, 463)}, 1000: 1207, 40000: 1207},
    "site 81, edited in the middle": {**{l: 1770 for l in (1, 62, 63, 64, 96, 163, 213, 263, 313, 363, 463)}, 1000: 1207, 40000: 1207},
    "site 105, edited first": {**{l: 846 for l in (1, 128, 129, 130, 162, 229, 279, 329, 379, 429, 529)}, 1000: 477, 40000: 477},
    "two gaps, the second varied": {1: 1770, 63: 1770, 263: 1770, 1000: 1207},
}
TWIN_BOTH_WANT = {1: 3540, 63: 3540, 263: 3540, 1000: 2414}  # [e(L), twin(e(L))]: both gaps at L


def with_length(paths, path_id, gap_pos, length):
    out = [list(p) for p in paths]
    out[path_id][gap_pos] = -length
    return out


def cov_bits(length):
    """bits a path of that length keeps in the coverage bitmap (paired_cov_build)"""
    return ((length + 64 + 31) // 32) * 32


def path_len(path):
    g = graph()[1]
    return sum(-x if x < 0 else g.node_len(x) for x in path)


def make_oracle(libs="B", trimmed=False, penalty_a=PENALTY_A):
    """libs: "B", or "AB" (A first, as the contexts add them)"""
    import oracle_py as op
    o = op.Oracle()
    o.set_graph(*graph()[1].packed())
    if libs == "AB":
        o.add_paired(*reads_a(), 0.01, op.paired_cfg(240.0, 24.0, penalty_constant=penalty_a))
    o.add_paired(*reads_b(trimmed), 0.01, op.paired_cfg(400.0, 40.0, penalty_constant=PENALTY_B))
    return o


@functools.lru_cache(maxsize=None)
def oracle_profile(name, libs="B", trimmed=False, penalty_a=PENALTY_A):
    """per length of the case's profile (value, floored counts, total_len, [bad_bases per read set]); computed once"""
    paths, path_id, gap_pos, lens = cases()[name]
    o = make_oracle(libs, trimmed, penalty_a)
    rows = []
    for l in lens:
        v, z, tl = o.calc_prob(with_length(paths, path_id, gap_pos, l), fresh=True)
        rows.append((v, z.tolist(), tl, [int(o.paired_probs(r)[1]) for r in range(o.num_sets())]))
    return rows


def make_ctx(libs="B", trimmed=False, penalty_a=PENALTY_A, device=0, flag=None, gap_fallback=False):
    from gaml_amd import api
    c = api.Context(device=device)
    c.set_graph(*graph()[1].packed())
    if libs == "AB":
        c.add_paired(api.paired_cfg(240.0, 24.0, penalty_constant=penalty_a), *reads_a())
    c.add_paired(api.paired_cfg(400.0, 40.0, penalty_constant=PENALTY_B), *reads_b(trimmed))
    if flag is not None:
        c.set_gap_penalty_device(flag)
    if gap_fallback:
        c.debug_set_knob(api.Knob.GAP_FALLBACK, 1)
    return c
