"""Inputs shared by the aligner's hard-case tests (tests/test_aligner_hard_cases_host.py, tests/test_gpu_aligner_hard_cases.py):
tandem repeats and a two-letter stretch in and across nodes, reads with one inserted or deleted base, dense read piles
over the planted regions. Deterministic from the read length; numpy only."""
import numpy as np

from gaml_amd import synth

PERIODS = (1, 2, 3, 7, 16, 23, 61)
_ACGT = np.frombuffer(b"ACGT", np.uint8)
_CODE = np.zeros(256, np.int64)  # the seed code of a base (G 0, A 1, T 2, C 3; anything else 0: reference graph.h:326-331)
for _c, _v in zip(b"GATC", (0, 1, 2, 3)):
    _CODE[_c] = _v


def default_dense(L):
    """Extra pairs per planted region: 100 where reads are short (a 16-base read has a record at every copy of a short
    period, so the record counts explode: the GPU twin stays light), 1,500 at L = 100 (one junction window then holds more
    than 1,024 records of one mate, and a step of junction_moves more than 2,048 hits), 300 elsewhere."""
    return 100 if L <= 31 else 1500 if L == 100 else 300


def _unit(rng, period):
    """A random unit that is no repetition of a shorter one."""
    while True:
        u = _ACGT[rng.integers(0, 4, period)]
        if all(period % q or not (u == np.tile(u[:q], period // q)).all() for q in range(1, period)):
            return u


def _substitute(reads, err, rng):
    hit = rng.random(reads.shape) < err
    other = _ACGT[rng.integers(0, 4, reads.shape)]
    return np.where(hit & (other != reads), other, reads)


def _dense_pairs(genome, lo, hi, n, read_len, mean, sd, err, rng):
    """n innie pairs (synth.make_paired_reads' convention) whose fragments overlap genome[lo:hi]."""
    G = len(genome)
    flen = np.minimum(np.maximum(read_len + 10, np.rint(rng.normal(mean, sd, n))).astype(np.int64), G)
    start = lo - flen + 1 + (rng.random(n) * (hi - lo + flen - 1)).astype(np.int64)
    start = np.clip(start, 0, G - flen)
    ar = np.arange(read_len, dtype=np.int64)
    m1 = genome[start[:, None] + ar]
    m2 = synth.revcomp(genome[(start + flen - read_len)[:, None] + ar])
    return _substitute(m1, err, rng), _substitute(m2, err, rng)


def _indels(reads, L, frac, rng):
    """reads [n, L + 2] -> [n, L]: a share `frac` of the rows gets one inserted or one deleted base at a random
    position of the first L, then every row is cut to L. Returns the reads and the flags of the edited rows."""
    n = len(reads)
    flag = rng.random(n) < frac
    out = np.ascontiguousarray(reads[:, :L]).copy()
    for i in np.flatnonzero(flag):
        p = int(rng.integers(0, L))
        if rng.random() < 0.5:
            row = np.concatenate([reads[i, :p], _ACGT[rng.integers(0, 4, 1)], reads[i, p:]])
        else:
            row = np.concatenate([reads[i, :p], reads[i, p + 1:]])
        out[i] = row[:L]
    return out, flag


def hard_case(L, n_uniform=3000, n_dense=None):
    """(graph, packed reads (b1, o1, b2, o2), per-mate indel flags, planted regions [(start, end, period)], path sets).
    Genome of 30,000 bases; tandem repeats of the periods PERIODS (120 bases for period 1, else 400) alternately centred on
    a node boundary and inside a long node; 500 bases of random A / T across a node boundary (period 0 in `regions`).
    Reads of exactly L bases: n_uniform pairs all over the genome (insert 2.2 L +- 0.2 L, 1 % substitutions) and n_dense
    more per region with fragments overlapping it; 30 % of the mates carry one inserted or deleted base. Path sets: the
    genome walk, the walk cut in three with the middle third as its twin walk, one path per node."""
    G, seed = 30_000, 500 + L
    n_dense = default_dense(L) if n_dense is None else n_dense
    rng = np.random.default_rng(seed)
    genome = synth.make_genome(G, seed).copy()
    cuts = synth.cut_lengths(G, seed, long_rng=(600, 3000), short_rng=(20, 340))
    ends = np.cumsum(cuts)
    longs = [i for i in range(0, len(cuts) - 1, 2) if cuts[i] >= 900 and ends[i] - cuts[i] >= 300 and ends[i] + 300 <= G]
    assert len(longs) >= len(PERIODS) + 1, "too few long nodes for the planted regions"
    pick = [longs[(k * len(longs)) // (len(PERIODS) + 1)] for k in range(len(PERIODS) + 1)]  # distinct long nodes, spread out
    regions = []
    for k, period in enumerate(PERIODS):
        n = 120 if period == 1 else 400
        node = pick[k]
        centre = int(ends[node]) if k % 2 == 0 else int(ends[node] - cuts[node] // 2)  # its right boundary / its middle
        lo = centre - n // 2
        genome[lo:lo + n] = np.resize(_unit(rng, period), n)
        regions.append((lo, lo + n, period))
    lo = int(ends[pick[-1]]) - 250
    genome[lo:lo + 500] = np.frombuffer(b"AT", np.uint8)[rng.integers(0, 2, 500)]
    regions.append((lo, lo + 500, 0))
    g = synth.make_graph(genome, cuts)
    mean, sd = 2.2 * L, 0.2 * L
    pr = synth.make_paired_reads(genome, n_uniform, L + 2, mean, sd, 0.01, seed)
    m1, m2 = [pr.mate1], [pr.mate2]
    for lo, hi, _ in regions:
        a, b = _dense_pairs(genome, lo, hi, n_dense, L + 2, mean, sd, 0.01, rng)
        swap = (np.arange(len(a)) & 1).astype(bool)  # mates swapped on odd ids, as in the uniform part
        a[swap], b[swap] = b[swap].copy(), a[swap].copy()
        m1.append(a)
        m2.append(b)
    m1, f1 = _indels(np.concatenate(m1), L, 0.3, rng)
    m2, f2 = _indels(np.concatenate(m2), L, 0.3, rng)
    walk = synth.genome_walk(g)
    k = len(walk) // 3
    sets = [[walk], [walk[:k], [x ^ 1 for x in reversed(walk[k:2 * k])], walk[2 * k:]], [[x] for x in walk]]
    return g, (*synth.pack_reads(m1), *synth.pack_reads(m2)), (f1, f2), regions, sets


def junction_moves(g, regions):
    """Path sets for the small-batch routes: one path per node, then one more join per step -- the two paths on either side
    of a node boundary that lies in a planted region become one, so every step brings the junction windows (both
    orientations) that hold that repeat; where a region covers a whole short node the second join makes a three-node path."""
    walk = synth.genome_walk(g)
    ends = np.cumsum([g.node_len(x) for x in walk])
    steps, paths = [[[x] for x in walk]], [[x] for x in walk]
    for i in range(len(walk) - 1):
        if not any(lo < ends[i] < hi for lo, hi, _ in regions):
            continue
        k = next(k for k, p in enumerate(paths) if p[-1] == walk[i])
        paths = paths[:k] + [paths[k] + paths[k + 1]] + paths[k + 2:]
        steps.append(paths)
    return steps


def max_seed(read):
    """Index of the last base of the earliest 15-mer of `read` with the largest scrambled seed code (reference
    graph.cc:1245, 1289-1323) -- the seed the index files the read under."""
    c = _CODE[np.asarray(read, np.uint8)]
    codes = np.zeros(len(c) - 14, np.int64)
    for q in range(15):
        codes = codes * 4 + c[q:q + len(codes)]
    return int(np.argmax(codes ^ 0x2204abcd)) + 14


def n_collision_case(L=100):
    """(graph, packed reads, ids of the colliding reads in mate 1, the node with the N run, path sets). A run of 60 N in
    one node codes like G in the seed index, so a read with G in place of the N lands in the bucket of a window seed that
    is not literally in the read. The eight bases in front of the run (and, as a reverse complement, behind it) are those
    with the largest scrambled code, so a 15-mer of eight such bases and seven N is the index seed of every read that
    holds it. Pairs copied error-free from the flanks of the run, then pairs whose mate 1 copies the node across the left
    edge of the run (forward) or the right edge (reverse complement) with G at the N positions as stored."""
    G, seed = 4000, 77
    genome = synth.make_genome(G, seed).copy()
    run = (900, 960)
    genome[run[0]:run[1]] = ord("N")
    top = np.frombuffer(b"GATC", np.uint8)[[3 ^ ((0x2204abcd >> (2 * (14 - q))) & 3) for q in range(8)]]
    genome[run[0] - 8:run[0]] = top
    genome[run[1]:run[1] + 8] = synth.revcomp(top)
    g = synth.make_graph(genome, [1800, 200, 2000])
    pr = synth.make_paired_reads(genome, 600, L, 2.2 * L, 0.2 * L, 0.0, seed)
    clear = (pr.frag_start + pr.frag_len <= run[0]) | (pr.frag_start >= run[1])
    m1, m2 = [pr.mate1[clear]], [pr.mate2[clear]]
    n_flank = int(clear.sum())
    collide = []
    for strand in (0, 1):
        for inside in range(20, 56, 7):  # N positions the copy covers: far more than the three edits an extension accepts
            lo = run[1] - inside if strand else run[0] - (L - inside)
            r = synth.revcomp(genome[lo:lo + L]) if strand else genome[lo:lo + L].copy()
            at = np.flatnonzero(r == ord("N"))
            r[at] = ord("G")
            assert max_seed(r) == at.min() + 6  # eight flank bases + seven of the run: a seed the read does not hold literally
            mate = genome[lo + 3 * L:lo + 4 * L].copy() if strand else synth.revcomp(genome[lo + 2 * L:lo + 3 * L])
            collide.append(n_flank + len(collide))
            m1.append(r[None, :])
            m2.append(mate[None, :])
    m1, m2 = np.concatenate(m1), np.concatenate(m2)
    sets = [[[0], [2], [4]], [[0, 2, 4]], [[5, 3, 1]]]
    return g, (*synth.pack_reads(m1), *synth.pack_reads(m2)), collide, 0, sets
