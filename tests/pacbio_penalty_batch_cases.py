"""Inputs of the tests of batches with PENALISED PacBio sets (tests/test_gpu_pacbio_penalty_batch.py) and of their host-side
check (tests/test_pacbio_penalty_cases_host.py).

Fixture P: graph, walk and paired reads of pacbio_batch_cases.FixtureA with a SPARSE PacBio set (60 reads of 2,000 bases) that
carries a coverage penalty: every candidate of the one-edit family then has bad bases, five distinct values among them, and
six of the unrelated sets have, all distinct (BAD_*: the CPU oracle's per set, FLOORED_*: the PacBio reads it floors). The
150-read set of FixtureA covers the assembly too well: most of its candidates have none.

Fixture C: the crafted records of tests/test_gpu_other_sets.py::test_pacbio_coverage_sweep_on_crafted_intervals (nested,
identical and touching intervals, records below GetMinReadProb) under 8 path sets of one chunk. COUNTS_C states how many
intervals each contig of each set brings to the sweep -- the fixed (-1000, 2000), one per node, one per counted record of every
occurrence of a cached sub-walk -- which is what decides between the block-per-contig kernel and the general chain."""
import math

import numpy as np

import pacbio_batch_cases as pc
from gaml_amd import synth

twin = pc.twin

# ---------------------------------------------------------------------------------------------------------------------
# fixture P
# ---------------------------------------------------------------------------------------------------------------------
N_PACBIO_P = 60
PACBIO_KW_P = dict(weight=0.5, min_prob_per_base=-1.1, penalty_constant=0.0001)
STEP_P = 400.0
PAIRED_PENALTY = dict(penalty_constant=0.001, penalty_step=20)  # the paired set's, where a test penalises both (tests/test_gpu_multi.py)
BAD_CANDIDATES = [625, 1123, 625, 1624, 625, 1234, 515, 625]
FLOORED_CANDIDATES = [6, 6, 8, 13, 6, 6, 15, 13]
BAD_UNRELATED = [1869, 1381, 0, 10718, 0, 1494, 2013, 1371, 0]
FLOORED_UNRELATED = [0, 0, 53, 60, 60, 53, 1, 25, 60]


def distinct_paths(sets):
    """the distinct paths of a family of path sets (the graphs here have no node that normalises to another)"""
    return sorted({tuple(p) for s in sets for p in s})


class FixtureP(pc.FixtureA):
    def __init__(self):
        super().__init__()
        self.pb = synth.make_pacbio_records(self.g, self.walk, N_PACBIO_P, 2000, 0.15, 55)

    def context(self, device=0, paired=True, paired_penalty=False, onepass=None):
        """(context, paired handle or None, PacBio handle); onepass: None leaves the switch as the context starts"""
        from gaml_amd import api
        c = api.Context(device=device)
        c.set_graph(*self.g.packed())
        prs = None
        if paired:
            prs = c.add_paired(api.paired_cfg(300.0, 30.0, weight=1.0, **(PAIRED_PENALTY if paired_penalty else {})), *self.paired_args)
        pacbio = c.add_pacbio(api.single_cfg(mismatch_prob=0.15, penalty_step=STEP_P, **PACBIO_KW_P), self.pb.lens)
        for wk, rec, lp in zip(self.pb.walks, self.pb.recs, self.pb.logps):
            c.put_pacbio_records(pacbio, wk, rec, lp)
        if onepass is not None:
            c.set_pacbio_penalty_onepass(onepass)
        return c, prs, pacbio

    def oracle(self, paired=True):
        """(oracle, its PacBio handle)"""
        import oracle_py as op
        o = op.Oracle()
        o.set_graph(*self.g.packed())
        if paired:
            o.add_paired(*self.paired_args, 0.01, op.paired_cfg(300.0, 30.0, weight=1.0))
        rs = o.add_pacbio(self.pb.lens, 0.15, op.single_cfg(step=STEP_P, **PACBIO_KW_P))
        for wk, rec, lp in zip(self.pb.walks, self.pb.recs, self.pb.logps):
            o.pacbio_put(rs, wk, rec, lp)
        return o, rs


# ---------------------------------------------------------------------------------------------------------------------
# fixture C
# ---------------------------------------------------------------------------------------------------------------------
G_C, SEED_C, N_READS_C, READ_LEN_C = 120_000, 97, 400, 1500
STEPS_C = (30.0, 0.5, 777.25)
CFG_C = dict(penalty_constant=0.002, min_prob_per_base=-1.2)
GOOD_LP, BAD_LP = -900.0, -5000.0  # GetMinReadProb of 1,500 bases at 15 % lies between them: the second kind is not counted
# intervals per contig, per path set of FixtureC.sets() in its order
COUNTS_C = [[641], [69, 564], [100, 502, 7], [60], [33, 56, 35, 38, 47, 39, 22, 14, 25, 43, 37, 42, 26, 38, 28], [75, 75, 75], [619], []]
LARGEST_C = 641  # the whole walk's
# the oracle's bad_bases per set at STEPS_C: int(begin + 0.5) never passes a position, so nothing is bad at 0.5
BAD_C = {30.0: [262, 262, 260, 1680, 252, 0, 292, 0], 0.5: [0] * 8, 777.25: [21683, 20941, 21144, 23808, 12061, 3312, 22798, 0]}


class FixtureC:
    def __init__(self):
        self.genome = synth.make_genome(G_C, SEED_C)
        self.g = synth.make_graph(self.genome, synth.cut_lengths(G_C, SEED_C, long_rng=(2500, 6000)))
        self.walk = synth.genome_walk(self.g)
        self.lens = np.full(N_READS_C, READ_LEN_C, np.int32)
        go = self.g.packed()[1]
        node_len = lambda x: int(go[x + 1] - go[x])
        rng = np.random.default_rng(5)
        rid = 0
        self.records = []  # (sub-walk, rec3, logp)
        for sub in synth.all_subwalks_for_pacbio(self.g, self.walk, READ_LEN_C):
            span = sum(node_len(x) for x in sub)
            recs, lps = [], []
            k = int(rng.integers(0, 5))
            anchors = rng.integers(0, max(1, span - 10), size=k)
            for a in anchors:
                a = int(a)
                e = int(min(span + 40, a + rng.integers(1, 1800)))
                for rep in range(int(rng.integers(1, 3))):  # identical copies
                    recs.append((a, e, rid % N_READS_C)); lps.append(GOOD_LP if rng.random() < 0.8 else BAD_LP); rid += 1
                if rng.random() < 0.5:  # one that starts exactly where this one ends, one nested inside
                    recs.append((e, e + int(rng.integers(1, 900)), rid % N_READS_C)); lps.append(GOOD_LP); rid += 1
                    if e - a > 4:
                        recs.append((a + 1, e - 1, rid % N_READS_C)); lps.append(GOOD_LP); rid += 1
            self.records.append((list(sub), np.array(recs, np.int32).reshape(-1, 3), np.array(lps, np.float64)))

    def sets(self):
        w = self.walk
        return [
            [w],                                               # the three path sets of the crafted-intervals test
            [w[:6], w[6:]],
            [w[:4] + [-700] + w[5:11], w[11:], w[2:3]],
            [twin(w)],                                         # the twin walk: no record lies under it
            [w[k:k + 4] for k in range(0, len(w), 4)],         # the walk cut at every fourth node
            [w[3:9]] * 3,                                      # one path listed three times
            [w[:7] + [-700] + w[8:]],                          # a contig with a 700-base gap (in place of a short node: covered at step 0.5)
            [],
        ]

    def context(self, step, onepass=None, cap=0, device=0):
        from gaml_amd import api
        c = api.Context(device=device)
        c.set_graph(*self.g.packed())
        rs = c.add_pacbio(api.single_cfg(mismatch_prob=0.15, penalty_step=step, **CFG_C), self.lens)
        for sub, rec, lp in self.records:
            c.put_pacbio_records(rs, sub, rec, lp)
        if onepass is not None:
            c.set_pacbio_penalty_onepass(onepass)
        if cap:
            c.debug_set_knob(api.Knob.PACBIO_SWEEP_CAP, cap)
        return c, rs

    def oracle(self, step):
        import oracle_py as op
        o = op.Oracle()
        o.set_graph(*self.g.packed())
        rs = o.add_pacbio(self.lens, 0.15, op.single_cfg(step=step, **CFG_C))
        for sub, rec, lp in self.records:
            o.pacbio_put(rs, sub, rec, lp)
        return o, rs

    def interval_count(self, path):
        """what `path` brings to the coverage sweep (graph.cc:3198-3222): the fixed interval, one per node, and of every
        occurrence of a cached sub-walk (the lookups of graph.cc:2438-2454) its records that clear GetMinReadProb"""
        min_lp = math.log(0.15) * (READ_LEN_C * 0.25) + math.log(1.0 - 4 * 0.15) * (READ_LEN_C * 0.75)
        assert BAD_LP < min_lp < GOOD_LP
        counted = {tuple(sub): int((lp >= min_lp).sum()) for sub, _, lp in self.records}
        n = 1 + sum(1 for x in path if x >= 0 and self.g.node_len(x) > 0)
        for sub in synth.all_subwalks_for_pacbio(self.g, list(path), READ_LEN_C):
            n += counted.get(tuple(sub), 0)
        return n
