"""Inputs of the paired + PacBio batch tests (tests/test_gpu_pacbio_batch.py) and of their host-side check
(tests/test_pacbio_batch_cases_host.py): BASELINE config 4 in small -- one paired set (weight 1) and one PacBio set
(weight 0.5) over the same graph -- with a family of candidates one edit away from one assembly and a family of unrelated
path sets. FLOORED_*: the PacBio reads the oracle floors per set (of N_PACBIO), which is how the families are known to hit
both branches of the floor, sub-walks that do not occur and sub-walks that occur several times."""
from gaml_amd import synth

G, SEED = 60_000, 55
N_PAIRS, N_PACBIO, PACBIO_LEN = 3000, 150, 2000
PACBIO_KW = dict(weight=0.5, min_prob_per_base=-1.1)
FLOORED_CANDIDATES = [20, 18, 26, 29, 20, 20, 47, 33]
FLOORED_UNRELATED = [0, 0, 128, 150, 150, 132, 3, 52, 150]


def twin(path):
    return [x ^ 1 if x >= 0 else x for x in reversed(path)]


class FixtureA:
    def __init__(self):
        self.genome = synth.make_genome(G, SEED)
        self.g = synth.make_graph(self.genome, synth.cut_lengths(G, SEED, long_rng=(900, 4000)))
        self.walk = synth.genome_walk(self.g)
        self.pr = synth.make_paired_reads(self.genome, N_PAIRS, 150, 300.0, 30.0, 0.01, SEED)
        self.pb = synth.make_pacbio_records(self.g, self.walk, N_PACBIO, PACBIO_LEN, 0.15, SEED)
        self.paired_args = (*synth.pack_reads(self.pr.mate1), *synth.pack_reads(self.pr.mate2))

    def base(self):
        """the walk cut into 6 paths: five of 7 nodes and the rest"""
        w = self.walk
        return [w[k:k + 7] for k in range(0, 35, 7)] + [w[35:]]

    def candidates(self):
        b, w = self.base(), self.walk
        return [
            b,                                                      # the assembly itself
            [b[0] + b[1]] + b[2:],                                  # two paths joined
            b[:2] + [b[2][:3], b[2][3:]] + b[3:],                   # one split
            b[:3] + [[x ^ 1 for x in reversed(b[3])]] + b[4:],      # one reversed
            b + [w[10:14]],                                         # a 4-node stretch as a second path: count 2
            b[:1] + [b[1] + [-120] + b[2]] + b[3:],                 # two joined through a gap
            b[:2] + b[3:],                                          # a path dropped
            b[:5] + [b[5][:-3]],                                    # a path shortened by 3 nodes
        ]

    def unrelated(self):
        w, k = self.walk, len(self.walk) // 2
        return [
            [w],
            [w[:k], w[k:]],
            [[x] for x in w[:20]],
            [twin(w)],
            [],
            [w[3:9]] * 3,
            [w[:8] + [-60] + w[9:]],
            [w[5:40]],
            [w[:1]],
        ]

    def context(self, pacbio_penalty=0.0, single=False, device=0):
        from gaml_amd import api
        c = api.Context(device=device)
        c.set_graph(*self.g.packed())
        paired = c.add_paired(api.paired_cfg(300.0, 30.0, weight=1.0), *self.paired_args)
        pacbio = c.add_pacbio(api.single_cfg(mismatch_prob=0.15, penalty_constant=pacbio_penalty, **PACBIO_KW), self.pb.lens)
        for wk, rec, lp in zip(self.pb.walks, self.pb.recs, self.pb.logps):
            c.put_pacbio_records(pacbio, wk, rec, lp)
        if single:
            sr = synth.make_single_reads(self.genome, 500, 100, 0.01, SEED + 1)
            c.add_single(api.single_cfg(weight=0.25), *synth.pack_reads(sr))
        return c, paired, pacbio

    def oracle(self):
        import oracle_py as op
        o = op.Oracle()
        o.set_graph(*self.g.packed())
        o.add_paired(*self.paired_args, 0.01, op.paired_cfg(300.0, 30.0, weight=1.0))
        rs = o.add_pacbio(self.pb.lens, 0.15, op.single_cfg(**PACBIO_KW))
        for wk, rec, lp in zip(self.pb.walks, self.pb.recs, self.pb.logps):
            o.pacbio_put(rs, wk, rec, lp)
        return o
