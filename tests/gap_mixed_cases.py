"""Inputs of the mixed gap-profile tests (tests/test_gap_mixed_host.py, tests/test_gpu_gap_mixed.py): one graph of 40 kbp
with a paired set, a single-end set and a PacBio set over it, in the five layouts a context may hold them in, a walk cut
into three paths with one node replaced by a gap, and PacBio records filed under sub-walks that contain the gap entry with
one particular length (so that one column of a pass differs from its neighbours)."""
import numpy as np

import gap_oracle as go
from gaml_amd import synth

G, SEED = 40_000, go.SEED
N_PAIRS, N_SINGLE, N_PACBIO, PACBIO_LEN = 2000, 2000, 100, 1500
LAYOUTS = ("paired+pacbio", "paired+single", "pacbio", "single", "paired+single+pacbio")
PACBIO_KW = dict(weight=0.5, min_prob_per_base=-1.1)
SINGLE_KW = dict(weight=0.25)
CUTS = (14, 30)  # the walk as three paths: [:14], [14:30], [30:]


def nine_lengths(base):
    """test_gpu_gap.py's "nine lengths" ([100, 67, 1, 99, 101, 200, 33, 150, 68]) around another base length: the base first,
    shorter and longer ones mixed, a pass of eight and a pass of one"""
    out = [base, 2 * base // 3 + 1, 1, base - 1, base + 1, 2 * base, base // 3, base + 50, 2 * base // 3 + 2]
    assert len(set(out)) == 9 and min(out) >= 1, out
    return out


def model_enumerate(fx, ids, path, max_len):
    """GetPacbioAligments' lookups (graph.cc:2412-2454) for one path: hits (sub-walk id, begin) in order, and misses"""
    lens = np.array([fx.g.node_len(x) if x >= 0 else -x for x in path], np.int64)
    ends = np.cumsum(lens)
    begins = ends - lens
    hits, misses = [], 0
    for i in range(len(path)):
        for j in range(i, len(path)):
            k = ids.get(tuple(path[i:j + 1]))
            if k is None:
                misses += 1
            else:
                hits.append((k, int(begins[i])))
            if ends[j] - ends[i] > max_len:
                break
    return hits, misses


class Fixture:
    def __init__(self):
        self.genome = synth.make_genome(G, SEED)
        self.g = synth.make_graph(self.genome, synth.cut_lengths(G, SEED, long_rng=(900, 2500)))
        self.walk = synth.genome_walk(self.g)
        assert len(self.walk) > CUTS[1] + 8, len(self.walk)
        self.pr = synth.make_paired_reads(self.genome, N_PAIRS, 100, go.INSERT_MEAN, go.INSERT_STD, 0.01, SEED)
        self.sr = synth.make_single_reads(self.genome, N_SINGLE, 100, 0.01, SEED)  # as test_gpu_gap.py::test_routes makes them
        self.pb = synth.make_pacbio_records(self.g, self.walk, N_PACBIO, PACBIO_LEN, 0.15, SEED)
        self.paired_args = (*synth.pack_reads(self.pr.mate1), *synth.pack_reads(self.pr.mate2))
        self.single_args = synth.pack_reads(self.sr)

    def node_len(self, site):
        return self.g.node_len(self.walk[site])

    def three_paths(self, site, length=None, path_id=0):
        """the walk cut at CUTS, node `site` (a position of the walk, inside path `path_id`) replaced by a gap:
        (paths, path_id, gap_pos)"""
        w = list(self.walk)
        w[site] = -(self.node_len(site) if length is None else length)
        paths = [w[:CUTS[0]], w[CUTS[0]:CUTS[1]], w[CUTS[1]:]]
        start = (0,) + CUTS
        gap_pos = site - start[path_id]
        assert 0 <= gap_pos < len(paths[path_id]) and paths[path_id][gap_pos] < 0
        return paths, path_id, gap_pos

    def gap_records(self, site, length, reads=(3, 4, 5, 50)):
        """records under the sub-walk [node before the gap, -length, node behind it]: cached for that length alone"""
        sub = [self.walk[site - 1], -length, self.walk[site + 1]]
        rec = np.array([[10 + r, 10 + r + PACBIO_LEN, r] for r in reads], np.int32)
        lp = np.linspace(-1480.0, -1560.0, len(reads))
        return sub, rec, lp

    def walk_ids(self, records=()):
        """sub-walk -> id as a context numbers them: in the order they were first put"""
        ids = {}
        for wk in list(self.pb.walks) + [r[0] for r in records]:
            ids.setdefault(tuple(wk), len(ids))
        return ids

    def model_counts(self, paths, records=()):
        """(occurrences of every cached sub-walk in `paths`, lookups that found nothing)"""
        ids = self.walk_ids(records)
        counts, misses = np.zeros(len(ids), np.int32), 0
        for p in paths:
            hits, m = model_enumerate(self, ids, list(p), int(self.pb.lens.max()))
            misses += m
            for k, _ in hits:
                counts[k] += 1
        return counts, misses

    def context(self, layout, mixed=False, devices=None, device=0, pacbio_penalty=0.0, paired_penalty=0.0, gap_fallback=False, records=()):
        """(context, {kind: handle}); records: (sub-walk, rec3, logp) triples put behind the fixture's own"""
        from gaml_amd import api
        kinds = layout.split("+")
        c = api.Context(device=device) if devices is None else api.Context(devices=devices)
        c.set_graph(*self.g.packed())
        h = {}
        if "paired" in kinds:
            h["paired"] = c.add_paired(api.paired_cfg(go.INSERT_MEAN, go.INSERT_STD, penalty_constant=paired_penalty), *self.paired_args)
        if "single" in kinds:
            h["single"] = c.add_single(api.single_cfg(**SINGLE_KW), *self.single_args)
        if "pacbio" in kinds:
            h["pacbio"] = c.add_pacbio(api.single_cfg(mismatch_prob=0.15, penalty_constant=pacbio_penalty, **PACBIO_KW), self.pb.lens)
            for wk, rec, lp in list(zip(self.pb.walks, self.pb.recs, self.pb.logps)) + list(records):
                c.put_pacbio_records(h["pacbio"], wk, rec, lp)
        if gap_fallback:
            c.debug_set_knob(api.Knob.GAP_FALLBACK, 1)
        if mixed:
            c.set_gap_mixed_device(True)
        return c, h

    def oracle(self, layout, records=()):
        import oracle_py as op
        kinds = layout.split("+")
        o = op.Oracle()
        o.set_graph(*self.g.packed())
        if "single" in kinds:  # (the oracle scores in the reference's order whatever the order of creation; handles are not compared)
            o.add_single(*self.single_args, 0.01, op.single_cfg(**SINGLE_KW))
        if "paired" in kinds:
            o.add_paired(*self.paired_args, 0.01, op.paired_cfg(go.INSERT_MEAN, go.INSERT_STD))
        if "pacbio" in kinds:
            rs = o.add_pacbio(self.pb.lens, 0.15, op.single_cfg(**PACBIO_KW))
            for wk, rec, lp in list(zip(self.pb.walks, self.pb.recs, self.pb.logps)) + list(records):
                o.pacbio_put(rs, wk, rec, lp)
        return o
