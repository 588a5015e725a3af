"""A context gives back what it took: eight contexts, one after the other, each with a single-end set, a paired set with a
coverage penalty and a PacBio set, each used through every route that allocates (blocking calls, a batch whose second path
set brings a junction the first did not have, a compaction, the single-end device routes in alternate cycles) and then
destroyed. The device's free memory after the eighth destroy is what it was after the second, up to the allocator's chunks
(DESIGN 4 has the measurements behind MARGIN)."""
import pytest

from gaml_amd import synth

pytestmark = pytest.mark.gpu

G, SEED = 16_000, 77
CYCLES = 8
MARGIN = 0  # bytes; see DESIGN 4


class Inputs:
    def __init__(self):
        self.genome = synth.make_genome(G, SEED)
        self.g = synth.make_graph(self.genome, synth.cut_lengths(G, SEED, long_rng=(600, 1500)))
        w = synth.genome_walk(self.g)
        k = len(w) // 2
        self.base = [w[:k], w[k:]]
        self.later = [w[:k - 1] + w[k + 2:]]  # joins two nodes no earlier path had side by side: new windows at the junction
        self.single = synth.pack_reads(synth.make_single_reads(self.genome, 400, 100, 0.01, SEED))
        pr = synth.make_paired_reads(self.genome, 400, 100, 300.0, 30.0, 0.01, SEED)
        self.paired = (*synth.pack_reads(pr.mate1), *synth.pack_reads(pr.mate2))
        self.pb = synth.make_pacbio_records(self.g, w, 60, 1500, 0.15, SEED)


def one_cycle(inp, cycle):
    from gaml_amd import api
    c = api.Context(device=0)
    try:
        c.set_graph(*inp.g.packed())
        c.add_single(api.single_cfg(weight=0.25), *inp.single)
        c.add_paired(api.paired_cfg(300.0, 30.0, penalty_constant=0.0002), *inp.paired)
        pb = c.add_pacbio(api.single_cfg(mismatch_prob=0.15, weight=0.5, min_prob_per_base=-1.1), inp.pb.lens)
        for wk, rec, lp in zip(inp.pb.walks, inp.pb.recs, inp.pb.logps):
            c.put_pacbio_records(pb, wk, rec, lp)
        c.set_single_device(cycle % 2 == 1)
        c.set_single_onepass(cycle % 2 == 1)
        first = c.calc_prob(inp.base)
        again = c.calc_prob(inp.base)
        assert again[0] == first[0]
        both = c.calc_prob_batch([inp.base, inp.later])
        assert both[0][0] == first[0]
        c.compact_tables()
        assert c.calc_prob(inp.later)[0] == both[1][0]
        return first[0]
    finally:
        c.close()


def test_eight_contexts_leave_the_device_memory_as_they_found_it():
    import torch
    inp = Inputs()
    free, values = [], []
    torch.cuda.mem_get_info(0)  # (the framework's own context comes with the first question)
    for cycle in range(CYCLES):
        values.append(one_cycle(inp, cycle))
        free.append(torch.cuda.mem_get_info(0)[0])
    print("free bytes after each destroy:", free)
    print("after the second minus after the eighth:", free[1] - free[-1], "margin", MARGIN)
    assert len(set(values)) == 1, values
    assert free[1] - free[-1] <= MARGIN, (free, MARGIN)
