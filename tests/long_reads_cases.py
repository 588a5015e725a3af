"""Inputs shared by the long-read aligner tests (tests/test_long_reads_host.py, tests/test_gpu_aligner_long_reads.py)."""
from gaml_amd import synth


def long_read_case(L, n=3000):
    """The inputs of tests/test_gpu_aligner.py's record test at read length L: genome with two planted repeats, graph,
    paired reads (insert 2.2 L +- 0.2 L, 0.5 % errors) and the three path sets."""
    G, seed = 90_000, 81 + L
    genome = synth.plant_repeats(synth.make_genome(G, seed), 2, 900, seed)
    g = synth.make_graph(genome, synth.cut_lengths(G, seed, long_rng=(600, 5000), short_rng=(20, 340)))
    pr = synth.make_paired_reads(genome, n, L, 2.2 * L, 0.2 * L, 0.005, seed)
    walk = synth.genome_walk(g)
    k = len(walk) // 3
    sets = [[walk], [walk[:k], [x ^ 1 for x in reversed(walk[k:2 * k])], walk[2 * k:]], [[x] for x in walk]]
    return g, pr, sets
