"""Incremental planning of a read set WITH a coverage penalty, on the host (no GPU). The penalty's bitmap layout used to
force whole-set planning; now the table entries carry path slots and the layout maps a slot to its bit region. After
every step of an annealing-style walk
  * the occurrence tables equal those of a context that plans every set from scratch (PLAN_WHOLE_SET), and
  * the coverage layout of the call (debug_cov_layout) gives every path a region of its own that holds it, names the
    same region by slot and by position, and lists the contig starts the sweep needs."""
import numpy as np

from gaml_amd import synth


def _tables(ctx, rs, mate):
    tab, info = ctx.debug_table_occurrences(rs, mate)
    return tab[np.lexsort((tab[:, 0], tab[:, 4], tab[:, 3]))], info


def _contig_starts(g, path):
    """events of type 1 (graph.cc:1826,1833-1835): coordinate 0, and the coordinate behind every gap"""
    starts, cur = [0], 0
    for x in path:
        if x < 0:
            cur += -x
            starts.append(cur)
        else:
            cur += g.node_len(x)
    return starts, cur


def _check_layout(ctx, g, rs, paths):
    lay = ctx.debug_cov_layout(rs)
    n = len(paths)
    slots, slot_base, path_base, start_off, starts = lay["slots"], lay["slot_base"], lay["path_base"], lay["start_off"], lay["starts"]
    assert len(slots) == n and len(path_base) == n + 1 and len(start_off) == n + 1
    assert len(set(slots.tolist())) == n  # a slot names one path
    assert path_base[0] == 0 and start_off[0] == 0
    assert lay["total_bits"] == path_base[n] and len(starts) == start_off[n]
    want_starts = []
    for k, p in enumerate(paths):
        s, length = _contig_starts(g, p)
        want_starts += s
        bits = int(path_base[k + 1] - path_base[k])  # position order is monotone: regions are disjoint
        assert bits % 32 == 0 and path_base[k] % 32 == 0
        assert bits >= length + 64, (k, bits, length)
        assert slots[k] < len(slot_base) and slot_base[slots[k]] == path_base[k], k
        assert start_off[k + 1] - start_off[k] == len(s)
    assert starts.tolist() == want_starts


def test_penalised_set_plans_incrementally_with_a_slot_layout(built):
    from gaml_amd import api
    seed = 3
    G, n = 90_000, 2500
    genome = synth.plant_repeats(synth.make_genome(G, seed), 3, 700, seed)
    g = synth.make_graph(genome, synth.cut_lengths(G, seed, long_rng=(600, 3500), short_rng=(25, 330)))
    pr = synth.make_paired_reads(genome, n, 100, 240.0, 24.0, 0.01, seed)
    reads = (*synth.pack_reads(pr.mate1), *synth.pack_reads(pr.mate2))
    inc, ref = api.Context(device=-1), api.Context(device=-1)
    ref.debug_set_knob(api.Knob.PLAN_WHOLE_SET, 1)  # every set planned from scratch
    for c in (inc, ref):
        c.set_graph(*g.packed())
        c.add_paired(api.paired_cfg(240.0, 24.0, penalty_constant=0.0002), *reads)
    rs = 0
    start, seq = synth.sa_sequence(g, 260, seed=seed, threshold=400)
    rng = np.random.default_rng(seed)
    sets = [start]
    for k, s in enumerate(seq):
        sets.append(s)
        if rng.random() < 0.15:
            sets.append(sets[int(rng.integers(0, len(sets)))])  # jump back to an earlier set (a rejected move)
        if rng.random() < 0.05:
            sets.append([])  # an empty assembly
        if k % 40 == 7:
            sets.append([[-50] + s[0]] + s[1:])        # a leading gap
            sets.append(s[:2] + [[]] + s[2:])          # an empty path
            sets.append(s[:1] + [s[1] + [-9, -30]] + s[2:])  # two gaps in a row, the second one trailing
    used_incremental = 0
    for k, ps in enumerate(sets):
        inc.debug_prepare(ps)
        ref.debug_prepare(ps)
        for mate in (0, 1):
            a, info = _tables(inc, rs, mate)
            b, info_ref = _tables(ref, rs, mate)
            assert not info_ref["incremental"]
            assert np.array_equal(a, b), (k, mate)
        used_incremental += info["incremental"]
        _check_layout(inc, g, rs, ps)
        _check_layout(ref, g, rs, ps)
        if not info_ref["incremental"]:  # planned from scratch: slots are positions
            assert ref.debug_cov_layout(rs)["slots"].tolist() == list(range(len(ps)))
    assert used_incremental > len(sets) // 2  # the penalty no longer forces whole-set planning
