"""Read sets with a coverage penalty on the incremental, resident route (GPU).

A penalised set used to plan every call from scratch, send whole tables through the ring and score its compact class in
the general form. Now it plans incrementally, patches the resident copy of the tables (plus its coverage layout, written
whole per call) and marks coverage from the memo / streamed-value bodies of the scoring kernel (its COV instantiation).
Over an annealing-style walk of 121 path sets, for pairs of one length combination and for trimmed mates (several
combinations: the length-code tables):
  * four contexts -- default, PLAN_WHOLE_SET (every set planned from scratch), NO_RESIDENT_TABLES (whole tables through the
    ring), NO_COV_INSTANCE (the compact class in its general form, marking through the same slot layout) -- agree bit for bit, and the default one really takes the new route (incremental planning, static pairs, bytes written);
  * the default context agrees with the oracle at every step (bad_bases and floored counts exactly);
  * calls of other kinds in between -- stream-ordered (ring route), calc_partials, a table fold, a batch, a gap-length
    search -- leave the resident copy and the layout usable: a twin that only makes blocking calls gets the same results;
  * sets whose windows occur several times (the kernels' GEN instantiation) are scored like everything else."""
import functools

import numpy as np
import pytest

from gaml_amd import synth

pytestmark = pytest.mark.gpu

G, SEED, N_PAIRS, PENALTY = 150_000, 17, 2_500, 0.0002


def _pack(reads):
    offs = np.zeros(len(reads) + 1, np.int64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    return np.concatenate([np.asarray(r, np.uint8) for r in reads]), offs


@functools.lru_cache(maxsize=None)
def _case(trimmed):
    """graph, reads, the walk's path sets and the oracle's result for every one of them (computed once, never changed)"""
    import oracle_py as op
    genome = synth.plant_repeats(synth.make_genome(G, SEED), 3, 800, SEED)
    g = synth.make_graph(genome, synth.cut_lengths(G, SEED, long_rng=(600, 4000), short_rng=(25, 330)))
    pr = synth.make_paired_reads(genome, N_PAIRS, 100, 240.0, 24.0, 0.01, SEED)
    m1, m2 = list(pr.mate1), list(pr.mate2)
    if trimmed:
        rng = np.random.default_rng(3)
        for i in range(0, N_PAIRS, 3):
            m1[i] = m1[i][: int(rng.integers(70, 100))]
        for i in range(1, N_PAIRS, 5):
            m2[i] = m2[i][: int(rng.integers(80, 100))]
    reads = (*_pack(m1), *_pack(m2))
    start, seq = synth.sa_sequence(g, 120, seed=5, threshold=400)
    sets = [start] + seq
    orc = op.Oracle()
    orc.set_graph(*g.packed())
    ors = orc.add_paired(*reads, 0.01, op.paired_cfg(240.0, 24.0, penalty_constant=PENALTY))
    want = []
    for ps in sets:
        v, z, tl = orc.calc_prob(ps, fresh=True)
        probs, bad = orc.paired_probs(ors)
        want.append((v, z.tolist(), tl, int(bad), probs.copy()))
    return g, reads, sets, want


def _ctx(case, knob=None):
    """knob: the name of an api.Knob to set to 1"""
    from gaml_amd import api
    g, reads = case[0], case[1]
    c = api.Context(device=0)
    if knob is not None:
        c.debug_set_knob(api.Knob[knob], 1)
    c.set_graph(*g.packed())
    c.add_paired(api.paired_cfg(240.0, 24.0, penalty_constant=PENALTY), *reads)
    return c


def _call(c, ps):
    v, z, tl = c.calc_prob(ps)
    return v, z.tolist(), tl, c.bad_bases(0)


@pytest.mark.parametrize("trimmed", [False, True])
def test_oracle_inputs_exercise_the_penalty(trimmed):
    """what the walk is chosen for: uncovered bases on every set, several values of them, many floored reads"""
    want = _case(trimmed)[3]
    bads = [w[3] for w in want]
    assert len(want) == 121 and all(b > 0 for b in bads)
    assert len(set(bads)) == (12 if trimmed else 10)
    assert (min(bads), max(bads)) == ((4673, 6346) if trimmed else (5723, 7233))
    floored = [w[1][0][0] for w in want]
    assert (min(floored), max(floored)) == ((924, 951) if trimmed else (926, 952))


@pytest.mark.parametrize("trimmed", [False, True])
def test_three_routes_agree_bit_for_bit(trimmed):
    case = _case(trimmed)
    sets = case[2]
    dflt, scratch, ring, general = _ctx(case), _ctx(case, "PLAN_WHOLE_SET"), _ctx(case, "NO_RESIDENT_TABLES"), _ctx(case, "NO_COV_INSTANCE")
    incremental = 0
    bytes_dflt = bytes_ring = 0.0
    for k, ps in enumerate(sets):
        a, b, c = _call(dflt, ps), _call(scratch, ps), _call(ring, ps)
        print(k, a, dflt.last_phases()[6], ring.last_phases()[6])
        assert a == b, (k, a, b)
        assert a == c, (k, a, c)
        d = _call(general, ps)
        assert a == d, (k, a, d)
        if k % 25 == 0:
            pa = dflt.read_probs(0)
            assert np.array_equal(pa, scratch.read_probs(0)) and np.array_equal(pa, ring.read_probs(0)), k
            assert np.array_equal(pa, general.read_probs(0)), k
        inc = dflt.debug_table_occurrences(0)[1]["incremental"]
        assert not scratch.debug_table_occurrences(0)[1]["incremental"]
        incremental += inc
        if inc:
            bytes_dflt += dflt.last_phases()[6]
            bytes_ring += ring.last_phases()[6]
    print("incremental steps", incremental, "bytes written on them: default", bytes_dflt, "NO_RESIDENT_TABLES", bytes_ring)
    assert incremental > len(sets) // 2
    assert dflt.table_stats(0)["static_index_pairs"] > 0
    # a patch of the resident copy + the coverage layout against whole tables through the ring
    assert bytes_dflt < 0.5 * bytes_ring, (bytes_dflt, bytes_ring)


@pytest.mark.parametrize("trimmed", [False, True])
def test_default_route_against_the_oracle(trimmed):
    """tolerances of test_gpu_paired.py::_check"""
    case = _case(trimmed)
    sets, want = case[2], case[3]
    c = _ctx(case)
    seen = set()
    for k, (ps, w) in enumerate(zip(sets, want)):
        v, z, tl, bad = _call(c, ps)
        assert (z, tl, bad) == (w[1], w[2], w[3]), (k, z, tl, bad, w[1:4])
        np.testing.assert_allclose(c.read_probs(0), w[4], rtol=4e-16, atol=0)
        assert abs(v - w[0]) <= 1e-9 * abs(w[0]), (k, v, w[0])
        seen.add(bad)
    assert len(seen - {0}) >= 2


def _with_gap(sets):
    """a set of the walk with a gap in some path, a twin path added: (paths, path id, gap position)"""
    for ps in sets[40:]:
        for i, p in enumerate(ps):
            for q, x in enumerate(p):
                if x < 0 and 0 < q < len(p) - 1:
                    twin = [y ^ 1 for y in reversed(ps[(i + 1) % len(ps)]) if y >= 0]
                    return ps + [twin], i, q
    raise AssertionError("the walk has no set with a gap")


@pytest.mark.parametrize("trimmed", [False, True])
def test_route_transitions_and_repeats(trimmed):
    """Twin: blocking calls only (and the same table fold: it reorders the pairs, and with them the final sum). Counts,
    total_len and bad_bases are compared exactly, per-read probabilities exactly. The value is the twin's bit for bit as
    long as both contexts have made the same evaluations in the same order (up to the batch at step 60); from there on
    the device context has evaluated sets the twin has not and may rebuild its record tables at other calls, so the sum
    of 2,500 logs may be taken in another order: within 1e-12 relative -- at most 2,500 roundings of 2^-53 each, 2.8e-13."""
    import torch
    case = _case(trimmed)
    g, sets = case[0], case[2]
    dev, twin = _ctx(case), _ctx(case)
    part = torch.zeros(4, dtype=torch.float64, device="cuda")
    stream = torch.cuda.default_stream().cuda_stream

    diverged = False  # the two contexts' call sequences differ from the batch on

    def same(a, b, k):
        assert a[1:] == b[1:], (k, a, b)
        if diverged:
            assert abs(a[0] - b[0]) <= 1e-12 * abs(b[0]), (k, a, b)
        else:
            assert a[0] == b[0], (k, a, b)

    walk = synth.genome_walk(g)
    cut = len(walk) // 2
    repeats = [walk[:cut] + walk[cut - 3:cut] + walk[cut:]]  # a duplicated stretch: its windows occur twice (GEN instantiation)
    gap_set, gap_path, gap_pos = _with_gap(sets)
    for k, ps in enumerate(sets):
        want = _call(twin, ps)
        if k % 10 == 3:    # stream-ordered: whole tables and the layout through a ring slot, partials finished on the device
            tl = dev.calc_partials_async(ps, part.data_ptr(), stream)
            dev.sync()
            torch.cuda.synchronize()
            p = part.cpu().numpy()
            v, z = dev.combine_partials(p, tl)
            same((v, z.tolist(), tl, int(p[2])), want, k)
        elif k % 10 == 7:  # partials through the blocking entry point
            p, tl = dev.calc_partials(ps)
            v, z = dev.combine_partials(p, tl)
            same((v, z.tolist(), tl, int(p[0][2])), want, k)
        else:
            same(_call(dev, ps), want, k)
            if k % 20 == 0:
                assert np.array_equal(dev.read_probs(0), twin.read_probs(0)), k
        if k == 50:
            dev.compact_tables()
            twin.compact_tables()
        if k == 60:  # a batch (a penalised set: one call per set), then on with blocking calls
            diverged = True
            got = dev.calc_prob_batch([sets[58], sets[31], sets[59]])
            for s, r in zip((58, 31, 59), got):
                w = _call(twin, sets[s])
                same((r[0], r[1].tolist(), r[2], w[3]), w, k)
        if k == 70:  # a gap-length search (the penalty sends it to the fallback: sequential blocking calls)
            length, trace = dev.fix_gap_length(gap_set, gap_path, gap_pos)
            st = dev.gap_stats()
            assert st["device_lengths"] == 0 and st["fallback_lengths"] > 0
            fixed = [list(p) for p in gap_set]
            fixed[gap_path][gap_pos] = -length
            same(_call(dev, fixed), _call(twin, fixed), k)
            same(_call(dev, gap_set), _call(twin, gap_set), k)  # a gap and a twin path
        if k == 80:
            same(_call(dev, repeats), _call(twin, repeats), k)
    same(_call(dev, sets[-1]), _call(twin, sets[-1]), "end")
    assert dev.debug_table_occurrences(0)[1]["incremental_calls"] > len(sets) // 2


@pytest.mark.parametrize("trimmed", [False, True])
def test_repeated_windows_against_the_oracle(trimmed):
    import oracle_py as op
    case = _case(trimmed)
    g, reads, sets = case[0], case[1], case[2]
    orc = op.Oracle()
    orc.set_graph(*g.packed())
    ors = orc.add_paired(*reads, 0.01, op.paired_cfg(240.0, 24.0, penalty_constant=PENALTY))
    c = _ctx(case)
    walk = synth.genome_walk(g)
    cut = len(walk) // 2
    gap_set = _with_gap(sets)[0]
    for ps in (sets[0], [walk[:cut] + walk[cut - 3:cut] + walk[cut:]], sets[1], gap_set, sets[2]):
        v, z, tl, bad = _call(c, ps)
        wv, wz, wtl = orc.calc_prob(ps, fresh=True)
        wprobs, wbad = orc.paired_probs(ors)
        assert (z, tl, bad) == (wz.tolist(), wtl, int(wbad))
        assert wbad > 0
        np.testing.assert_allclose(c.read_probs(0), wprobs, rtol=4e-16, atol=0)
        assert abs(v - wv) <= 1e-9 * abs(wv)
