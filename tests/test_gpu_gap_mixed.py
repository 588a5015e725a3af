"""gaml_hip_gap_profile and gaml_hip_fix_gap_length on the device route of contexts that hold single-end and / or PacBio
sets (Context.set_gap_mixed_device): a profile gives what the fallback's batches, single calls and the oracle give; a
single-end set's table of every length, derived on the device from the one the host built, equals the table a twin builds
for that length; a PacBio set's count columns equal a restatement of the reference's enumeration; searches follow the
reference's; nothing is left behind; contexts the route does not serve stay on the fallback. Inputs: tests/gap_mixed_cases.py."""
import numpy as np
import pytest

import gap_mixed_cases as gm
import gap_oracle as go
from gaml_amd import synth

pytestmark = pytest.mark.gpu

SITE = 5       # the walk position replaced by a gap: a node of 100 bases
CACHED = 67    # the length a gap-spanning PacBio sub-walk is cached for: the second of the nine lengths


@pytest.fixture(scope="module")
def fx():
    f = gm.Fixture()
    assert f.node_len(SITE) == 100
    return f


def _lens(fx):
    lens = gm.nine_lengths(fx.node_len(SITE))
    assert lens == [100, 67, 1, 99, 101, 200, 33, 150, 68] and lens[1] == CACHED  # "nine lengths" of test_gpu_gap.py
    return lens


def _records(fx, layout):
    return [fx.gap_records(SITE, CACHED)] if "pacbio" in layout else []


def _launches(c, h):
    return tuple(c.pacbio_stats(h[k])["multi_launches"] if k == "pacbio" else c.single_stats(h[k])["multi_launches"] for k in ("single", "pacbio") if k in h)


def _warm(ctxs, sets, base):
    """every window of `sets` aligned and folded into the record tables: the same device state on every context"""
    for c in ctxs:
        for s in sets:
            c.calc_prob(s)
        c.compact_tables()
        c.calc_prob(base)


def _same(got, want, rel):
    bit_equal = 0
    for k, (a, b) in enumerate(zip(got, want)):
        assert a[2] == b[2], (k, a[2], b[2])
        assert a[1].tolist() == b[1].tolist(), (k, a[1].tolist(), b[1].tolist())
        assert abs(a[0] - b[0]) <= rel * abs(b[0]), (k, a[0], b[0])
        bit_equal += a[0] == b[0]
    assert len(got) == len(want)
    return bit_equal


@pytest.fixture(scope="module")
def oracle_values(fx):
    """the oracle's (value, zeros, total length) of the nine sets per layout, computed once"""
    paths, path_id, gap_pos = fx.three_paths(SITE)
    out = {}
    for layout in gm.LAYOUTS:
        o = fx.oracle(layout, _records(fx, layout))
        out[layout] = [o.calc_prob(go.with_length(paths, path_id, gap_pos, l), fresh=True) for l in _lens(fx)]
    return out


@pytest.mark.parametrize("layout", gm.LAYOUTS)
def test_profile_on_every_layout(fx, oracle_values, layout):
    """1. Nine lengths, switch on: two device passes, no fallback; the values are the bits of calc_prob_batch on a twin with
    the switch off (both contexts warm: every window folded into the record tables, as the bit-for-bit batch tests do),
    within 1e-13 of single calls and 1e-9 of the oracle; with the switch off the same layout reports the fallback."""
    lens, rec = _lens(fx), _records(fx, layout)
    paths, path_id, gap_pos = fx.three_paths(SITE)
    sets = [go.with_length(paths, path_id, gap_pos, l) for l in lens]
    (dev, h), (off, _), (one, _), (fb, hf) = (fx.context(layout, mixed=True, records=rec), fx.context(layout, records=rec),
                                              fx.context(layout, records=rec), fx.context(layout, records=rec))
    assert dev.gap_mixed_device() and not off.gap_mixed_device()
    _warm([dev, off, one, fb], sets, paths)
    before = _launches(dev, h)
    got = dev.gap_profile(paths, path_id, gap_pos, lens)
    assert dev.gap_stats() == {"calls": 1, "device_lengths": 9, "fallback_lengths": 0, "device_passes": 2}
    assert [a - b for a, b in zip(_launches(dev, h), before)] == [2] * len(before), (before, _launches(dev, h))
    batch = off.calc_prob_batch(sets)
    for k, (a, b) in enumerate(zip(got, batch)):
        print(layout, lens[k], repr(a[0]), repr(b[0]), a[1].tolist(), a[2])
    assert _same(got, batch, 0.0) == 9
    _same(got, [one.calc_prob(s) for s in sets], 1e-13)
    _same(got, oracle_values[layout], 1e-9)
    # the switch off: the fallback, same bits
    want = fb.gap_profile(paths, path_id, gap_pos, lens)
    st = fb.gap_stats()
    assert st["device_lengths"] == 0 and st["device_passes"] == 0 and st["fallback_lengths"] == 9, st
    assert _same(got, want, 0.0) == 9
    if "pacbio" in layout:  # the cached gap-spanning sub-walk counts at its length alone
        plain = fx.context(layout, mixed=True)[0]
        _warm([plain], sets, paths)
        differs = [a[0] != b[0] for a, b in zip(got, plain.gap_profile(paths, path_id, gap_pos, lens))]
        assert differs == [l == CACHED for l in lens], differs


def _single_cases(fx):
    w = fx.walk
    first = fx.three_paths(SITE)
    last = fx.three_paths(35, path_id=2)
    again = ([w[:8] + [-60] + w[4:8] + w[9:14], w[14:30], w[30:]], 0, 8)  # nodes 4..7 on both sides of the gap: list entries of one path
    two = ([w[:3] + [-fx.node_len(3)] + w[4:9] + [-fx.node_len(9)] + w[10:14], w[14:30], w[30:]], 0, 9)
    return {"gap in the first path": first, "gap in the last path": last, "windows on both sides": again, "two gaps": two}


@pytest.mark.parametrize("layout", ["single", "paired+single"])
@pytest.mark.parametrize("name", ["gap in the first path", "gap in the last path", "windows on both sides", "two gaps"])
def test_derived_single_end_tables(fx, layout, name):
    """2. Region g of a pass of 8 and of a pass of 1 equals, entry for entry, the occurrences a twin lists for that length;
    a pass holds delta 0, negative and positive deltas."""
    paths, path_id, gap_pos = _single_cases(fx)[name]
    base = -paths[path_id][gap_pos]
    lens = gm.nine_lengths(base)
    assert lens[0] == base and min(lens[:8]) < base < max(lens[:8])
    (dev, h), (twin, ht) = fx.context(layout, mixed=True), fx.context(layout)
    twin.calc_prob(paths)
    want = {}
    for l in lens:
        twin.calc_prob(go.with_length(paths, path_id, gap_pos, l))
        want[l] = twin.debug_occurrences(ht["single"]).copy()
    wids = want[base][:, 0].tolist()
    if name == "windows on both sides":
        assert len(wids) > len(set(wids))
    if name == "gap in the first path":
        assert (want[base][:, 1] != want[base + 1][:, 1]).sum() > len(paths[0]) // 2  # the later paths' entries move too
    for batch in (lens[:8], lens):
        dev.gap_profile(paths, path_id, gap_pos, batch)
        in_pass = batch[8 * ((len(batch) - 1) // 8):]
        for g, l in enumerate(in_pass):
            got = dev.debug_gap_single_table(h["single"], g)
            assert np.array_equal(got, want[l]), (name, g, l)
        from gaml_amd import api
        with pytest.raises(api.GamlHipError):
            dev.debug_gap_single_table(h["single"], len(in_pass))
        # what a call with the last length leaves: the occurrence list, the staged bytes of ONE table
        assert np.array_equal(dev.debug_occurrences(h["single"]), want[batch[-1]])
        assert dev.single_stats(h["single"])["table_bytes"] == twin.single_stats(ht["single"])["table_bytes"]
    assert dev.gap_stats()["fallback_lengths"] == 0 and dev.gap_stats()["device_passes"] == 3


@pytest.mark.parametrize("layout", ["pacbio", "paired+pacbio"])
def test_pacbio_count_columns(fx, layout):
    """3. Column g of a pass equals the enumeration of the path set with that length; the cached gap-spanning sub-walk shows
    up in exactly one column; a pass of 3 leaves columns 3..7 at zero; misses count every length scored."""
    rec = _records(fx, layout)
    paths, path_id, gap_pos = fx.three_paths(SITE)
    lens = _lens(fx)[:8]
    dev, h = fx.context(layout, mixed=True, records=rec)
    rs = h["pacbio"]
    gap_id = fx.walk_ids(rec)[tuple(rec[0][0])]
    m0 = dev.pacbio_stats(rs)["misses"]
    dev.gap_profile(paths, path_id, gap_pos, lens)
    want_misses, in_column = 0, []
    for g, l in enumerate(lens):
        want, miss = fx.model_counts(go.with_length(paths, path_id, gap_pos, l), rec)
        got = dev.debug_gap_pacbio_counts(rs, g)
        assert np.array_equal(got, want), (g, l, np.flatnonzero(got != want))
        want_misses += miss
        in_column.append(int(got[gap_id]))
    assert in_column == [1 if l == CACHED else 0 for l in lens], in_column
    assert dev.pacbio_stats(rs)["misses"] - m0 == want_misses
    dev.gap_profile(paths, path_id, gap_pos, [150, CACHED, 3])
    cols = [dev.debug_gap_pacbio_counts(rs, g) for g in range(8)]
    assert [int(c[gap_id]) for c in cols] == [0, 1, 0, 0, 0, 0, 0, 0]
    assert cols[0].sum() > 0 and all(not c.any() for c in cols[3:])
    assert dev.bad_bases(rs) == 0


@pytest.mark.parametrize("layout", gm.LAYOUTS)
def test_search_follows_the_reference(fx, layout):
    """4. fix_gap_length, cold and then warm: length and trace are those of the reference's search driven by a twin's blocking
    calls (tests/gap_oracle.py), on the device route alone."""
    rec = _records(fx, layout)
    paths, path_id, gap_pos = fx.three_paths(SITE)
    cur = -paths[path_id][gap_pos]
    (dev, h), (twin, _) = fx.context(layout, mixed=True, records=rec), fx.context(layout, records=rec)
    for rnd in ("cold", "warm"):
        before = dev.gap_stats()
        length, trace = dev.fix_gap_length(paths, path_id, gap_pos)
        want = go.Search(lambda l: twin.calc_prob(go.with_length(paths, path_id, gap_pos, l))[0], cur)
        st = dev.gap_stats()
        print(layout, rnd, "length", length, "evaluations", len(trace), "passes", st["device_passes"] - before["device_passes"],
              "lengths", st["device_lengths"] - before["device_lengths"])
        assert length == want.length and [l for l, _ in trace] == [l for l, _ in want.trace]
        for (l, v), (_, wv) in zip(trace, want.trace):
            print(l, repr(v), repr(wv))
        if rnd == "warm":
            assert [v for _, v in trace] == [v for _, v in want.trace]
        else:
            assert all(abs(v - wv) <= 1e-13 * abs(wv) for (_, v), (_, wv) in zip(trace, want.trace))
        assert st["fallback_lengths"] == 0 and st["device_passes"] - before["device_passes"] < len(set(l for l, _ in trace)), st
        for c in (dev, twin):
            c.compact_tables()
            c.calc_prob(paths)


def test_nothing_is_left_behind(fx):
    """5. After a mixed device profile the next calls -- single, batched, the per-read values of every set -- are a twin's that
    ran the same profile on the fallback; a record put afterwards (the set's generation moves) is in the next profile."""
    layout = "paired+single+pacbio"
    rec = _records(fx, layout)
    paths, path_id, gap_pos = fx.three_paths(SITE)
    lens = _lens(fx)
    sets = [go.with_length(paths, path_id, gap_pos, l) for l in lens]
    (dev, h), (twin, ht) = fx.context(layout, mixed=True, records=rec), fx.context(layout, records=rec)
    _warm([dev, twin], sets, paths)
    got, want = dev.gap_profile(paths, path_id, gap_pos, lens), twin.gap_profile(paths, path_id, gap_pos, lens)
    assert dev.gap_stats()["fallback_lengths"] == 0 and twin.gap_stats()["device_lengths"] == 0
    assert _same(got, want, 0.0) == 9
    for k in h:  # the per-read values of the last length
        assert np.array_equal(dev.read_probs(h[k]), twin.read_probs(ht[k])), k
    w = fx.walk
    other = [w[10:20], [x ^ 1 for x in reversed(w[22:30])], w[30:]]
    edited = go.with_length(paths, path_id, gap_pos, 77)
    _same([dev.calc_prob(s) for s in (other, edited, paths)], [twin.calc_prob(s) for s in (other, edited, paths)], 1e-13)
    _same(dev.calc_prob_batch([other, edited, paths, sets[3]]), twin.calc_prob_batch([other, edited, paths, sets[3]]), 1e-13)
    for k in h:
        assert np.array_equal(dev.read_probs(h[k]), twin.read_probs(ht[k])), k
        if k != "pacbio":
            assert dev.window_count(h[k], 0) == twin.window_count(ht[k], 0)
    # a new record under another gap-spanning sub-walk: the next profile counts it
    new = fx.gap_records(SITE, 150, reads=(7, 8))
    for c, hh in ((dev, h), (twin, ht)):
        c.put_pacbio_records(hh["pacbio"], *new)
    got2, want2 = dev.gap_profile(paths, path_id, gap_pos, lens), twin.gap_profile(paths, path_id, gap_pos, lens)
    _same(got2, want2, 1e-13)
    moved = [abs(a[0] - b[0]) > 1e-12 * abs(b[0]) for a, b in zip(got2, got)]  # (the calls in between added windows: the paired sums may differ in their last bits)
    assert moved == [l == 150 for l in lens], moved
    gap_id = fx.walk_ids(rec + [new])[tuple(new[0])]
    assert int(dev.debug_gap_pacbio_counts(h["pacbio"], 0)[gap_id]) == 0  # (the last pass: length 68)
    dev.gap_profile(paths, path_id, gap_pos, [150])
    assert int(dev.debug_gap_pacbio_counts(h["pacbio"], 0)[gap_id]) == 1


@pytest.mark.parametrize("kind", ["pacbio penalty", "two devices", "GAP_FALLBACK", "paired penalty"])
def test_contexts_that_stay_on_the_fallback(fx, kind):
    """6. With the switch on these still report the fallback, and give the values of the same context with the switch off."""
    layout = "paired+single+pacbio"
    rec = _records(fx, layout)
    kw = {"pacbio penalty": dict(pacbio_penalty=0.0001), "two devices": dict(devices=[0, 0]), "GAP_FALLBACK": dict(gap_fallback=True),
          "paired penalty": dict(paired_penalty=0.0005)}[kind]
    paths, path_id, gap_pos = fx.three_paths(SITE)
    lens = _lens(fx)
    (on, _), (off, _) = fx.context(layout, mixed=True, records=rec, **kw), fx.context(layout, records=rec, **kw)
    assert on.gap_mixed_device() or kind == "two devices"
    if kind == "pacbio penalty":
        on.set_pacbio_penalty_onepass(True)  # (whatever that switch says)
    got, want = on.gap_profile(paths, path_id, gap_pos, lens), off.gap_profile(paths, path_id, gap_pos, lens)
    st = on.gap_stats()
    assert st["device_lengths"] == 0 and st["device_passes"] == 0 and st["fallback_lengths"] == 9, st
    _same(got, want, 1e-13)
    if kind in ("two devices", "GAP_FALLBACK"):  # the same values as the device route's
        _same(fx.context(layout, mixed=True, records=rec)[0].gap_profile(paths, path_id, gap_pos, lens), got, 1e-13)
    length, trace = on.fix_gap_length(paths, path_id, gap_pos)
    assert on.gap_stats()["device_lengths"] == 0
    if kind == "paired penalty":  # ... and with the other switch the paired set goes along
        on.set_gap_penalty_device(True)
        _same(on.gap_profile(paths, path_id, gap_pos, lens), want, 1e-13)
        assert on.gap_stats()["device_lengths"] == 9


@pytest.mark.parametrize("cap", [1, 3])
def test_single_end_layout_under_a_capped_grid(fx, cap):
    """7a. single_score_multi_kernel under the development build's grid cap: the bits of the fallback under the same cap (its
    single calls run single_score_kernel over the same grid), within 1e-13 of the uncapped values."""
    from gaml_amd import api
    paths, path_id, gap_pos = fx.three_paths(SITE)
    lens = _lens(fx)
    (dev, h), (twin, _), (free, _) = fx.context("single", mixed=True), fx.context("single"), fx.context("single", mixed=True)
    for c in (dev, twin):
        c.debug_set_knob(api.Knob.GRID_CAP_SETS, cap)
    got, want = dev.gap_profile(paths, path_id, gap_pos, lens), twin.gap_profile(paths, path_id, gap_pos, lens)
    assert dev.gap_stats()["device_passes"] == 2 and twin.gap_stats()["device_passes"] == 0
    assert _same(got, want, 0.0) == 9
    _same(got, free.gap_profile(paths, path_id, gap_pos, lens), 1e-13)


def _tiny_paths(fx, n_windows):
    w = fx.walk
    if n_windows == 1:
        return [[-30] + w[:2]], 0, 0  # a leading gap: every occurrence lies behind it
    return [w[:1] + [-fx.node_len(1)] + w[2:2 * n_windows]], 0, 1


@pytest.mark.parametrize("n_windows", [1, 15, 16, 17])
def test_tables_kernel_on_small_tables(fx, n_windows):
    """7b. gap_single_tables_kernel over tables of 1, 15, 16 and 17 windows (a fresh context holds the windows of the one path
    set it has seen): the smallest shapes at which a tail or a stride can go wrong."""
    paths, path_id, gap_pos = _tiny_paths(fx, n_windows)
    base = -paths[path_id][gap_pos]
    lens = [base, base + 9, max(1, base - 7), base + 1000, 1 if base > 8 else 2]
    (dev, h), (twin, ht) = fx.context("single", mixed=True), fx.context("single")
    got = dev.gap_profile(paths, path_id, gap_pos, lens)
    assert dev.single_stats(h["single"])["windows"] == n_windows and dev.gap_stats()["device_passes"] == 1
    for g, l in enumerate(lens):
        want = twin.calc_prob(go.with_length(paths, path_id, gap_pos, l))
        assert got[g][0] == want[0] and got[g][1].tolist() == want[1].tolist() and got[g][2] == want[2], (g, l)
        assert np.array_equal(dev.debug_gap_single_table(h["single"], g), twin.debug_occurrences(ht["single"])), (g, l)


def test_tables_kernel_on_a_few_thousand_windows():
    """7c. ... and over a table of a few thousand windows: several blocks per region, each with a stride of its own."""
    from gaml_amd import api
    G = 400_000
    genome = synth.make_genome(G, 7)
    g = synth.make_graph(genome, synth.cut_lengths(G, 7, long_rng=(101, 140), short_rng=(40, 60)))
    w = synth.genome_walk(g)
    sr = synth.pack_reads(synth.make_single_reads(genome, 2000, 100, 0.01, 7))
    base = g.node_len(w[101])
    paths = [w[:101] + [-base] + w[102:2000], w[2000:]]
    ctxs = []
    for mixed in (True, False):
        c = api.Context(device=0)
        c.set_graph(*g.packed())
        rs = c.add_single(api.single_cfg(), *sr)
        c.set_gap_mixed_device(mixed)
        ctxs.append(c)
    dev, twin = ctxs
    lens = [base, base + 11, 1, base + 5000]
    got = dev.gap_profile(paths, 0, 101, lens)
    assert dev.single_stats(rs)["windows"] > 3000 and dev.gap_stats() == {"calls": 1, "device_lengths": 4, "fallback_lengths": 0, "device_passes": 1}
    for k, l in enumerate(lens):
        want = twin.calc_prob(go.with_length(paths, 0, 101, l))
        assert got[k][0] == want[0] and got[k][1].tolist() == want[1].tolist() and got[k][2] == want[2], (k, l)
        occ = twin.debug_occurrences(rs)
        assert len(occ) > 2500
        assert np.array_equal(dev.debug_gap_single_table(rs, k), occ), (k, l)
