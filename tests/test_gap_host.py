"""The gap-length search without a GPU: the restatement of FixGapLength (tests/gap_oracle.py) over the oracle on the
checked inputs, the argument checks of gaml_hip_gap_profile / gaml_hip_fix_gap_length on a host-only context, the
exported symbols, and the documented moves.cc patch against the text the gap driver compiles."""
import ctypes as C
import os

import numpy as np
import pytest

import gap_oracle as go

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (site, start) -> (length left in the entry, evaluations, state): verified over the oracle, see test below
PINS = {
    (5, 1): (67, 33, 1), (5, 7): (67, 29, 1), (5, 100): (67, 25, 2), (5, 311): (67, 31, 2), (5, 900): (67, 35, 2),
    (7, 1): (75, 29, 1), (7, 7): (75, 29, 1), (7, 111): (75, 25, 2), (7, 344): (75, 31, 2), (7, 900): (75, 35, 2),
    (9, 1): (57, 31, 1), (9, 7): (57, 29, 1), (9, 58): (57, 3, 0), (9, 185): (57, 27, 2), (9, 900): (57, 35, 2),
}


@pytest.fixture(scope="module")
def inputs(built):
    return go.make_inputs()


def test_search_over_the_oracle_has_no_close_comparison(inputs):
    """Every comparison the search makes on the checked inputs (first probes, doubling bound, ternary steps) is between
    values at least 1e-10 apart, relative -- two orders above what the GPU agrees with the oracle to -- so the GPU must
    follow the same trajectory in every case. (The two evaluations of a span-2 interval are the same path set twice,
    moves.cc:704-706: equal by construction, and both outcomes keep the lower end.) Ends, evaluation counts and states
    are pinned: 25-35 evaluations per search, 3 where the start is already a local optimum."""
    g, pr, walk = inputs
    assert [g.node_len(walk[i]) for i in go.GAP_SITES] == [100, 111, 58]
    o = go.make_oracle(g, pr)
    seen = {}
    for i in go.GAP_SITES:
        for start in go.start_lengths(g.node_len(walk[i])):
            s = go.oracle_search(o, go.gap_set(walk, i, start), 0, i)
            print(f"site {i} start {start}: -> {s.length}, state {s.state}, {len(s.trace)} evaluations, closest comparison {s.closest:.3g}")
            assert s.closest >= 1e-10, (i, start, s.closest)
            seen[(i, start)] = (s.length, len(s.trace), s.state)
    assert seen == PINS
    # the quirk: a start that is a local optimum keeps the LAST probed length, cur - 1, not cur
    assert PINS[(9, 58)] == (57, 3, 0)


def test_restatement_quirks():
    """The decisions of moves.cc:694-800 on hand-made likelihood curves."""
    peak = lambda top: (lambda l: -abs(l - top) - 1000.0)
    # neither direction wins: the entry keeps the last probe, cur - 1, or cur + 1 when cur is 1
    s = go.Search(peak(40), 40)
    assert (s.length, s.state, [l for l, _ in s.trace]) == (39, 0, [40, 41, 39])
    s = go.Search(peak(1), 1)
    assert (s.length, s.state, [l for l, _ in s.trace]) == (2, 0, [1, 2])
    # flat: all comparisons are strict
    s = go.Search(lambda l: -5.0, 9)
    assert (s.length, s.state) == (8, 0)
    # up: the bound doubles while the value does not drop (more than once here), then the ternary search on [cur + 1, bound]
    s = go.Search(peak(100), 10)
    assert s.state == 1 and [l for l, _ in s.trace][:7] == [10, 11, 9, 20, 40, 80, 160]
    assert 98 <= s.length <= 100  # the search ends on an interval of span <= 2 around the peak and keeps its LOWER end
    # a span of 2 evaluates its lower end twice and keeps it
    s = go.Search(peak(1), 3)
    assert s.state == 2 and [l for l, _ in s.trace] == [3, 4, 2, 1, 1] and s.length == 1
    # p(mid1) >= p(mid2) keeps the lower part
    s = go.Search(lambda l: -5.0 if l <= 30 else -6.0 - l, 31)
    assert s.state == 2 and s.length == 1


def _host_ctx(g, pr):
    from gaml_amd import api, synth
    c = api.Context(device=-1)
    c.set_graph(*g.packed())
    c.add_paired(api.paired_cfg(go.INSERT_MEAN, go.INSERT_STD), *synth.pack_reads(pr.mate1), *synth.pack_reads(pr.mate2))
    return c


def test_host_only_context_refuses(built):
    from gaml_amd import api, synth
    genome = synth.make_genome(20_000, 5)
    g = synth.make_graph(genome, synth.cut_lengths(20_000, 5))
    pr = synth.make_paired_reads(genome, 200, 100, 600.0, 40.0, 0.01, 5)
    walk = synth.genome_walk(g)
    c = _host_ctx(g, pr)
    paths = [walk[:3] + [-20] + walk[4:], walk[1:3]]

    def code(fn, *a):
        with pytest.raises(api.GamlHipError) as e:
            fn(*a)
        return e.value.code

    assert code(c.gap_profile, paths, 0, 3, [20, 21]) == api.ENODEVICE
    assert code(c.fix_gap_length, paths, 0, 3) == api.ENODEVICE
    for fn, tail in ((c.gap_profile, ([20],)), (c.fix_gap_length, ())):
        assert code(fn, paths, 2, 3, *tail) == api.EINVAL    # path_id out of range
        assert code(fn, paths, -1, 3, *tail) == api.EINVAL
        assert code(fn, paths, 0, len(paths[0]), *tail) == api.EINVAL  # gap_pos out of range
        assert code(fn, paths, 0, -1, *tail) == api.EINVAL
        assert code(fn, paths, 0, 2, *tail) == api.EINVAL    # not a gap
        assert code(fn, paths, 1, 3, *tail) == api.EINVAL    # gap_pos beyond the shorter path
    assert code(c.gap_profile, paths, 0, 3, [20, 0]) == api.EINVAL  # a length < 1
    assert code(c.gap_profile, paths, 0, 3, [2**31 - 1]) == api.EINVAL  # total length beyond int32
    huge = [walk[:3] + [-(2**31 - 1)] + walk[4:]]
    assert code(c.fix_gap_length, huge, 0, 3) == api.EINVAL
    # n_lens < 0 / == 0 through the raw ABI
    flat, offs = api._flat(paths)
    L = api.lib()
    probs = np.zeros(1)
    one = np.array([20], np.int32)
    assert L.gaml_hip_gap_profile(c._h, flat, offs, 2, 0, 3, one.ctypes.data, -1, probs.ctypes.data, None, None) == api.EINVAL
    assert L.gaml_hip_gap_profile(c._h, flat, offs, 2, 0, 3, None, 0, None, None, None) == api.OK
    assert c.gap_profile(paths, 0, 3, []) == []
    st = c.gap_stats()
    assert st["device_lengths"] == 0 and st["fallback_lengths"] == 0 and st["device_passes"] == 0


def test_symbols_are_exported(built):
    for name in ("libgaml_hip.so", "libgaml_hip_dev.so"):
        L = C.CDLL(os.path.join(ROOT, "gaml_amd", name))
        for sym in ("gaml_hip_gap_profile", "gaml_hip_fix_gap_length", "gaml_hip_gap_stats"):
            assert hasattr(L, sym), (name, sym)
    hdr = open(os.path.join(ROOT, "include", "gaml_hip.h")).read()
    assert "int gaml_hip_gap_profile(" in hdr and "int gaml_hip_fix_gap_length(" in hdr and "int gaml_hip_gap_stats(" in hdr


def _strip(lines):
    return [ln.strip() for ln in lines if ln.strip()]


def test_driver_runs_the_documented_patch(built):
    """The lines between the gap driver's BEGIN / END markers are the code block of INTEGRATION.md §8."""
    assert os.path.exists(os.path.join(ROOT, "tests", "mock_ref", "_build", "gap_driver"))
    src = open(os.path.join(ROOT, "tests", "mock_ref", "gap_driver.cc")).read()
    block = src.split("// BEGIN moves.cc:729-800 as patched\n")[1].split("// END")[0].split("\n")
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = doc[doc.index("## 8. Optional: the gap-length search"):]
    assert "moves.cc:729-800" in sec and "moves.cc:694-727" in sec
    new_side = sec.split("```cpp\n")[2].split("\n```")[0].split("\n")  # (the first block is the method's declaration)
    assert _strip(block) == _strip(new_side)
    assert sum("prob_calc.FixGapLength(paths, path_id, gap_pos)" in ln for ln in new_side) == 1
    assert "| `gaml_hip_gap_profile`, `gaml_hip_fix_gap_length`" in doc[doc.index("## 2. The C ABI"):doc.index("## 3. ")]
