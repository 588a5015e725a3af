"""The inputs of the penalised gap-profile tests (tests/gap_penalty_cases.py), checked without a GPU: the oracle gives the
pinned bad_bases, every profile mixes the directions and the region-size changes the device route must handle, the
searches compare no two values too close to follow, and the per-context switch exists on a host-only context."""
import os

import pytest

import gap_oracle as go
import gap_penalty_cases as gp

SEARCH_STARTS, SEARCH_DROPPED, SEARCH_ENDS = gp.SEARCH_STARTS, gp.SEARCH_DROPPED, gp.SEARCH_ENDS


def test_oracle_gives_the_pinned_bad_bases(built):
    for name, want in gp.WANT.items():
        paths, path_id, gap_pos, lens = gp.cases()[name]
        got = {l: r[3][0] for l, r in zip(lens, gp.oracle_profile(name))}
        print(name, got)
        assert set(want) <= set(got), name
        assert {l: got[l] for l in want} == want, name
    o = gp.make_oracle()
    got = {}
    for l in gp.TWIN_BOTH_WANT:
        e = gp.edited81(l)
        o.calc_prob([e, gp.twin(e)], fresh=True)
        got[l] = int(o.paired_probs(0)[1])
    assert got == gp.TWIN_BOTH_WANT
    # the profile's form of that case (the twin keeps 63): the edited path's share moves alone
    twin = {l: r[3][0] for l, r in zip(gp.SHORT_LENS, gp.oracle_profile("twin in the set"))}
    assert twin[63] == 3540 and twin[1000] == 1207 + 1770, twin


def test_profiles_mix_directions_and_region_sizes(built):
    g = gp.graph()[1]
    for name, (paths, path_id, gap_pos, lens) in gp.cases().items():
        assert paths[path_id][gap_pos] == -lens[0] and len(set(lens)) == len(lens), name
        base = gp.path_len(paths[path_id])
        d = [l - lens[0] for l in lens]
        dbits = [gp.cov_bits(base + x) - gp.cov_bits(base) for x in d]
        assert min(d) < 0 and d[0] == 0 and max(d) > 0, name
        for sign in (-1, 1):
            same = [x for x, b in zip(d, dbits) if x * sign > 0 and b == 0]
            other = [x for x, b in zip(d, dbits) if x * sign > 0 and b != 0]
            assert same and other, (name, sign, list(zip(d, dbits)))
        assert all(b % 32 == 0 for b in dbits) and any(b != x for b, x in zip(dbits, d) if x), name
        bads = [r[3][0] for r in gp.oracle_profile(name)]
        assert all(b > 0 for b in bads), (name, bads)
        # (in front of a leading gap there is nothing a pair could straddle it from: its bad_bases is the same at every length)
        assert len(set(bads)) >= (1 if name == "leading gap" else 2), (name, bads)
        assert len({r[0] for r in gp.oracle_profile(name)}) == len(lens), name  # every length its own value
    assert len(gp.SITE81_LENS) == 13 and len(gp.SITE105_LENS) == 13  # two passes
    w = gp.graph()[2]
    assert (g.node_len(w[81]), g.node_len(w[105])) == (63, 129)


def test_second_library_does_not_depend_on_the_length(built):
    rows = gp.oracle_profile("site 81, edited first", "AB")
    assert len({r[3][0] for r in rows}) == 1 and rows[0][3][0] > 0, [r[3] for r in rows]
    assert [r[3][1] for r in rows] == [r[3][0] for r in gp.oracle_profile("site 81, edited first")]


def test_searches_have_no_close_comparison(built):
    o = gp.make_oracle()
    for name in SEARCH_STARTS:
        paths, path_id, gap_pos, _ = gp.cases()[name]
        for start in SEARCH_STARTS[name] + SEARCH_DROPPED[name]:
            s = go.oracle_search(o, gp.with_length(paths, path_id, gap_pos, start), path_id, gap_pos)
            print(f"{name} from {start}: -> {s.length}, state {s.state}, {len(s.trace)} evaluations, closest comparison {s.closest:.3g}")
            if start in SEARCH_STARTS[name]:
                assert s.closest >= 1e-9, (name, start, s.closest)
                assert s.length == SEARCH_ENDS[name] and len(s.trace) >= 19
            else:
                assert s.closest < 1e-9, (name, start, s.closest)  # (why it was dropped)


def test_host_only_context_keeps_the_flag(built):
    from gaml_amd import api
    c = gp.make_ctx(device=-1)
    assert c.gap_penalty_device() is False
    c.set_gap_penalty_device(True)
    assert c.gap_penalty_device() is True
    paths, path_id, gap_pos, lens = gp.cases()["site 81, edited first"]
    for fn, tail in ((c.gap_profile, (lens[:3],)), (c.fix_gap_length, ())):
        with pytest.raises(api.GamlHipError) as e:
            fn(paths, path_id, gap_pos, *tail)
        assert e.value.code == api.ENODEVICE
    c.set_gap_penalty_device(False)
    assert c.gap_penalty_device() is False
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gaml_hip.h")).read()
    assert "int gaml_hip_set_gap_penalty_device(" in hdr and "int gaml_hip_get_gap_penalty_device(" in hdr


def test_environment_turns_the_flag_on(built, monkeypatch):
    from gaml_amd import api
    monkeypatch.setenv("GAML_HIP_GAP_PENALTY", "device")
    assert api.Context(device=-1).gap_penalty_device() is True
    monkeypatch.setenv("GAML_HIP_GAP_PENALTY", "fallback")
    assert api.Context(device=-1).gap_penalty_device() is False
    monkeypatch.delenv("GAML_HIP_GAP_PENALTY")
    assert api.Context(device=-1).gap_penalty_device() is False
