"""The mixed gap-profile route (gaml_hip_set_gap_mixed_device) without a GPU: the per-context switch exists on host-only
contexts and follows GAML_HIP_GAP_MIXED; the PacBio enumeration split into what the lengths of a gap share and the growths
that reach the gap equals the whole enumeration (the library's own, and a restatement of graph.cc:2438-2454 here); and the
rule the device route derives a single-end set's tables by -- ranks at or behind the gap move by the difference of the
lengths, nothing else moves -- holds between the occurrence lists of the set prepared with two lengths."""
import os

import numpy as np
import pytest

import gap_mixed_cases as gm
import gap_oracle as go


@pytest.fixture(scope="module")
def fx(built):
    return gm.Fixture()


def test_host_only_context_keeps_the_flag(fx):
    from gaml_amd import api
    c, h = fx.context("paired+single+pacbio", device=-1)
    assert c.gap_mixed_device() is False
    c.set_gap_mixed_device(True)
    assert c.gap_mixed_device() is True
    paths, path_id, gap_pos = fx.three_paths(5)
    for fn, tail in ((c.gap_profile, ([40, 41, 39],)), (c.fix_gap_length, ())):
        with pytest.raises(api.GamlHipError) as e:
            fn(paths, path_id, gap_pos, *tail)
        assert e.value.code == api.ENODEVICE
    c.set_gap_mixed_device(False)
    assert c.gap_mixed_device() is False
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "gaml_hip.h")).read()
    assert "int gaml_hip_set_gap_mixed_device(" in hdr and "int gaml_hip_get_gap_mixed_device(" in hdr
    dbg = open(os.path.join(root, "include", "gaml_hip_debug.h")).read()
    for name in ("gaml_hip_debug_gap_single_table(", "gaml_hip_debug_gap_pacbio_counts(", "gaml_hip_debug_pacbio_gap_enum("):
        assert name in dbg, name


def test_environment_turns_the_flag_on(built, monkeypatch):
    from gaml_amd import api
    monkeypatch.setenv("GAML_HIP_GAP_MIXED", "device")
    assert api.Context(device=-1).gap_mixed_device() is True
    assert api.Context(device=-1).gap_penalty_device() is False  # (a switch of its own)
    monkeypatch.setenv("GAML_HIP_GAP_MIXED", "fallback")
    assert api.Context(device=-1).gap_mixed_device() is False
    monkeypatch.delenv("GAML_HIP_GAP_MIXED")
    assert api.Context(device=-1).gap_mixed_device() is False


def _enum_cases(fx):
    """(name, path, gap_pos, lengths): one path each"""
    w = fx.walk
    L = gm.PACBIO_LEN  # the longest read: a growth is cut once it has passed that many bases behind its first node
    mid = w[:5] + [-fx.node_len(5)] + w[6:12]
    two = w[:3] + [-fx.node_len(3)] + w[4:7] + [-fx.node_len(7)] + w[8:12]
    far = w[4:9] + [-fx.node_len(9)] + w[10:14]  # the node in front of this gap is shorter than the longest read
    assert 1 < L - fx.node_len(8) - 1
    return [
        ("gap at the first entry", [-fx.node_len(1)] + w[2:8], 0, [fx.node_len(1), 1, 700, 5000]),
        ("gap in the middle", mid, 5, [fx.node_len(5), 1, 2, 640, 3000]),
        ("gap as the last-but-one entry", w[2:9] + [-fx.node_len(9)] + w[10:11], 7, [fx.node_len(9), 1, 900, 2500]),
        ("two gaps, the second edited", two, 7, [fx.node_len(7), 1, 77, 1200, 4000]),
        # the start right in front of the gap grows through it while the gap is no longer than the longest read
        ("a growth cut at the gap", mid, 5, [L - 1, L, L + 1]),
        # ... and the start two entries in front of it (a long node between them) is cut by a far shorter gap
        ("a growth cut at the gap, from further away", far, 5, [L - fx.node_len(8) - 1, L - fx.node_len(8), L - fx.node_len(8) + 1]),
    ]


def test_split_enumeration_equals_the_whole_one(fx):
    site, cached = 5, 640
    extra = [fx.gap_records(site, cached),  # a sub-walk that contains -640: cached for exactly one of the lengths
             ([-77] + fx.walk[8:9], *fx.gap_records(7, 77)[1:]),  # ... and one that starts AT the second gap of the two-gap path
             (fx.walk[7:9] + [-(gm.PACBIO_LEN - fx.node_len(8))], *fx.gap_records(5, 1)[1:])]  # ... and one that ends at the gap, at a cut-off length
    c, h = fx.context("pacbio", device=-1, records=extra)
    ids = fx.walk_ids(extra)
    assert c.pacbio_stats(h["pacbio"])["subwalks"] == len(ids)
    max_len = int(fx.pb.lens.max())
    seen_hit_with_gap, cut_changes = 0, 0
    for name, path, gap_pos, lens in _enum_cases(fx):
        per_len = []
        for l in lens:
            whole = list(path)
            whole[gap_pos] = -l
            hits, misses = c.debug_pacbio_gap_enum(h["pacbio"], path, gap_pos, l)  # (raises when the library's own check differs)
            want_hits, want_misses = gm.model_enumerate(fx, ids, whole, max_len)
            print(name, l, len(hits), "hits,", misses, "misses")
            assert [tuple(x) for x in hits.tolist()] == want_hits, (name, l)
            assert misses == want_misses, (name, l)
            gap_ids = {k for wk, k in ids.items() if -l in wk}
            seen_hit_with_gap += sum(1 for k, _ in want_hits if k in gap_ids)
            per_len.append((len(want_hits), want_misses))
        if name.startswith("a growth cut"):
            # below and at the cut-off the growth goes on behind the gap, above it it stops there: fewer lookups
            total = [a + b for a, b in per_len]
            assert total[0] == total[1] and total[2] < total[1], (name, per_len)
            cut_changes += 1
        if name == "gap in the middle":
            n640 = [sum(1 for k, _ in gm.model_enumerate(fx, ids, path[:gap_pos] + [-l] + path[gap_pos + 1:], max_len)[0] if k == ids[tuple(extra[0][0])]) for l in lens]
            assert n640 == [1 if l == cached else 0 for l in lens], n640
    assert seen_hit_with_gap >= 3 and cut_changes == 2
    # the entry refuses what is not a gap
    from gaml_amd import api
    with pytest.raises(api.GamlHipError):
        c.debug_pacbio_gap_enum(h["pacbio"], fx.walk[:6], 2, 10)


@pytest.mark.parametrize("path_id,site", [(0, 5), (1, 19), (2, 35), (0, 1)])
def test_single_end_rule_ranks_behind_the_gap_move(fx, path_id, site):
    """Occurrences are visited path by path, contig by contig, and a shift is stv + the running total over ALL paths: between
    two lengths every occurrence whose rank lies behind the gap moves by the difference -- the later paths' too -- and nothing
    else differs. first_rank is counted independently: the occurrences of the set cut off at the gap."""
    c, h = fx.context("single", device=-1)
    rs = h["single"]
    base = fx.node_len(site)
    paths, pid, gap_pos = fx.three_paths(site, path_id=path_id)
    c.debug_prepare(paths)
    a = c.debug_occurrences(rs).copy()
    front = paths[:pid] + [paths[pid][:gap_pos]]
    c.debug_prepare(front)
    first_rank = len(c.debug_occurrences(rs))
    assert np.array_equal(c.debug_occurrences(rs), a[:first_rank])
    assert a[:, 4].tolist() == list(range(len(a))) and set(a[:, 3].tolist()) == {0}  # ranks in visiting order, path 0 in every entry
    if path_id < 2:
        assert first_rank < len(a)
    for l in (1, base - 1, base + 1, 3 * base + 7):
        c.debug_prepare(go.with_length(paths, pid, gap_pos, l))
        b = c.debug_occurrences(rs)
        want = a.copy()
        want[first_rank:, 1] += l - base
        assert np.array_equal(b, want), (path_id, site, l)
    print(path_id, site, "first_rank", first_rank, "of", len(a), "windows", c.single_stats(rs)["windows"])
