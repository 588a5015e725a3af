"""The work-split cases of tests/grid_split_cases.py on the CPU, before any GPU is involved: the declared classes are the host
model's, no two pairs of a class share the oracle's per-read value (apart from the declared floored pairs), the floored pairs
sit at the slots the case names -- the first and the last of every class among them -- and the round arithmetic the sizes
were chosen for holds for every (part, cap) the GPU tests use. The classes with several records per mate and the delta lists
belong to the device tables: tests/test_gpu_grid_split.py checks them (pair_classes, debug_delta_check)."""
import math

import numpy as np
import pytest

import crafted_records_cases as cc
import grid_split_cases as gs

SPLIT = gs.split_cases()
FULL = [c for c in SPLIT if c.with_others]


@pytest.mark.parametrize("case", SPLIT, ids=repr)
def test_classes_are_the_host_models(built, case):
    b = cc.Built(case)
    assert b.n == case.n_reads() and b.n <= 17_000
    for s in case.all_path_sets():
        for w in cc.windows_of(s):
            assert w in b.windows
    ctx, rs = b.library(device=-1)
    ctx.debug_prepare(case.path_sets[0])  # the set the tables are built under: [B]'s window is not part of them
    st, fold = ctx.debug_static_check(rs), ctx.debug_fold_check(rs)
    assert st["violations"] == 0 and fold["violations"] == 0
    assert st["static_pairs"] == case.expected_static(device=False) == len(case.order["static"]), st
    assert st["other_pairs"] == len(case.order.get("rest", ())) and st["static_pairs"] + st["other_pairs"] == fold["compact_pairs"][0] == case.expected_classes()[0]
    if case.with_others:
        assert st["distance"] == 3 and st["edits_or_code"] == gs.N_REST - 3  # why the rest has no static index: as declared
        assert case.expected_classes() == [gs.N_STATIC + gs.N_REST, gs.N_TWO, gs.N_FOUR, gs.N_MORE] and gs.N_FOUR > cc.FOLD_BELOW
    assert ctx.aligner_stats()["windows"] == 0
    ctx.close()


@pytest.mark.parametrize("case", SPLIT, ids=repr)
def test_every_pair_has_a_value_of_its_own_and_the_floored_pairs_sit_where_declared(built, case):
    b = cc.Built(case)
    o, ors = b.oracle()
    n = case.ins_n
    for paths in (gs.S_MAIN, gs.S_GEN):
        v, zeros, tl = o.calc_prob(paths, fresh=True)
        probs, _ = o.paired_probs(ors)
        assert o.windows_aligned(ors, 0) == 0 and o.windows_aligned(ors, 1) == 0
        floor = math.exp(case.cfg["min_prob_start"] + case.cfg["min_prob_per_base"] * 200)
        floored = {b.first[name] for name in case.floored}
        below = set(np.flatnonzero(probs / (2.0 * tl) < floor).tolist()) if len({p.lens for p in case.patterns}) == 1 else None
        assert int(zeros[0][0]) == len(floored), (case.name, zeros.tolist(), len(floored))
        if below is not None:
            assert below == floored, (case.name, sorted(below ^ floored)[:5])
        for part, names in case.order.items():
            rids = [b.first[name] for name in names]
            live = [r for r in rids if r not in floored]
            vals = probs[live]
            assert (vals > 0.0).all(), (case.name, part)
            assert len(set(vals.tolist())) == len(live), f"{case.name}, {part}: two pairs share a per-read value"
            marked = [k for k, r in enumerate(rids) if r in floored]
            if part == "delta" and not names:
                continue
            assert marked[0] == 0 and marked[-1] == len(rids) - 1 and len(marked) >= 2, (case.name, part, marked)
            for r in (r for r in rids if r in floored):  # no term at all, or (static part) a term far below the floor
                p = next(q for q in case.patterns if q.name == b.who[r][0])
                assert probs[r] == 0.0 if p.term == () else 0.0 < probs[r] / (2.0 * tl) < floor * 1e-40, b.label(r)
    o.calc_prob(gs.S_NONE, fresh=True)
    assert not o.paired_probs(ors)[0].any()  # under [E] no pair scores: what the GPU tests wipe the per-read values with
    assert n - 2 > 900 > gs.D_LO + gs.N_STATIC // 13 and gs.FAR_STATIC[2] < n


def test_slot_order_model():
    """The order dictionaries name every read once; the static part ends in the three pairs without a record, the delta pairs
    are static pairs, five of them with six records in [B]'s window."""
    case = gs.split_case("split_one_combo")
    b = cc.Built(case)
    names = [n for part in ("static", "rest", "two", "four", "more") for n in case.order[part]]
    assert sorted(b.first[n] for n in names) == list(range(b.n))
    assert case.order["static"][-3:] == ["static_mate2_missing", "static_mate1_missing", "static_both_missing"]
    assert set(case.order["delta"]) <= set(case.order["static"]) and len(case.order["delta"]) == gs.N_DELTA
    long_lists = [n for n in case.order["delta"] if sum(1 for r in next(p for p in case.patterns if p.name == n).recs if r[1] == cc.WB) > 4]
    assert len(long_lists) == gs.N_SPILL
    # dirty slots are spread over the static part's rounds, not gathered in one
    slots = [case.order["static"].index(n) for n in case.order["delta"]]
    assert min(slots) < 1024 and max(slots) > 6 * 1024 - 4 * 1024 and len({s // 1024 for s in slots}) >= 6
    for name in ("static_1024", "static_1025"):
        c = gs.split_case(name)
        assert c.n_reads() == len(c.order["static"]) == int(name[-4:]) and c.expected_classes() == [c.n_reads(), 0, 0, 0]


@pytest.mark.parametrize("caps", list(gs.CAPS), ids=str)
@pytest.mark.parametrize("no_memo", [False, True], ids=["memo", "no_memo"])
def test_round_arithmetic(caps, no_memo):
    """Under every cap every part's busiest lane (wave) makes three rounds or more and the last round is ragged. The one
    exception is stated: the static part under one block ends in a round of 513 slots that every lane enters -- there the
    tail is the clamped index (two slots a lane, lane 0 three); the sibling case of 1,025 slots has the ragged second round."""
    case = gs.split_case("split_one_combo")
    sizes = case.sizes(no_memo)
    for part in gs.PARTS:
        n, blocks = sizes[part], gs.CAPS[caps][part]
        if n == 0:
            assert part == "static" and no_memo
            continue
        # (four slots a lane: the widest round any body of the part has, so the fewest rounds; without a memo class 0 is
        # paired_compact_body's, two slots a lane and iteration)
        per = 2 * gs.K_BLOCK if no_memo and part == "rest" else gs.PER_ROUND[part]
        r, last = gs.rounds(n, blocks, per)
        assert r >= 3, (part, caps, n, r)
        assert n > blocks * per * 2
        if (part, blocks) == ("static", 1):
            assert last == 513 and not gs.ragged(n, blocks, per)
        else:
            assert gs.ragged(n, blocks, per), (part, caps, n, last)
        if per == 4 * gs.K_BLOCK:  # ... and so is it when the body takes two (paired_compact_body) or one per lane and round
            for lanes_take in (2, 1):
                assert gs.rounds(n, blocks, lanes_take * gs.K_BLOCK)[0] >= 3
    assert gs.rounds(1024, 1, 1024) == (1, 1024) and gs.rounds(1025, 1, 1024) == (2, 1) and gs.ragged(1025, 1, 1024)
    assert [gs.block_of_slot(s, 3, 1024) for s in (0, 255, 256, 767, 768, 3071, 3072)] == [0, 0, 1, 2, 0, 2, 0]
    assert [gs.block_of_slot(s, 3, gs.WAVES) for s in (0, 3, 4, 11, 12)] == [0, 0, 1, 2, 0]


def test_single_end_and_pacbio_sizes():
    assert tuple(gs.SINGLE_READS) == tuple(gs.PACBIO_READS) == gs.BLOCK_COUNTS
    for blocks, n in gs.SINGLE_READS.items():
        assert -(-n // gs.K_BLOCK) == blocks
    for blocks, n in gs.PACBIO_READS.items():
        assert -(-n // gs.WAVES) == blocks
    for cap in gs.SET_CAPS:  # the largest case under the caps: three trips or more, a ragged last one
        r, last = gs.rounds(gs.N_SINGLE, cap, gs.K_BLOCK)
        assert r >= 3 and min(last, cap * gs.K_BLOCK) % 64 != 0
        r, last = gs.rounds(gs.PACBIO_READS[33], cap, gs.WAVES)
        assert r >= 3 and last % gs.WAVES != 0


def test_single_end_reads_have_values_of_their_own(built):
    case = gs.single_case(gs.N_SINGLE)
    b = cc.Built(case)
    o, rs = b.oracle()
    seen = []
    for paths in gs.SINGLE_SETS[:3]:
        v, probs, o3 = o.single_detail(rs, paths)
        assert o.windows_aligned(rs, 0) == 0
        live = probs[probs > 0.0]
        assert len(set(live.tolist())) == len(live) and len(live) > 0.8 * b.n
        seen.append(probs)
        assert 0 < int(o3[0]) < b.n  # some reads below the floor, some above
    none = [i for i in range(b.n) if i % 500 == 0 or i == b.n - 1]
    assert not seen[0][none].any() and seen[0][1] > 0 and seen[0][b.n - 2] > 0
    twice = [i for i in range(b.n) if i % 11 == 5 and i % 7 != 3 and 60 + i % 191 <= 100 and i not in none]
    assert len(twice) > 50 and (seen[1][twice] == 2 * seen[2][twice]).all() and not seen[0][twice].any()  # [C] twice, once, not at all
    three = [i for i in range(b.n) if i % 7 == 3 and i not in none]
    m, M = 0.01, 0.96
    for i in three[:40]:  # the later record of the two on one position counts, beside the junction window's
        L, e = 60 + i % 191, i // 191
        want = m ** e * M ** (L - e) + m ** min(e + 2, L) * M ** (L - min(e + 2, L))
        assert abs(seen[0][i] - want) <= 1e-14 * want, b.label(i)
    assert not o.single_detail(rs, gs.SINGLE_SETS[3])[1].any()


def test_pacbio_reads_have_values_of_their_own(built):
    pc = gs.pacbio_case(gs.PACBIO_READS[33])
    o, rs = pc.oracle()
    per_read = np.zeros(pc.n, np.int64)
    for s, (rec, lp) in pc.recs.items():
        per_read += np.bincount(rec[:, 2], minlength=pc.n)
        assert len(set(lp.tolist())) == len(lp)
    assert per_read.tolist() == [gs.PACBIO_RECORDS[r % 6] for r in range(pc.n)]
    want, lp, o3 = o.pacbio_detail(rs, gs.PACBIO_SETS[0])
    fin = np.isfinite(lp)
    assert len(set(lp[fin].tolist())) == int(fin.sum()) and 0 < int(o3[0]) < pc.n
    floor = -10.0 - 0.7 * gs.PACBIO_LEN
    assert (lp[fin] < floor).any() and (lp[fin] > floor).any() and (~fin).sum() >= pc.n // 6  # below the floor, above it, no record
    # sub-walk counts 0, 1 and 3 under the first set
    once, lp1, _ = o.pacbio_detail(rs, gs.PACBIO_SETS[1])
    assert (lp[fin] >= lp1[fin]).all() and (lp[fin] > lp1[fin]).any()
    assert not np.isfinite(o.pacbio_detail(rs, gs.PACBIO_SETS[3])[1]).any()
    assert len(pc.recs[(gs.B ^ 1,)][1]) > 0 and len(pc.recs[(gs.A ^ 1,)][1]) == 0
