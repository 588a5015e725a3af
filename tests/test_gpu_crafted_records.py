"""The hand-made records of tests/crafted_records_cases.py on the GPU: per case a fresh context and a fresh oracle get the
same puts; the blocking call agrees with the oracle per read, the record tables hold the classes the case declares, and the
batch, incremental and gap-profile routes give the blocking call's bits. Messages name case, pattern and read, so that a
failure names the branch (the pattern's `aim`)."""
import math

import numpy as np
import pytest

import crafted_records_cases as cc

pytestmark = pytest.mark.gpu

CASES = cc.cases()
RTOL = 4e-16  # per-read probabilities (the project's bound)


def _same_value(got, want, rel):
    return got == want or (math.isfinite(want) and abs(got - want) <= rel * abs(want))


def _oracle_reads(case, o, ors, paths):
    """(value, zeros, total_len, per-read probabilities, bad_bases) of the oracle on `paths`, evaluated afresh"""
    v, z, tl = o.calc_prob(paths, fresh=True)
    if case.single:
        _, probs, o3 = o.single_detail(ors, paths)
        return v, z, tl, probs, int(o3[2])
    probs, bad = o.paired_probs(ors)
    return v, z, tl, probs, bad


def _assert_reads(b, got, want, what):
    bad = np.flatnonzero(~(np.abs(got - want) <= RTOL * np.abs(want)))
    assert bad.size == 0, f"{what}: {b.label(int(bad[0]))}: library {got[bad[0]]!r}, oracle {want[bad[0]]!r} ({bad.size} reads differ)"


def _assert_bits(b, got, want, what):
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    assert bad.size == 0, f"{what}: {b.label(int(bad[0]))}: {got[bad[0]]!r} != {want[bad[0]]!r} ({bad.size} reads differ)"


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_blocking_call_against_the_oracle(case):
    b = cc.Built(case)
    ctx, rs = b.library()
    o, ors = b.oracle()
    for k, paths in enumerate(case.path_sets):
        got, zeros, tl = ctx.calc_prob(paths)
        want, wzeros, wtl, wprobs, wbad = _oracle_reads(case, o, ors, paths)
        what = f"{case.name}, path set {k}"
        assert tl == wtl and zeros.tolist() == wzeros.tolist(), (what, zeros.tolist(), wzeros.tolist())
        _assert_reads(b, ctx.read_probs(rs), wprobs, what)
        assert _same_value(got, want, 1e-12), (what, got, want)
        if case.family == "D":
            assert ctx.bad_bases(rs) == wbad == cc.expected_bad_bases(case, paths)[0], what
        if k == 0 and not case.single:  # the tables of the first call: the classes the patterns declare
            assert ctx.pair_classes(rs).tolist() == case.expected_classes(), what
            assert ctx.table_stats(rs)["static_index_pairs"] == case.expected_static(), what
            t, s, f = ctx.debug_tables_check(rs), ctx.debug_static_check(rs), ctx.debug_fold_check(rs)
            assert t["mismatches"] == 0 and t["compared"] > 0 and t["pairs"] == b.n, t
            assert s["violations"] == 0 and f["violations"] == 0, (s, f)
    assert ctx.aligner_stats()["windows"] == 0
    assert [o.windows_aligned(ors, mt) for mt in b.mates] == [0] * len(b.mates)
    ctx.close()


def _probs_of(b, paths, knobs=()):
    ctx, rs = b.library(knobs=knobs)
    v, z, tl = ctx.calc_prob(paths)
    out = (v, z.tolist(), ctx.read_probs(rs).copy(), ctx.pair_classes(rs).tolist(), ctx.table_stats(rs)["static_index_pairs"])
    assert ctx.aligner_stats()["windows"] == 0
    ctx.close()
    return out


@pytest.mark.parametrize("name", ["A_mean300", "A_mean220"])
def test_looked_up_terms_are_the_per_pair_terms(name):
    """logterm_kernel's claim: a pair whose edits are both < 7, whose length code is < 4 and whose distance is < ins_n reads
    its term from the memo, and that term has the bits of the same records under a length code >= 4 (four other
    combinations of lengths in front) and of the same records with the memo switched off."""
    from gaml_amd import api
    case, late = cc.case(name), cc.late_codes(name)
    b, bl = cc.Built(case), cc.Built(late)
    paths = case.path_sets[0]
    v, z, probs, classes, static = _probs_of(b, paths)
    vl, zl, probs_late, classes_late, static_late = _probs_of(bl, paths)
    vn, zn, probs_off, _, static_off = _probs_of(b, paths, knobs=((api.Knob.NO_MEMO, 1),))
    assert static == case.expected_static() > 10 and static_late == late.expected_static() == 7 and static_off == 0
    assert classes == case.expected_classes() and classes_late == late.expected_classes()
    _assert_bits(b, probs_late[late.fillers:], probs, f"{name}: length code >= {cc.MEMO_CODES} against the memo")
    _assert_bits(b, probs_off, probs, f"{name}: NO_MEMO against the memo")
    assert zn == z and _same_value(vn, v, 1e-13)  # (the memo also holds log(term): log(t) - log(2T) against log(t / 2T))
    n = case.ins_n
    in_memo = 0
    for p in case.patterns:
        for rid in b.reads_of(p.name):
            if p.term and p.term[2] >= n:  # at dist >= ins_n: exactly 0.0, and floored (the floor is positive)
                assert probs[rid] == 0.0 and probs_late[rid + late.fillers] == 0.0, b.label(rid)
            elif p.term and p.cls == "static":
                in_memo += 1
                assert probs[rid] > 0.0 or p.term[2] >= n - 2, b.label(rid)
    assert in_memo >= 15
    assert z[0][0] >= sum(p.copies for p in case.patterns if not p.term or p.term[2] >= n)


@pytest.mark.parametrize("name", ["A_floor_default", "A_floor_high", "A_floor_underflow"])
def test_floors(name):
    case = cc.case(name)
    b = cc.Built(case)
    v, z, probs, classes, static = _probs_of(b, case.path_sets[0])
    n = case.ins_n
    zero = [rid for p in case.patterns for rid in b.reads_of(p.name) if not p.term or p.term[2] >= n]
    assert all(probs[r] == 0.0 for r in zero) and len(zero) == 5
    if name == "A_floor_default":
        assert z[0][0] >= len(zero) and z[0][0] < b.n and math.isfinite(v)
    elif name == "A_floor_high":
        assert z[0] == [b.n, b.n] and math.isfinite(v)  # the floor sits above every value
    else:
        assert z[0][0] == 0 and v == -math.inf and static == 0  # a floor of 0.0: nothing is floored, log(0) for a read without a term


def test_fold_threshold_moves_the_class_not_the_values():
    """1,024 pairs with four records per mate are scored one wave per pair, 1,025 one lane per pair: pair_classes() shows it.
    The two kernels add a pair's sixteen terms in different orders (a lane's loop, a wave's shuffle tree), so the per-read
    probabilities are held to the project's bound against the same oracle values, not to equal bits (measured: 1 ulp
    apart); floored counts are equal and the pairs the threshold does not move keep their bits."""
    lo, hi = cc.case(f"B_fold{cc.FOLD_BELOW}"), cc.case(f"B_fold{cc.FOLD_BELOW + 1}")
    bl, bh = cc.Built(lo), cc.Built(hi)
    vl, zl, pl, cl, _ = _probs_of(bl, lo.path_sets[0])
    vh, zh, ph, ch, _ = _probs_of(bh, hi.path_sets[0])
    assert cl == [2, 1, 0, cc.FOLD_BELOW] and ch == [2, 1, cc.FOLD_BELOW + 1, 0]
    o, ors = bl.oracle()
    o.calc_prob(lo.path_sets[0], fresh=True)
    want, _ = o.paired_probs(ors)
    _assert_reads(bl, pl, want, "class folded")
    _assert_reads(bl, ph[:cc.FOLD_BELOW], want[:cc.FOLD_BELOW], "class kept")
    assert len(set(pl[:cc.FOLD_BELOW].tolist())) == 1 and len(set(ph[:cc.FOLD_BELOW + 1].tolist())) == 1  # every copy alike
    _assert_bits(bl, ph[cc.FOLD_BELOW + 1:], pl[cc.FOLD_BELOW:], "the pairs of the other classes")
    assert zl[0][0] == zh[0][0] == 0 and math.isfinite(vl) and math.isfinite(vh)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_batch_gives_the_blocking_calls_bits(case):
    b = cc.Built(case)
    sets = cc.batch_sets(case)
    assert len(sets) == 8
    modes = (False, True) if case.single else (False,)
    one, rs1 = b.library()
    want = []
    for s in sets:
        v, z, tl = one.calc_prob(s)
        want.append((v, z.tolist(), tl, one.bad_bases(rs1) if case.family == "D" else 0))
    for onepass in modes:
        ctx, rs = b.library()
        if onepass:
            ctx.set_single_onepass(True)
        got = ctx.calc_prob_batch(sets)
        for k, ((v, z, tl), (wv, wz, wtl, wbad)) in enumerate(zip(got, want)):
            what = f"{case.name}, batch entry {k}, onepass {onepass}"
            assert tl == wtl and z.tolist() == wz, (what, z.tolist(), wz)
            assert v == wv or (math.isnan(v) and math.isnan(wv)), (what, v, wv)
        if case.family == "D":
            assert ctx.debug_batch_bad_bases(rs) == [w[3] for w in want], case.name
        if case.single:  # the one-pass route was taken when asked for, and only then
            launches = ctx.single_stats(rs)["multi_launches"]
            assert (launches > 0) == onepass, (case.name, onepass, launches)
        assert ctx.aligner_stats()["windows"] == 0
        ctx.close()
    one.close()


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_incremental_call_gives_a_fresh_contexts_bits(case):
    """Score path_sets[0], then a set that differs from it in one path: value, floored counts and per-read probabilities of
    the second call are those of a fresh context that scores that set directly."""
    b = cc.Built(case)
    s0, s1 = case.path_sets[0], case.path_sets[1]
    assert sum(1 for p, q in zip(s0, s1) if p != q) + abs(len(s0) - len(s1)) == 1
    inc, rs = b.library()
    inc.calc_prob(s0)
    v, z, tl = inc.calc_prob(s1)
    fresh, rsf = b.library()
    wv, wz, wtl = fresh.calc_prob(s1)
    assert tl == wtl and z.tolist() == wz.tolist() and (v == wv), (case.name, v, wv, z.tolist(), wz.tolist())
    _assert_bits(b, inc.read_probs(rs), fresh.read_probs(rsf), f"{case.name}: second call against a fresh context")
    if case.family == "D":
        assert inc.bad_bases(rs) == fresh.bad_bases(rsf)
    assert inc.aligner_stats()["windows"] == 0 and fresh.aligner_stats()["windows"] == 0
    inc.close()
    fresh.close()


@pytest.mark.parametrize("name", ["A_mean300", "A_mean220"])
def test_gap_profile_equals_single_calls(name):
    """Over the gap of [A, -g, B] the pair with a mate on either side has a term whose distance moves with g, through the
    table and past its end. The profile's sums run in another order than a single call's: 1e-13 relative, like
    tests/test_gpu_gap.py; floored counts and lengths are equal."""
    case = cc.case(name)
    b = cc.Built(case)
    paths, pid, pos, lens = case.gap
    dev, rs = b.library()
    got = dev.gap_profile(paths, pid, pos, lens)
    one, rs1 = b.library()
    o, ors = b.oracle()
    across = b.first["across_gap"]
    seen = []
    for (v, z, tl), l in zip(got, lens):
        s = cc.gap_paths(case.gap, l)
        wv, wz, wtl = one.calc_prob(s)
        assert tl == wtl and z.tolist() == wz.tolist() and _same_value(v, wv, 1e-13), (name, l, v, wv)
        ov, oz, otl, oprobs, _ = _oracle_reads(case, o, ors, s)
        assert otl == tl and oz.tolist() == z.tolist() and _same_value(v, ov, 1e-12), (name, l, v, ov)
        _assert_reads(b, one.read_probs(rs1), oprobs, f"{name}, gap {l}")
        seen.append(one.read_probs(rs1)[across])
    assert (seen[0] > 0.0 or name == "A_mean220") and seen[-1] == 0.0  # 160 + g runs past ins_n
    assert dev.aligner_stats()["windows"] == 0 and one.aligner_stats()["windows"] == 0
    dev.close()
    one.close()
