"""The hand-made records of tests/crafted_records_cases.py on the CPU: every case builds, its windows are complete (neither
the library nor the oracle aligns anything), the oracle's pair term agrees with exact arithmetic, and the oracle does with
every pattern what the case says of it (which record survived, which marks the sweep counts). The classes of
pair_classes() belong to the device tables: tests/test_gpu_crafted_records.py checks them."""
import math

import numpy as np
import pytest

import crafted_records_cases as cc

CASES = cc.cases()
PAIRED = [c for c in CASES if not c.single]


def _mp_term(cfg, e1, e2, L1, L2, dist):
    """m^(e1+e2) M^(L1+L2-e1-e2) exp(-z^2/2) / (sd sqrt(2 pi)) at 60 digits; the config's doubles are taken as exact binary
    values, M = 1 - 4 m as the double the oracle computes (gaml.cc:813,854)."""
    import mpmath as mp
    mp.mp.dps = 60
    m, M = mp.mpf(cfg["mismatch"]), mp.mpf(1.0 - 4 * cfg["mismatch"])
    mean, sd = mp.mpf(cfg["mean"]), mp.mpf(cfg["sd"])
    z = (mp.mpf(dist) - mean) / sd
    return m ** (e1 + e2) * M ** (L1 + L2 - e1 - e2) * mp.exp(-z * z / 2) / (sd * mp.sqrt(2 * mp.pi)), z


def _oracle_probs(case, paths=None):
    b = cc.Built(case)
    o, rs = b.oracle()
    before = [o.windows_aligned(rs, mt) for mt in b.mates]
    v, zeros, tl = o.calc_prob(case.path_sets[0] if paths is None else paths, fresh=True)
    assert [o.windows_aligned(rs, mt) for mt in b.mates] == before
    probs, bad = o.paired_probs(rs)
    return b, probs, bad, zeros


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_every_window_is_put_and_nothing_is_aligned(built, case):
    """Every window of every path set a test scores is filed before the first call, on both sides."""
    b = cc.Built(case)
    assert b.n == case.n_reads() and b.n <= 3000
    for s in case.all_path_sets():
        for w in cc.windows_of(s):
            assert w in b.windows
    ctx, rs = b.library(device=-1)
    o, ors = b.oracle()
    for mt in b.mates:
        assert o.windows_aligned(ors, mt) == 0
        for w in b.windows:  # both sides hold the records in the same order: (position, read), equal keys in filing order
            want = b.records(mt, w)
            want = want[np.lexsort((np.arange(len(want)), want[:, 2], want[:, 0]))]
            assert np.array_equal(o.window_records(ors, mt, list(w)), want), w
            assert np.array_equal(ctx.window_records(rs, mt, list(w)), want), w
    for k, s in enumerate(case.all_path_sets()):
        ctx.debug_prepare(s)
        o.calc_prob(s, fresh=True)
        if k == 0 and not case.single:  # what the host restatement of the table build offers: the compact class and its static part
            st, fold = ctx.debug_static_check(rs), ctx.debug_fold_check(rs)
            assert st["violations"] == 0 and fold["violations"] == 0
            assert st["static_pairs"] == case.expected_static(device=False), st
            assert st["static_pairs"] + st["other_pairs"] == fold["compact_pairs"][0] == case.expected_classes()[0], (st, fold)
    assert ctx.aligner_stats()["windows"] == 0
    assert [o.windows_aligned(ors, mt) for mt in b.mates] == [0] * len(b.mates)
    ctx.close()


def test_oracle_put_refuses_what_the_library_refuses(built):
    b = cc.Built(cc.case("A_total64"))
    o, rs = b.oracle()
    win = [cc.E]  # not filed by the case
    for bad in [(5, 101, 3, 0), (5, 300, 3, 0), (5, -1, 3, 0), (5, 1, 3, 2), (5, 1, 3, -1), (-1, 1, 3, 0), (10_000_000, 1, 3, 0),
                (5, 1, 64, 0), (5, 1, -1, 0)]:
        with pytest.raises(ValueError):
            o.put_window_records(rs, 0, win, [bad])
        assert o.window_records(rs, 0, win) is None
    for args in ((rs, 2, win), (rs, -1, win), (rs + 1, 0, win), (rs, 0, [10_000]), (rs, 0, [-5])):
        with pytest.raises(ValueError):
            o.put_window_records(*args, [(5, 1, 3, 0)])
    assert o.put_window_records(rs, 0, win, [(7, 1, 3, 0), (5, 2, 9, 1), (5, 3, 4, 0), (5, 4, 9, 0)]) == 4
    assert o.window_records(rs, 0, win).tolist() == [[5, 3, 4, 0], [5, 2, 9, 1], [5, 4, 9, 0], [7, 1, 3, 0]]  # stable
    with pytest.raises(RuntimeError):
        o.put_window_records(rs, 0, win, [])  # already cached
    assert o.put_window_records(rs, 1, win, []) == 0 and len(o.window_records(rs, 1, win)) == 0  # empty: cached, no hits
    assert o.windows_aligned(rs, 0) == 0


def test_ins_n_is_where_the_gaussian_ends(built):
    import oracle_py as op
    for mean, sd in ((300.0, 30.0), (220.0, 10.0)):
        n = cc.ins_n(mean, sd)
        ip = op.lib().orc_insert_prob
        assert ip(float(n - 1), mean, sd) > 0.0 and ip(float(n), mean, sd) == 0.0 and ip(float(n + 1000), mean, sd) == 0.0
        assert int(mean + 5 * sd) < n - 2


def test_oracle_pair_term_against_exact_arithmetic(built):
    """Every single-term pair of families A and D: the oracle's per-read probability against the term at 60 digits, within
    (16 + 4 z^2) 2^-53 relative (two pow results and a product per mate, a subtraction, a division, a square and a halving in
    the exponent, whose rounding exp multiplies by z^2 / 2). Terms below 1e-290 (denormal or zero in f64) are left to the
    comparison with the library: only the ins_n edge and the (255, 255) pair may be among them.
    Largest ratio met: 0.19 of the bound (1,700 terms)."""
    worst, where, compared, left_out = 0.0, None, 0, []
    for case in PAIRED:
        if case.family not in ("A", "D"):
            continue
        b, probs, _, _ = _oracle_probs(case)
        n = case.ins_n
        for p in case.patterns:
            if p.term is None:
                continue
            for rid in b.reads_of(p.name):
                if p.term == ():
                    assert probs[rid] == 0.0, b.label(rid)
                    continue
                e1, e2, d = p.term
                L1, L2 = p.lens
                if d >= n:
                    assert probs[rid] == 0.0, b.label(rid)  # for dist >= ins_n the oracle's term is exactly 0.0
                    continue
                want, z = _mp_term(case.cfg, e1, e2, L1, L2, d)
                if want < 1e-290:
                    left_out.append((case.name, p.name))
                    assert d >= n - 2 or (e1, e2) == (255, 255), b.label(rid)
                    continue
                bound = (16 + 4 * float(z) ** 2) * 2.0 ** -53
                ratio = float(abs(probs[rid] - want) / want) / bound
                compared += 1
                if ratio > worst:
                    worst, where = ratio, b.label(rid)
                assert ratio <= 1.0, f"{b.label(rid)}: oracle {probs[rid]!r}, exact {float(want)!r}, {ratio:.3f} of the bound"
    print(f"{compared} terms compared, worst ratio {worst:.3f} at {where}; left out: {sorted(set(left_out))}")
    assert compared >= 150 and worst < 1.0, f"worst ratio {worst:.3f} at {where}"


@pytest.mark.parametrize("case", [c for c in PAIRED if c.family in ("B", "C")], ids=repr)
def test_oracle_keeps_the_records_the_case_says(built, case):
    """Several terms per pair: the oracle's sum against the stated terms (which record survived the overwrite rule and the
    position filter shows in the edits). A sum of k terms of one sign: k more roundings."""
    b, probs, _, _ = _oracle_probs(case)
    for p in case.patterns:
        if p.terms is None:
            continue
        want = sum(_mp_term(case.cfg, e1, e2, *p.lens, d)[0] for e1, e2, d in p.terms)
        zmax = max([abs(float(_mp_term(case.cfg, e1, e2, *p.lens, d)[1])) for e1, e2, d in p.terms] or [0.0])
        for rid in b.reads_of(p.name):
            if not p.terms:
                assert probs[rid] == 0.0
            else:
                assert abs(probs[rid] - want) <= (16 + 4 * zmax ** 2 + len(p.terms)) * 2.0 ** -53 * want, b.label(rid)


def test_candidate_counts_multiply_the_term(built):
    case = cc.case("B_candidates")
    b = cc.Built(case)
    o, rs = b.oracle()
    base = first = None
    for n, s in zip(cc.CAND_COUNTS, case.path_sets):
        o.calc_prob(s, fresh=True)
        probs, _ = o.paired_probs(rs)
        per_path = probs / n
        if base is None:
            base, first = per_path, probs.copy()
        rid = b.first["one_rec"]
        assert probs[rid] > 0 and abs(per_path[rid] - base[rid]) <= 1e-13 * base[rid], n  # n paths, n equal terms
        r1, r2 = b.first["overwritten"], b.first["two_recs"]
        assert probs[r1] > 0 and probs[r2] > probs[r1]
        t = float(_mp_term(case.cfg, 1, 2, 100, 100, 110)[0])
        assert abs(probs[r2] - 2 * n * t) <= 1e-13 * probs[r2], n  # 2 n terms, all the same double
        assert probs[b.first["beside"]] == first[b.first["beside"]] > 0  # the real walk: once


@pytest.mark.parametrize("case", [c for c in PAIRED if c.family == "D"], ids=repr)
def test_bad_bases_of_the_oracle_equal_the_plain_sweep(built, case):
    for s in case.path_sets:
        want, decided = cc.expected_bad_bases(case, s)
        _, _, bad, _ = _oracle_probs(case, s)
        assert bad == want and want > 0, (s, bad, want)
    if case.name == "D_coverage":
        _, decided = cc.expected_bad_bases(case, case.path_sets[0])
        for k, q, p, counted in cc.D_EXPECT:
            assert decided[(k, q, p)] == counted, (k, q, p)
        # the pair below the coverage threshold scores and leaves no mark
        assert not any(q == 2800 or p == 2800 for (_, q, p) in decided)


@pytest.mark.parametrize("case", [c for c in CASES if c.single], ids=repr)
def test_single_end_reads_count_what_the_case_says(built, case):
    m, M = case.cfg["mismatch"], 1.0 - 4 * case.cfg["mismatch"]
    b = cc.Built(case)
    o, rs = b.oracle()
    for s in case.path_sets:
        _, edits = cc.expected_single(case, s)
        v, probs, o3 = o.single_detail(rs, s)
        assert o.windows_aligned(rs, 0) == 0
        for rid in range(b.n):
            want = math.fsum(m ** e * M ** (100 - e) for e in edits[rid])
            assert abs(probs[rid] - want) <= 1e-14 * want, (b.label(rid), edits[rid])
    if b.n > 1:
        _, edits = cc.expected_single(case, case.path_sets[0])
        got = {name: edits[b.first[name]] for name in ("once", "outside", "solo_unused", "several", "same_abs_pos", "same_key", "same_key_swapped",
                                                       "two_paths", "two_paths_two_recs", "none", "edit64", "editL")}
        assert got == {"once": [0], "outside": [], "solo_unused": [], "several": [0, 1, 2], "same_abs_pos": [3], "same_key": [4], "same_key_swapped": [1],
                       "two_paths": [0, 0], "two_paths_two_recs": [0, 0, 2, 2], "none": [], "edit64": [64], "editL": [100]}


def test_case_list_reaches_the_sizes_and_boundaries():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    assert [cc.case(f"A_total{n}").n_reads() for n in cc.CLASS_SIZES] == list(cc.CLASS_SIZES)
    assert cc.case("A_sizes_mixed").expected_classes() == [257 + 255, 65, 0, 64]
    assert cc.case("B_fold1024").expected_classes() == [2, 1, 0, 1024] and cc.case("B_fold1025").expected_classes() == [2, 1, 1025, 0]
    assert cc.case("A_floor_underflow").expected_static() == 0 and cc.case("A_floor_default").expected_static() == 7
    a = cc.case("A_mean300")
    assert a.ins_n - 1 > int(300 + 5 * 30) and {p.term[2] for p in a.patterns if p.term} >= {100, 101, 300, 449, 450, a.ins_n - 2, a.ins_n - 1,
                                                                                           a.ins_n, a.ins_n + 1000}
    late = cc.late_codes("A_mean300")
    assert late.n_reads() == a.n_reads() + 4 and late.expected_static() == 4 + 3
    assert [len(cc.case(f"E_single{n}").patterns) and cc.case(f"E_single{n}").n_reads() for n in (1, 64, 257, 1500)] == [1, 64, 257, 1500]
