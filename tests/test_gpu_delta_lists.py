"""Every route of the device delta-list maintenance (gaml_amd/csrc/delta_dev.hip.h, paired_delta_apply in
paired_tables.hip.h) against a host check. The scenarios of tests/delta_cases.py (kept honest on the CPU by
tests/test_delta_cases_host.py) activate as many records and windows as a launch needs: one-block launches with 1, 2, 4 and
8 records per thread, a window cut across launches, multi-block launches with and without a window list in device memory.
Three contexts walk each scenario -- the default, DELTA_ONE_BLOCK (one-block launches only) and DELTA_POLICY = NO_LISTS (the tables
rebuilt) -- next to the oracle. After every step gaml_hip_debug_delta_check compares the live tables and lists with the
host restatement read by read, gaml_hip_debug_delta_routes says which launches ran, and the values are compared: bit for
bit between the two list-keeping contexts (same lists, same order; only the numbering may differ), rtol 4e-16 per read
against the rebuilt tables and the oracle, 1e-13 / 1e-9 for the likelihood (a sum in another order / the oracle).

Left out on purpose: the flag a multi-block launch raises when more than 8,192 of its 49,152 records hash to one of its 32
bins -- no honest input reaches it, and the bin capacity sizes the kernel's LDS. The record tables' class of pairs with 3 to
4 records per mate holds pairs only above 1,024 of them (below, they are scored one wave per pair with the longer ones):
the scenario medium-pieces builds its tables from both strands of the whole walk to have it."""
from functools import lru_cache

import numpy as np
import pytest

import delta_cases as dc
import oracle_py as op

pytestmark = pytest.mark.gpu

ROUTE_KEYS = ("one", "two", "four", "eight", "multi_block", "multi_block_wlist", "windows_cut")


def _ctx(fix, knobs=None):
    """knobs: {name of an api.Knob: value}"""
    from gaml_amd import api
    g, pr, _ = dc.fixture(fix)
    c = api.Context(device=0)
    c.debug_set_knob(api.Knob.REBUILD_DIVISOR, 2)  # no rebuild beside the evaluations below pairs / 2 records on the lists
    for k, v in (knobs or {}).items():
        c.debug_set_knob(api.Knob[k], v)
    c.set_graph(*g.packed())
    rs = c.add_paired(api.paired_cfg(*dc.INSERT), *dc.packed_reads(pr))
    return c, rs


@lru_cache(maxsize=None)
def _oracle(fix):
    g, pr, _ = dc.fixture(fix)
    orc = op.Oracle()
    orc.set_graph(*g.packed())
    ors = orc.add_paired(*dc.packed_reads(pr), 0.01, op.paired_cfg(*dc.INSERT))
    return orc, ors


_ORACLE_VALUES = {}


def _want(fix, paths):
    """(likelihood, floored counts, total length, per-read probabilities) of the oracle; computed once per path set"""
    key = (fix, tuple(tuple(p) for p in paths))
    if key not in _ORACLE_VALUES:
        orc, ors = _oracle(fix)
        v, z, tl = orc.calc_prob(paths, fresh=True)
        _ORACLE_VALUES[key] = (v, z.copy(), tl, orc.paired_probs(ors)[0].copy())
    return _ORACLE_VALUES[key]


def _route_step(before, after):
    d = {k: after[k] - before[k] for k in ROUTE_KEYS}
    d["launches"] = d["one"] + d["two"] + d["four"] + d["eight"]
    d["min_block"] = after["min_block"]
    return d


def _assert_route(got, want, what):
    """`want` names launch counters and what the step must add to them (a pair: at least, at most). One-block launches:
    either per kind ("one", "two", "four", "eight"; a kind it does not name: none) or only their number ("launches");
    multi-block launches it does not name: none; "windows_cut" it does not name: none, unless only the number of one-block
    launches is given (where they are cut depends on the windows' sizes). "min_block": the smallest block of a <1> launch."""
    want = dict(want)
    if "launches" not in want:
        for k in ("one", "two", "four", "eight"):
            want.setdefault(k, 0)
        want.setdefault("windows_cut", 0)
    for k in ("multi_block", "multi_block_wlist"):
        want.setdefault(k, 0)
    if want["multi_block"]:
        want.setdefault("launches", 0)
    for k, v in want.items():
        lo, hi = v if isinstance(v, tuple) else (v, v)
        assert lo <= got[k] <= hi, (what, k, got, want)


def _assert_against(got, probs, want, what, oracle):
    v, z, tl = got
    wv, wz, wtl, wprobs = want
    assert z.tolist() == wz.tolist() and tl == wtl, what
    assert abs(v - wv) <= (1e-9 if oracle else 1e-13) * abs(wv), (what, v, wv)
    np.testing.assert_allclose(probs, wprobs, rtol=4e-16, atol=0, err_msg=what)


def _check_lists(c, rs, what):
    r = c.debug_delta_check(rs)
    print(f"{what}: {r}")
    assert r["rc"] == 0 and r["mismatches"] == 0 and r["compared"] > 0, (what, r)
    return r


def _walk(sc_name, fix, steps, expect, oracle_steps, with_rebuilt=True):
    """the three contexts over `steps`; returns them with the per-step kind counters of the default context"""
    knobs = [None, {"DELTA_ONE_BLOCK": 1}] + ([{"DELTA_POLICY": 1}] if with_rebuilt else [])  # (1: api.DeltaPolicy.NO_LISTS)
    ctxs = [_ctx(fix, k) for k in knobs]
    kinds = []
    for k, paths in enumerate(steps):
        before = [c.debug_delta_routes(rs) for c, rs in ctxs[:2]]
        vals = [c.calc_prob(paths) for c, _ in ctxs]
        probs = [c.read_probs(rs) for c, rs in ctxs]
        what = f"{sc_name} step {k}"
        for i, (c, rs) in enumerate(ctxs[:2]):
            after = c.debug_delta_routes(rs)
            step = _route_step(before[i], after)
            print(f"{what}, {'DELTA_ONE_BLOCK' if i else 'default'}: {after['last_records'] if k else 0} records in {after['last_windows'] if k else 0} windows, launches {step}")
            if k > 0:
                _assert_route(step, expect[k - 1][i], what)
                lo, hi = expect[k - 1][2]  # the activation is what the CPU test measured for this step
                assert lo <= after["last_records"] <= hi, (what, after)
            r = _check_lists(c, rs, f"{what}, {'DELTA_ONE_BLOCK' if i else 'default'}")
            if k > 0:
                assert r["on_lists"] > 0, (what, r)
            if i == 0:
                kinds.append(r)
        # the lists are the same records in the same order, whichever launches wrote them: equal bits per read (the
        # numbering, and with it the order of the final sum, may differ)
        assert np.array_equal(probs[0], probs[1]), what
        assert vals[0][1].tolist() == vals[1][1].tolist() and vals[0][2] == vals[1][2] and abs(vals[0][0] - vals[1][0]) <= 1e-13 * abs(vals[1][0]), what
        if with_rebuilt:
            _assert_against(vals[0], probs[0], (vals[2][0], vals[2][1], vals[2][2], probs[2]), what + " against rebuilt tables", oracle=False)
            st = ctxs[2][0].table_stats(ctxs[2][1])
            assert st["delta_updates"] == 0 and st["dirty_pairs"] == 0, st
        if k in oracle_steps:
            _assert_against(vals[0], probs[0], _want(fix, paths), what + " against the oracle", oracle=True)
    return ctxs, kinds


def _batch_compact_close(sc_name, fix, ctxs, sets):
    """the last step once more through calc_prob_batch with two earlier sets (the delta body of the batch kernel, the
    wave-per-pair path over spill lists): bit-equal to single calls; then the lists folded into the tables"""
    for i, (c, rs) in enumerate(ctxs[:2]):
        what = f"{sc_name} {'DELTA_ONE_BLOCK' if i else 'default'}"
        batch = c.calc_prob_batch(sets)
        for (bv, bz, btl), paths in zip(batch, sets):
            sv, sz, stl = c.calc_prob(paths)
            assert bv == sv and bz.tolist() == sz.tolist() and btl == stl, (what, bv, sv)
        v, z, tl = c.calc_prob(sets[0])
        probs = c.read_probs(rs)
        _check_lists(c, rs, what + " after the batch")
        c.compact_tables()
        v2, z2, tl2 = c.calc_prob(sets[0])
        assert c.table_stats(rs)["dirty_pairs"] == 0
        t = c.debug_tables_check(rs)
        assert t["mismatches"] == 0 and t["compared"] > 0, t
        np.testing.assert_allclose(c.read_probs(rs), probs, rtol=4e-16, atol=0)
        assert z2.tolist() == z.tolist() and tl2 == tl and abs(v2 - v) <= 1e-13 * abs(v)
    for c, _ in ctxs:
        c.close()


def _expect(sc):
    return [(d, k22, (rlo, rhi)) for rlo, rhi, _, _, d, k22 in sc.expect]


@pytest.mark.parametrize("sc", [s for s in dc.scenarios() if s.fixture != "large"], ids=repr)
def test_scenario_routes_lists_and_values(sc):
    ctxs, kinds = _walk(sc.name, sc.fixture, sc.steps, _expect(sc), oracle_steps=range(len(sc.steps)))
    last = kinds[-1]
    if sc.name == "small-junction-walk":  # both strands of everything: every aligned pair is on the lists, some with 3 to 4 records
        assert last["on_lists"] > 2000 and last["stride_2"] > 0 and last["stride_4"] > 0 and last["left_out"] > 0, last
    if sc.name == "medium-pieces":  # the tables hold every class: pairs come to the lists from those with 2, 3 to 4 and more records
        assert last["from_two"] > 0 and last["from_four"] > 0 and last["from_more"] > 0 and last["left_out"] > 0, last
    else:
        assert last["from_static"] > 0, last  # pairs without a record in the tables: new to the lists from the compact class's static part
    sets = [sc.steps[-1], sc.steps[0], sc.steps[-2] if len(sc.steps) > 2 else sc.steps[0][1:]]
    _batch_compact_close(sc.name, sc.fixture, ctxs, sets)


def test_large_activation_two_multi_block_launches():
    """53,149 records of 64 windows at once: two multi-block launches (49,152 records, then the rest; the window at the
    cut in both) by default, seven one-block launches with DELTA_ONE_BLOCK. The oracle is called once, on the final set."""
    sc = dc.scenario("large-0-31")
    ctxs, kinds = _walk(sc.name, sc.fixture, sc.steps, _expect(sc), oracle_steps=(len(sc.steps) - 1,))
    assert kinds[-1]["on_lists"] > 20_000, kinds[-1]
    _batch_compact_close(sc.name, sc.fixture, ctxs, [sc.steps[-1], sc.steps[0], sc.steps[0][1:]])


def test_spill_lists_are_made_grow_and_double():
    """The medium fixture's repeat: pairs fresh from the more-than-2-records classes, lists that move from the fixed
    stride to the spill area, spill lists that grow twice; then an annealing walk over pairs that are on the lists."""
    steps = dc.spill_steps()
    expect = [(d, k22, rec) for (d, k22), rec in zip(dc.SPILL_ROUTES, dc.SPILL_RECORDS)]
    ctxs, kinds = _walk("spill", "medium", steps, expect, oracle_steps=range(len(steps)))
    assert kinds[0]["on_lists"] == 0
    # step 1: the repeat's reads come from the more-than-4-records class (3 records a mate: folded into it) to a full stride
    assert kinds[1]["from_more"] >= 100 and kinds[1]["stride_4"] >= 100 and kinds[1]["long_lists"] == 0, kinds[1]
    assert kinds[1]["from_static"] > 0 and kinds[1]["from_two"] > 0, kinds[1]
    assert kinds[2]["long_lists"] >= 100, kinds[2]                         # step 2: from the stride to the spill area
    assert kinds[3]["long_lists"] > kinds[2]["long_lists"], kinds[3]       # step 3: more of them, the earlier ones longer
    assert kinds[4]["long_lists"] >= kinds[3]["long_lists"], kinds[4]
    # step 4, the twins: also pairs whose mates lie in two windows (a fragment across a short node: the compact class's other part)
    assert kinds[4]["from_compact"] > 0, kinds[4]
    walk = dc.sa_walk_steps()
    moved = 0
    for k, paths in enumerate(walk):
        before = [c.debug_delta_routes(rs) for c, rs in ctxs[:2]]
        vals = [c.calc_prob(paths) for c, _ in ctxs]
        probs = [c.read_probs(rs) for c, rs in ctxs]
        what = f"annealing step {k}"
        after = [c.debug_delta_routes(rs) for c, rs in ctxs[:2]]
        for i in range(2):
            step = _route_step(before[i], after[i])
            assert step["multi_block"] == 0 and step["launches"] <= 1, (what, step)  # (a move activates a junction or a twin: a few hundred records)
            moved += step["launches"]
        assert np.array_equal(probs[0], probs[1]) and vals[0][1].tolist() == vals[1][1].tolist() and abs(vals[0][0] - vals[1][0]) <= 1e-13 * abs(vals[1][0]), what
        _assert_against(vals[0], probs[0], (vals[2][0], vals[2][1], vals[2][2], probs[2]), what + " against rebuilt tables", oracle=False)
        if k % 8 == 7 or k == len(walk) - 1:
            for i, (c, rs) in enumerate(ctxs[:2]):
                assert _check_lists(c, rs, f"{what}, {'DELTA_ONE_BLOCK' if i else 'default'}")["long_lists"] >= 100
            _assert_against(vals[0], probs[0], _want("medium", paths), what + " against the oracle", oracle=True)
    assert moved >= 10  # (five or more activating moves, two contexts)
    _batch_compact_close("spill", "medium", ctxs, [walk[-1], steps[-1], steps[2]])


@pytest.mark.parametrize("name", ["medium-0-4", "large-0-31"])
def test_multi_block_numbering_is_a_function_of_the_input(name):
    """Bins are filled by atomics; the order inside them must not reach the numbering (delta index, spill index) or the
    value: two fresh contexts, equal bits."""
    sc = dc.scenario(name)
    runs = []
    for rep in range(2):
        c, rs = _ctx(sc.fixture)
        vals = [c.calc_prob(paths)[0] for paths in sc.steps]
        assert c.debug_delta_routes(rs)["multi_block"] >= 1
        reads, spill = c.debug_delta_numbering(rs)
        runs.append((vals, reads.copy(), spill.copy(), c.read_probs(rs)))
        c.close()
    assert runs[0][0] == runs[1][0]
    assert len(runs[0][1]) > 1000 and np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])
    assert len(np.unique(runs[0][1])) == len(runs[0][1])  # a pair has one index
    assert np.array_equal(runs[0][3], runs[1][3])


# ---- a full store: the spill area with room for 64 long lists (DELTA_SPILL_CAP), the medium fixture's repeat needs 665 at step 2
def _overflow_ctx():
    c, rs = _ctx("medium", {"DELTA_SPILL_CAP": 64})
    steps = dc.spill_steps()
    for paths in steps[:2]:
        v, z, tl = c.calc_prob(paths)
        _assert_against((v, z, tl), c.read_probs(rs), _want("medium", paths), "before the overflow", oracle=True)
    assert _check_lists(c, rs, "before the overflow")["long_lists"] == 0
    return c, rs, steps


def _off_repeat_steps(base):
    """two more activations that make no long list: the twins of the first two long nodes (no copy of the repeat)"""
    _, _, longs = dc.fixture("medium")
    return [base + [[longs[0] ^ 1]], base + [[longs[0] ^ 1], [longs[1] ^ 1]]]


def test_overflow_blocking_call_reports_and_recovers():
    from gaml_amd import api
    c, rs, steps = _overflow_ctx()
    with pytest.raises(api.GamlHipError) as e:  # the 65th long list: the launch changes nothing and raises the flag
        c.calc_prob(steps[2])
    assert e.value.code == api.ESTATE and "gaml_hip_compact_tables" in str(e.value), e.value
    c.compact_tables()
    v, z, tl = c.calc_prob(steps[2])
    _assert_against((v, z, tl), c.read_probs(rs), _want("medium", steps[2]), "after compact_tables", oracle=True)
    r = _check_lists(c, rs, "after compact_tables")
    assert r["on_lists"] == 0 and c.table_stats(rs)["dirty_pairs"] == 0
    for k, paths in enumerate(_off_repeat_steps(steps[2])):  # the context goes on working
        v, z, tl = c.calc_prob(paths)
        _assert_against((v, z, tl), c.read_probs(rs), _want("medium", paths), f"step {k} after the overflow", oracle=True)
        assert _check_lists(c, rs, f"step {k} after the overflow")["on_lists"] > 0
    c.close()


def test_overflow_batch_reports_or_scores_every_record():
    """The same store, filled by the maintenance launch of a batch: an error, or the oracle's values -- never values that
    lack the records the launch could not take in."""
    from gaml_amd import api
    c, rs, steps = _overflow_ctx()
    sets = [steps[2], steps[1], steps[0]]
    try:
        got = c.calc_prob_batch(sets)
    except api.GamlHipError as e:
        print("batch over a full store:", e)
        assert e.code == api.ESTATE and "gaml_hip_compact_tables" in str(e), e
        got = None
    if got is not None:
        for (v, z, tl), paths in zip(got, sets):
            wv, wz, wtl, _ = _want("medium", paths)
            print(f"batch over a full store returned {v!r}, oracle {wv!r}")
            assert z.tolist() == wz.tolist() and tl == wtl and abs(v - wv) <= 1e-9 * abs(wv), (v, wv)
    c.compact_tables()
    for (v, z, tl), paths in zip(c.calc_prob_batch(sets), sets):
        wv, wz, wtl, _ = _want("medium", paths)
        assert z.tolist() == wz.tolist() and tl == wtl and abs(v - wv) <= 1e-9 * abs(wv), (v, wv)
    _check_lists(c, rs, "batch after compact_tables")
    c.close()


def test_overflow_gap_profile_reports_or_scores_every_record():
    from gaml_amd import api
    c, rs, steps = _overflow_ctx()
    # step 2's set with a gap between its first two paths: the same windows, the same maintenance launch
    paths = [steps[2][0] + [-150] + steps[2][1]] + steps[2][2:]
    lens = [100, 150, 220]
    want = [_want("medium", [paths[0][:1] + [-l] + paths[0][2:]] + paths[1:]) for l in lens]

    def same(got):
        for (v, z, tl), (wv, wz, wtl, _) in zip(got, want):
            print(f"gap profile returned {v!r}, oracle {wv!r}")
            assert z.tolist() == wz.tolist() and tl == wtl and abs(v - wv) <= 1e-9 * abs(wv), (v, wv)
    try:
        got = c.gap_profile(paths, 0, 1, lens)
    except api.GamlHipError as e:
        print("gap profile over a full store:", e)
        assert e.code == api.ESTATE and "gaml_hip_compact_tables" in str(e), e
        got = None
    if got is not None:
        same(got)
    c.compact_tables()
    same(c.gap_profile(paths, 0, 1, lens))
    _check_lists(c, rs, "gap profile after compact_tables")
    c.close()
