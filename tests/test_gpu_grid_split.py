"""How the scoring kernels deal their work out to blocks, lanes, waves and rounds (tests/grid_split_cases.py, held to what
it claims by tests/test_grid_split_host.py). The grid-cap knobs of the development build bring every class of
paired_score_kernel, and every launch sized by grid_for, down to 1-3 blocks, so that a case of a few thousand reads runs
every stride loop for three rounds and more with a ragged last one -- the `more` / `nbase` refill and the clamped tail of
paired_static4_body, the pipelined pairs of paired_compact_body, the wave votes of the classes with several records while
some lanes have left the loop, the item-to-wave assignment of the wave-per-pair blocks, the ticket groups of grid_finish.

Every capped call is held to
  * the launch it was meant to be: debug_block_partials shows every class at its capped block count, and the rounds that
    follow from the layout and the class sizes are three or more;
  * an uncapped twin context on the same puts and calls: per-read values bit for bit (which lane, round or wave scores a
    pair does not change that pair's arithmetic), the value within 1e-13 (two orders of the same additions,
    tests/test_gpu_batch.py);
  * the oracle: per read within 4e-16, floored counts and total length equal, the value within 1e-12
    (tests/test_gpu_crafted_records.py);
  * every pair exactly once: the per-block floored counts are those the case's slot order predicts and sum to the call's.
Before the capped call the context scores a path set under which no pair scores: every per-read value is 0.0 then, a
skipped slot shows as 0.0 where the reference is positive. Messages name case, part, slot and read.

Worst differences met (MI355X): per read 0 against the oracle (every value equal), the value 1.1e-14 against the oracle and
1.6e-16 against the uncapped twin ("The work split under capped grids")."""
from functools import lru_cache

import numpy as np
import pytest

import crafted_records_cases as cc
import grid_split_cases as gs

pytestmark = pytest.mark.gpu

RTOL = 4e-16        # per-read probabilities (the project's bound)
VALUE_ORACLE = 1e-12
VALUE_TWIN = 1e-13
PATHS = {"main": gs.S_MAIN, "gen": gs.S_GEN}
# (case, path set): each another body or instantiation of paired_score_kernel
VARIANTS = [("split_one_combo", "main"), ("split_two_combos", "main"), ("split_no_memo", "main"), ("split_penalty", "main"),
            ("split_penalty_general", "main"), ("split_one_combo", "gen")]
SETS_CAP = {"all1": 1, "all3": 3, "mixed": 2}  # GRID_CAP_SETS beside the class caps: the coverage sweeps


def _knobs(case, caps):
    from gaml_amd import api
    out = [(api.Knob[name], v) for name, v in case.knobs]
    if caps is not None:
        out += [(api.Knob[gs.KNOB_OF_PART[part]], v) for part, v in gs.CAPS[caps].items()] + [(api.Knob.GRID_CAP_SETS, SETS_CAP[caps])]
    return tuple(out)


@lru_cache(maxsize=None)
def _built(name):
    return cc.Built(gs.split_case(name))


@lru_cache(maxsize=None)
def _where(name):
    """read -> (part, slot) in the case's slot order (a delta pair: its slot in the static part)"""
    case, b = gs.split_case(name), _built(name)
    return {b.first[n]: (part, k) for part in ("static", "rest", "two", "four", "more") for k, n in enumerate(case.order.get(part, ()))}


def _label(name, rid):
    part, slot = _where(name)[rid]
    delta = " (delta pair)" if _built(name).who[rid][0].startswith("delta") else ""
    return f"{name}, {part} slot {slot}{delta}, read {rid}"


@lru_cache(maxsize=None)
def _oracle(name, paths_key):
    case, b = gs.split_case(name), _built(name)
    o, ors = b.oracle()
    v, z, tl = o.calc_prob(PATHS[paths_key], fresh=True)
    probs, bad = o.paired_probs(ors)
    assert o.windows_aligned(ors, 0) == 0 and o.windows_aligned(ors, 1) == 0
    return v, z.tolist(), tl, probs, bad


def _score(name, paths_key, caps):
    """tables under [A]; a set under which nothing scores (every per-read value 0.0); then the call under test"""
    case, b = gs.split_case(name), _built(name)
    ctx, rs = b.library(knobs=_knobs(case, caps))
    ctx.calc_prob(gs.S_BUILD)
    classes = ctx.pair_classes(rs).tolist()
    static = ctx.table_stats(rs)["static_index_pairs"]
    ctx.calc_prob(gs.S_NONE)
    assert not ctx.read_probs(rs).any(), f"{name}: values left under a path set without a window of the case"
    v, z, tl = ctx.calc_prob(PATHS[paths_key])
    sums, zeros, lay = ctx.debug_block_partials(rs)
    out = dict(v=v, z=z.tolist(), tl=tl, probs=ctx.read_probs(rs).copy(), sums=sums, zeros=zeros, lay=lay, classes=classes, static=static,
               bad=ctx.bad_bases(rs), delta=ctx.debug_delta_check(rs))
    assert ctx.aligner_stats()["windows"] == 0
    ctx.close()
    return out


@lru_cache(maxsize=None)
def _twin(name, paths_key):
    return _score(name, paths_key, None)


def _part_blocks(lay):
    b0a, b0, b01, b012, main, total = lay[:6]
    return dict(static=b0a, rest=b0 - b0a, two=b01 - b0, four=b012 - b01, delta=main - b012, more=total - main)


def _part_sizes(r):
    return dict(static=r["static"], rest=r["classes"][0] - r["static"], two=r["classes"][1], four=r["classes"][2], delta=r["delta"]["on_lists"],
                more=r["classes"][3] + r["delta"]["long_lists"])


def _bits(name, got, want, what):
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    assert bad.size == 0, f"{what}: {_label(name, int(bad[0]))}: {got[bad[0]]!r} != {want[bad[0]]!r} ({bad.size} reads differ)"
    return 0.0


def _close(name, got, want, what):
    err = np.abs(got - want)
    bad = np.flatnonzero(~(err <= RTOL * np.abs(want)))
    assert bad.size == 0, f"{what}: {_label(name, int(bad[0]))}: library {got[bad[0]]!r}, oracle {want[bad[0]]!r} ({bad.size} reads differ)"
    nz = want > 0
    return float((err[nz] / want[nz]).max())


def _predicted_block_zeros(name, blocks, no_memo):
    """floored pairs per block from the case's slot order (the delta pairs: only their sum; the long lists ride with the
    wave-per-pair items behind the table pairs)"""
    case, b = gs.split_case(name), _built(name)
    floored = set(case.floored)
    order = {part: list(case.order[part]) for part in ("static", "rest", "two", "four", "more")}
    if no_memo:  # one class 0, the pairs without a record at its end
        order["rest"] = order["static"][:-3] + order["rest"] + order["static"][-3:]
        order["static"] = []
    deltas = set(case.order["delta"])
    out = {}
    for part in ("static", "rest", "two", "four", "more"):
        per = np.zeros(blocks[part], np.int64)
        for slot, n in enumerate(order[part]):
            if n in floored and n not in deltas:
                per[gs.block_of_slot(slot, blocks[part], gs.PER_ROUND[part])] += 1
        out[part] = per.tolist()
    return out, sum(1 for n in deltas if n in floored)


@pytest.mark.parametrize("caps", list(gs.CAPS))
@pytest.mark.parametrize("name,paths_key", VARIANTS, ids=[f"{n}-{p}" for n, p in VARIANTS])
def test_capped_call(name, paths_key, caps):
    case = gs.split_case(name)
    what = f"{name} under {paths_key}, caps {caps}"
    no_memo = ("NO_MEMO", 1) in case.knobs
    got, twin = _score(name, paths_key, caps), _twin(name, paths_key)
    wv, wz, wtl, wprobs, wbad = _oracle(name, paths_key)
    # ---- the launch is the one intended
    blocks, sizes = _part_blocks(got["lay"]), _part_sizes(got)
    want_blocks = dict(gs.CAPS[caps], static=0) if no_memo else dict(gs.CAPS[caps])
    assert blocks == want_blocks, (what, got["lay"])
    assert len(got["sums"]) == got["lay"][5] == got["lay"][7] == sum(blocks.values()), (what, got["lay"])
    assert sizes == case.sizes(no_memo) and got["classes"] == case.expected_classes(), (what, sizes, got["classes"])
    assert got["delta"]["mismatches"] == 0 and got["delta"]["from_static" if not no_memo else "from_compact"] == gs.N_DELTA, (what, got["delta"])
    for part in gs.PARTS:
        if blocks[part]:
            r = gs.rounds(sizes[part], blocks[part], gs.PER_ROUND[part])[0]
            assert r >= 3, f"{what}: {part} makes {r} rounds in {blocks[part]} blocks"
    tb = _part_blocks(twin["lay"])
    assert all(tb[part] > gs.CAPS[caps][part] for part in gs.PARTS if blocks[part]), (what, twin["lay"])  # the caps do lower the grid
    # ---- per read: the uncapped twin's bits, the oracle's value
    _bits(name, got["probs"], twin["probs"], f"{what}: capped against uncapped")
    worst = _close(name, got["probs"], wprobs, what)
    # ---- every pair exactly once
    assert got["z"] == wz == twin["z"] and got["tl"] == wtl, (what, got["z"], wz)
    rel_o, rel_t = abs(got["v"] - wv) / abs(wv), abs(got["v"] - twin["v"]) / abs(twin["v"])
    print(f"{what}: value {got['v']!r}, oracle {rel_o:.2e}, twin {rel_t:.2e}, worst read {worst:.2e}, layout {got['lay']}")
    assert rel_o <= VALUE_ORACLE and rel_t <= VALUE_TWIN, (what, got["v"], wv, twin["v"])
    assert int(got["zeros"].sum()) == got["z"][0][0] == len(case.floored), (what, got["zeros"].tolist())
    pred, pred_delta = _predicted_block_zeros(name, blocks, no_memo)
    at = 0
    for part in gs.PARTS:
        have = got["zeros"][at:at + blocks[part]].tolist()
        at += blocks[part]
        if part == "delta":
            assert sum(have) == pred_delta, f"{what}: floored delta pairs per block {have}, {pred_delta} declared"
        else:
            assert have == pred[part], f"{what}: floored pairs per block of {part}: {have}, the slot order gives {pred[part]}"
    if case.cfg["penalty_constant"] > 0:
        assert got["bad"] == wbad == twin["bad"] == _expected_bad(name, paths_key) > 0, (what, got["bad"], wbad)


@lru_cache(maxsize=None)
def _expected_bad(name, paths_key):
    return cc.expected_bad_bases(gs.split_case(name), PATHS[paths_key])[0]


@pytest.mark.parametrize("name", ["static_1024", "static_1025"])
def test_static_part_at_the_round_boundary(name):
    """One block, one round of 1,024 slots exactly (`more` is false at the boundary), and one slot more (a second round in
    which lane 0 alone has a pair and every index of its refill but the first is clamped)."""
    from gaml_amd import api
    case, b = gs.split_case(name), _built(name)
    o, ors = b.oracle()
    wv, wz, wtl = o.calc_prob(gs.S_BUILD, fresh=True)
    wprobs, _ = o.paired_probs(ors)
    res = []
    for cap in (1, 0):
        ctx, rs = b.library(knobs=((api.Knob.GRID_CAP_COMPACT, cap),))
        ctx.calc_prob(gs.S_BUILD)
        ctx.calc_prob(gs.S_NONE)
        assert not ctx.read_probs(rs).any()
        v, z, tl = ctx.calc_prob(gs.S_BUILD)
        sums, zeros, lay = ctx.debug_block_partials(rs)
        res.append((v, z.tolist(), ctx.read_probs(rs).copy(), lay, zeros))
        assert ctx.table_stats(rs)["static_index_pairs"] == case.n_reads() and ctx.pair_classes(rs).tolist() == case.expected_classes()
        ctx.close()
    (v, z, probs, lay, zeros), (tv, tz, tprobs, tlay, _) = res
    assert lay[0] == 1 and tlay[0] == -(-case.n_reads() // 512) and gs.rounds(case.n_reads(), 1, 1024)[0] == (1 if name == "static_1024" else 2)
    _bits(name, probs, tprobs, f"{name}: one block against {tlay[0]}")
    _close(name, probs, wprobs, name)
    assert z == wz.tolist() == tz and z[0][0] == len(case.floored) == int(zeros.sum())
    assert abs(v - wv) <= VALUE_ORACLE * abs(wv) and abs(v - tv) <= VALUE_TWIN * abs(tv)


BATCH_SETS = [gs.S_MAIN, gs.S_MAIN[::-1], gs.S_BUILD, [[cc.B]], gs.S_GEN, [[cc.B], [cc.A], [cc.A]], gs.S_NONE, gs.S_MAIN]


@pytest.mark.parametrize("caps", list(gs.CAPS))
@pytest.mark.parametrize("name", ["split_one_combo", "split_two_combos", "split_penalty"])
def test_batch_under_caps_gives_the_blocking_calls_bits(name, caps):
    """paired_score_multi_kernel takes its grid from the same paired_base_args: eight sets in one pass under the caps give
    the bits of eight blocking calls under the caps, and agree with the oracle. Both contexts have made the same calls
    before (tables under [A], then [B] activated: the same delta lists)."""
    case, b = gs.split_case(name), _built(name)
    cov = case.cfg["penalty_constant"] > 0
    ctxs = []
    for _ in range(2):
        ctx, rs = b.library(knobs=_knobs(case, caps))
        for s in (gs.S_BUILD, gs.S_NONE, gs.S_MAIN):
            ctx.calc_prob(s)
        ctxs.append((ctx, rs))
    (many, rs), (one, rs1) = ctxs
    want = []
    for s in BATCH_SETS:
        v, z, tl = one.calc_prob(s)
        want.append((v, z.tolist(), tl, one.bad_bases(rs1) if cov else 0))
    before = many.table_stats(rs)
    got = many.calc_prob_batch(BATCH_SETS)
    after = many.table_stats(rs)
    assert after["batches_patched"] + after["batches_full"] > before["batches_patched"] + before["batches_full"], (name, before, after)  # one pass, not eight calls
    o, ors = b.oracle()
    for k, ((v, z, tl), (wv, wz, wtl, wbad)) in enumerate(zip(got, want)):
        what = f"{name}, caps {caps}, batch entry {k}"
        assert tl == wtl and z.tolist() == wz, (what, z.tolist(), wz)
        assert v == wv, (what, v, wv)
        ov, oz, otl = o.calc_prob(BATCH_SETS[k], fresh=True)
        assert oz.tolist() == wz and otl == tl and (v == ov or abs(v - ov) <= VALUE_ORACLE * abs(ov)), (what, v, ov)
        if cov:
            assert o.paired_probs(ors)[1] == wbad, what
    if cov:
        assert many.debug_batch_bad_bases(rs) == [w[3] for w in want], name
    sums, zeros, lay = many.debug_block_partials(rs, len(BATCH_SETS) - 1)
    assert _part_blocks(lay) == gs.CAPS[caps] and int(zeros.sum()) == want[-1][1][0][0], (name, caps, lay)
    _bits(name, many.read_probs(rs), one.read_probs(rs1), f"{name}, caps {caps}: the batch's last set")
    for ctx, _ in ctxs:
        assert ctx.aligner_stats()["windows"] == 0
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# launches sized by grid_for: single-end, PacBio, coverage sweeps
# ---------------------------------------------------------------------------------------------------------------------
def _single_run(b, cap, onepass=False):
    from gaml_amd import api
    ctx, rs = b.library(knobs=((api.Knob.GRID_CAP_SETS, cap),) if cap else ())
    if onepass:
        ctx.set_single_onepass(True)
    return ctx, rs


@lru_cache(maxsize=None)
def _single_built(n):
    return cc.Built(gs.single_case(n))


@pytest.mark.parametrize("blocks", gs.BLOCK_COUNTS)
def test_single_end_under_caps(blocks):
    """A launch of `blocks` blocks by its read count, and the same reads under GRID_CAP_SETS 1 and 3 (the largest case also
    at every other block count of the list, reached by the cap): per read the uncapped launch's bits and the oracle's value,
    floored counts exact, values within bound; then a batch of eight sets through single_score_multi_kernel."""
    n = gs.SINGLE_READS[blocks]
    b = _single_built(n)
    case = b.case
    o, ors = b.oracle()
    want = [o.single_detail(ors, s) for s in gs.SINGLE_SETS]
    caps = (0,) + gs.SET_CAPS + (tuple(c for c in gs.BLOCK_COUNTS if c not in gs.SET_CAPS and c < blocks) if blocks == 33 else ())
    twin = None
    for cap in caps:
        ctx, rs = _single_run(b, cap)
        res = []
        for s in gs.SINGLE_SETS:  # (before each the set under which nothing scores: a skipped read would keep its 0.0)
            ctx.calc_prob(gs.SINGLE_SETS[3])
            assert not ctx.read_probs(rs).any(), (case.name, cap)
            v, z, tl = ctx.calc_prob(s)
            res.append((v, z.tolist(), tl, ctx.read_probs(rs).copy()))
        if twin is None:
            twin = res
        for k, ((v, z, tl, probs), (wv, wprobs, o3), (tv, tz, ttl, tprobs)) in enumerate(zip(res, want, twin)):
            what = f"{case.name}, set {k}, GRID_CAP_SETS {cap}"
            bad = np.flatnonzero(probs.view(np.uint64) != tprobs.view(np.uint64))
            assert bad.size == 0, f"{what}: read {bad[0]} (lane {bad[0] % 256}, trip {bad[0] // (256 * max(cap, 1))}): {probs[bad[0]]!r} != {tprobs[bad[0]]!r} ({bad.size} differ)"
            bad = np.flatnonzero(~(np.abs(probs - wprobs) <= RTOL * np.abs(wprobs)))
            assert bad.size == 0, f"{what}: read {bad[0]}: library {probs[bad[0]]!r}, oracle {wprobs[bad[0]]!r} ({bad.size} differ)"
            assert z == tz == [[int(o3[0]), n]] and tl == ttl == int(o3[1]), (what, z, o3.tolist())
            assert v == wv or abs(v - wv) <= VALUE_ORACLE * abs(wv), (what, v, wv)
            assert v == tv or abs(v - tv) <= VALUE_TWIN * abs(tv), (what, v, tv)
        ctx.close()
    sets = cc.batch_sets(case)
    for cap in gs.SET_CAPS:
        (many, rs), (one, rs1) = _single_run(b, cap, onepass=True), _single_run(b, cap)
        got = many.calc_prob_batch(sets)
        for k, (s, (v, z, tl)) in enumerate(zip(sets, got)):
            wv, wz, wtl = one.calc_prob(s)
            assert (v, z.tolist(), tl) == (wv, wz.tolist(), wtl), (case.name, cap, k, v, wv)
            ov, oz, otl = o.calc_prob(s, fresh=True)
            assert oz.tolist() == z.tolist() and otl == tl and (v == ov or abs(v - ov) <= VALUE_ORACLE * abs(ov)), (case.name, cap, k, v, ov)
        assert np.array_equal(many.read_probs(rs), one.read_probs(rs1))
        assert many.single_stats(rs)["multi_launches"] == 1 and one.single_stats(rs1)["multi_launches"] == 0
        many.close()
        one.close()


@pytest.mark.parametrize("blocks", gs.BLOCK_COUNTS)
def test_pacbio_under_caps(blocks):
    """The same for the PacBio scorer, one read per wave: records per read on both sides of a wave's 64 lanes, sub-walk
    counts 0, 1 and 3; per read the uncapped launch's bits, the oracle's within 1e-12 (tests/test_gpu_pacbio_batch.py);
    with a coverage penalty bad_bases is the oracle's under every cap; a batch through pacbio_score_multi_kernel."""
    from gaml_amd import api
    n = gs.PACBIO_READS[blocks]
    pc = gs.pacbio_case(n)
    caps = (0,) + gs.SET_CAPS + (tuple(c for c in gs.BLOCK_COUNTS if c not in gs.SET_CAPS and c < blocks) if blocks == 33 else ())
    for penalty in (0.0, 0.0001):
        o, ors = pc.oracle(penalty)
        want = [o.pacbio_detail(ors, s) for s in gs.PACBIO_SETS]
        twin = None
        for cap in caps:
            ctx, rs = pc.library(knobs=((api.Knob.GRID_CAP_SETS, cap),) if cap else (), penalty=penalty)
            res = []
            for s in gs.PACBIO_SETS:  # (before each the set under which no read has an alignment: every value -inf)
                ctx.calc_prob(gs.PACBIO_SETS[3])
                assert not np.isfinite(ctx.read_probs(rs)).any(), (n, cap)
                v, z, tl = ctx.calc_prob(s)
                res.append((v, z.tolist(), tl, ctx.read_probs(rs).copy(), ctx.bad_bases(rs)))
            if twin is None:
                twin = res
            for k, ((v, z, tl, lp, bad), (wv, wlp, o3), (tv, tz, ttl, tlp, tbad)) in enumerate(zip(res, want, twin)):
                what = f"pacbio{n}, penalty {penalty}, set {k}, GRID_CAP_SETS {cap}"
                diff = np.flatnonzero(lp.view(np.uint64) != tlp.view(np.uint64))
                assert diff.size == 0, f"{what}: read {diff[0]} (wave {diff[0] % (4 * max(cap, 1))}): {lp[diff[0]]!r} != {tlp[diff[0]]!r} ({diff.size} differ)"
                fin = np.isfinite(wlp)
                assert (np.isfinite(lp) == fin).all(), what
                np.testing.assert_allclose(lp[fin], wlp[fin], rtol=1e-12, atol=0, err_msg=what)
                assert z == tz == [[int(o3[0]), n]] and tl == ttl == int(o3[1]), (what, z, o3.tolist())
                assert bad == tbad == (int(o3[2]) if penalty > 0 else 0), (what, bad, tbad, int(o3[2]))  # (without a penalty the library does not sweep)
                assert v == wv or abs(v - wv) <= VALUE_ORACLE * abs(wv), (what, v, wv)
                assert v == tv or abs(v - tv) <= VALUE_TWIN * abs(tv), (what, v, tv)
            ctx.close()
    sets = gs.PACBIO_SETS + [s[::-1] for s in gs.PACBIO_SETS]
    o, ors = pc.oracle()
    for cap in gs.SET_CAPS:
        (many, rs), (one, rs1) = pc.library(knobs=((api.Knob.GRID_CAP_SETS, cap),)), pc.library(knobs=((api.Knob.GRID_CAP_SETS, cap),))
        got = many.calc_prob_batch(sets)
        for k, (s, (v, z, tl)) in enumerate(zip(sets, got)):
            wv, wz, wtl = one.calc_prob(s)
            assert (v, z.tolist(), tl) == (wv, wz.tolist(), wtl), (n, cap, k, v, wv)
            ov, _, o3 = o.pacbio_detail(ors, s)
            assert z.tolist() == [[int(o3[0]), n]] and (v == ov or abs(v - ov) <= VALUE_ORACLE * abs(ov)), (n, cap, k, v, ov)
        assert np.array_equal(many.read_probs(rs), one.read_probs(rs1))
        assert many.pacbio_stats(rs)["multi_launches"] == 1 and one.pacbio_stats(rs1)["multi_launches"] == 0
        many.close()
        one.close()
