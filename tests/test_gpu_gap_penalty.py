"""gaml_hip_gap_profile / gaml_hip_fix_gap_length on the device route for read sets WITH a coverage penalty
(Context.set_gap_penalty_device): every length's coverage layout is derived on the device beside its tables
(gap_tables_kernel's third grid row), every length marks into a bitmap of its own and one sweep serves a pass. Checked on
the inputs of tests/gap_penalty_cases.py, where bad_bases is positive and depends on the gap's length: routes, values
against batches, single calls and the oracle, the derived layouts against what the host lays out for the same set, the
search against the reference's over the oracle, and what a profile leaves behind."""
import numpy as np
import pytest

import gap_oracle as go
import gap_penalty_cases as gp

pytestmark = pytest.mark.gpu

# (case, libraries, trimmed reads, library A's penalty)
CONFIGS = [(name, "B", False, gp.PENALTY_A) for name in gp.cases()] + [
    ("site 81, edited first", "B", True, gp.PENALTY_A),            # several length codes
    ("site 81, edited in the middle", "AB", False, gp.PENALTY_A),  # B beside A, both penalised
    ("site 81, edited first", "AB", False, 0.0),                   # B beside A, A without a penalty
]


def _bads(c, n):
    bads = [c.debug_batch_bad_bases(r) for r in range(c.num_readsets())]
    assert all(len(b) == n for b in bads), (n, [len(b) for b in bads])
    return [[int(bads[r][k]) for r in range(len(bads))] for k in range(n)]


def _profile(c, paths, path_id, gap_pos, lens):
    got = c.gap_profile(paths, path_id, gap_pos, lens)
    return [(v, z.tolist(), tl, b) for (v, z, tl), b in zip(got, _bads(c, len(lens)))]


def _batch(c, sets):
    got = c.calc_prob_batch(sets)
    return [(v, z.tolist(), tl, b) for (v, z, tl), b in zip(got, _bads(c, len(sets)))]


def _call(c, ps):
    v, z, tl = c.calc_prob(ps)
    return v, z.tolist(), tl, [int(c.bad_bases(r)) for r in range(c.num_readsets())]


def _same(got, want, rel, what):
    """floored counts, total lengths and bad_bases exactly, the value within rel; returns how many values are bit-equal"""
    assert len(got) == len(want), what
    for k, (a, b) in enumerate(zip(got, want)):
        assert a[1:] == b[1:], (what, k, a, b)
        assert abs(a[0] - b[0]) <= rel * abs(b[0]), (what, k, a[0], b[0])
    return sum(a[0] == b[0] for a, b in zip(got, want))


def _device_route(st, n_lens, calls=1):
    assert st["device_lengths"] == n_lens and st["fallback_lengths"] == 0 and st["device_passes"] == (n_lens + 7) // 8 and st["calls"] == calls, st


def test_routes():
    """The flag opens the device route to a penalised context; Knob.GAP_FALLBACK still wins over it; without the flag the
    context reports the fallback. Same values on all three."""
    paths, path_id, gap_pos, lens = gp.cases()["site 81, edited first"]
    dev = gp.make_ctx(flag=True)
    assert dev.gap_penalty_device()
    ref = _profile(dev, paths, path_id, gap_pos, lens)
    _device_route(dev.gap_stats(), len(lens))
    assert len({r[3][0] for r in ref}) == 2 and all(r[3][0] > 0 for r in ref), [r[3] for r in ref]
    from gaml_amd import api
    dev.debug_set_knob(api.Knob.GAP_FALLBACK, 1)
    got = _profile(dev, paths, path_id, gap_pos, lens)
    st = dev.gap_stats()
    assert st["device_lengths"] == len(lens) and st["fallback_lengths"] == len(lens) and st["device_passes"] == 2, st
    _same(got, ref, 1e-13, "GAP_FALLBACK over the flag")
    off = gp.make_ctx()
    assert not off.gap_penalty_device()
    got = _profile(off, paths, path_id, gap_pos, lens)
    st = off.gap_stats()
    assert st["device_lengths"] == 0 and st["device_passes"] == 0 and st["fallback_lengths"] == len(lens), st
    _same(got, ref, 1e-13, "without the flag")
    # switched off again, the first context is back on the fallback
    dev.debug_set_knob(api.Knob.GAP_FALLBACK, 0)
    dev.set_gap_penalty_device(False)
    _same(_profile(dev, paths, path_id, gap_pos, lens[:3]), ref[:3], 1e-13, "flag off again")
    assert dev.gap_stats()["fallback_lengths"] == len(lens) + 3 and dev.gap_stats()["device_lengths"] == len(lens)


@pytest.mark.parametrize("name,libs,trimmed,penalty_a", CONFIGS)
def test_values(name, libs, trimmed, penalty_a):
    """1e-13 relative against twin contexts with other call sequences (the bound of test_gpu_gap.py and
    test_gpu_penalty_batch.py for that situation: their sums are taken in another order); 1e-9 against the oracle, whose
    bad_bases must be met exactly -- one base moves the value by 5e-4 on |v| ~ 1e2."""
    paths, path_id, gap_pos, lens = gp.cases()[name]
    sets = [gp.with_length(paths, path_id, gap_pos, l) for l in lens]
    dev, many, one = (gp.make_ctx(libs, trimmed, penalty_a, flag=f) for f in (True, None, None))
    got = _profile(dev, paths, path_id, gap_pos, lens)
    _device_route(dev.gap_stats(), len(lens))
    eq_b = _same(got, _batch(many, sets), 1e-13, "batch")
    eq_s = _same(got, [_call(one, s) for s in sets], 1e-13, "single calls")
    print(f"{name} / {libs}{' trimmed' if trimmed else ''}: {len(lens)} lengths, {eq_b} bit-equal to the batch call, {eq_s} to single calls; bad_bases {[g[3] for g in got]}")
    want = gp.oracle_profile(name, libs, trimmed, penalty_a)
    penalised = [r for r in range(dev.num_readsets()) if libs == "B" or r == 1 or penalty_a > 0]
    for k, (a, w) in enumerate(zip(got, want)):
        assert a[1] == w[1] and a[2] == w[2], (k, a, w)
        assert [a[3][r] for r in penalised] == [w[3][r] for r in penalised], (k, a[3], w[3])
        assert abs(a[0] - w[0]) <= 1e-9 * abs(w[0]), (k, a[0], w[0])
    if libs == "AB" and penalty_a == 0.0:
        assert all(a[3][0] == 0 for a in got)
    assert len({a[3][-1] for a in got}) >= (1 if name == "leading gap" else 2)
    for mate in (0, 1):
        assert dev.window_count(dev.num_readsets() - 1, mate) == one.window_count(one.num_readsets() - 1, mate)
    # warm, with another base length and the lengths in other passes: the same bits
    again = _profile(dev, paths, path_id, gap_pos, lens[::-1])
    assert [a[0] for a in again] == [a[0] for a in got][::-1]
    assert [a[1:] for a in again] == [a[1:] for a in got][::-1]
    st = dev.gap_stats()
    assert st["calls"] == 2 and st["device_lengths"] == 2 * len(lens) and st["device_passes"] == 2 * ((len(lens) + 7) // 8) and st["fallback_lengths"] == 0, st


@pytest.mark.parametrize("name", ["site 81, edited first", "site 81, edited in the middle", "edited last", "leading gap",
                                  "two gaps, the second varied", "two gaps, the first varied"])
def test_layout(name):
    """Region g's layout of the pass equals what the host lays out for the set planned with lens[g] (a twin context that
    has just scored it, whole-set planning: slots in set order)."""
    from gaml_amd import api
    paths, path_id, gap_pos, lens = gp.cases()[name]
    lens = lens[:8]
    dev, twin = gp.make_ctx(flag=True), gp.make_ctx()
    twin.debug_set_knob(api.Knob.PLAN_WHOLE_SET, 1)
    dev.gap_profile(paths, path_id, gap_pos, lens)
    _device_route(dev.gap_stats(), len(lens))
    lays = [dev.debug_gap_cov_layout(0, g) for g in range(len(lens))]
    with pytest.raises(api.GamlHipError):
        dev.debug_gap_cov_layout(0, len(lens))
    totals = set()
    for g, l in enumerate(lens):
        twin.calc_prob(gp.with_length(paths, path_id, gap_pos, l))
        want, got = twin.debug_cov_layout(0), lays[g]
        for key in ("path_base", "start_off", "starts"):
            assert np.array_equal(got[key], want[key]), (name, l, key, got[key], want[key])
        assert got["total_bits"] == want["total_bits"] == int(got["path_base"][-1]), (name, l)
        for lay in (got, want):  # a path's slot names its region; slots not in use hold 0
            sb = lay["slot_base"].copy()
            for k, s in enumerate(lay["slots"]):
                assert sb[s] == lay["path_base"][k], (name, l, k)
                sb[s] = 0
            assert not sb.any(), (name, l)
        if np.array_equal(got["slots"], want["slots"]):
            n = min(len(got["slot_base"]), len(want["slot_base"]))
            assert np.array_equal(got["slot_base"][:n], want["slot_base"][:n]), (name, l)
        totals.add(got["total_bits"])
    assert len(totals) >= 3, totals  # the regions' sizes differ between the lengths, and not by the lengths' difference


@pytest.mark.parametrize("name", sorted(gp.SEARCH_STARTS))
def test_search(name):
    """fix_gap_length follows the reference's search over the oracle evaluation for evaluation (no comparison there is
    closer than 1e-9 relative from these start lengths: tests/test_gap_penalty_cases_host.py)."""
    paths, path_id, gap_pos, _ = gp.cases()[name]
    o = gp.make_oracle()
    dev = gp.make_ctx(flag=True)
    for start in gp.SEARCH_STARTS[name]:
        ps = gp.with_length(paths, path_id, gap_pos, start)
        want = go.oracle_search(o, ps, path_id, gap_pos)
        before = dev.gap_stats()
        length, trace = dev.fix_gap_length(ps, path_id, gap_pos)
        after = dev.gap_stats()
        passes = after["device_passes"] - before["device_passes"]
        print(f"{name} from {start}: -> {length}, {len(trace)} evaluations, {passes} device passes, {after['device_lengths'] - before['device_lengths']} lengths scored")
        assert length == want.length == gp.SEARCH_ENDS[name], (start, length, want.length)
        assert [l for l, _ in trace] == [l for l, _ in want.trace], start
        for (l, v), (_, wv) in zip(trace, want.trace):
            assert abs(v - wv) <= 1e-9 * abs(wv), (start, l, v, wv)
        assert after["device_lengths"] > before["device_lengths"] and after["fallback_lengths"] == 0, after
        assert passes < len(trace), (passes, len(trace))


def test_afterwards():
    """Behind a profile the resident copy, its coverage layout included, describes the set with the base length: a blocking
    call, a batch, and another profile after compact_tables give what a twin context gives that scored the same sets one
    by one."""
    paths, path_id, gap_pos, lens = gp.cases()["site 81, edited in the middle"]
    w = gp.graph()[2]
    sets = [gp.with_length(paths, path_id, gap_pos, l) for l in lens]
    dev, twin = gp.make_ctx(flag=True), gp.make_ctx()
    ref = _profile(dev, paths, path_id, gap_pos, lens)
    singles = [_call(twin, s) for s in sets]
    _same(ref, singles, 1e-13, "profile")
    _call(twin, sets[0])  # (the profile leaves the set with the base length behind)
    near = [paths[0], paths[1][:-1], paths[2]]   # an incremental edit of the profiled set
    other = [w[10:40], gp.twin(w[45:70]), w[100:120]]
    for ps in (near, other, sets[0]):
        _same([_call(dev, ps)], [_call(twin, ps)], 1e-13, "blocking call after a profile")
        assert np.array_equal(dev.read_probs(0), twin.read_probs(0))
    dev.gap_profile(paths, path_id, gap_pos, lens[:4])
    _call(twin, sets[0])
    batch = [near, sets[5], other, sets[11], sets[1]]
    _same(_batch(dev, batch), _batch(twin, batch), 1e-13, "batch after a profile")
    for c in (dev, twin):
        c.compact_tables()
    got = _profile(dev, paths, path_id, gap_pos, lens)
    _same(got, [_call(twin, s) for s in sets], 1e-13, "profile after compact_tables")
    assert [g[1:] for g in got] == [r[1:] for r in ref]
    st = dev.gap_stats()
    assert st["fallback_lengths"] == 0 and st["device_lengths"] == 2 * len(lens) + 4, st
