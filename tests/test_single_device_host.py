"""The switch that sends single-end sets to the device route (gaml_hip_set_single_device / GAML_HIP_SINGLE_DEVICE=1),
gaml_hip_single_device_stats, the two-pass window registration behind the switch and the index arithmetic of the device
table build (gaml_amd/csrc/single_tables.hip.h), on host-only contexts and in numpy. No device needed."""
import os
import subprocess
import sys

import numpy as np
import pytest

import single_table_cases as stc
from gaml_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gaml_hip_set_single_device", "gaml_hip_get_single_device", "gaml_hip_single_device_stats")


def _context(single_device=None):
    from gaml_amd import api
    genome = synth.make_genome(20_000, 7)
    g = synth.make_graph(genome, synth.cut_lengths(20_000, 7, long_rng=(900, 2500)))
    c = api.Context(device=-1)
    if single_device is not None:
        c.set_single_device(single_device)
    c.set_graph(*g.packed())
    pr = synth.make_paired_reads(genome, 40, 100, 250.0, 25.0, 0.01, 7)
    paired = c.add_paired(api.paired_cfg(250.0, 25.0), *synth.pack_reads(pr.mate1), *synth.pack_reads(pr.mate2))
    single = c.add_single(api.single_cfg(), *synth.pack_reads(synth.make_single_reads(genome, 600, 100, 0.01, 8)))
    return c, g, paired, single


def test_the_entry_points_are_declared_and_exported_by_both_libraries(built):
    header = open(os.path.join(ROOT, "include", "gaml_hip.h")).read()
    for lib in ("libgaml_hip.so", "libgaml_hip_dev.so"):
        out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "gaml_amd", lib)], text=True)
        exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
        for name in NAMES:
            assert "int %s(" % name in header and name in exported, (lib, name)
        assert ("gaml_hip_debug_single_table_check" in exported) == (lib == "libgaml_hip_dev.so")


def test_the_switch_is_off_by_default_and_round_trips(built):
    from gaml_amd import api
    assert os.environ.get("GAML_HIP_SINGLE_DEVICE") is None
    c = _context()[0]
    assert c.get_single_device() is False and api.lib().gaml_hip_get_single_device(c._h) == 0
    c.set_single_device(True)
    assert c.get_single_device() is True
    c.set_single_device(False)
    assert c.get_single_device() is False
    assert api.lib().gaml_hip_set_single_device(None, 1) == api.EINVAL and api.lib().gaml_hip_get_single_device(None) == 0


@pytest.mark.parametrize("value, want", [("1", True), (None, False)])
def test_the_environment_sets_what_a_new_context_starts_with(built, value, want):
    code = ("import sys; sys.path.insert(0, %r); from gaml_amd import api; c = api.Context(device=-1); print(int(c.get_single_device())); "
            "c.set_single_device(%r); print(int(c.get_single_device()))") % (ROOT, not want)
    env = dict(os.environ, GAML_HIP_FLAVOUR="dev")
    env.pop("GAML_HIP_SINGLE_DEVICE", None)
    if value is not None:
        env["GAML_HIP_SINGLE_DEVICE"] = value
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == [str(int(want)), str(int(not want))]


def test_stats_on_a_host_only_context(built):
    """Nothing reaches a device: windows aligned there, device builds and mirrored records stay 0 whatever the flag says, and
    a host-only context never scores, so no table is built on the host either."""
    from gaml_amd import api
    for on in (False, True):
        c, g, paired, single = _context(on)
        walk = synth.genome_walk(g)
        assert c.single_device_stats(single) == {"aligned_windows": 0, "device_builds": 0, "mirrored_records": 0, "host_builds": 0}
        c.align_window(single, 0, walk[:1])
        c.debug_prepare([walk[:6]])
        st = c.single_device_stats(single)
        assert (st["aligned_windows"], st["device_builds"], st["mirrored_records"]) == (0, 0, 0) and st["host_builds"] >= 0
        assert c.single_stats(single)["records"] > 0
        chk = c.debug_single_table_check(single)  # host-only: the sizes and zeros
        assert chk["compared"] >= 600 and (chk["first"], chk["extra"], chk["sizes"]) == (0, 0, 0)
        for rs in (paired, -1, 2):
            with pytest.raises(api.GamlHipError) as e:
                c.single_device_stats(rs)
            assert e.value.code == api.EINVAL, rs


def test_two_pass_registration_gives_the_one_pass_windows_and_records(built):
    """With the flag on, prepare_single_host registers every contig of every path first and aligns the pending windows as one
    batch (the host aligner here), then takes the occurrences; with it off, contig by contig. Same windows under the same
    ids, same records, same occurrences, path set after path set."""
    off, g, _, s_off = _context(False)
    on, _, _, s_on = _context(True)
    start, seq = synth.sa_sequence(g, 12, seed=3, threshold=300)
    walk = synth.genome_walk(g)
    for paths in [start] + seq + [[walk], [walk[:5] + [-60] + walk[7:], walk[3:9]]]:
        off.debug_prepare(paths)
        on.debug_prepare(paths)
        assert on.window_count(s_on, 0) == off.window_count(s_off, 0) > 0
        assert np.array_equal(on.debug_occurrences(s_on), off.debug_occurrences(s_off))
        assert on.single_stats(s_on) == off.single_stats(s_off)
    n_windows, with_records = off.window_count(s_off, 0), 0
    for wid in range(n_windows):
        w = off.debug_window_walk(s_off, 0, wid)
        assert on.debug_window_walk(s_on, 0, wid) == w
        a, b = off.window_records(s_off, 0, w), on.window_records(s_on, 0, w)
        assert np.array_equal(a, b), w
        with_records += len(a) > 0
    assert with_records > 5


# ---- the index arithmetic of the device build against build_read_major, both restated in numpy ----------------------------

def _flags(r):
    return (r[2] & 0xff) | ((r[4] & 1) << 8)


def build_read_major_restated(records, n):
    """host_model.cc's build_read_major, statement by statement: count per read, start[] as the running sum of cnt - 1, then
    the records in (window id, pool order) with seen[]."""
    cnt = np.zeros(n + 1, np.int64)
    for r in records:
        cnt[r[3] + 1] += 1
    start, extras = np.zeros(n + 1, np.int64), 0
    for i in range(n):
        start[i] = extras
        extras += cnt[i + 1] - 1 if cnt[i + 1] > 1 else 0
    first = np.tile(np.array([-1, 0, 0, 0], np.int64), (n, 1))
    extra = np.tile(np.array([-1, 0, 0, 0], np.int64), (extras, 1))
    seen = np.zeros(n, np.int64)
    for r in records:
        at = r[3]
        q = [r[0], r[1], _flags(r), 0]
        s = seen[at]
        seen[at] += 1
        if s == 0:
            q[2] |= (cnt[at + 1] - 1) << 9
            q[3] = start[at]
            first[at] = q
        else:
            extra[start[at] + s - 1] = q
    return first, extra


def device_build_restated(records, n):
    """single_tables.hip.h: keys = reads, payload = sequence index; stable sort; head flags and their inclusive prefix H;
    head at b with L records: first[read], flags |= (L - 1) << 9, link = b + 1 - H(b); every other p: extra[p - H(p)]."""
    A = len(records)
    first = np.tile(np.array([-1, 0, 0, 0], np.int64), (n, 1))
    if A == 0:
        return first, np.zeros((0, 4), np.int64)
    keys = records[:, 3].astype(np.int64)
    order = np.argsort(keys, kind="stable")  # the payload after the sort
    k = keys[order]
    head = np.ones(A, np.int64)
    head[1:] = k[1:] != k[:-1]
    H = np.cumsum(head)
    extra = np.tile(np.array([-1, 0, 0, 0], np.int64), (A - int(H[-1]), 1))
    q = np.stack([records[order, 0], records[order, 1], _flags(records[order].T), np.zeros(A, np.int64)], axis=1).astype(np.int64)
    p = np.arange(A)
    b = np.flatnonzero(head)
    L = np.diff(np.append(b, A))
    q[b, 2] |= (L - 1) << 9
    q[b, 3] = b + 1 - H[b]
    first[k[b]] = q[b]
    rest = np.flatnonzero(head == 0)
    extra[(p - H)[rest]] = q[rest]
    return first, extra


@pytest.mark.parametrize("case", stc.cases(), ids=repr)
def test_device_index_arithmetic_equals_build_read_major(built, case):
    from gaml_amd import api
    assert all(hasattr(api.lib(), n) for n in NAMES)  # the build this restates is in the library
    seen_any = False
    for _, counts, records in stc.replay(case):
        records = records.astype(np.int64)
        assert len(records) == counts["records"] and len(np.unique(records[:, 3])) == counts["reads"]
        assert counts["extras"] == counts["records"] - counts["reads"]
        if case.n_reads <= 1000:
            want = build_read_major_restated(records, case.n_reads)
        else:  # (the literal loop over 70,000 reads is slow in Python: its statements vectorised, same arrays)
            want = _read_major_vectorised(records, case.n_reads)
            small = records[records[:, 3] < 40]
            a, b = build_read_major_restated(small, 40), _read_major_vectorised(small, 40)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        got = device_build_restated(records, case.n_reads)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), case
        assert len(got[1]) == counts["extras"]
        seen_any = True
    assert seen_any


def _read_major_vectorised(records, n):
    cnt = np.bincount(records[:, 3], minlength=n)
    more = np.maximum(cnt - 1, 0)
    start = np.cumsum(more) - more
    first = np.tile(np.array([-1, 0, 0, 0], np.int64), (n, 1))
    extra = np.tile(np.array([-1, 0, 0, 0], np.int64), (int(more.sum()), 1))
    seen = np.zeros(n, np.int64)
    for r in records:
        at, s = r[3], seen[r[3]]
        seen[at] += 1
        q = [r[0], r[1], _flags(r), 0]
        if s == 0:
            q[2] |= (cnt[at] - 1) << 9
            q[3] = start[at]
            first[at] = q
        else:
            extra[start[at] + s - 1] = q
    return first, extra


@pytest.mark.parametrize("case", stc.cases()[:6], ids=repr)
def test_the_cases_hold_what_they_state_on_a_host_only_context(built, case):
    """The records fed through put_window_records and named through debug_prepare: single_stats counts what the case states."""
    from gaml_amd import api
    g, walk = stc.graph()
    for on in (False, True):
        c = api.Context(device=-1)
        c.set_single_device(on)
        c.set_graph(*g.packed())
        rs = c.add_single(api.single_cfg(), *synth.pack_reads(stc.reads(case.n_reads)))
        for step in case.steps:
            if step[0] == "put":
                c.put_window_records(rs, 0, [walk[step[1]]], np.ascontiguousarray(_aligment(api, step[2])))
            elif step[0] == "align":
                c.align_window(rs, 0, [walk[step[1]]])
            else:
                c.debug_prepare([[walk[x]] for x in step[1]])
                assert c.single_stats(rs)["records"] == step[2]["records"]


def _aligment(api, r):
    out = np.zeros(len(r), api.ALIGMENT)
    out["position"], out["edit_dist"], out["read_id"], out["orientation"] = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
    return out
