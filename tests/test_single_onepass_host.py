"""The switch that lets single-end sets go along on calc_prob_batch's one-pass routes (gaml_hip_set_single_onepass /
GAML_HIP_SINGLE_BATCH=onepass) and gaml_hip_single_stats, on host-only contexts. No device needed."""
import os
import subprocess
import sys

import pytest

from gaml_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _context():
    from gaml_amd import api
    genome = synth.make_genome(20_000, 7)
    g = synth.make_graph(genome, synth.cut_lengths(20_000, 7, long_rng=(900, 2500)))
    c = api.Context(device=-1)
    c.set_graph(*g.packed())
    pr = synth.make_paired_reads(genome, 40, 100, 250.0, 25.0, 0.01, 7)
    paired = c.add_paired(api.paired_cfg(250.0, 25.0), *synth.pack_reads(pr.mate1), *synth.pack_reads(pr.mate2))
    single = c.add_single(api.single_cfg(), *synth.pack_reads(synth.make_single_reads(genome, 300, 100, 0.01, 8)))
    return c, g, paired, single


def test_the_switch_is_off_by_default_and_round_trips(built):
    from gaml_amd import api
    assert os.environ.get("GAML_HIP_SINGLE_BATCH") is None
    c = _context()[0]
    assert c.single_onepass() is False and api.lib().gaml_hip_get_single_onepass(c._h) == 0
    c.set_single_onepass(True)
    assert c.single_onepass() is True
    c.set_single_onepass(False)
    assert c.single_onepass() is False
    assert api.lib().gaml_hip_set_single_onepass(None, 1) == api.EINVAL and api.lib().gaml_hip_get_single_onepass(None) == 0


@pytest.mark.parametrize("value, want", [("onepass", True), ("sequential", False)])
def test_the_environment_sets_what_a_new_context_starts_with(built, value, want):
    code = ("import sys; sys.path.insert(0, %r); from gaml_amd import api; c = api.Context(device=-1); print(int(c.single_onepass())); "
            "c.set_single_onepass(%r); print(int(c.single_onepass()))") % (ROOT, not want)
    env = dict(os.environ, GAML_HIP_SINGLE_BATCH=value, GAML_HIP_FLAVOUR="dev")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == [str(int(want)), str(int(not want))]


def test_single_stats_report_windows_and_records(built):
    """`windows` counts every registered window, so it moves with align_window. `records` counts what the read-major table
    holds (include/gaml_hip.h): the records of windows that some scored path set has named -- 0 right after align_window,
    above 0 once a path set names the windows. A host-only context cannot score, so the test names them through
    debug_prepare, the development build's entry point for the host half of a scoring call."""
    from gaml_amd import api
    c, g, paired, single = _context()
    assert c.single_stats(single) == {"windows": 0, "records": 0, "table_bytes": 0, "multi_launches": 0}
    walk = synth.genome_walk(g)
    n0 = c.align_window(single, 0, walk[:1])
    n1 = c.align_window(single, 0, walk[1:3])
    assert n0 + n1 > 0
    st = c.single_stats(single)
    # aligned, but no scored path set has named them: the read-major table holds the records of windows that were
    assert st["windows"] == c.window_count(single, 0) == 2 and st["records"] == 0
    c.debug_prepare([walk[:6]])  # registration + occurrences of a path set, as a scoring call does them on the host
    st = c.single_stats(single)
    occ = c.debug_occurrences(single)
    named = sorted(set(int(w) for w in occ[:, 0]))
    assert st["windows"] == c.window_count(single, 0) >= len(named) > 0
    assert st["records"] > 0 and st["table_bytes"] == 0 and st["multi_launches"] == 0
    c.debug_prepare([walk[:6], walk[2:5]])  # the same windows again: nothing is counted twice
    assert c.single_stats(single)["records"] == st["records"]
    for rs in (paired, -1, 2):
        with pytest.raises(api.GamlHipError) as e:
            c.single_stats(rs)
        assert e.value.code == api.EINVAL, rs


def test_the_entry_points_are_declared(built):
    from gaml_amd import api
    header = open(os.path.join(ROOT, "include", "gaml_hip.h")).read()
    for name in ("gaml_hip_set_single_onepass", "gaml_hip_get_single_onepass", "gaml_hip_single_stats"):
        assert "int %s(" % name in header and hasattr(api.lib(), name), name
