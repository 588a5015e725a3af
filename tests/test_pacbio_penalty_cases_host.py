"""What the batches with penalised PacBio sets rest on, checked without a device: the fixtures of
tests/pacbio_penalty_batch_cases.py on the CPU oracle (the stated bad_bases and floored counts; bad_bases of a path set is
the sum of its paths' scored alone; the declared interval counts), and the switch, its environment variable and
gaml_hip_pacbio_penalty_stats on host-only contexts."""
import os
import subprocess
import sys

import pytest

import pacbio_penalty_batch_cases as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fp(built):
    return pp.FixtureP()


@pytest.fixture(scope="module")
def fc(built):
    return pp.FixtureC()


def _detail(o, rs, paths):
    o3 = o.pacbio_detail(rs, paths)[2]
    return int(o3[2]), int(o3[0])  # bad_bases, floored reads


def test_fixture_p_is_what_the_cases_file_states(fp):
    o, rs = fp.oracle()
    for sets, bad, floored in ((fp.candidates(), pp.BAD_CANDIDATES, pp.FLOORED_CANDIDATES), (fp.unrelated(), pp.BAD_UNRELATED, pp.FLOORED_UNRELATED)):
        got = [_detail(o, rs, s) for s in sets]
        print(got)
        assert [g[0] for g in got] == bad and [g[1] for g in got] == floored
    assert all(b > 0 for b in pp.BAD_CANDIDATES) and len(set(pp.BAD_CANDIDATES)) == 5
    nz = [b for b in pp.BAD_UNRELATED if b]
    assert len(nz) == 6 and len(set(nz)) == 6
    for fl in (pp.FLOORED_CANDIDATES, pp.FLOORED_UNRELATED):  # both branches of the floor
        assert any(0 < x < pp.N_PACBIO_P for x in fl)
    assert 0 in pp.FLOORED_UNRELATED and pp.N_PACBIO_P in pp.FLOORED_UNRELATED
    # the candidates share most of their paths: a chunk sweeps each distinct path once
    assert len(pp.distinct_paths(fp.candidates())) == 13 < sum(len(s) for s in fp.candidates())


def test_bad_bases_of_a_set_is_the_sum_over_its_paths(fp, fc):
    """CalcScoreForPacbio (graph.cc:3183-3251) sweeps every path on its own and adds the counts up: what lets a chunk sweep a
    path once, whichever sets list it and how often."""
    o, rs = fp.oracle()
    for sets in (fp.candidates(), fp.unrelated()):
        for s in sets:
            assert _detail(o, rs, s)[0] == sum(_detail(o, rs, [p])[0] for p in s), s
    for step in pp.STEPS_C:
        o, rs = fc.oracle(step)
        alone = {}
        for k, s in enumerate(fc.sets()):
            for p in s:
                if tuple(p) not in alone:
                    alone[tuple(p)] = _detail(o, rs, [p])[0]
            assert _detail(o, rs, s)[0] == sum(alone[tuple(p)] for p in s) == pp.BAD_C[step][k], (step, k)


def test_fixture_c_counts_and_values(fc):
    sets = fc.sets()
    assert len(sets) == 8  # one chunk
    assert [[fc.interval_count(p) for p in s] for s in sets] == pp.COUNTS_C
    assert max(max(c) for c in pp.COUNTS_C if c) == pp.LARGEST_C == pp.COUNTS_C[0][0]
    assert sum(1 for c in pp.COUNTS_C for x in c if x == pp.LARGEST_C) == 1  # one below the largest count: exactly one contig leaves the block kernel
    assert len(pp.distinct_paths(sets)) == 24
    for step in (30.0, 777.25):
        assert sum(1 for b in pp.BAD_C[step] if b) >= 6
    assert not any(pp.BAD_C[0.5])


def test_the_switch_is_off_by_default_and_round_trips(fp):
    from gaml_amd import api
    assert os.environ.get("GAML_HIP_PACBIO_PENALTY_BATCH") is None
    c, paired, pacbio = fp.context(device=-1)
    L = api.lib()
    assert c.get_pacbio_penalty_onepass() is False and L.gaml_hip_get_pacbio_penalty_onepass(c._h) == 0
    c.set_pacbio_penalty_onepass(True)
    assert c.get_pacbio_penalty_onepass() is True
    c.set_pacbio_penalty_onepass(False)
    assert c.get_pacbio_penalty_onepass() is False
    assert L.gaml_hip_set_pacbio_penalty_onepass(None, 1) == api.EINVAL and L.gaml_hip_get_pacbio_penalty_onepass(None) == 0
    # a host-only context has swept nothing; a handle that is no PacBio set is refused
    assert c.pacbio_penalty_stats(pacbio) == {"chunks": 0, "block_contigs": 0, "chain_contigs": 0, "memo_paths": 0}
    for rs in (paired, -1, 2):
        with pytest.raises(api.GamlHipError) as e:
            c.pacbio_penalty_stats(rs)
        assert e.value.code == api.EINVAL, rs
    with pytest.raises(api.GamlHipError) as e:
        c.debug_pacbio_batch_bad_bases(paired)
    assert e.value.code == api.EINVAL
    assert c.debug_pacbio_batch_bad_bases(pacbio) == []


@pytest.mark.parametrize("value, want", [("onepass", True), ("sequential", False)])
def test_the_environment_sets_what_a_new_context_starts_with(built, value, want):
    code = ("import sys; sys.path.insert(0, %r); from gaml_amd import api; c = api.Context(device=-1); print(int(c.get_pacbio_penalty_onepass())); "
            "c.set_pacbio_penalty_onepass(%r); print(int(c.get_pacbio_penalty_onepass()))") % (ROOT, not want)
    env = dict(os.environ, GAML_HIP_PACBIO_PENALTY_BATCH=value, GAML_HIP_FLAVOUR="dev")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == [str(int(want)), str(int(not want))]


def test_the_entry_points_are_declared(built):
    from gaml_amd import api
    header = open(os.path.join(ROOT, "include", "gaml_hip.h")).read()
    for name in ("gaml_hip_set_pacbio_penalty_onepass", "gaml_hip_get_pacbio_penalty_onepass", "gaml_hip_pacbio_penalty_stats"):
        assert "int %s(" % name in header and hasattr(api.lib(), name), name
    debug = open(os.path.join(ROOT, "include", "gaml_hip_debug.h")).read()
    assert "gaml_hip_debug_pacbio_batch_bad_bases(" in debug and "gaml_hip_debug_pacbio_batch_bad_bases(" not in header
    assert int(api.Knob.PACBIO_SWEEP_CAP) == api.KNOB_COUNT - 1
