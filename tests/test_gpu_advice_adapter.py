"""ProbCalculator::AdviceCandidates of include/gaml_hip_prob_calculator.h, driven the way the moves.cc patch of
INTEGRATION.md §7 calls it: tests/mock_ref/advice_driver.cc compiles that patch's text (checked here against the
document) over the declaration mock, and its lists must equal the library's through ctypes, on one device and on
GAML_HIP_DEVICES=0,0."""
import os
import re
import subprocess

import pytest

from gaml_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "mock_ref", "_build", "advice_driver")


def _strip(lines):
    return [ln.strip() for ln in lines if ln.strip()]


def test_driver_runs_the_documented_patch(built):
    """The lines between the driver's BEGIN / END markers are the new side of the INTEGRATION.md §7 diff."""
    assert os.path.exists(DRIVER)
    src = open(os.path.join(ROOT, "tests", "mock_ref", "advice_driver.cc")).read()
    block = src.split("// BEGIN moves.cc:948-986 as patched\n")[1].split("// END")[0].split("\n")
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = doc[doc.index("## 7. Optional: the advice move"):]
    diff = sec.split("```diff\n")[1].split("\n```")[0].split("\n")
    new_side = [ln[1:] for ln in diff if ln[:1] in ("+", " ")]
    assert _strip(block) == _strip(new_side)
    assert sum("rand() % 5" in ln for ln in new_side) == 2 and sum("AdviceCandidates" in ln for ln in new_side) == 2


@pytest.mark.gpu
@pytest.mark.parametrize("devices", ["", "0,0"])
def test_advice_candidates_equal_the_ctypes_lists(tmp_path, devices):
    from gaml_amd import api
    d = str(tmp_path)
    G, seed, threshold, moves = 60_000, 43, 500, 40
    genome = synth.make_genome(G, seed)
    g = synth.make_graph(genome, synth.cut_lengths(G, seed, long_rng=(600, 2500)))
    synth.write_lastgraph(os.path.join(d, "LastGraph"), g)
    pr = synth.make_paired_reads(genome, 4000, 100, 1500.0, 150.0, 0.01, seed)
    sr = synth.make_single_reads(genome, 500, 100, 0.01, seed)
    f1, f2, fs = (os.path.join(d, n) for n in ("a_1.fastq", "a_2.fastq", "s.fastq"))
    synth.write_fastq(f1, pr.mate1, "p", 1)
    synth.write_fastq(f2, pr.mate2, "p", 2)
    synth.write_fastq(fs, sr, "s", None)
    env = dict(os.environ)
    env.pop("GAML_HIP_DEVICES", None)
    if devices:
        env["GAML_HIP_DEVICES"] = devices
    out = subprocess.run([DRIVER, os.path.join(d, "LastGraph"), f1, f2, "1500", "150", str(threshold), "7", str(moves), fs],
                         capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr
    rows = re.findall(r"move (\d+) path ([-\d ]+) flags (\d) (\d) cands (\d+)((?: -?\d+)*)", out.stdout)
    assert len(rows) == moves, out.stdout[:2000]

    # the same calls through ctypes: single set first, then the paired one (the adapter's order of creation)
    ctx = api.Context(device=0)
    ctx.load_graph(os.path.join(d, "LastGraph"))
    ctx.add_single_fastq(api.single_cfg(weight=0.5), fs)
    rs = ctx.add_paired_fastq(api.paired_cfg(1500.0, 150.0), f1, f2)
    assert rs == 1
    ctx.calc_prob([list(range(0, g.n_nodes, 2))])
    ctx.advice_build(rs, threshold)
    n, seen = g.n_nodes, 0
    for k, path, only_out, allow_gaps, count, cands in rows:
        path = [int(x) for x in path.split()]
        reach = [(path[-1] + 2 * j) % n for j in range(1, 9)]
        got = ctx.advice_candidates(rs, path, reach, only_out == "1", False)
        if allow_gaps == "1":  # drawn so, or the retry after an empty list: the same registrations either way
            got = ctx.advice_candidates(rs, path, reach, only_out == "1", True)
        else:
            assert len(got) > 0
        want = [int(x) for x in cands.split()]
        assert len(want) == int(count) and got.tolist() == want, (k, path)
        seen += len(want)
    assert seen > 0
