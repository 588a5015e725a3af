"""The scenarios of tests/delta_cases.py activate what their routes need -- no GPU needed: a host-only context. Every step's
records and windows (gaml_hip_debug_prepare, the windows its occurrence lists name for the first time, their records) lie
in the range that makes paired_delta_apply (gaml_amd/csrc/paired_tables.hip.h) choose the launch the scenario is for, and
stay under the size above which a call rebuilds the tables instead of extending the lists. tests/test_gpu_delta_lists.py
asserts the launches themselves; were gaml_amd/synth.py ever to change, this fails here instead of the GPU test quietly
running the smallest kernel seven times."""
import numpy as np
import pytest

import delta_cases as dc


def _host_ctx(fix):
    from gaml_amd import api
    g, pr, _ = dc.fixture(fix)
    ctx = api.Context(device=-1)
    ctx.set_graph(*g.packed())
    rs = ctx.add_paired(api.paired_cfg(*dc.INSERT), *dc.packed_reads(pr))
    return ctx, rs


@pytest.mark.parametrize("sc", dc.scenarios(), ids=repr)
def test_scenario_steps_activate_what_their_route_needs(built, sc):
    ctx, rs = _host_ctx(sc.fixture)
    got, _ = dc.measure(ctx, rs, sc.steps)
    n = dc.FIXTURES[sc.fixture][1]
    assert len(got) == len(sc.expect)
    for k, ((records, windows, pairs), (rlo, rhi, wlo, whi, _, _)) in enumerate(zip(got, sc.expect)):
        print(f"{sc.name} step {k + 1}: {records} records in {windows} windows (wanted {rlo}..{rhi} in {wlo}..{whi}), "
              f"at most {pairs} pairs on the lists before it: {pairs + records} of at most {dc.hard_limit(n)}")
        assert rlo <= records <= rhi and wlo <= windows <= whi
        assert pairs + records <= dc.hard_limit(n)
    ctx.close()


def test_fixture_figures_the_routes_were_planned_with(built):
    """What the scenario table quotes: long nodes per fixture, and the records of the medium fixture's first long nodes."""
    assert [len(dc.fixture(f)[2]) for f in ("small", "medium", "large")] == [22, 50, 114]
    ctx, rs = _host_ctx("medium")
    _, _, longs = dc.fixture("medium")
    steps = [[]] + [[[x] for x in longs[:k]] for k in range(1, 11)]
    got, _ = dc.measure(ctx, rs, steps)
    cumulative = np.cumsum([r for r, _, _ in got]).tolist()
    print("medium fixture, records of the first k long nodes:", cumulative)
    assert cumulative == [914, 1392, 1736, 2601, 4783, 5009, 5879, 6504, 7790, 8571]
    ctx.close()


def test_spill_scenario_makes_long_lists_and_grows_them(built):
    ctx, rs = _host_ctx("medium")
    steps = dc.spill_steps()
    got, per_read = dc.measure(ctx, rs, steps)
    n = dc.FIXTURES["medium"][1]
    longest = [np.maximum(p[0], p[1]) for p in per_read]
    over4 = [int((m > 4).sum()) for m in longest]
    for k, (records, windows, pairs) in enumerate(got):
        print(f"spill step {k + 1}: {records} records in {windows} windows, {over4[k + 1]} reads with more than 4 records on a mate "
              f"(longest list {int(longest[k + 1].max())}), at most {pairs} pairs on the lists before it: {pairs + records} of at most {dc.hard_limit(n)}")
        lo, hi = dc.SPILL_RECORDS[k]
        assert lo <= records <= hi and windows <= 64 and pairs + records <= dc.hard_limit(n)
    # tables: no list longer than 4, but hundreds of 3 (pairs of the more-than-2-records classes that are new to the lists)
    assert over4[0] == 0 and int((longest[0] == 3).sum()) >= 100
    assert over4[1] == 0 and int((longest[1] == 4).sum()) >= 100            # step 1: still at the fixed stride, full
    assert over4[2] >= 100                                                  # step 2: from the stride to the spill area
    grew3 = int(((longest[3] > longest[2]) & (longest[2] > 4)).sum())       # step 3: a spill list grows ...
    grew4 = int(((longest[4] > longest[3]) & (longest[3] > 4)).sum())       # ... and again, to twice its length
    print(f"spill lists that grow at step 3: {grew3}, at step 4: {grew4}")
    assert grew3 >= 100 and grew4 >= 100 and int(longest[4].max()) == 12
    # the annealing walk that follows: small activations only (one-block launches), far from a rebuild
    after_spill = int((np.maximum(per_read[-1][0] - per_read[0][0], per_read[-1][1] - per_read[0][1]) > 0).sum())
    walk, _ = dc.measure(ctx, rs, [steps[-1]] + dc.sa_walk_steps())
    print("annealing walk, records per step:", [r for r, _, _ in walk], "after", after_spill, "pairs on the lists")
    assert sum(r > 0 for r, _, _ in walk) >= 5 and max(r for r, _, _ in walk) <= 3000
    assert after_spill + sum(r for r, _, _ in walk) <= dc.hard_limit(n)
    ctx.close()
