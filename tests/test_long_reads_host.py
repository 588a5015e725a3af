"""The host aligner on reads of 255 to 510 bases against the oracle -- no GPU needed: a host-only context. The host
aligner is the referee of tests/test_gpu_aligner_long_reads.py, so it is pinned here first (reference
AlignSubpathInternal graph.cc:839-899, ProcessHit graph.cc:753-837)."""
import pytest

import oracle_py as op
from gaml_amd import synth
from long_reads_cases import long_read_case


@pytest.mark.parametrize("L", [255, 300, 510])
def test_host_aligner_equals_oracle_on_long_reads(built, L):
    from gaml_amd import api
    g, pr, sets = long_read_case(L)
    gb, go = g.packed()
    reads = (*synth.pack_reads(pr.mate1), *synth.pack_reads(pr.mate2))
    ctx = api.Context(device=-1)
    ctx.set_graph(gb, go)
    rs = ctx.add_paired(api.paired_cfg(2.2 * L, 0.2 * L), *reads)
    orc = op.Oracle()
    orc.set_graph(gb, go)
    ors = orc.add_paired(*reads, 0.01, op.paired_cfg(2.2 * L, 0.2 * L))
    n_windows = n_records = 0
    for paths in sets:  # after every path set both sides hold the same window cache (graph.cc:447-533)
        orc.calc_prob(paths, fresh=True)
        ctx.debug_prepare(paths)
        for mate in (0, 1):
            keys = orc.window_keys(ors, mate)
            assert ctx.window_count(rs, mate) == len(keys)
            have = {tuple(ctx.debug_window_walk(rs, mate, w)) for w in range(ctx.window_count(rs, mate))}
            assert have == {tuple(key) for key in keys}
            for key in keys:
                ref = orc.window_records(ors, mate, key)
                got = ctx.window_records(rs, mate, key)
                assert got is not None, key
                assert got.shape == ref.shape and (got == ref).all(), key
                n_windows += 1
                n_records += len(ref)
    print(f"L = {L}: {n_windows} windows, {n_records} records compared, all identical")
    assert n_windows > 0 and n_records > 0  # (not a comparison of empty windows)
