"""The host aligner against the oracle on tandem repeats, a two-letter stretch and reads with an inserted or deleted base
(tests/aligner_hard_cases.py) -- no GPU needed: a host-only context. The host aligner is the referee of
tests/test_gpu_aligner_hard_cases.py, so it is pinned here first: the earliest seed among equal maxima of a span
(reference graph.cc:1289-1323), extensions that leave the seed's diagonal (ProcessHit graph.cc:753-837), reads with several
records in one window and their order (graph.cc:841, 891, 895-897), down to the shortest reads the device takes."""
import numpy as np
import pytest

import oracle_py as op
from aligner_hard_cases import hard_case


@pytest.mark.parametrize("L", [16, 17, 31, 100, 254, 255, 510])
def test_host_aligner_equals_oracle_on_hard_cases(built, L):
    from gaml_amd import api
    g, reads, indel, regions, sets = hard_case(L)
    gb, go = g.packed()
    ctx = api.Context(device=-1)
    ctx.set_graph(gb, go)
    rs = ctx.add_paired(api.paired_cfg(2.2 * L, 0.2 * L), *reads)
    orc = op.Oracle()
    orc.set_graph(gb, go)
    ors = orc.add_paired(*reads, 0.01, op.paired_cfg(2.2 * L, 0.2 * L))
    n_windows = n_records = n_indel = n_several = largest = max_edit = 0
    for paths in sets:  # after every path set both sides hold the same window cache (graph.cc:447-533)
        orc.calc_prob(paths, fresh=True)
        ctx.debug_prepare(paths)
        n_windows = n_records = n_indel = n_several = largest = 0  # (the cache only grows: the last set's figures cover all)
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
                if len(ref):  # Aligment = (position, edit distance, read, orientation)
                    n_indel += int(indel[mate][ref[:, 2]].sum())
                    n_several += int((np.bincount(ref[:, 2]) > 1).sum())
                    largest = max(largest, len(ref))
                    max_edit = max(max_edit, int(ref[:, 1].max()))
    print(f"L = {L}: {n_windows} windows, {n_records} records compared, all identical; {n_indel} records of reads with an inserted "
          f"or deleted base, {n_several} (read, window) with several records, largest window {largest} records, edit distance up to {max_edit}")
    assert n_windows > 0 and n_records > 0  # (not a comparison of empty windows)
    assert n_indel > 0
    if L <= 31:
        assert n_several > 0
    if L == 100:
        assert largest > 1024
