"""gaml_hip_pacbio_stats on a host-only context: what the record cache of a PacBio set holds. No device needed."""
import numpy as np
import pytest

from gaml_amd import synth


def test_pacbio_stats_report_the_record_cache(built):
    from gaml_amd import api
    genome = synth.make_genome(20_000, 7)
    g = synth.make_graph(genome, synth.cut_lengths(20_000, 7, long_rng=(900, 2500)))
    walk = synth.genome_walk(g)
    pr = synth.make_paired_reads(genome, 40, 100, 250.0, 25.0, 0.01, 7)
    c = api.Context(device=-1)
    c.set_graph(*g.packed())
    paired = c.add_paired(api.paired_cfg(250.0, 25.0), *synth.pack_reads(pr.mate1), *synth.pack_reads(pr.mate2))
    pacbio = c.add_pacbio(api.single_cfg(mismatch_prob=0.15), np.full(30, 1200, np.int32))
    assert c.pacbio_stats(pacbio) == {"subwalks": 0, "records": 0, "misses": 0, "multi_launches": 0}
    filed = 0
    for k, (sub, n) in enumerate([(walk[:1], 3), (walk[:2], 0), (walk[1:4], 5), (walk[:1], 2)]):  # the last one: a sub-walk filed before
        rec = np.array([[10 * r, 10 * r + 1100, (7 * r + k) % 30] for r in range(n)], np.int32).reshape(-1, 3)
        c.put_pacbio_records(pacbio, sub, rec, np.linspace(-900.0, -1000.0, n))
        filed += n
        st = c.pacbio_stats(pacbio)
        assert st["subwalks"] == min(k + 1, 3) and st["records"] == filed, (k, st)
    assert c.pacbio_stats(pacbio) == {"subwalks": 3, "records": 10, "misses": 0, "multi_launches": 0}
    for rs in (paired, -1, 2):
        with pytest.raises(api.GamlHipError) as e:
            c.pacbio_stats(rs)
        assert e.value.code == api.EINVAL, rs


def test_pacbio_stats_is_declared(built):
    import os
    from gaml_amd import api
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "int gaml_hip_pacbio_stats(" in open(os.path.join(root, "include", "gaml_hip.h")).read()
    assert hasattr(api.lib(), "gaml_hip_pacbio_stats")
