"""Inputs of the single-end batch tests (tests/test_gpu_single_batch.py) and of their host-side check
(tests/test_single_batch_cases_host.py): the graph and the two families of tests/pacbio_batch_cases.py -- 8 candidates one
edit away from one assembly, 9 unrelated path sets -- and the single-end set FixtureA.context(single=True) adds, in three
layouts: the single-end set alone (BASELINE config 1 in small), beside the paired set, beside the paired and the PacBio set.
FLOORED_*: the single-end reads the oracle floors per set (of N_SINGLE); the rest have a value above 0; bad_bases is 0
everywhere."""
import pacbio_batch_cases as pc
from gaml_amd import synth

N_SINGLE, SINGLE_LEN = 500, 100
SINGLE_KW = dict(weight=0.25)
FLOORED_CANDIDATES = [416, 414, 417, 416, 416, 416, 426, 427]
FLOORED_UNRELATED = [407, 412, 317, 407, 500, 480, 414, 434, 481]
LAYOUTS = ("single", "paired+single", "paired+pacbio+single")


class Fixture(pc.FixtureA):
    def __init__(self):
        super().__init__()
        self.sr = synth.make_single_reads(self.genome, N_SINGLE, SINGLE_LEN, 0.01, pc.SEED + 1)  # what context(single=True) adds
        self.single_args = synth.pack_reads(self.sr)

    def layout(self, name, onepass=False, device=0):
        """(context, {"single": handle, "paired": handle or None, "pacbio": handle or None})"""
        from gaml_amd import api
        if name == "paired+pacbio+single":
            c, paired, pacbio = self.context(single=True, device=device)
            single = c.num_readsets() - 1
        else:
            c = api.Context(device=device)
            c.set_graph(*self.g.packed())
            pacbio = None
            paired = c.add_paired(api.paired_cfg(300.0, 30.0, weight=1.0), *self.paired_args) if name == "paired+single" else None
            single = c.add_single(api.single_cfg(**SINGLE_KW), *self.single_args)
        if onepass:
            c.set_single_onepass(True)
        return c, {"single": single, "paired": paired, "pacbio": pacbio}

    def oracle_single(self):
        """(oracle, handle) with the single-end set alone"""
        import oracle_py as op
        o = op.Oracle()
        o.set_graph(*self.g.packed())
        return o, o.add_single(*self.single_args, 0.01, op.single_cfg(**SINGLE_KW))

    def oracle_layout(self, name):
        import oracle_py as op
        if name == "single":
            return self.oracle_single()[0]
        o = op.Oracle()
        o.set_graph(*self.g.packed())
        o.add_paired(*self.paired_args, 0.01, op.paired_cfg(300.0, 30.0, weight=1.0))
        if name == "paired+pacbio+single":
            rs = o.add_pacbio(self.pb.lens, 0.15, op.single_cfg(**pc.PACBIO_KW))
            for wk, rec, lp in zip(self.pb.walks, self.pb.recs, self.pb.logps):
                o.pacbio_put(rs, wk, rec, lp)
        o.add_single(*self.single_args, 0.01, op.single_cfg(**SINGLE_KW))
        return o
