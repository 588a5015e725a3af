"""pacbio_dp_kernel at real read lengths against exact arithmetic (tests/pacbio_dp_reference.py: the same sum in
decimal.Decimal at 50 digits, no scaling, one log at the end).

Why not the oracle at 1e-9: a 4 kbp alignment is worth e^-3000, which only the kernel's own format -- a double times a
power of two shared by a 15-column chunk -- can hold; the reads of tests/test_gpu_pacbio_sam.py (<= 900 bases) all fit
a plain double, 1e-9 relative on a log of -3000 is 3e-6 on the probability, and the oracle rounds in log space at
every cell. Here the inputs go to e^-8000 and below, the error rate runs from 1e-4 to 0.24, row widths sit on both
sides of the LDS / global-scratch switch, and batched runs must reproduce single runs bit for bit.

The bound. Every term of the DP is non-negative, so nothing cancels and rounding errors add to first order. With
u = 2^-53, R band rows, n read bases, T rows whose computed cells include column n, and `want` the exact log:

    |got - want| <= u * (16 * (R + n) + (T + 8) * |want|)

  * a path through the band has at most R + n steps;
  * a step costs at most about 12 roundings: the two products and the add of the cell update; four multiply-adds of
    the scan; the powers g^2, g^4, g^8 of the left weight, carrying 1, 3 and 7 roundings over 2, 4 and 8 steps; the
    weights themselves, exp(log(match)) on the device, at most 3u for match >= 0.04. The 12 is rounded up to 16;
  * ldexp is exact; flushing inputs 2^1022 or more below their chunk's largest is invisible at this scale;
  * the result is log(cell) + S ln 2 with |S ln 2| about |want|: about 4 roundings relative to |want|, doubled to 8
    (the reference's own conversion to a double is one more);
  * one log-sum-exp per row that contains column n: T roundings relative to |want|.

For a 4 kbp read with full clip boxes that is about 8e-11 absolute on a log near -3000. The bound is a derivation; the
largest error / bound ratio seen on hardware is recorded in DESIGN.md, section 3."""
import numpy as np
import pytest

import pacbio_dp_reference as R
from gaml_amd import api
from oracle import oracle_py as O

pytestmark = pytest.mark.gpu


class _Worst:
    def __init__(self):
        self.ratio, self.rel, self.n = 0.0, 0.0, 0

    def report(self, what):
        print(f"{what}: {self.n} finite cases, worst error / bound {self.ratio:.4f}, worst relative error {self.rel:.3e}")


def _check(ctx, case, worst):
    """One alignment alone through the kernel: band exact, value within the bound, -inf exactly where the sum is 0."""
    ref = R.reference(case)
    got, lo, hi = ctx.debug_sam_logprob(case.target, case.read, case.line, case.mismatch, with_band=True)
    _, _, olo, ohi = O.sam_band(case.line, len(case.target))
    assert np.array_equal(lo, olo) and np.array_equal(hi, ohi), case.name
    if np.isinf(ref.logprob):
        print(f"{case.name}: got {got!r} want -inf")
        assert got == ref.logprob, (case.name, got)
        return got
    err, bound = abs(got - ref.logprob), R.bound(ref, len(case.read))
    print(f"{case.name}: m {case.mismatch:g} n {len(case.read)} R {ref.rows} T {ref.lse_terms} width {int((hi - lo + 1).max())} "
          f"got {got!r} want {ref.logprob!r} error {err:.3e} bound {bound:.3e} ratio {err / bound:.4f}")
    worst.n += 1
    worst.ratio = max(worst.ratio, err / bound)
    worst.rel = max(worst.rel, err / abs(ref.logprob))
    assert np.isfinite(got) and err <= bound, (case.name, got, ref.logprob, err, bound)
    return got


def test_long_reads_against_exact_arithmetic():
    """4 and 6 kbp reads, both strands, wrong-place records kept, clip boxes at the 200 cap: e^-2000 .. e^-8000."""
    ctx, worst = api.Context(), _Worst()
    cases = R.long_read_cases()
    assert {c.line.split("\t")[1] for c in cases} == {"0", "16"}
    for c in cases:
        _check(ctx, c, worst)
    worst.report("long reads")
    assert worst.n == len(cases)


def test_error_models():
    """mismatch_prob from 1e-4 to 0.24 (where a match is less likely than a mismatch), true and wrong-place records."""
    ctx, worst = api.Context(), _Worst()
    cases = R.error_model_cases()
    assert {c.mismatch for c in cases} == set(R.ERROR_RATES)
    for c in cases:
        _check(ctx, c, worst)
    worst.report("error models")
    assert worst.n == len(cases)


def test_chunk_and_lane_geometry():
    """Row widths 15 .. 34 across the LDS / scratch switch, column |read| on every lane of its chunk, both clip boxes
    at the cap, the first base, the separator, the end of the mirrored half, 'N' against 'N'."""
    ctx, worst = api.Context(), _Worst()
    cases, wanted = R.geometry_cases()
    by_name = {c.name: c for c in cases}
    for name, w in wanted.items():  # asserted here too, so the coverage cannot drift away from the kernel test
        assert R.max_row_width(by_name[name]) == w, name
    assert sorted(wanted[f"width{w}"] for w in R.GEOMETRY_WIDTHS) == [15, 16, 30, 31, 32, 33, 34]
    lens = sorted(len(c.read) for c in cases if c.name.startswith("len"))
    assert lens == list(range(lens[0], lens[0] + 15))
    for c in cases:
        _check(ctx, c, worst)
    worst.report("geometry")
    assert worst.n == len(cases) - 1  # across_separator is the one zero


def _fresh(g, rb, ro, names, mismatch):
    ctx = api.Context()
    ctx.set_graph(*g.packed())
    rs = ctx.add_pacbio_reads(api.single_cfg(min_prob_per_base=-1.0, mismatch_prob=mismatch), rb, ro, names)
    return ctx, rs


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def test_batched_equals_alone_bit_for_bit():
    """A job's arithmetic does not depend on its group, its neighbours' lengths, its scratch offset or the block it
    lands in: every filed value equals the single-alignment run of the same line, bit for bit, for batches that fill
    a wavefront partly, exactly, and several blocks with a ragged last one; and in reversed order."""
    g, walk, rb, ro, names, header, lines, cases = R.batch_world()
    dbg, worst = api.Context(), _Worst()
    alone = np.array([_check(dbg, c, worst) for c in cases])
    worst.report("batch lines alone")
    lens = [len(c.read) for c in cases]
    assert min(lens[0::2]) > 4 * max(lens[1::2])  # long, short, long, short within a wavefront
    orc = O.Oracle()
    orc.set_graph(*g.packed())
    ors = orc.add_pacbio_reads(rb, ro, names, R.BATCH_MISMATCH, O.single_cfg(min_prob_per_base=-1.0))
    assert orc.pacbio_ingest_sam(ors, walk, header + "\n" + "\n".join(lines) + "\n") == len(lines)
    orec, _ = orc.pacbio_records(ors, walk)
    jobs_seen = []
    for k in (1, 3, 4, 5, 15, 16, 17, 67):
        ctx, rs = _fresh(g, rb, ro, names, R.BATCH_MISMATCH)
        assert ctx.pacbio_ingest_sam(rs, walk, header + "\n" + "\n".join(lines[:k]) + "\n") == k
        rec = ctx.pacbio_records(rs, walk)
        assert rec is not None and len(rec) == k
        assert np.array_equal(rec["position"], orec[:k, 0]) and np.array_equal(rec["position_end"], orec[:k, 1])
        assert np.array_equal(rec["read_id"], orec[:k, 2])
        same = _bits(rec["logprob"]) == _bits(alone[:k])
        assert same.all(), (k, np.flatnonzero(~same).tolist(), rec["logprob"][~same].tolist(), alone[:k][~same].tolist())
        jobs_seen.append(int(ctx.pacbio_dp_stats(rs)["jobs"]))
        assert jobs_seen[-1] == k
    assert any(j % 4 for j in jobs_seen) and any(j > 16 for j in jobs_seen)
    ctx, rs = _fresh(g, rb, ro, names, R.BATCH_MISMATCH)
    assert ctx.pacbio_ingest_sam(rs, walk, header + "\n" + "\n".join(lines[::-1]) + "\n") == len(lines)
    rec = ctx.pacbio_records(rs, walk)
    assert np.array_equal(rec["read_id"], orec[::-1, 2]) and np.array_equal(rec["position"], orec[::-1, 0])
    same = _bits(rec["logprob"]) == _bits(alone[::-1])
    assert same.all(), np.flatnonzero(~same).tolist()


def test_gapped_multi_node_walk():
    """A walk with a 57-base gap: what is filed where and for which read equals the oracle's, each value the exact one."""
    g, gapped, ps, cases = R.gapped_world()
    rb = np.frombuffer("".join(ps.reads).encode(), np.uint8)
    ro = np.zeros(len(ps.reads) + 1, np.int64)
    ro[1:] = np.cumsum([len(r) for r in ps.reads])
    orc = O.Oracle()
    orc.set_graph(*g.packed())
    ors = orc.add_pacbio_reads(rb, ro, ps.names, R.GAPPED_MISMATCH, O.single_cfg(min_prob_per_base=-1.0))
    ctx, rs = _fresh(g, rb, ro, ps.names, R.GAPPED_MISMATCH)
    filed = ctx.pacbio_ingest_sam(rs, gapped, ps.sam)
    assert filed == orc.pacbio_ingest_sam(ors, gapped, ps.sam) and filed > 0.8 * len(cases)
    # a line's record: (start, end) relative to the first node of its sub-walk, and the read
    node_len = [g.node_len(x) if x >= 0 else -x for x in gapped]
    begins = np.concatenate([[0], np.cumsum(node_len)[:-1]])
    by_place = {}
    for c in cases:
        f = O.sam_band(c.line, len(c.target))[0]
        rid = ps.names.index(c.line.split("\t")[0].split("/")[0])
        assert (f["tstart"], f["tend"], rid) not in by_place
        by_place[(f["tstart"], f["tend"], rid)] = c
    worst, n_zero = _Worst(), 0
    for key in orc.pacbio_keys(ors):
        orec, _ = orc.pacbio_records(ors, list(key))
        got = ctx.pacbio_records(rs, list(key))
        assert got is not None and len(got) == len(orec), key
        assert np.array_equal(got["position"], orec[:, 0]) and np.array_equal(got["position_end"], orec[:, 1])
        assert np.array_equal(got["read_id"], orec[:, 2])
        ib = [i for i in range(len(gapped)) if tuple(gapped[i:i + len(key)]) == key]
        assert len(ib) == 1
        for r in got:
            c = by_place[(int(r["position"]) + int(begins[ib[0]]), int(r["position_end"]) + int(begins[ib[0]]), int(r["read_id"]))]
            ref, val = R.reference(c), float(r["logprob"])
            if np.isinf(ref.logprob):
                assert val == ref.logprob, c.name
                n_zero += 1
                continue
            err, bound = abs(val - ref.logprob), R.bound(ref, len(c.read))
            print(f"{c.name}: got {val!r} want {ref.logprob!r} error {err:.3e} bound {bound:.3e} ratio {err / bound:.4f}")
            worst.n += 1
            worst.ratio = max(worst.ratio, err / bound)
            worst.rel = max(worst.rel, err / abs(ref.logprob))
            assert np.isfinite(val) and err <= bound, (c.name, val, ref.logprob, err, bound)
    worst.report("gapped walk")
    assert worst.n + n_zero == filed and worst.n > 0.5 * len(cases)
    spans = [O.sam_band(c.line, len(c.target))[0] for c in cases]
    assert any("N" in c.target[f["posstart"]:f["posend"]] for c, f in zip(cases, spans))  # some rows are the gap's 'N's
