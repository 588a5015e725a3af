"""The exact referee of the PacBio alignment DP (tests/pacbio_dp_reference.py) and the inputs of
tests/test_gpu_pacbio_dp.py, checked without a GPU: the Decimal DP against an explicit enumeration of alignment paths
and against the oracle's logdouble DP on every shared input, the depth of those inputs (far below what a plain double
holds), and the host side's `max_width` -- the kernel's scratch sizing -- against the materialised band on random and
adversarial CIGARs."""
import math

import numpy as np

import pacbio_dp_reference as R
from gaml_amd import api
from oracle import oracle_py as O

RTOL = 1e-10  # the suite's number for "a DP against another statement of the same sum" (test_oracle_golden.py)


def _enumerate_paths(line, target, read, mism):
    """Sum over every monotone path through the banded cell set, one path at a time (exponential: tiny inputs)."""
    match = 1.0 - 4 * mism

    def pm(a, b):
        if a == "\n" or b == "\n":
            return 0.0
        return match if a == b else mism

    f, r0, lo, hi = O.sam_band(line, len(target))
    n = len(read)
    cells = {(r0 + i, c) for i in range(len(lo)) for c in range(int(lo[i]), int(hi[i]) + 1)}

    def usable(r, c):  # a cell the DP computes (graph.cc:2246-2255)
        return (r, c) in cells and 1 <= c <= n and 0 <= r + f["posstart"] - 1 < len(target)

    total = 0.0

    def walk(r, c, w):
        nonlocal total
        if c == n:
            total += w  # every computed cell of the last column is summed (graph.cc:2279-2281)
        for dr, dc in ((1, 1), (1, 0), (0, 1)):
            rr, cc = r + dr, c + dc
            if not usable(rr, cc):
                continue
            g = target[rr + f["posstart"] - 1]
            step = pm(g, read[cc - 1]) if (dr, dc) == (1, 1) else pm(g, "-") if (dr, dc) == (1, 0) else pm("-", read[cc - 1])
            if step > 0.0:
                walk(rr, cc, w * step)

    for (r, c) in sorted(cells):
        if c == 0:  # free start in column 0: value 1, never recomputed
            for dr, dc in ((1, 1), (0, 1)):
                rr, cc = r + dr, c + dc
                if usable(rr, cc):
                    g = target[rr + f["posstart"] - 1]
                    step = pm(g, read[cc - 1]) if dr else pm("-", read[cc - 1])
                    if step > 0.0:
                        walk(rr, cc, step)
    return total


def test_reference_against_explicit_path_enumeration():
    """The six tiny cases of test_alignment_dp_against_explicit_path_enumeration, at its tolerance."""
    half = "ACGTTGCAAGCT"
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    target = half + "\n" + "".join(comp[ch] for ch in reversed(half))
    cases = [
        ("q/1\t0\tp\t3\t1\t4M\t*\t0\t4\tTTGC\t*", "TTGC"),
        ("q/1\t0\tp\t2\t1\t2M1I2M\t*\t0\t4\tGTATG\t*", "GTATG"),
        ("q/1\t0\tp\t4\t1\t2M1D2M\t*\t0\t5\tTGAA\t*", "TGAA"),
        ("q/1\t16\tp\t2\t1\t3M\t*\t0\t3\tAGC\t*", "GCT"),
        ("q/1\t0\tp\t10\t1\t4M\t*\t0\t4\tGCTA\t*", "GCTA"),
        ("q/1\t0\tp\t5\t1\t2M\t*\t0\t2\tGC\t*\tXS:i:2\tXE:i:4\tXQ:i:4", "AGCT"),
    ]
    for line, read in cases:
        total = _enumerate_paths(line, target, read, 0.15)
        ref = R.exact_logprob(line, target, read, 0.15)
        assert total > 0.0 and math.isfinite(ref.logprob), line
        assert abs(ref.logprob - math.log(total)) <= RTOL * abs(ref.logprob), (line, ref, math.log(total))
        assert ref.rows == len(O.sam_band(line, len(target))[2]) and 1 <= ref.lse_terms <= ref.rows


def test_reference_agrees_with_the_oracle_on_every_shared_input():
    """Every case of the GPU module is well formed: the oracle's logdouble DP and the Decimal DP agree to 1e-10, and
    are -inf together."""
    worst = 0.0
    cases = R.all_cases()
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        ref = R.reference(c)
        orc = O.sam_alignment_logprob(c.line, c.target, c.read, c.mismatch)
        if np.isinf(ref.logprob) or np.isinf(orc):
            assert ref.logprob == orc, (c.name, ref.logprob, orc)
            continue
        rel = abs(orc - ref.logprob) / abs(ref.logprob)
        worst = max(worst, rel)
        assert rel <= RTOL, (c.name, orc, ref.logprob)
    print(f"oracle against the exact reference: worst relative difference {worst:.3e} over {len(cases)} cases")


def test_inputs_force_the_scaled_format():
    """exp(-745) is below the smallest subnormal double: a kernel that dropped, clamped or misplaced the shared
    exponent cannot produce these values."""
    longs = [R.reference(c).logprob for c in R.long_read_cases()]
    assert len(longs) >= 12 and all(np.isfinite(longs))
    assert sum(v < -745.0 for v in longs) >= 0.75 * len(longs), sorted(longs)
    assert min(longs) < -8000.0, min(longs)
    for m in R.ERROR_RATES:  # every error model has finite cases, its wrong-place records far below a double's range
        vals = [R.reference(c).logprob for c in R.error_model_cases() if c.mismatch == m]
        assert vals and all(np.isfinite(vals)) and min(vals) < -745.0, (m, vals)
    batch = [R.reference(c).logprob for c in R.batch_world()[7]]
    assert sum(v < -745.0 for v in batch) >= 20 and sum(v > -745.0 for v in batch) >= 20


def test_geometry_cases_hit_what_they_aim_at():
    cases, wanted = R.geometry_cases()
    by_name = {c.name: c for c in cases}
    assert sorted(wanted[f"width{w}"] for w in R.GEOMETRY_WIDTHS) == [15, 16, 30, 31, 32, 33, 34]
    for name, w in wanted.items():
        assert R.max_row_width(by_name[name]) == w, (name, R.max_row_width(by_name[name]), w)
    lens = sorted(len(c.read) for c in cases if c.name.startswith("len"))
    assert lens == list(range(lens[0], lens[0] + 15))
    for name in R.CLIP_CAPPED:
        c = by_name[name]
        sh, _ = api.debug_sam_shape(c.line, len(c.target))
        f = O.sam_band(c.line, len(c.target))[0]
        assert sh["bl"] == 200 and sh["el"] == 200 and f["sstart"] > 200 and f["slen"] - f["send"] >= 200, (name, sh, f)
    f = O.sam_band(by_name["pos0"].line, len(by_name["pos0"].target))[0]
    assert f["posstart"] == 0
    c = by_name["mirrored_end"]
    assert O.sam_band(c.line, len(c.target))[0]["posend"] == len(c.target)
    c = by_name["across_separator"]
    f = O.sam_band(c.line, len(c.target))[0]
    assert f["posstart"] < c.target.index("\n") < f["posend"]
    assert "N" in by_name["n_run"].read and "N" in by_name["n_run"].target
    c = by_name["into_separator"]
    assert O.sam_band(c.line, len(c.target))[0]["posend"] == c.target.index("\n") + 2
    for c in cases:  # one zero on purpose: the kernel must say -inf there, and only there
        assert np.isfinite(R.reference(c).logprob) == (c.name != "across_separator"), c.name


# ---------------------------------------------------------------------------------------------------------------------
# max_width, the scratch sizing of the kernel, against the materialised band
# ---------------------------------------------------------------------------------------------------------------------
TOTAL = 2 * 5000 + 1


def _sam(cigar, pos=700, flag=0, tags=()):
    return "\t".join(["q/1", str(flag), "p", str(pos), "1", cigar, "*", "0", "50", "ACGTACGTAC", "*", *tags])


def _check_width(line, with_oracle=False):
    _, _, lo, hi = api.debug_sam_band(line, TOTAL)
    if with_oracle:  # the oracle materialises the cell list: too slow for thousands of lines
        _, _, olo, ohi = O.sam_band(line, TOTAL)
        assert np.array_equal(lo, olo) and np.array_equal(hi, ohi), line
    sh, _ = api.debug_sam_shape(line, TOTAL)
    widest = int((hi - lo + 1).max())
    assert sh["max_width"] >= widest, (line, widest, sh)
    return widest


def _random_cigar(rng):
    style = int(rng.integers(0, 6))
    ops = []
    if style == 0:  # anything, zero-length operations included
        for _ in range(int(rng.integers(1, 14))):
            ops.append((int(rng.integers(0, 9)), "MID"[int(rng.integers(3))]))
    elif style == 1:  # long insertion runs separated by a single M or D
        for _ in range(int(rng.integers(2, 8))):
            ops.append((int(rng.integers(1, 120)), "I"))
            ops.append((1, "MD"[int(rng.integers(2))]))
    elif style == 2:  # leading and trailing insertions on 1-5 rows: both clip boxes inside one 5-row window
        ops.append((int(rng.integers(1, 320)), "I"))
        rows = int(rng.integers(1, 6))
        for _ in range(rows):
            ops.append((1, "MD"[int(rng.integers(2))]))
            if rng.random() < 0.3:
                ops.append((int(rng.integers(0, 40)), "I"))
        ops.append((int(rng.integers(1, 320)), "I"))
    elif style == 3:  # only insertions
        for _ in range(int(rng.integers(1, 4))):
            ops.append((int(rng.integers(0, 300)), "I"))
    elif style == 4:  # long deletion runs between insertions
        for _ in range(int(rng.integers(1, 6))):
            ops.append((int(rng.integers(1, 60)), "D"))
            ops.append((int(rng.integers(0, 50)), "I"))
            ops.append((int(rng.integers(0, 4)), "M"))
    else:  # adjacent insertion operations with zero-length operations between them
        for _ in range(int(rng.integers(1, 6))):
            ops += [(int(rng.integers(1, 30)), "I"), (0, "MD"[int(rng.integers(2))]), (int(rng.integers(1, 30)), "I"),
                    (int(rng.integers(1, 4)), "M")]
    return "".join(f"{n}{c}" for n, c in ops)


def _random_tags(rng):
    u = rng.random()
    if u < 0.4:
        return ()
    xs = int(rng.choice([1, 2, 5, 150, 199, 200, 201, 202, 260, 900]))
    tail = int(rng.choice([0, 1, 4, 150, 198, 199, 200, 201, 260, 900]))
    xe = xs + int(rng.integers(1, 60))
    return (f"XS:i:{xs}", f"XE:i:{xe}", f"XQ:i:{xe - 1 + tail}")


def test_max_width_bounds_every_row_of_random_and_adversarial_cigars():
    rng = np.random.default_rng(2024)
    seen_wide, seen_capped = 0, 0
    for _ in range(4000):
        line = _sam(_random_cigar(rng), pos=int(rng.choice([0, 1, 3, 150, 700])), flag=int(rng.choice([0, 16])),
                    tags=_random_tags(rng))
        w = _check_width(line)
        seen_wide += w > 32
        seen_capped += api.debug_sam_shape(line, TOTAL)[0]["bl"] == 200
    assert seen_wide > 500 and seen_capped > 100
    fixed = [
        _sam("300I1M300I"), _sam("300I1D300I"), _sam("1M"), _sam("0M"), _sam("250I"), _sam("0I0M0D"), _sam("*"),
        _sam("199I3M199I"), _sam("200I3M200I"), _sam("201I3M201I"), _sam("500D"), _sam("2M500D2M"), _sam("90I1M90I1M90I1M90I1M90I1M90I"),
        _sam("90I1D90I1D90I1D90I1D90I1D90I"), _sam("5M0D0I0M5I0D5I5M"), _sam("1M250I1M250I1M"),
        _sam("3M", tags=("XS:i:260", "XE:i:263", "XQ:i:520")), _sam("3M", pos=2, tags=("XS:i:260", "XE:i:263", "XQ:i:520")),
        _sam("3M", flag=16, tags=("XS:i:201", "XE:i:204", "XQ:i:403")), _sam("1D", tags=("XS:i:150", "XE:i:150", "XQ:i:299")),
        _sam("5S10M"), _sam("4M3D4M", tags=("XS:i:1", "XE:i:9", "XQ:i:8")),
        # a leading run keeps column 0 in rows 0..2; their windows reach path row 6: seven runs in one widened row, where
        # max_width once counted the five longest (390 cells against a bound of 382)
        _sam("11I1M38I1M109I1D109I1D10I1M104I1M", pos=0), _sam("1I1M90I1M90I1M90I1M90I1M90I1M90I1M"),
        _sam("1M80I1M80I1M80I1M80I1M80I1M80I1M", tags=("XS:i:4", "XE:i:6", "XQ:i:5")),
    ]
    for line in fixed:
        _check_width(line, with_oracle=True)
    # every line the GPU module sends to the kernel
    for c in R.all_cases():
        _, _, lo, hi = api.debug_sam_band(c.line, len(c.target))
        sh, _ = api.debug_sam_shape(c.line, len(c.target))
        assert sh["max_width"] >= int((hi - lo + 1).max())
