"""An exact referee for the PacBio alignment DP, and the inputs the DP tests share.

`exact_logprob` restates AligmentProbability (reference graph.cc:2175-2297) in linear space with decimal.Decimal at 50
digits. Decimal's exponent range is unbounded for this purpose, so a value like e^-9000 needs no scaling and no log
until the very end: nothing here shares the kernel's number format (a double times a power of two per 15-column
chunk) or the oracle's (a log-space double per cell). The cell set is the oracle's (`oracle_py.sam_band`); the cell
rules are those of tests/test_oracle_golden.py::test_alignment_dp_against_explicit_path_enumeration.

The case generators live here so that tests/test_pacbio_dp_reference_host.py (CPU: reference against the oracle, the
cases are well formed and deep enough) and tests/test_gpu_pacbio_dp.py (the kernel against the reference) draw the
same inputs. Everything is seeded; results are cached per process."""
import decimal
import functools
from collections import namedtuple

import numpy as np

import oracle_py as O
from gaml_amd import synth

PREC = 50
U = 2.0 ** -53

# one DP call: the SAM line, "path + '\n' + reverse complement", the whole read (fastq orientation) and the error rate
Case = namedtuple("Case", "name line target read mismatch")
Ref = namedtuple("Ref", "logprob rows lse_terms")


def _pm(a, b, match, mismatch, zero):  # MatchProbability, graph.h:555-564
    if a == "\n" or b == "\n":
        return zero
    return match if a == b else mismatch


def exact_logprob(line, target, read, mismatch):
    """(log probability or -inf, band rows R, rows T whose computed cells include column |read|)."""
    f, r0, lo, hi = O.sam_band(line, len(target))
    n, posstart, tlen = len(read), f["posstart"], len(target)
    with decimal.localcontext() as dc:
        dc.prec = PREC
        dc.Emax = decimal.MAX_EMAX
        dc.Emin = decimal.MIN_EMIN
        zero, one = decimal.Decimal(0), decimal.Decimal(1)
        match = decimal.Decimal(1.0 - 4 * mismatch)  # the doubles the library starts from
        mism = decimal.Decimal(mismatch)
        left_w = [_pm("-", ch, match, mism, zero) for ch in read]
        total, terms = zero, 0
        prev, plo, phi = [], 0, -1
        for i in range(len(lo)):
            l, h = int(lo[i]), int(hi[i])
            cur = [zero] * (h - l + 1)
            if l <= 0 <= h:
                cur[-l] = one  # column 0: the free start
            gi = r0 + i + posstart - 1
            if 0 <= gi < tlen:
                g = target[gi]
                up_w = _pm(g, "-", match, mism, zero)
                for c in range(max(l, 1), min(h, n) + 1):
                    v = zero
                    if plo <= c - 1 <= phi:
                        v += prev[c - 1 - plo] * _pm(g, read[c - 1], match, mism, zero)
                    if plo <= c <= phi:
                        v += prev[c - plo] * up_w
                    if c - 1 >= l:
                        v += cur[c - 1 - l] * left_w[c - 1]
                    cur[c - l] = v
                if max(l, 1) <= n <= h:
                    total += cur[n - l]
                    terms += 1
            prev, plo, phi = cur, l, h
        logp = float(total.ln()) if total > 0 else -np.inf
    return Ref(logp, len(lo), terms)


@functools.lru_cache(maxsize=None)
def reference(case):
    return exact_logprob(case.line, case.target, case.read, case.mismatch)


def bound(ref, read_len):
    """|got - want| allowed for a double-precision evaluation: see the derivation in tests/test_gpu_pacbio_dp.py."""
    return U * (16.0 * (ref.rows + read_len) + (ref.lse_terms + 8) * abs(ref.logprob))


def max_row_width(case):
    _, _, lo, hi = O.sam_band(case.line, len(case.target))
    return int((hi - lo + 1).max())


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def _one_node(length, seed):
    g = synth.make_graph(synth.make_genome(length, seed), [length])
    seq = synth.walk_string(g, [0])
    return g, seq + "\n" + synth.revcomp_str(seq)


def _sam_cases(prefix, ps, target, mismatch):
    rd = dict(zip(ps.names, ps.reads))
    out = []
    for k, line in enumerate(ps.sam.split("\n")[1:-1]):
        out.append(Case(f"{prefix}[{k}]", line, target, rd[line.split("\t")[0].split("/")[0]], mismatch))
    return out


LONG_SPECS = ((4000, 0.15, 31, 6), (6000, 0.05, 32, 6))  # read_len, mismatch_prob, seed, reads


@functools.lru_cache(maxsize=None)
def long_read_cases():
    """4 and 6 kbp reads cut from a one-node path, both strands, wrong-place secondary records kept, unaligned ends of
    up to 250 bases on most reads (clip boxes at the 200 cap)."""
    out = []
    for read_len, m, seed, n_reads in LONG_SPECS:
        g, target = _one_node(read_len + 2500, seed)
        ps = synth.make_pacbio_sam(g, [0], n_reads, read_len, seed, max_clip=250, clip_frac=0.7, secondary=0.5)
        out += _sam_cases(f"long{read_len}", ps, target, m)
    return tuple(out)


ERROR_RATES = (1e-4, 0.01, 0.05, 0.15, 0.2, 0.24)  # at 0.24 match = 0.04 < mismatch


@functools.lru_cache(maxsize=None)
def error_model_cases():
    """About 2-3 kbp reads whose true substitution / insertion / deletion rates follow the model's mismatch_prob; every
    read also has a wrong-place record (at 1e-4 that one is below -10000 while the true one is near 0)."""
    out = []
    for k, m in enumerate(ERROR_RATES):
        g, target = _one_node(4200, 50 + k)
        ps = synth.make_pacbio_sam(g, [0], 2, 3000, 60 + k, sub=m, ins=m, dele=m, secondary=1.0)
        out += _sam_cases(f"m{m:g}", ps, target, m)
    return tuple(out)


GEOMETRY_WIDTHS = (15, 16, 30, 31, 32, 33, 34)  # rows up to 32 cells stay in LDS, wider ones use the global scratch
GEOMETRY_MISMATCH = 0.15
CLIP_CAPPED = ("clip200_both", "clip200_both_mirrored")  # both clip boxes at the 200 cap
_HALF = 3000


def _rand(rng, n):
    return "".join("ACGT"[int(x)] for x in rng.integers(0, 4, n))


def _noisy(rng, s, rate=0.08):
    return "".join("ACGT"[int(rng.integers(4))] if rng.random() < rate else ch for ch in s)


def _line(flag, pos, cigar, span, seq_len, tags=()):
    return "\t".join(["q/1", str(flag), "p", str(pos), "254", cigar, "*", "0", str(span), "A" * seq_len, "*", *tags])


@functools.lru_cache(maxsize=None)
def geometry_cases():
    """Crafted lines. Returns (cases, wanted) where wanted maps a case name to the exact widest row it must have."""
    rng = np.random.default_rng(77)
    half = _rand(rng, _HALF)
    target = half + "\n" + synth.revcomp_str(half)
    m = GEOMETRY_MISMATCH
    cases, wanted = [], {}

    # one insertion run of k bases between matched stretches: the widest row is k + 9 cells (five path rows = the run
    # and four diagonal steps, widened by 2 on both sides), so the rows around it go LDS -> scratch -> LDS
    for w in GEOMETRY_WIDTHS:
        k, a, b, pos = w - 9, 700, 600, 200 + w
        read = _noisy(rng, half[pos:pos + a]) + _rand(rng, k) + _noisy(rng, half[pos + a:pos + a + b])
        name = f"width{w}"
        cases.append(Case(name, _line(0, pos, f"{a}M{k}I{b}M", a + b, len(read)), target, read, m))
        wanted[name] = w
    # two runs within five rows add up
    read = _noisy(rng, half[900:1400]) + _rand(rng, 13) + half[1400:1402] + _rand(rng, 12) + _noisy(rng, half[1402:1900])
    cases.append(Case("width34_two_runs", _line(0, 900, "500M13I2M12I498M", 1000, len(read)), target, read, m))
    wanted["width34_two_runs"] = 34

    # 15 consecutive read lengths: column |read| sits on each lane 1..15 of its chunk
    for n in range(1201, 1216):
        read = _noisy(rng, half[300:300 + n - 2]) + "GT"
        read = read[:400] + read[403:800] + "ACG" + read[800:]  # 400M 3D 397M 3I ...
        cig = f"400M3D397M3I{n - 800}M"
        cases.append(Case(f"len{n}", _line(0, 300, cig, n, len(read)), target, read, m))
        assert len(read) == n

    # both clip boxes at the 200 cap on a long alignment: XS - 1 = 259 unaligned bases in front, XQ - XE + 1 = 251 behind
    core = _noisy(rng, half[400:2400])
    core = core[:900] + core[905:]  # 900M 5D 1095M
    read = _rand(rng, 259) + core + _rand(rng, 251)
    tags = ("XS:i:260", f"XE:i:{260 + len(core)}", f"XQ:i:{len(read)}")
    cases.append(Case("clip200_both", _line(0, 400, "900M5D1095M", 2000, len(core), tags), target, read, m))
    # the same read on the mirrored strand: the boxes swap ends, the front box reaches above the first base of the half
    tags = ("XS:i:252", f"XE:i:{252 + len(core)}", f"XQ:i:{len(read)}")
    rc = synth.revcomp_str(read)
    cases.append(Case("clip200_both_mirrored", _line(16, 400, "900M5D1095M", 2000, len(core), tags), target, rc, m))

    # placement: row 1 on the first base, into the separator, the mirrored strand at the very end of the string
    r1 = _noisy(rng, half[0:800])
    cases.append(Case("pos0", _line(0, 0, "800M", 800, 800), target, r1, m))
    # the separator row passes nothing on: a read that has to cross it scores zero, one that ends within the band's
    # reach of it (column |read| is in the band two rows before the path gets there) does not
    r2 = _noisy(rng, half[_HALF - 500:]) + _rand(rng, 300)
    cases.append(Case("across_separator", _line(0, _HALF - 500, "800M", 800, 800), target, r2, m))
    r3 = _noisy(rng, half[_HALF - 798:]) + "AC"
    cases.append(Case("into_separator", _line(0, _HALF - 798, "800M", 800, 800), target, r3, m))
    tail = target[len(target) - 798:]  # the CIGAR is reversed with the strand: 498M 2I 300M along the second half
    cases.append(Case("mirrored_end", _line(16, 0, "300M2I498M", 798, 800), target, _noisy(rng, tail[:498]) + "CA" + _noisy(rng, tail[498:]), m))
    front = _rand(rng, 120)
    tags = ("XS:i:121", "XE:i:721", "XQ:i:720")
    cases.append(Case("clip_above_row_one", _line(0, 3, "600M", 600, 600, tags), target, front + _noisy(rng, half[3:603]), m))

    # a gapped walk: 57 'N' path bases against a read that carries 'N's too (equal letters match, whatever they are)
    left, right = _rand(rng, 900), _rand(rng, 900)
    nhalf = left + "N" * 57 + right
    ntarget = nhalf + "\n" + synth.revcomp_str(nhalf)
    nread = _noisy(rng, left[200:]) + "N" * 20 + _rand(rng, 17) + "N" * 20 + _noisy(rng, right[:700])
    cases.append(Case("n_run", _line(0, 200, "1457M", 1457, 1457), ntarget, nread, m))
    cases.append(Case("n_run_mirrored", _line(16, 200, "1457M", 1457, 1457), ntarget, synth.revcomp_str(nread), m))
    return tuple(cases), wanted


BATCH_MISMATCH = 0.15
BATCH_LINES = 67


@functools.lru_cache(maxsize=None)
def batch_world():
    """(graph, walk, read bases, read offsets, names, header, lines, cases): 67 SAM lines on a one-node walk, long and
    short reads alternating so that one wavefront carries alignments of very different lengths. Every line is filed
    under the walk itself, in SAM order."""
    g, target = _one_node(5200, 41)
    long_ps = synth.make_pacbio_sam(g, [0], 32, 2600, 42, max_clip=120, clip_frac=0.5)
    short_ps = synth.make_pacbio_sam(g, [0], 32, 160, 43, clip_frac=0.5)
    names = list(long_ps.names) + ["s" + x[1:] for x in short_ps.names]
    reads = list(long_ps.reads) + list(short_ps.reads)
    long_lines = long_ps.sam.split("\n")[1:-1]
    short_lines = ["s" + l[1:] for l in short_ps.sam.split("\n")[1:-1]]
    lines = [l for pair in zip(long_lines, short_lines) for l in pair][:BATCH_LINES]
    assert len(lines) == BATCH_LINES
    rd = dict(zip(names, reads))
    cases = tuple(Case(f"batch[{k}]", l, target, rd[l.split("\t")[0].split("/")[0]], BATCH_MISMATCH) for k, l in enumerate(lines))
    rb = np.frombuffer("".join(reads).encode(), np.uint8)
    ro = np.zeros(len(reads) + 1, np.int64)
    ro[1:] = np.cumsum([len(r) for r in reads])
    return g, [0], rb, ro, names, "@HD\tVN:1.0", lines, cases


GAPPED_MISMATCH = 0.15


@functools.lru_cache(maxsize=None)
def gapped_world():
    """(graph, walk with a 57-base gap, PacbioSam, cases): the multi-node case of test_path_with_gap_and_tiny_nodes."""
    gen = synth.make_genome(30000, 13)
    g = synth.make_graph(gen, synth.cut_lengths(30000, 13, long_rng=(1500, 4000)))
    walk = synth.genome_walk(g)
    gapped = walk[:3] + [-57] + walk[4:8]
    ps = synth.make_pacbio_sam(g, gapped, 40, 700, 5)
    seq = synth.walk_string(g, gapped)
    cases = tuple(_sam_cases("gapped", ps, seq + "\n" + synth.revcomp_str(seq), GAPPED_MISMATCH))
    return g, gapped, ps, cases


def debug_cases():
    """Every case that goes through the single-alignment entry point."""
    return long_read_cases() + error_model_cases() + geometry_cases()[0] + batch_world()[7]


def all_cases():
    return debug_cases() + gapped_world()[3]
