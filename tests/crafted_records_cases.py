"""Hand-made alignment records at the branch points of the paired and single-end scorers: the single source of
tests/test_crafted_records_host.py (CPU) and tests/test_gpu_crafted_records.py. Pure Python and numpy.

Nothing here is aligned: reads are random bases, every window a case scores is filed from outside
(gaml_hip_put_window_records / the oracle's orc_put_window_records), windows without crafted records with an empty list.
A case is a list of PAIR PATTERNS -- records (mate, window, position, edit, orientation) -- each repeated over `copies`
consecutive read ids, a config, its path sets and what it expects of pair_classes() and static_index_pairs after the first
blocking call on path_sets[0]. Every pattern declares its class by hand (`cls`), so a pattern that lands on the other side of
its boundary fails the count. A record's position counts from the start of its window's first node (graph.cc:577: the
scorers add the node's start in the path)."""
import math
from functools import lru_cache

import numpy as np

from gaml_amd import synth

NODE_LENS = (6000, 4000, 120, 200, 5000)  # two nodes below kWindowTail, three far above it
A, B, C, D, E = 0, 2, 4, 6, 8             # node 2i is piece i forward, 2i + 1 its twin
WINDOW_TAIL = 300                         # kMinSubpathLength graph.cc:27
SEED = 4242
FOLD_BELOW = 1024                         # GAML_FOLD_CLASS2_BELOW
MEMO_CODES = 4                            # kMemoCodes
CLASS_SIZES = (1, 63, 64, 65, 255, 256, 257)
DEFAULT_CFG = dict(mean=300.0, sd=30.0, mismatch=0.01, penalty_constant=0.0, penalty_step=50.0, min_prob_per_base=-0.7,
                   min_prob_start=-10.0)


@lru_cache(maxsize=None)
def graph():
    return synth.make_graph(synth.make_genome(sum(NODE_LENS), SEED), list(NODE_LENS))


def node_len(x):
    return NODE_LENS[x >> 1]


def contigs(path):
    """[(start in the path, nodes)] of a path's stretches between gap entries (graph.cc:1808-1824)."""
    out, cur, at, start = [], [], 0, 0
    for x in path:
        if x < 0:
            out.append((start, cur))
            at += -x
            cur, start = [], at
        else:
            cur.append(x)
            at += node_len(x)
    out.append((start, cur))
    return out


def windows_of(paths):
    """The window rule (oracle positions_only_path / precompute_for_paths, graph.cc:447-598): node i's window extends until
    the tail behind it exceeds 300 bases, and a node longer than 300 also has a window of its own."""
    out = []
    for p in paths:
        for _, ctg in contigs(p):
            for i in range(len(ctg)):
                w, tail = [ctg[i]], 0
                for x in ctg[i + 1:]:
                    tail += node_len(x)
                    w.append(x)
                    if tail > WINDOW_TAIL:
                        break
                for key in (tuple(w), (ctg[i],)) if node_len(ctg[i]) > WINDOW_TAIL else (tuple(w),):
                    if key not in out:
                        out.append(key)
    return out


def occurrences(paths):
    """{window: [(path index, path position of the window's position 0, visiting rank)]} in visiting order."""
    occ = {}
    for k, p in enumerate(paths):
        rank = 0
        for start, ctg in contigs(p):
            at = start
            for i in range(len(ctg)):
                w, tail = [ctg[i]], 0
                for x in ctg[i + 1:]:
                    tail += node_len(x)
                    w.append(x)
                    if tail > WINDOW_TAIL:
                        break
                look = [tuple(w)] + ([(ctg[i],)] if node_len(ctg[i]) > WINDOW_TAIL and len(w) > 1 else [])
                for key in look:
                    occ.setdefault(key, []).append((k, at, rank))
                    rank += 1
                at += node_len(ctg[i])
    return occ


def ins_n(mean, sd):
    """Length of the insert-size table (paired_host_tabs): the first distance behind the mean whose Gaussian is exactly
    0.0 in f64."""
    d = 0
    while True:
        z = (float(d) - mean) / sd
        if math.exp(-z * z / 2.0) / (math.sqrt(2 * math.pi) * sd) == 0.0 and float(d) > mean:
            return d
        d += 1


def pair_dist(p1, o1, p2, o2, L1, L2):
    """The orientation rule and insert distance of graph.cc:1864-1876 on path positions; None: no term."""
    if o1 == o2:
        return None
    if p1 < p2:
        return p2 - p1 + L2 if (o1, o2) == (0, 1) else None
    return p1 - p2 + L1 if (o1, o2) == (1, 0) else None


class Pattern:
    """recs: [(mate, window, position, edit, orientation)] in the order they are filed; cls: 'static' (compact class with a
    static memo index, kStaticZero included), 'compact', 'two', 'four', 'more'; term: (e1, e2, distance) when the pair has
    exactly one term under path_sets[0], () when it has none, a list of them when it has several, None when not stated."""
    def __init__(self, name, recs, cls, copies=1, lens=(100, 100), term=None, aim=""):
        self.name, self.recs, self.cls, self.copies, self.lens, self.aim = name, recs, cls, copies, lens, aim
        # every term of the pair under path_sets[0], in any order; None: not stated
        self.terms = None if term is None else [] if term == () else list(term) if isinstance(term, list) else [term]

    @property
    def term(self):
        return None if self.terms is None or len(self.terms) > 1 else tuple(self.terms[0]) if self.terms else ()

    def __repr__(self):
        return self.name


class Case:
    def __init__(self, name, family, patterns, path_sets, cfg=None, single=False, gap=None, fillers=0):
        self.name, self.family, self.patterns, self.path_sets, self.single, self.gap = name, family, patterns, path_sets, single, gap
        self.cfg = dict(DEFAULT_CFG, **(cfg or {}))
        self.fillers = fillers  # pairs without records in front, each with a length combination of its own

    def __repr__(self):
        return self.name

    @property
    def ins_n(self):
        return ins_n(self.cfg["mean"], self.cfg["sd"])

    @property
    def floor_positive(self):
        return all(math.exp(self.cfg["min_prob_start"] + self.cfg["min_prob_per_base"] * v) > 0.0 for v in range(0, 601))

    def expected_classes(self):
        """pair_classes() after the first call: [compact, <= 2 records, <= 4, more]; a class of 3-4 records with at most
        FOLD_BELOW pairs goes to the last one (tb_pairkey_kernel)."""
        n = {"static": self.fillers, "compact": 0, "two": 0, "four": 0, "more": 0}
        for p in self.patterns:
            n[p.cls] += p.copies
        if 0 < n["four"] <= FOLD_BELOW:
            n["more"] += n["four"]
            n["four"] = 0
        return [n["static"] + n["compact"], n["two"], n["four"], n["more"]]

    def expected_static(self, device=True):
        """static_index_pairs; device=False: what the host restatement (debug_static_check) counts, whatever the floor"""
        if device and not self.floor_positive:
            return 0  # paired_static_ins_n: no static indices without a positive floor
        return self.fillers + sum(p.copies for p in self.patterns if p.cls == "static")

    def n_reads(self):
        return self.fillers + sum(p.copies for p in self.patterns)

    def all_path_sets(self):
        """Every path set a test of the case scores: its own, the eight of the batch test and the gap profile's."""
        out = list(self.path_sets) + batch_sets(self)
        if self.gap:
            out += [self.gap[0]] + [gap_paths(self.gap, l) for l in self.gap[3]]
        return out


FILLER_LENS = ((61, 62), (62, 61), (63, 64), (64, 63))


class Built:
    """A case turned into arrays: lens[mate], packed random reads, records per (mate, window) in filing order, and who
    each read is."""
    def __init__(self, case):
        self.case = case
        n = case.n_reads()
        self.n = n
        self.lens = [np.zeros(n, np.int64), np.zeros(n, np.int64)]
        self.who = []
        recs = {}
        rid = 0
        for k in range(case.fillers):
            self.lens[0][rid], self.lens[1][rid] = FILLER_LENS[k]
            self.who.append(("filler", k))
            rid += 1
        self.first = {}
        for p in case.patterns:
            self.first[p.name] = rid
            for c in range(p.copies):
                self.lens[0][rid], self.lens[1][rid] = p.lens
                for (mate, win, pos, edit, orient) in p.recs:
                    recs.setdefault((mate, tuple(win)), []).append((pos, edit, rid, orient))
                self.who.append((p.name, c))
                rid += 1
        assert rid == n
        self.recs = {k: np.array(v, np.int32).reshape(-1, 4) for k, v in recs.items()}
        mates = (0,) if case.single else (0, 1)
        wins = []
        for s in case.all_path_sets():
            for w in windows_of(s):
                if w not in wins:
                    wins.append(w)
        for (_, w) in self.recs:
            if w not in wins:
                wins.append(w)
        self.windows = wins
        self.mates = mates
        rng = np.random.default_rng(SEED + 1)
        self.reads = []
        for mt in mates:
            offs = np.zeros(n + 1, np.int64)
            offs[1:] = np.cumsum(self.lens[mt])
            bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=int(offs[-1]))]
            self.reads.append((np.ascontiguousarray(bases), offs))

    def label(self, rid):
        name, c = self.who[rid]
        return f"{self.case.name}/{name} copy {c} (read {rid})"

    def reads_of(self, name):
        p = next(q for q in self.case.patterns if q.name == name)
        return range(self.first[name], self.first[name] + p.copies)

    def records(self, mate, win):
        return self.recs.get((mate, tuple(win)), np.zeros((0, 4), np.int32))

    # ---- the two sides, fed the same puts
    def library(self, device=0, knobs=()):
        from gaml_amd import api
        c, k = self.case.cfg, self.case
        ctx = api.Context(device=device)
        for knob, v in knobs:
            ctx.debug_set_knob(knob, v)
        ctx.set_graph(*graph().packed())
        if k.single:
            rs = ctx.add_single(api.single_cfg(c["penalty_constant"], c["penalty_step"], c["min_prob_per_base"], c["min_prob_start"], 1.0,
                                               c["mismatch"]), *self.reads[0])
        else:
            rs = ctx.add_paired(api.paired_cfg(c["mean"], c["sd"], c["penalty_constant"], c["penalty_step"], c["min_prob_per_base"],
                                               c["min_prob_start"], 1.0, c["mismatch"]), *self.reads[0], *self.reads[1])
        for mt in self.mates:
            for w in self.windows:
                r = self.records(mt, w)
                a = np.zeros(len(r), api.ALIGMENT)
                if len(r):
                    a["position"], a["edit_dist"], a["read_id"], a["orientation"] = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
                ctx.put_window_records(rs, mt, list(w), a)
        return ctx, rs

    def oracle(self):
        import oracle_py as op
        c, k = self.case.cfg, self.case
        o = op.Oracle()
        o.set_graph(*graph().packed())
        if k.single:
            rs = o.add_single(*self.reads[0], c["mismatch"], op.single_cfg(c["penalty_constant"], c["penalty_step"], c["min_prob_per_base"],
                                                                          c["min_prob_start"], 1.0))
        else:
            rs = o.add_paired(*self.reads[0], *self.reads[1], c["mismatch"],
                              op.paired_cfg(c["mean"], c["sd"], c["penalty_constant"], c["penalty_step"], c["min_prob_per_base"],
                                            c["min_prob_start"], 1.0))
        for mt in self.mates:
            for w in self.windows:
                o.put_window_records(rs, mt, list(w), self.records(mt, w))
        return o, rs


def batch_sets(case):
    """Eight path sets made from the case's: the sets, their reversals, and splits of the first."""
    s0, s1 = case.path_sets[0], case.path_sets[min(1, len(case.path_sets) - 1)]
    h = max(1, len(s0) // 2)
    out = [s0, s0[::-1], s0[:h], s0[h:], s1, s1[::-1], s0[:1] + s1[-1:], case.path_sets[-1]]
    return [list(s) for s in out]


def gap_paths(gap, length):
    paths, pid, pos, _ = gap
    out = [list(p) for p in paths]
    out[pid][pos] = -int(length)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# pattern makers
# ---------------------------------------------------------------------------------------------------------------------
WA, WB, WC, WE = (A,), (B,), (C,), (E,)


def pair(name, p1, o1, p2, o2, cls, e1=0, e2=0, lens=(100, 100), w1=WA, w2=WA, copies=1, aim="", same_path=True):
    """One record per mate; the term follows from pair_dist on the path positions (the two windows start at the same path
    position when they are the same window; same_path=False: they lie on different paths)."""
    d = pair_dist(p1, o1, p2, o2, *lens) if same_path else None
    return Pattern(name, [(0, w1, p1, e1, o1), (1, w2, p2, e2, o2)], cls, copies, lens, () if d is None else (e1, e2, d), aim)


def fwd(name, d, cls, base=1000, **kw):
    """x.pos < y.pos, orientations (0, 1), distance d"""
    L2 = kw.get("lens", (100, 100))[1]
    return pair(name, base, 0, base + d - L2, 1, cls, **kw)


def rev(name, d, cls, base=1000, **kw):
    """x.pos >= y.pos (equal when d is mate 1's length), orientations (1, 0), distance d"""
    L1 = kw.get("lens", (100, 100))[0]
    return pair(name, base + d - L1, 1, base, 0, cls, **kw)


def general(p):
    """The same single term in the two-record class: mate 1 gets a second record whose orientation rules it out against
    mate 2's (so the term goes through pair_term, kernels.hip.h, not through the compact class's tables)."""
    (m0, w0, p0, e0, o0), (m1, w1, p1, e1, o1) = p.recs
    return Pattern(p.name + "+2", [p.recs[0], (0, w0, 5900, 0, o1), p.recs[1]], "two", p.copies, p.lens, p.term, p.aim)


# ---------------------------------------------------------------------------------------------------------------------
# A. one record per mate: the pair term
# ---------------------------------------------------------------------------------------------------------------------
EDITS_100 = [((0, 0), "static"), ((6, 6), "static"), ((6, 7), "compact"), ((7, 6), "compact"), ((7, 7), "compact"),  # memo: edit < 7
             ((63, 63), "compact"), ((63, 64), "two"), ((64, 0), "two"), ((0, 64), "two"), ((100, 100), "two")]       # tb_rec8_fits: edit < 64
ORIENT_ORDER = [(o1, o2, rel) for o1 in (0, 1) for o2 in (0, 1) for rel in ("<", ">", "==")]


def family_a_patterns(mean, sd):
    n, end = ins_n(mean, sd), int(mean + 5 * sd)
    L = 100
    pats = []
    # edit counts on both sides of 7 and 64 (compact_prep, tb_class_kernel, tb_rec8_fits), at the mean
    for (e1, e2), cls in EDITS_100:
        pats.append(fwd(f"edits{e1}_{e2}", int(mean), cls, e1=e1, e2=e2, aim="edit < 7 / edit < 64"))
    # distances: x.pos == y.pos (the `else` branch, dist = L1), the reference's table end (graph.cc:1801-1804, 1877-1882)
    # and the end of the library's table (pair_term, compact_term_tables: dist >= ins_n)
    pats.append(rev("dist_L_same_pos_10", L, "static", aim="x.pos == y.pos scores as (1, 0)"))
    pats.append(pair("dist_L_same_pos_01", 1000, 0, 1000, 1, "compact", aim="x.pos == y.pos does not score as (0, 1)"))
    for d, cls in ((L + 1, "static"), (int(mean), "static"), (end - 1, "static"), (end, "static"), (n - 2, "static"), (n - 1, "static"),
                   (n, "compact"), (n + 1000, "compact")):
        for mk in (fwd, rev):
            p = mk(f"{mk.__name__}_dist{d}", d, cls, aim="dist against ins_n / (int)(mean + 5 sd)")
            pats += [p, general(p)]
    # all four orientations, each with x.pos <, > and == y.pos (graph.cc:1864-1876)
    for o1, o2, rel in ORIENT_ORDER:
        p1, p2 = {"<": (1000, 1200), ">": (1200, 1000), "==": (1100, 1100)}[rel]
        scores = pair_dist(p1, o1, p2, o2, L, L) is not None
        pats.append(pair(f"orient{o1}{o2}{rel}", p1, o1, p2, o2, "static" if scores else "compact", aim="orientation rule x order"))
    assert sum(1 for p in pats if p.name.startswith("orient") and p.term != ()) == 3
    # the mates on different paths of the set: no term; a mate / both mates without a record: kStaticZero
    pats.append(pair("other_path", 1000, 0, 1200, 1, "compact", w1=WA, w2=WB, same_path=False, aim="y.path != x.path"))
    pats.append(Pattern("mate2_missing", [(0, WA, 1000, 0, 0)], "static", term=(), aim="kStaticZero"))
    pats.append(Pattern("mate1_missing", [(1, WA, 1000, 0, 1)], "static", term=(), aim="kStaticZero"))
    pats.append(Pattern("both_missing", [], "static", term=(), aim="kStaticZero"))
    # across the gap of the gap profile's path [A, -g, B]: a term only there, its distance moves with g
    pats.append(pair("across_gap", 5950, 0, 10, 1, "compact", w1=WA, w2=WB, same_path=False, aim="gap profile"))
    return pats


A_SETS = [[[A], [B]], [[A], [B ^ 1]], [[B], [A]]]
A_GAP = ([[A, -10, B]], 0, 1, [1, 160, 1300])


def case_a(name, cfg, fillers=0):
    c = dict(DEFAULT_CFG, **cfg)
    pats = family_a_patterns(c["mean"], c["sd"])
    if fillers:  # every combination of lengths now has a code >= kMemoCodes: nothing but kStaticZero is static
        for p in pats:
            if p.cls == "static" and len(p.recs) == 2:
                p.cls = "compact"
    return Case(name, "A", pats, A_SETS, cfg, gap=A_GAP, fillers=fillers)


LEN_COMBOS = [((100, 100), "static"), ((100, 90), "static"), ((90, 100), "static"), ((80, 80), "static"),  # codes 0-3: in the memo
              ((110, 70), "compact"), ((70, 110), "compact")]                                              # codes 4, 5: lc >= kMemoCodes


def case_a_lencodes():
    pats = []
    for (L1, L2), cls in LEN_COMBOS:  # the same records under every combination; the distance follows the lengths
        pats.append(pair(f"len{L1}_{L2}_fwd", 1000, 0, 1200, 1, cls, e1=2, e2=3, lens=(L1, L2), copies=3, aim="lc < kMemoCodes"))
        pats.append(pair(f"len{L1}_{L2}_rev", 1200, 1, 1000, 0, cls, e1=6, e2=0, lens=(L1, L2), copies=2, aim="lc < kMemoCodes"))
    # edits on both sides of 7 under the first combination, with other combinations' terms behind them in the memo
    pats += [fwd(f"edits{e1}_{e2}", 300, "compact", e1=e1, e2=e2, aim="edit < 7 with four codes in the memo") for e1, e2 in ((6, 7), (7, 6), (7, 7))]
    return Case("A_lencodes", "A", pats, A_SETS)


def case_a_len300():
    pats = [fwd("edits255_255", 450, "two", e1=255, e2=255, lens=(300, 300), aim="edit up to min(255, L)"),
            fwd("edits6_6", 450, "static", e1=6, e2=6, lens=(300, 300)),
            fwd("edits64_6", 450, "two", e1=64, e2=6, lens=(300, 300)),
            rev("same_pos", 300, "static", lens=(300, 300))]
    return Case("A_len300", "A", pats, A_SETS)


def case_a_floor(name, cfg):
    n = ins_n(300.0, 30.0)
    pats = [fwd("mean", 300, "static", copies=3), fwd("edits7_7", 300, "compact", e1=7, e2=7), fwd("edits64_0", 300, "two", e1=64),
            fwd("at_ins_n", n, "compact"), general(fwd("at_ins_n", n, "compact")), fwd("before_ins_n", n - 1, "static"),
            Pattern("mate2_missing", [(0, WA, 1000, 0, 0)], "static", term=()), Pattern("both_missing", [], "static", term=(), copies=2)]
    return Case(name, "A", pats, A_SETS, cfg)


def case_sizes(n):
    """n pairs in the whole read set, all of one class (n = 1: one pair in the whole set)"""
    return Case(f"A_total{n}", "A", [fwd("mean", 300, "static", copies=n, aim="class walked in waves / blocks of 256")], A_SETS)


def case_sizes_mixed():
    recs4 = [(0, WA, 1000 + 40 * k, k, 0) for k in range(3)] + [(1, WA, 1250 + 40 * k, 0, 1) for k in range(4)]
    recs5 = [(0, WA, 1000 + 40 * k, k, 0) for k in range(5)] + [(1, WA, 1250, 0, 1)]
    pats = [fwd("static", 300, "static", copies=257), fwd("compact", 300, "compact", e1=7, copies=255), general(fwd("gen", 310, "two", copies=65)),
            Pattern("four", recs4, "four", copies=63), Pattern("more", recs5, "more", copies=1)]
    return Case("A_sizes_mixed", "A", pats, A_SETS)


# ---------------------------------------------------------------------------------------------------------------------
# B. several records and candidates
# ---------------------------------------------------------------------------------------------------------------------
K1K2 = [(1, 1), (2, 1), (1, 2), (2, 2), (3, 1), (3, 3), (4, 4), (5, 1), (1, 5), (5, 5)]  # tb_class_kernel: 1, 2, 4, more


def multi(name, k1, k2, copies=1, win=WA):
    """k1 records of mate 1 (orientation 0) in front of k2 of mate 2 (orientation 1): k1 * k2 terms, edits tell them apart"""
    recs = [(0, win, 1000 + 40 * k, k, 0) for k in range(k1)] + [(1, win, 1250 + 40 * k, k, 1) for k in range(k2)]
    m = max(k1, k2)
    cls = "static" if m <= 1 else "two" if m <= 2 else "four" if m <= 4 else "more"
    terms = [(i, j, 250 + 40 * (j - i) + 100) for i in range(k1) for j in range(k2)]
    return Pattern(name, recs, cls, copies, term=terms, aim="records per mate 1 / 2 / 4 / more")


def case_b_records():
    pats = [multi(f"k{k1}_{k2}", k1, k2, copies=3) for k1, k2 in K1K2]
    # candidates of one pair on two paths: four combinations, the two on the same path count (y.path != x.path)
    pats.append(Pattern("two_paths", [(0, WA, 1000, 0, 0), (0, WB, 2000, 1, 0), (1, WA, 1200, 0, 1), (1, WB, 2210, 1, 1)], "two", copies=2,
                        term=[(0, 0, 300), (1, 1, 310)], aim="same-path combinations only"))
    return Case("B_records", "B", pats, A_SETS)


def case_b_fold(copies):
    """the 3-4-record class at GAML_FOLD_CLASS2_BELOW and one above it"""
    return Case(f"B_fold{copies}", "B", [multi("k4_4", 4, 4, copies=copies), multi("k1_1", 1, 1, copies=2), multi("k2_2", 2, 2, copies=1)],
                [[[A]], [[A], [B]]])


CAND_COUNTS = (31, 32, 33, 64, 65, 128, 129)  # kGenCands = 32, live_mask_src's 64, kOvfCap = 128


def case_b_candidates():
    """a short node's window in N one-node paths beside the real walk: N candidates per record"""
    pats = [Pattern("one_rec", [(0, WC, 5, 1, 0), (1, WC, 15, 2, 1)], "static", copies=2, aim="candidates = N"),
            # two records per mate, two terms per path and both the same double (equal edits, distance 110 either way round): the
            # sum of 2 N equal terms does not depend on the order the scorer visits them in, so the per-read bound of 4e-16
            # holds at every N. (With four different terms per path the library's record-major order and the reference's
            # path-major order part by a few ulp per hundred terms: 3.8e-15 measured at N = 64, 256 terms.)
            Pattern("two_recs", [(0, WC, 5, 1, 0), (0, WC, 50, 1, 1), (1, WC, 15, 2, 1), (1, WC, 40, 2, 0)], "two", copies=2, aim="candidates = 2 N"),
            Pattern("overwritten", [(0, WC, 5, 1, 0), (0, WC, 5, 4, 0), (1, WC, 15, 0, 1)], "two", aim="later record at the same position, N times"),
            fwd("beside", 300, "static", copies=2)]
    return Case("B_candidates", "B", pats, [[[A]] + [[C]] * n for n in CAND_COUNTS])


# ---------------------------------------------------------------------------------------------------------------------
# C. overwrite rule (graph.cc:583-592) and position filter (:577)
# ---------------------------------------------------------------------------------------------------------------------
WAB = (A, B)
P_FILTER = 6050  # the largest position any record of A's windows has in family C: B's windows are filtered at P - 5


def case_c():
    y = (1, WA, 5200, 0, 1)
    yb = (1, WB, 300, 0, 1)
    pats = [
        # junction window first, then the node alone, same path position: the node's record survives (edit 3)
        Pattern("junction_then_solo", [(0, WAB, 5000, 1, 0), (0, WA, 5000, 3, 0), y], "static", term=(3, 0, 300),
                aim="a later window's record wins; dominated record"),
        # equal (position, read) inside one window: the stable sort keeps the filing order, the later one survives
        Pattern("same_key_1_then_4", [(0, WA, 5000, 1, 0), (0, WA, 5000, 4, 0), y], "two", term=(4, 0, 300), aim="input order decides"),
        Pattern("same_key_4_then_1", [(0, WA, 5000, 4, 0), (0, WA, 5000, 1, 0), y], "two", term=(1, 0, 300), aim="input order decides"),
        # a record of [A, B] in B's part at P; B's own window at P - 6 (dropped), P - 5 (kept), P (overwrites)
        Pattern("filter_P-6", [(0, WAB, P_FILTER, 0, 0), (0, WB, P_FILTER - 6000 - 6, 2, 0), yb], "two", term=(0, 0, 350), aim="al.pos < max_pos - 5"),
        Pattern("filter_P-5", [(0, WAB, P_FILTER, 0, 0), (0, WB, P_FILTER - 6000 - 5, 2, 0), yb], "two", term=[(0, 0, 350), (2, 0, 355)],
                aim="al.pos < max_pos - 5"),
        Pattern("filter_P", [(0, WAB, P_FILTER, 0, 0), (0, WB, P_FILTER - 6000, 2, 0), yb], "two", term=(2, 0, 350), aim="overwrites at P"),
    ]
    return Case("C_overwrite_filter", "C", pats, [[[A, B]], [[A, B], [E]], [[E], [A, B]]])


# ---------------------------------------------------------------------------------------------------------------------
# D. coverage penalty (graph.cc:1883-1919; coverage_sweep_words)
# ---------------------------------------------------------------------------------------------------------------------
D_CFG = dict(mean=300.0, sd=30.0, penalty_constant=0.001, penalty_step=50.0)  # cov_move = 250, far = 450
COV_MOVE, FAR = 250, 450
D_PATHS = [[E, -500, E ^ 1], [A, -500, B], [B ^ 1], [A ^ 1]]
# marks per window (window positions); a single position is a pair on one position (x.pos == y.pos, orientations (1, 0)), a
# tuple a pair (0, 1) with its two marks
D_MARKS = {
    (E,): [(0, 31), (32, 63),  # bits 0, 31, 32, 63 of the first path
           313,                # 63 + 250: p - q == cov_move but p - lb < far
           700,                # counted (387): predecessor twelve words back
           950,                # p - q == cov_move, p - lb > far: not counted
           1201,               # p - q == cov_move + 1: counted
           1400, 2900],        # counted 1500; the 40/40 pair at 2800 must not split it
    (E ^ 1,): [0,              # a mark ON the contig start 5500: lb == p > q
               460,            # lb == q: counted (460)
               4992, 4993, 4994, 4995, 4996, 4997, 4998, 4999, 5000],  # the path's last positions, every one marked
    (A,): [300,                # first mark of the second path: no predecessor of its own, the path before ends in marks
           5900],              # counted
    (B,): [460, 710, 961],     # 460: a contig start in (q, p] although p - q and p - lb are large; 710: == cov_move; 961: counted
    (B ^ 1,): [199, 450,       # p - lb == far: not counted
               3999],          # the last base of the path
    (A ^ 1,): [200, 451],      # p - lb == far + 1: counted
}
# what the sweep has to do with some of them: (path, q, p, counted)
D_EXPECT = [(0, 63, 313, False), (0, 313, 700, True), (0, 700, 950, False), (0, 950, 1201, True), (0, 1400, 2900, True),
            (0, 2900, 5500, False), (0, 5500, 5960, True), (1, 300, 5900, True), (1, 5900, 6960, False), (1, 6960, 7210, False),
            (1, 7210, 7461, True), (2, 199, 450, False), (2, 450, 3999, True), (3, 200, 451, True)]


def case_d():
    pats = []
    for win, marks in D_MARKS.items():
        for m in marks:
            if isinstance(m, tuple):
                pats.append(pair(f"marks{win[0]}_{m[0]}_{m[1]}", m[0], 0, m[1], 1, "static", w1=win, w2=win, aim="two marks"))
            else:
                pats.append(pair(f"mark{win[0]}_{m}", m, 1, m, 0, "static", w1=win, w2=win, aim="one mark"))
    # below the coverage threshold exp(floor_start + floor_per_base * 2 L2): scores, leaves no mark
    pats.append(pair("no_mark_2800", 2800, 1, 2800, 0, "compact", e1=40, e2=40, w1=WE, w2=WE, aim="p1 p2 ip > thr"))
    return Case("D_coverage", "D", pats, [D_PATHS, D_PATHS[:3] + [[A ^ 1, C]], D_PATHS[::-1]], D_CFG)


def case_d_sizes():
    """coverage marks from every class: the same sweep when the marks come through pair_term (two-record class)"""
    pats = [general(pair(f"mark_{m}", m, 1, m, 0, "static", w1=WA, w2=WA)) for m in (300, 1000, 1250, 1501)]
    pats.append(pair("pairs", 2000, 0, 2200, 1, "static", copies=64))
    return Case("D_general", "D", pats, [[[A], [B]], [[A], [E]], [[B], [A]]], D_CFG)


def record_positions(case, paths):
    """per read: per mate the path positions [(path, position, edit, orientation)] of its records in windows that occur
    exactly once in `paths` (family D: every window does)"""
    occ = occurrences(paths)
    b = Built(case)
    out = [([], []) for _ in range(b.n)]
    for (mate, win), recs in b.recs.items():
        if win not in occ:
            continue
        assert len(occ[win]) == 1, win
        k, at, _ = occ[win][0]
        for pos, edit, rid, orient in recs.tolist():
            out[rid][mate].append((k, at + pos, edit, orient))
    return b, out


def term_f64(cfg, e1, e2, L1, L2, dist):
    """the pair term in plain doubles (only to decide on which side of a far-away threshold it lies)"""
    m, M = cfg["mismatch"], 1.0 - 4 * cfg["mismatch"]
    z = (dist - cfg["mean"]) / cfg["sd"]
    return (m ** e1 * M ** (L1 - e1)) * (m ** e2 * M ** (L2 - e2)) * math.exp(-z * z / 2.0) / (math.sqrt(2 * math.pi) * cfg["sd"])


def expected_bad_bases(case, paths):
    """The module's own sweep (the head of set_kernels.hip.h): per path the sorted marks; a mark p adds p - q, q the mark
    before it, when no contig start lies in (q, p], p - q > cov_move and p - (contig start before p) > mean + 5 sd."""
    cfg = case.cfg
    cov_move, far = cfg["mean"] - cfg["penalty_step"], cfg["mean"] + 5 * cfg["sd"]
    b, pos = record_positions(case, paths)
    marks = [[] for _ in paths]
    for rid, (xs, ys) in enumerate(pos):
        L1, L2 = int(b.lens[0][rid]), int(b.lens[1][rid])
        thr = math.exp(cfg["min_prob_start"] + cfg["min_prob_per_base"] * (L2 + L2))  # graph.cc:1855-1857
        for (k1, p1, e1, o1) in xs:
            for (k2, p2, e2, o2) in ys:
                d = pair_dist(p1, o1, p2, o2, L1, L2) if k1 == k2 else None
                if d is not None and term_f64(cfg, e1, e2, L1, L2, d) > thr:
                    marks[k1] += [max(p1, p2), min(p1, p2)]
    bad, decided = 0, {}
    for k, p in enumerate(paths):
        starts = [s for s, _ in contigs(p)]
        ms = sorted(marks[k])
        for q, pp in zip(ms, ms[1:]):
            lb = max(s for s in starts if s <= pp)
            counted = lb <= q and pp - q > cov_move and pp - lb > far
            decided[(k, q, pp)] = counted
            if counted:
                bad += pp - q
    return bad, decided


# ---------------------------------------------------------------------------------------------------------------------
# E. single-end set (graph.cc:1650-1743): mate 0 only
# ---------------------------------------------------------------------------------------------------------------------
E_SETS = [[[A, B], [C], [C]], [[A, B], [C], [D]], [[C], [A, B], [C]]]


def single_patterns(total):
    """the same reads whatever the total; `plain` fills up to `total` reads"""
    pats = [
        Pattern("once", [(0, WB, 500, 0, 0)], None, aim="one record, window occurs once"),
        Pattern("outside", [(0, WE, 10, 0, 0)], None, aim="window outside the scored paths"),
        Pattern("solo_unused", [(0, WA, 10, 0, 0)], None, aim="AddPositions looks at junction windows only"),
        Pattern("several", [(0, WAB, 100, 1, 0), (0, WAB, 200, 2, 1), (0, WB, 300, 0, 0)], None, aim="several records"),
        Pattern("same_abs_pos", [(0, WAB, 6100, 1, 0), (0, WB, 100, 3, 0)], None, aim="later window overwrites at the same absolute position"),
        Pattern("same_key", [(0, WB, 700, 1, 0), (0, WB, 700, 4, 1)], None, aim="d.k > x.k: input order decides"),
        Pattern("same_key_swapped", [(0, WB, 700, 4, 1), (0, WB, 700, 1, 0)], None, aim="d.k > x.k: input order decides"),
        Pattern("two_paths", [(0, WC, 5, 0, 0)], None, aim="per-path offset 1,000,000: both count"),
        Pattern("two_paths_two_recs", [(0, WC, 5, 2, 0), (0, WC, 6, 0, 1)], None, aim="per-path offset"),
        Pattern("none", [], None, aim="no record"),
        Pattern("edit64", [(0, WB, 900, 64, 0)], None, aim="edit 64"),
        Pattern("editL", [(0, WB, 901, 100, 1)], None, aim="edit L"),
    ]
    if total == 1:
        return [pats[0]]
    assert total >= len(pats) + 1
    return pats + [Pattern("plain", [(0, WB, 1000, 0, 0)], None, copies=total - len(pats))]


def case_e(total):
    return Case(f"E_single{total}", "E", single_patterns(total), E_SETS, single=True)


def expected_single(case, paths):
    """per read: the edits that count under `paths` (the later record at an absolute position wins; a window in two paths
    counts in both), from the module's own occurrence list -- junction windows only (AddPositions graph.cc:600-649)"""
    b = Built(case)
    occ = {}
    for k, p in enumerate(paths):
        rank = 0
        for start, ctg in contigs(p):
            at = start
            for i in range(len(ctg)):
                w, tail = [ctg[i]], 0
                for x in ctg[i + 1:]:
                    tail += node_len(x)
                    w.append(x)
                    if tail > WINDOW_TAIL:
                        break
                occ.setdefault(tuple(w), []).append((k, at, rank))
                rank += 1
                at += node_len(ctg[i])
    seen = [dict() for _ in range(b.n)]
    for k in range(len(paths)):
        cands = []
        for (mate, win), recs in b.recs.items():
            for (kk, at, rank) in occ.get(win, []):
                if kk == k:
                    cands += [(rank, j, rid, 1_000_000 * k + at + pos, edit) for j, (pos, edit, rid, _) in enumerate(recs.tolist())]
        for rank, j, rid, apos, edit in sorted(cands):
            seen[rid][apos] = edit
    return b, [sorted(s.values()) for s in seen]


# ---------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def cases():
    # (mismatch 0.04 in the first: at 0.01 the (100, 100) pair's 0.01^200 is below the smallest double)
    out = [case_a("A_mean300", dict(mismatch=0.04)), case_a("A_mean220", dict(mean=220.0, sd=10.0, mismatch=0.05)), case_a_lencodes(), case_a_len300(),
           case_a_floor("A_floor_default", {}),
           # min_prob_start = 80; with the per-base term at -0.1 the floor e^60 sits above every value
           case_a_floor("A_floor_high", dict(min_prob_start=80.0, min_prob_per_base=-0.1)),
           case_a_floor("A_floor_underflow", dict(min_prob_per_base=-5.0)),  # exp(-10 - 5 * 200) == 0.0
           case_sizes_mixed()]
    out += [case_sizes(n) for n in CLASS_SIZES]
    out += [case_b_records(), case_b_fold(FOLD_BELOW), case_b_fold(FOLD_BELOW + 1), case_b_candidates(), case_c(), case_d(), case_d_sizes()]
    out += [case_e(n) for n in (1, 64, 257, 1500)]
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


def late_codes(name):
    """The family-A case `name` with four pairs without records in front, each with lengths of its own: the case's own
    combination of lengths gets a code >= kMemoCodes. Read r of the case is read r + 4 here."""
    c = case(name)
    return case_a(name + "_late", {k: v for k, v in c.cfg.items() if DEFAULT_CFG[k] != v}, fillers=len(FILLER_LENS))
