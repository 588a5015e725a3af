"""Cases for the scoring kernels' work split -- which block, lane, wave and round scores which read: the single source of
tests/test_grid_split_host.py (CPU) and tests/test_gpu_grid_split.py. Built on Pattern / Case / Built of
tests/crafted_records_cases.py: nothing is aligned, every record is put from outside on the library and on the oracle.

The crafted cases repeat one pattern over many reads; a lane that scored its neighbour's slot would not show there. Here
every pair of a class has a term of its own -- (e1 + e2, distance) differs from pair to pair, so no two pairs of a class
share their per-read value -- and a few pairs per class are floored at known slots, the first and the last among them.

The grid-cap knobs of the development build (GRID_CAP_*, include/gaml_hip_debug.h) bring the block counts down to 1, 2 or 3,
so that a few thousand pairs run every class's stride loop for three rounds and more, the last one ragged inside a wave.
The sizes below are the smallest that do so under every cap the tests use (CAPS); the arithmetic stands beside each."""
from functools import lru_cache

import numpy as np

import crafted_records_cases as cc
from crafted_records_cases import A, B, C, D, E, WA, WB, Case, Pattern

K_BLOCK = 256          # kBlock: threads per block
WAVES = K_BLOCK // 64  # waves per block: the wave-per-pair blocks and the PacBio scorer hand out one item per wave
# The cap settings of the GPU tests, by the layout's parts: static part of class 0 (GRID_CAP_COMPACT), its rest
# (GRID_CAP_COMPACT_REST), the 2-record class (GRID_CAP_CLASS1), the 3-4-record class (GRID_CAP_CLASS2), delta pairs
# (GRID_CAP_DELTA), wave-per-pair blocks (GRID_CAP_OVERFLOW)
PARTS = ("static", "rest", "two", "four", "delta", "more")
CAPS = {"all1": dict.fromkeys(PARTS, 1), "all3": dict.fromkeys(PARTS, 3),
        "mixed": dict(static=3, rest=1, two=2, four=2, delta=1, more=1)}
KNOB_OF_PART = dict(static="GRID_CAP_COMPACT", rest="GRID_CAP_COMPACT_REST", two="GRID_CAP_CLASS1", four="GRID_CAP_CLASS2",
                    delta="GRID_CAP_DELTA", more="GRID_CAP_OVERFLOW")
# slots a block takes per round: paired_static4_body and paired_compact4_body four per lane, every other loop one per lane
# (paired_compact_body takes two per iteration: counted in rounds of one, it makes twice as many) or one per wave
PER_ROUND = dict(static=4 * K_BLOCK, rest=4 * K_BLOCK, two=K_BLOCK, four=K_BLOCK, delta=K_BLOCK, more=WAVES)

# The largest cap is 3 blocks. A class of n slots under a cap of b blocks makes ceil(n / (b * PER_ROUND)) rounds; the third
# round exists when n > 2 * 3 * PER_ROUND, and it is ragged inside a wave when n mod (b * PER_ROUND) is no multiple of 64.
N_STATIC = 2 * 3 * 1024 + 513  # 6,657 = 6 * 1,024 + 513: under 1 block 7 rounds, the last of 513 slots (lanes 0 .. 255 take two, lane 0 a
#                                third; in its last refill the clamp); under 3 blocks 3 rounds, the last of 513
N_REST = 2 * 3 * 1024 + 37     # 6,181: 7 rounds of 1,024 + 37 under 1 block, 3 rounds under 3, lanes 0 .. 36 of wave 0 in the last
N_TWO = 2 * 3 * 256 + 37       # 1,573: 7 trips under 1 block, 4 under 2 (3 * 512 + 37), 3 under 3 (2 * 768 + 37); 37 lanes of wave 0 last
N_FOUR = 2 * 3 * 256 + 37      # 1,573 > FOLD_BELOW: the class keeps its own blocks
N_DELTA = 2 * 3 * 256 + 37     # 1,573 pairs of the static part gain a record when [B] joins the path set
N_SPILL = 5                    # ... and five of them six: long lists, scored by the wave-per-pair blocks
N_MORE = 2 * 3 * WAVES + 1     # 25 pairs with five records on a mate; with the five long lists 30 items = 2 * 12 + 6: under 3
#                                blocks (12 waves) 3 rounds, six waves in the last; under 1 block (4 waves) 8 rounds, two waves in the last
MISMATCH = 0.04                # 0.04^20 0.84^180 stays far above the floor (crafted_records_cases.cases())
MEAN, SD = 300.25, 30.0        # a mean between two distances: no two distances have the same Gaussian
FAR_ALONG = 777                # this pair of a class lies 2,500 bases behind the others: an uncovered stretch for the coverage sweep to count
D_LO = 101                     # the smallest distance of a (0, 1) pair of 100-base reads


def _edits(s, row, rest):
    """edit counts with e1 + e2 = s: both below 7 (memo), or -- rest -- one of them at 7 or above (no static index)"""
    if rest:
        lo = (row % min(7, s - 6))
        return (s - lo, lo) if row % 2 else (lo, s - lo)
    lo, hi = max(0, s - 6), min(6, s)
    e1 = lo + row % (hi - lo + 1)
    return e1, s - e1


def _terms(n, rest=False):
    """n terms (e1, e2, distance), no two with the same (e1 + e2, distance): 13 (rest: 14) edit sums by as many distances
    as it takes, upwards from D_LO"""
    sums = list(range(7, 21)) if rest else list(range(13))
    return [(*_edits(sums[j % len(sums)], j // len(sums), rest), D_LO + j // len(sums)) for j in range(n)]


def _pair(name, term, cls, j, lens, extra=(), far=False):
    """x.pos < y.pos, orientations (0, 1); `extra`: further records of mate 1 that no record of mate 2 pairs with"""
    e1, e2, d = term
    base = 5000 if j == FAR_ALONG else 1000 + 3 * (j % 97)
    recs = [(0, WA, base, e1, 0)] + list(extra) + [(1, WA, base + d - lens[1], e2, 1)]
    return Pattern(name, recs, cls, 1, lens, () if far else (e1, e2, d))


def _ruled_out(k):
    """k records of mate 1 with mate 2's orientation: candidates without a term (graph.cc:1864-1876)"""
    return [(0, WA, 5900 - 10 * q, 0, 1) for q in range(k)]


def _class(prefix, n, cls, lens_of, rest=False, extra=(), n_far=3):
    """n pairs of one class: the first, the middle and the last have a distance of ins_n and beyond (no term: floored)"""
    far_at = {0: 0, n // 2: 1, n - 1: 2} if n_far == 3 else {0: 0, n - 1: 2}
    ins = cc.ins_n(MEAN, SD)
    pats, floored = [], []
    terms = _terms(n, rest)
    for j in range(n):
        if j in far_at:
            t = (terms[j][0], terms[j][1], ins + 500 * far_at[j])
            floored.append(f"{prefix}{j}")
        else:
            t = terms[j]
        pats.append(_pair(f"{prefix}{j}", t, cls, j, lens_of(j), extra, far=j in far_at))
    return pats, floored


# the static part of class 0: a term far below the floor (static all the same: its distance lies inside the table)
FAR_STATIC = (6, 6, 900)


def split_patterns(n_static, lens_of, with_others=True):
    """The patterns of a split case in read order, the names of the floored pairs, and per part the names in slot order.
    Record tables order a class by (window of mate 1, window of mate 2, read), a missing record last (build_pair_tables):
    every record here lies in one window, so a class is in read order with the pairs without a record at its end."""
    pats, floored, order = [], [], {}
    terms = _terms(n_static)
    n_delta = N_DELTA if with_others else 0
    deltas, static_names = [], []
    for j in range(n_static - 3):
        is_delta = j % 4 == 1 and len(deltas) < n_delta
        far = j in (0, 2048) or (is_delta and len(deltas) in (0, n_delta - 1))
        t = FAR_STATIC if far else terms[j]
        name = f"{'delta' if is_delta else 'static'}{j}"
        k = len(deltas)
        extra = []
        if is_delta:  # records in [B]'s window: in the tables only once [B] is part of a path set; five pairs get six of them
            extra = [(0, WB, 100 + (2 * k + q) % 3500, q % 3, 0) for q in range(6 if k % 300 == 7 and k < 300 * N_SPILL else 1)]
            deltas.append(name)
        p = _pair(name, t, "static", j, lens_of(j), extra)
        if far:
            floored.append(name)
        pats.append(p)
        static_names.append(name)
    # the last three slots of the static part: kStaticZero
    tail = [Pattern("static_mate2_missing", [(0, WA, 1000, 0, 0)], "static", term=()), Pattern("static_mate1_missing", [(1, WA, 1000, 0, 1)], "static", term=()),
            Pattern("static_both_missing", [], "static", term=())]
    pats += tail
    floored += [p.name for p in tail]
    order["static"] = static_names + [p.name for p in tail]
    order["delta"] = deltas
    if with_others:
        for part, n, cls, rest, extra in (("rest", N_REST, "compact", True, ()), ("two", N_TWO, "two", False, _ruled_out(1)),
                                          ("four", N_FOUR, "four", False, _ruled_out(2)), ("more", N_MORE, "more", False, _ruled_out(4))):
            ps, fl = _class(part, n, cls, lens_of, rest, extra, n_far=3 if n > 100 else 2)
            pats += ps
            floored += fl
            order[part] = [p.name for p in ps]
    return pats, floored, order


S_BUILD, S_NONE, S_MAIN, S_GEN = [[A]], [[E]], [[A], [B]], [[A], [A], [B]]


class SplitCase(Case):
    """path_sets: the set the record tables are built under, the set the capped call scores ([B] joins: the delta pairs gain
    their records), the same with [A] twice (GEN: every record has two candidates, every term counts twice) and a set under
    which no pair scores."""
    def __init__(self, name, n_static=N_STATIC, two_lens=False, cfg=None, knobs=(), with_others=True):
        lens_of = (lambda j: (100, 90) if j % 2 else (100, 100)) if two_lens else (lambda j: (100, 100))
        pats, self.floored, self.order = split_patterns(n_static, lens_of, with_others)
        super().__init__(name, "S", pats, [S_BUILD, S_MAIN, S_GEN, S_NONE], dict(dict(mean=MEAN, sd=SD, mismatch=MISMATCH), **(cfg or {})))
        self.knobs = tuple(knobs)  # (name of an api.Knob, value): the variant's own switches
        self.with_others = with_others

    def sizes(self, no_memo=False):
        """slots per part of the launch under S_MAIN (the wave-per-pair part: table pairs, then the long delta lists)"""
        n = {part: len(self.order.get(part, ())) for part in PARTS}
        n["more"] += N_SPILL if self.with_others else 0
        if no_memo:  # no static indices: class 0 is one range, scored by paired_compact_body through the rest's blocks
            n["rest"] += n["static"]
            n["static"] = 0
        return n


def rounds(n, blocks, per_round):
    """(rounds the busiest lane or wave makes, slots of the last round) of n slots over `blocks` blocks"""
    width = blocks * per_round
    return -(-n // width), n - (-(-n // width) - 1) * width


def ragged(n, blocks, per_round):
    """The last round leaves some lanes of one wave without a slot (a lane enters a round when its first slot exists) or,
    wave per item, some waves of one block."""
    last = rounds(n, blocks, per_round)[1]
    if per_round < K_BLOCK:
        return last % WAVES != 0
    return min(last, blocks * K_BLOCK) % 64 != 0


def block_of_slot(slot, blocks, per_round):
    """which of a part's blocks scores its slot number `slot` (every stride loop: slot = block * 256 + lane + k * blocks * 256;
    wave per item: item = block * 4 + wave + k * blocks * 4)"""
    unit = K_BLOCK if per_round >= K_BLOCK else WAVES
    return slot % (blocks * unit) // unit


@lru_cache(maxsize=None)
def split_cases():
    """The variants of the paired case, each another body or instantiation of paired_score_kernel, and two siblings of the
    static part alone at one full round (`more` is false at the boundary) and one slot more (a second round, one live lane)."""
    pen = dict(penalty_constant=0.001, penalty_step=50.0)
    return (SplitCase("split_one_combo"),                                       # the lean entry, ONE = true
            SplitCase("split_two_combos", two_lens=True),                       # the LDS tables of paired_main_body
            SplitCase("split_no_memo", knobs=(("NO_MEMO", 1),)),                # paired_compact_body, two per iteration
            SplitCase("split_penalty", cfg=pen),                                # the COV instantiation
            SplitCase("split_penalty_general", cfg=pen, knobs=(("NO_COV_INSTANCE", 1),)),
            SplitCase("static_1024", n_static=1024, with_others=False), SplitCase("static_1025", n_static=1025, with_others=False))


def split_case(name):
    return next(c for c in split_cases() if c.name == name)


# ---------------------------------------------------------------------------------------------------------------------
# single-end: one read per lane, grid = ceil(n / 256) blocks
# ---------------------------------------------------------------------------------------------------------------------
BLOCK_COUNTS = (1, 2, 15, 16, 17, 33)  # the ticket groups of grid_finish: fewer blocks than groups, one group short of full, full, one over, two rounds of groups and one over
SET_CAPS = (1, 3)                      # GRID_CAP_SETS
N_SINGLE = 32 * 256 + 37               # 8,229 reads: 33 blocks; under 1 block 33 trips, under 3 (768 a trip) 11, the last of 549:
#                                        two full blocks and 37 lanes of the third's wave 0
SINGLE_READS = {1: 201, 2: 256 + 37, 15: 14 * 256 + 37, 16: 16 * 256, 17: 16 * 256 + 1, 33: N_SINGLE}  # reads for a launch of that many blocks
SINGLE_SETS = [[[A, B]], [[A, B], [C], [C]], [[C], [A, B]], [[E]]]


def single_case(n):
    """n reads, each with a length and an edit count of its own (L = 60 + i mod 191, edit = i div 191 up to 43): no two
    reads share a value. Every seventh read has three records, two of them on one position (the later one counts); every
    eleventh has its record in a window that occurs twice in SINGLE_SETS[1]; read 0, every 500th and the last have none."""
    pats = []
    for i in range(n):
        L, e = 60 + i % 191, i // 191
        if i % 500 == 0 or i == n - 1:
            recs = []
        elif i % 7 == 3:
            recs = [(0, WB, 700 + i % 50, e + 1, 0), (0, WB, 700 + i % 50, e, 1), (0, cc.WAB, 100 + i % 50, min(e + 2, L), 0)]
        elif i % 11 == 5 and L <= 100:  # (the node is 120 bases long)
            recs = [(0, cc.WC, i % 20, e, 0)]
        else:
            recs = [(0, WB, 500 + i % 300, e, i % 2)]
        pats.append(Pattern(f"read{i}", recs, None, 1, (L, L)))
    return Case(f"single{n}", "E", pats, SINGLE_SETS, single=True)


# ---------------------------------------------------------------------------------------------------------------------
# PacBio: one read per wave, grid = ceil(n / 4) blocks
# ---------------------------------------------------------------------------------------------------------------------
PACBIO_READS = {1: 3, 2: 7, 15: 59, 16: 64, 17: 65, 33: 129}  # 129 = 32 * 4 + 1: under 1 block 33 trips, wave 0 alone in the last;
#                                                               under 3 blocks (12 waves) 11 trips, nine waves in the last
PACBIO_LEN = 500
PACBIO_RECORDS = (0, 1, 63, 64, 65, 130)  # per read: none, one lane, a wave less one, a full wave, one more, two trips and two
PACBIO_WALK = [A, B, C, D, E]
PACBIO_SETS = [[PACBIO_WALK, [C, D], [C, D]], [PACBIO_WALK], [[C, D]] * 3, [[A ^ 1]]]  # [C], [C, D], [D]: 3 times in the first
PACBIO_CFG = dict(min_prob_per_base=-0.7)  # floor: -10 - 0.7 * 500 = -360


class PacbioCase:
    """n reads; read r has PACBIO_RECORDS[r mod 6] records spread over the sub-walks of PACBIO_WALK and one sub-walk no path
    set has ([B ^ 1]: count 0), log probabilities all different, those of reads with r mod 7 >= 4 below the floor."""
    def __init__(self, n):
        from gaml_amd import synth
        self.n = n
        self.lens = np.full(n, PACBIO_LEN, np.int32)
        g = cc.graph()
        subs = [tuple(s) for s in synth.all_subwalks_for_pacbio(g, PACBIO_WALK, PACBIO_LEN)] + [(B ^ 1,), (A ^ 1,)]
        self.subs = subs
        filed = {s: ([], []) for s in subs}
        rng = np.random.default_rng(77)
        live = subs[:-1]  # ((A ^ 1,) stays empty: the path set under which nothing scores)
        for r in range(n):
            for q in range(PACBIO_RECORDS[r % 6]):
                s = live[(r + q) % len(live)]
                span = sum(cc.node_len(x) for x in s)
                pos = int(rng.integers(0, max(1, span - 10)))
                filed[s][0].append((pos, pos + PACBIO_LEN, r))
                filed[s][1].append(-300.0 - 15.0 * (r % 7) - 0.37 * q - float(rng.uniform(0, 0.3)))
        self.recs = {s: (np.array(v[0], np.int32).reshape(-1, 3), np.array(v[1], np.float64)) for s, v in filed.items()}

    def library(self, device=0, knobs=(), penalty=0.0):
        from gaml_amd import api
        ctx = api.Context(device=device)
        for knob, v in knobs:
            ctx.debug_set_knob(knob, v)
        ctx.set_graph(*cc.graph().packed())
        rs = ctx.add_pacbio(api.single_cfg(mismatch_prob=0.15, penalty_constant=penalty, **PACBIO_CFG), self.lens)
        for s in self.subs:
            ctx.put_pacbio_records(rs, list(s), *self.recs[s])
        return ctx, rs

    def oracle(self, penalty=0.0):
        import oracle_py as op
        o = op.Oracle()
        o.set_graph(*cc.graph().packed())
        rs = o.add_pacbio(self.lens, 0.15, op.single_cfg(penalty_constant=penalty, **PACBIO_CFG))
        for s in self.subs:
            o.pacbio_put(rs, list(s), *self.recs[s])
        return o, rs


@lru_cache(maxsize=None)
def pacbio_case(n):
    return PacbioCase(n)
