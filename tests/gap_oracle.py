"""The reference's gap-length search (FixGapLength, moves.cc:729-800 with its helper :694-727) restated over an
evaluator callback, and the inputs the gap tests share. `evaluate(length)` returns CalcProb of the path set with that
length in the gap: the oracle's, or a context's calc_prob."""
import numpy as np

from gaml_amd import synth

SEED, GENOME = 83, 120_000
INSERT_MEAN, INSERT_STD = 600.0, 40.0
GAP_SITES = (5, 7, 9)  # walk positions replaced by a gap; the nodes there are 100, 111 and 58 bases long


class Search:
    """One run: .length is what the reference leaves in the entry, .trace its evaluations [(length, value)] in order,
    .state 0 stay / 1 up / 2 down, .closest the smallest relative difference of two values it compared."""

    def __init__(self, evaluate, cur):
        self.evaluate, self.trace, self.closest, self.state = evaluate, [], float("inf"), 0
        self.length = self._run(cur)

    def _p(self, length):
        v = self.evaluate(length)
        self.trace.append((length, v))
        return v

    def _cmp(self, a, b):
        self.closest = min(self.closest, abs(a - b) / max(abs(a), abs(b)))

    def _ternary(self, lower, upper):  # moves.cc:694-727
        while True:
            if upper - lower <= 1:  # :697-700
                return lower
            if upper - lower == 2:  # :702-712: the lower end twice; whatever the comparison says, the lower end stays
                self._p(lower)
                self._p(lower)
                return lower
            mid1 = lower + (upper - lower) // 3  # :715-716
            mid2 = lower + (upper - lower) // 3 * 2
            p1, p2 = self._p(mid1), self._p(mid2)
            self._cmp(p1, p2)
            if p1 >= p2:  # :722-726
                upper = mid2
            else:
                lower = mid1

    def _run(self, cur):  # moves.cc:729-800
        assert cur > 0
        cur_p = self._p(cur)
        up_p = self._p(cur + 1)
        self._cmp(up_p, cur_p)
        last = cur + 1
        if cur == 1:  # :743-746
            if up_p > cur_p:
                self.state = 1
        else:  # :747-756
            down_p = self._p(cur - 1)
            last = cur - 1
            self._cmp(down_p, cur_p)
            if down_p > cur_p and cur_p > up_p:
                self.state = 2
            if up_p > cur_p and cur_p > down_p:
                self.state = 1
        if self.state == 0:  # :758-760: the entry keeps the last probed length
            return last
        if self.state == 1:  # :762-776
            last_p, bound = cur_p, 2 * cur
            while True:
                p = self._p(bound)
                self._cmp(p, last_p)
                if p < last_p:
                    break
                last_p = p
                bound *= 2
            return self._ternary(cur + 1, bound)
        return self._ternary(1, cur)  # :777-779


def make_inputs(n_pairs=24000, read_len=100):
    genome = synth.make_genome(GENOME, SEED)
    g = synth.make_graph(genome, synth.cut_lengths(GENOME, SEED, long_rng=(900, 4000)))
    pr = synth.make_paired_reads(genome, n_pairs, read_len, INSERT_MEAN, INSERT_STD, 0.01, SEED)
    return g, pr, synth.genome_walk(g)


def gap_set(walk, i, length):
    """The checked path set: the walk with node i replaced by a gap, and a second short path."""
    return [walk[:i] + [-length] + walk[i + 1:], walk[3:9]]


def start_lengths(true_len):
    return (1, 7, true_len, 3 * true_len + 11, 900)


def with_length(paths, path_id, gap_pos, length):
    out = [list(p) for p in paths]
    out[path_id][gap_pos] = -length
    return out


def make_oracle(g, pr):
    import oracle_py as op
    o = op.Oracle()
    o.set_graph(*g.packed())
    o.add_paired(*synth.pack_reads(pr.mate1), *synth.pack_reads(pr.mate2), 0.01, op.paired_cfg(INSERT_MEAN, INSERT_STD))
    return o


def oracle_search(o, paths, path_id, gap_pos):
    memo = {}

    def ev(length):  # (a value is a function of the length alone: the oracle scores each once)
        if length not in memo:
            memo[length] = o.calc_prob(with_length(paths, path_id, gap_pos, length))[0]
        return memo[length]
    return Search(ev, -paths[path_id][gap_pos])
