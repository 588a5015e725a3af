"""Hand-made alignment records of single-end sets for the read-major table's tests (tests/test_single_device_host.py,
tests/test_gpu_single_device.py): the records are fed through put_window_records, so no aligner decides what the table
holds. Every window is the one-node walk of a node of a small graph, and a path set of one-node paths names exactly the
windows of its nodes (a one-node contig's junction window is the node itself). numpy only.

A case is a list of steps:
  ("put", node, recs)      recs [k, 4] = position, edit distance, read, orientation: the window of `node` with these records
  ("align", node)          the window of `node` through align_window: registered, whatever it holds, named by no path
  ("score", nodes, counts) a path set of the one-node paths of `nodes`; counts = what the table must hold afterwards:
                           {"records": records of the windows named so far, "reads": reads with at least one of them,
                            "extras": records - reads}
replay(case) restates which records the table holds after every "score" step, in build_read_major's order."""
import os
import re

import numpy as np

from gaml_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READ_LEN = 16      # short reads keep the 70,000-read set at about a megabyte
NODE_LEN = 400
N_NODES = 8


def scan_tile():
    """kTbScanTile as gaml_amd/csrc/table_build.hip.h states it."""
    text = open(os.path.join(ROOT, "gaml_amd", "csrc", "table_build.hip.h")).read()
    return int(re.search(r"constexpr\s+int\s+kTbScanTile\s*=\s*(\d+)\s*;", text).group(1))


def graph():
    genome = synth.make_genome(N_NODES * NODE_LEN, 321)
    g = synth.make_graph(genome, [NODE_LEN] * N_NODES)
    return g, synth.genome_walk(g)


def reads(n):
    """n reads of READ_LEN random bases (their content never matters: every scored window comes with its records)"""
    rng = np.random.default_rng(1000 + n)
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (n, READ_LEN))]


def recs(rows):
    return np.asarray(rows, np.int32).reshape(-1, 4)


def _spread(read_ids, seed):
    """one record per entry of read_ids: positions and edits drawn, orientation alternating"""
    rng = np.random.default_rng(seed)
    k = len(read_ids)
    return np.stack([rng.integers(0, NODE_LEN - READ_LEN, k), rng.integers(0, 4, k), np.asarray(read_ids), np.arange(k) & 1], axis=1).astype(np.int32)


def _counts(records, n_reads_hit):
    return {"records": records, "reads": n_reads_hit, "extras": records - n_reads_hit}


class Case:
    def __init__(self, name, n_reads, steps):
        self.name, self.n_reads, self.steps = name, n_reads, steps

    def __repr__(self):
        return self.name


def _edges():
    # read 0 (the first) 1 record, read 49 (the last) 2, read 10 3, read 20 40 over three windows, read 30 1; the rest none
    w0 = [(5, 0, 0, 0), (7, 1, 49, 1), (9, 2, 10, 0)] + [(20 + 3 * k, k % 4, 20, k & 1) for k in range(20)]
    w1 = [(11, 0, 49, 0), (12, 3, 10, 1), (300, 0, 30, 1)] + [(40 + 2 * k, 1, 20, 0) for k in range(15)]
    w2 = [(1, 0, 10, 0)] + [(100 + k, 2, 20, 1) for k in range(5)]
    return Case("edges: reads with 0, 1, 2, 3 and 40 records", 50,
                [("put", 0, recs(w0)), ("put", 1, recs(w1)), ("put", 2, recs(w2)), ("score", [0, 1, 2], _counts(47, 5))])


def _every_read():
    rows = [[(10 * i + k, k, i, k & 1) for k in range(i % 3 + 1)] for i in range(7)]  # read i: i % 3 + 1 records
    flat = [r for per in rows for r in per]
    return Case("every read of the set has records", 7, [("put", 0, recs(flat[::2])), ("put", 1, recs(flat[1::2])), ("score", [0, 1], _counts(13, 7))])


def _no_read():
    return Case("no read has a record", 9, [("put", 0, recs([])), ("put", 1, recs([])), ("score", [0, 1], _counts(0, 0))])


def _one_window():
    return Case("one window with a single record", 5, [("put", 3, recs([(17, 1, 2, 1)])), ("score", [3], _counts(1, 1))])


def _empty_and_inactive():
    a = [(3, 0, 1, 0), (3, 1, 4, 1), (90, 0, 1, 1)]
    b = [(8, 2, 4, 0), (9, 0, 6, 0)]
    c = [(1, 0, 1, 0), (2, 0, 0, 1), (2, 1, 6, 0), (50, 3, 11, 1)]
    return Case("an empty window between two others; inactive windows, one of them named later", 12,
                [("put", 0, recs(a)), ("put", 1, recs([])), ("put", 2, recs(b)), ("put", 3, recs(c)), ("align", 4),
                 ("score", [0, 1, 2], _counts(5, 3)),          # reads 1, 4, 6; the windows of nodes 3 and 4 are cached but unnamed
                 ("score", [0, 1, 2], _counts(5, 3)),          # nothing new: no build
                 ("score", [0, 1, 2, 3], _counts(9, 5))])      # node 3's window joins: reads 0 and 11 come in


def _pool_order():
    a = [(4, 0, 2, 0), (6, 1, 3, 0), (8, 0, 2, 1)]
    b = [(1, 1, 3, 1), (5, 0, 2, 0), (7, 2, 0, 0)]
    return Case("windows activated against their pool order", 4,
                [("put", 0, recs(a)), ("put", 1, recs(b)), ("score", [1], _counts(3, 3)), ("score", [1, 0], _counts(6, 3))])


def _sort_passes(n):
    rng = np.random.default_rng(n)
    ids = np.concatenate([[0, n - 1, n - 1, 0, n // 2], rng.integers(0, n, 295)])
    r = _spread(ids, n)
    return Case("sort passes: %d reads" % n, n,
                [("put", 0, r[:180]), ("put", 1, r[180:]), ("score", [0, 1], _counts(300, len(np.unique(ids))))])


def _scan_tiles(total, tag):
    rng = np.random.default_rng(total)
    ids = rng.integers(0, 1000, total)
    r = _spread(ids, total)
    a, b = total // 3, total // 2
    return Case("scan tiles: %s records" % tag, 1000,
                [("put", 0, r[:a]), ("put", 1, r[a:b]), ("put", 2, r[b:]), ("score", [0, 1, 2], _counts(total, len(np.unique(ids))))])


def cases():
    t = scan_tile()
    return ([_edges(), _every_read(), _no_read(), _one_window(), _empty_and_inactive(), _pool_order()] +
            [_sort_passes(n) for n in (1, 255, 256, 257, 70_000)] +
            [_scan_tiles(t, "one tile of"), _scan_tiles(t + 1, "one tile and one more"), _scan_tiles(3 * t + 1, "three tiles and one more")])


def replay(case):
    """After every "score" step: (step index, counts, records [k, 5] = window id, position, edit, read, orientation of the
    windows named so far, in (window id, pool order) -- the order build_read_major walks them in). Window ids follow the
    order of the "put" / "align" steps; a window's records are kept in put_window_records' order, stable by (position, read)."""
    wins, out = [], []  # wins: [node, records or None (aligned: unknown, never named), active]
    for k, step in enumerate(case.steps):
        if step[0] == "put":
            r = step[2]
            order = np.lexsort((np.arange(len(r)), r[:, 2], r[:, 0])) if len(r) else np.zeros(0, np.int64)
            wins.append([step[1], r[order], False])
        elif step[0] == "align":
            wins.append([step[1], None, False])
        else:
            for w in wins:
                if w[0] in step[1]:
                    assert w[1] is not None, "a path names a window whose records the case does not know"
                    w[2] = w[2] or len(w[1]) > 0
            assert all(any(w[0] == node for w in wins) for node in step[1]), "a path names a node without a window: the aligner would run"
            rows = [np.concatenate([np.full((len(w[1]), 1), wid, np.int32), w[1]], axis=1) for wid, w in enumerate(wins) if w[2]]
            out.append((k, step[2], np.concatenate(rows) if rows else np.zeros((0, 5), np.int32)))
    return out
