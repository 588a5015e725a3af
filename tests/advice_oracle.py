"""The advice move of the reference (ExtendPathsAdv moves.cc:933-998), restated in Python over the oracle's window cache:
what tests/test_advice_host.py and tests/test_gpu_advice.py compare the library's gaml_hip_advice_* against."""
import numpy as np

from gaml_amd import synth

K_TAIL = 300  # kMinSubpathLength graph.cc:27


def junction(node_len, path, i):
    """cur_seq of GetSubpathsFromPath / GetPositions (graph.cc:686-697): node i plus following nodes until a gap or more
    than K_TAIL added bases; returns (window, index of its last node)."""
    w, tail, end = [path[i]], 0, i
    for j in range(i + 1, len(path)):
        if path[j] < 0:
            break
        tail += node_len[path[j]]
        w.append(path[j])
        end = j
        if tail > K_TAIL:
            break
    return w, end


def oracle_index(orc, rs, node_len, threshold, n_pairs):
    """BuildAdviceIndex (graph.cc:323-342) through the oracle's GetPositionsOnlyPath: (advice, advice1) per pair."""
    advice = [[] for _ in range(n_pairs)]
    advice1 = [[] for _ in range(n_pairs)]
    for i in range(len(node_len)):
        if node_len[i] <= threshold:
            continue
        seen = set()
        for pos, ed, read, orient in orc.positions_only_path(rs, 1, [i], 0):  # a pair's slots in order, first first
            read = int(read)
            if read in seen:
                continue
            seen.add(read)
            advice[read].append(i)
            if orient == 1:
                advice1[read].append(i)
    return advice, advice1


def oracle_candidates(orc, rs, node_len, path, advice1, reach, only_out, allow_gaps, n_pairs):
    """rs1.GetPositions (graph.cc:651-712) on the oracle's mate-1 cache, then moves.cc:964-973."""
    path = [int(x) for x in path]
    last_end = -1  # GetSubpathsFromPath: registration
    for i, x in enumerate(path):
        if x < 0:
            continue
        w, end = junction(node_len, path, i)
        if end != last_end and orc.window_records(rs, 0, w) is None:
            orc.align_window(rs, 0, w)
        last_end = end
    slots, cur = {}, 0
    for i, x in enumerate(path):
        if x < 0:
            cur += -x
            continue
        w, _ = junction(node_len, path, i)
        for seq in [w] + ([[x]] if node_len[x] > K_TAIL else []):
            recs = orc.window_records(rs, 0, seq)
            if recs is None:
                continue
            for pos, ed, read, orient in recs:
                v = slots.setdefault(int(read), [])
                a = int(pos) + cur
                for e in v:
                    if e[0] == a:
                        e[1] = int(orient)
                        break
                else:
                    v.append([a, int(orient)])
        cur += node_len[x]
    path_v = set(path) | {e ^ 1 for e in path}
    reach = set(int(x) for x in reach)
    cands = []
    for r in range(n_pairs):
        v = slots.get(r)
        if not v or v[0][1] != 0:
            continue
        for node in advice1[r]:
            if node in path_v and only_out:
                continue
            if node in reach or allow_gaps:
                cands.append(node)
    return cands


def pack_varlen(reads):
    offs = np.zeros(len(reads) + 1, np.int64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    return np.ascontiguousarray(np.concatenate(reads)), offs


def make_case(G=40_000, n_pairs=2_000, seed=5, insert=1500.0, sd=150.0, read_len=100, odd=30):
    """Genome with planted repeats, its graph, a jumping library; `odd` pairs with a 12-base mate 1 and `odd` with a
    300-base mate 2 (reads outside 16..254 bases)."""
    genome = synth.plant_repeats(synth.make_genome(G, seed), 4, 700, seed)
    g = synth.make_graph(genome, synth.cut_lengths(G, seed, long_rng=(250, 2500), short_rng=(40, 200)))
    pr = synth.make_paired_reads(genome, n_pairs, read_len, insert, sd, 0.01, seed)
    m1, m2 = [r for r in pr.mate1], [r for r in pr.mate2]
    if odd:
        longer = synth.make_paired_reads(genome, odd, 300, insert, sd, 0.01, seed + 1)
        for k in range(odd):
            m1[(7 + 13 * k) % n_pairs] = m1[(7 + 13 * k) % n_pairs][:12]
            m2[(11 + 17 * k) % n_pairs] = longer.mate2[k]
    return g, pack_varlen(m1), pack_varlen(m2)


def query_paths(g, n=12, seed=3):
    """An annealing-like set of walks: contigs of the genome walk, forward and reversed, some with gaps, some joined
    out of order (windows nobody has aligned yet)."""
    rng = np.random.default_rng(seed)
    walk = synth.genome_walk(g)
    out = []
    for k in range(n):
        a = int(rng.integers(0, len(walk) - 4))
        b = int(min(len(walk), a + rng.integers(3, 12)))
        p = list(walk[a:b])
        if k % 3 == 1 and len(p) > 3:  # a gap in place of a node
            c = int(rng.integers(1, len(p) - 1))
            p[c] = -max(1, g.node_len(p[c]))
        if k % 4 == 2:  # joined with another stretch: new junction windows
            c = int(rng.integers(0, len(walk) - 3))
            p = p + list(walk[c:c + 3])
        if k % 2 == 1:
            p = [x ^ 1 if x >= 0 else x for x in reversed(p)]
        out.append(p)
    return out


def overwrite_case(ctx_factory):
    """GetPositions' overwrite rule (graph.cc:708-723) with caller-supplied records: four pairs of poly-A reads (they align
    nowhere), records planted in the mate-1 windows of the walk [a, b] and in mate 2's window of a long node v.
      pair 0: [a, b] puts it at 10 forward, [a] at the same absolute position reverse -> its first slot ends reverse: out
      pair 1: [a, b] at 20 reverse, [a] at 20 forward -> the slot ends forward: in
      pair 2: [a, b] at 30 forward, [a] at 5 reverse (a second slot) -> the first slot stays forward: in
      pair 3: only [b], at 7 forward (absolute len(a) + 7) -> in
    Returns (ctx, rs, a, b, v)."""
    from gaml_amd import api
    genome = synth.make_genome(6_000, 3)
    g = synth.make_graph(genome, [1000, 60, 1200, 80, 1500, 70, 2090])
    a, b, v = 0, 4, 8
    reads = np.frombuffer(b"A" * 50, np.uint8)
    r = pack_varlen([reads] * 4)
    ctx = ctx_factory()
    ctx.set_graph(*g.packed())
    rs = ctx.add_paired(api.paired_cfg(1500.0, 150.0), *r, *r)

    def recs(rows):
        out = np.zeros(len(rows), api.ALIGMENT)
        for k, (pos, read, orient) in enumerate(rows):
            out[k] = (pos, 0, read, orient)
        return out
    ctx.put_window_records(rs, 0, [a, b], recs([(10, 0, 0), (20, 1, 1), (30, 2, 0)]))
    ctx.put_window_records(rs, 0, [a], recs([(5, 2, 1), (10, 0, 1), (20, 1, 0)]))
    ctx.put_window_records(rs, 0, [b], recs([(7, 3, 0)]))
    ctx.put_window_records(rs, 1, [v], recs([(40, 0, 1), (41, 1, 1), (42, 2, 1), (43, 3, 1)]))
    return ctx, rs, a, b, v
