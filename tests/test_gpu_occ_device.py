"""Occurrence tables of whole-set calls built on the device (gaml_amd/csrc/occ_device.hip.h): the route against the host
route (Knob.NO_OCC_DEVICE) in a second context fed the same calls -- values, zeros, total length and per-read probabilities bit-equal
-- the device tables against the host image entry by entry, the fallback when two paths share a window, and the
transitions to the routes that need the host images (incremental calls, batches, table rebuilds)."""
import numpy as np
import pytest

from gaml_amd import synth

pytestmark = pytest.mark.gpu


def _variants(walk, k=8):
    out = [[list(walk)]]
    n = len(walk)
    for i in range(1, k):
        cut = max(1, min(n - 1, (n * i) // k - ((n * i) // k) % 2))
        out.append([list(walk[:cut]), list(walk[cut:])])
    return out


def _pair(name, with_oracle=False):
    from gaml_amd import api
    wl = synth.WORKLOADS[name]
    genome, g = wl.build()
    pr = synth.make_paired_reads(genome, wl.n_pairs, wl.read_len, wl.insert_mean, wl.insert_std, wl.err, wl.seed)
    gb, go = g.packed()
    r1, r2 = synth.pack_reads(pr.mate1), synth.pack_reads(pr.mate2)
    ctxs = []
    for no_occ_device in (0, 1):
        c = api.Context(device=0)
        c.set_graph(gb, go)
        c.add_paired(api.paired_cfg(wl.insert_mean, wl.insert_std), *r1, *r2)
        c.debug_set_knob(api.Knob.NO_OCC_DEVICE, no_occ_device)
        ctxs.append(c)
    orc = None
    if with_oracle:
        import oracle_py as op
        orc = op.Oracle()
        orc.set_graph(gb, go)
        orc.add_paired(*r1, *r2, 0.01, op.paired_cfg(wl.insert_mean, wl.insert_std))
    return g, ctxs, orc


def _same(dev, host):
    assert dev[0] == host[0] and dev[2] == host[2] and np.array_equal(dev[1], host[1])


def _both(ctxs, paths):
    got = [c.calc_prob(paths) for c in ctxs]
    _same(got[0], got[1])
    assert np.array_equal(ctxs[0].read_probs(0), ctxs[1].read_probs(0))
    return got[0]


def test_headline_pattern_device_route():
    g, ctxs, _ = _pair("tiny")
    variants = _variants(synth.genome_walk(g))
    checked = 0
    for i in range(3 * len(variants)):
        _both(ctxs, variants[i % len(variants)])
        chk = ctxs[0].debug_occ_check(0)
        assert chk["mismatches"] == 0 and chk["lists"] == 0
        checked += chk["compared"] > 0
    r0, r1 = ctxs[0].debug_occ_route(0), ctxs[1].debug_occ_route(0)
    assert r0["device"] >= 2 * len(variants) and checked == r0["device"] and r0["fallbacks"] == 0
    assert r1["device"] == 0
    for c in ctxs:
        c.close()


def test_transitions_between_routes():
    g, ctxs, orc = _pair("tiny", with_oracle=True)
    walk = synth.genome_walk(g)
    variants = _variants(walk)
    rng = np.random.default_rng(5)
    paths = [list(walk)]
    sample = []
    for step in range(60):
        kind = step % 6
        if kind in (0, 3):  # headline: every path new (device route)
            p = variants[step % len(variants)]
            v = _both(ctxs, p)
            orc_v = orc.calc_prob(p, fresh=True)
        elif kind in (1, 2):  # annealing moves from the last set (incremental route; images rebuilt once)
            paths = synth.sa_move(rng, paths, g)
            p = paths
            v = _both(ctxs, p)
            orc_v = orc.calc_prob(p, fresh=True)
        elif kind == 4:  # a batch of moves (patches the images of the current set)
            cands = [synth.sa_move(rng, paths, g) for _ in range(4)]
            got = [c.calc_prob_batch(cands) for c in ctxs]
            for a, b in zip(*got):
                _same(a, b)
            for cand in cands:
                orc.calc_prob(cand, fresh=True)
            p, v, orc_v = None, None, None
        else:  # table rebuild between the calls
            for c in ctxs:
                c.compact_tables()
            p = variants[(step + 3) % len(variants)]
            v = _both(ctxs, p)
            orc_v = orc.calc_prob(p, fresh=True)
        if v is not None and step % 5 == 0:
            sample.append((v, orc_v))
    for v, w in sample:
        assert v[2] == w[2] and np.array_equal(np.ravel(v[1]), np.ravel(w[1])) and abs(v[0] - w[0]) <= 1e-12 * abs(w[0])
    assert ctxs[0].debug_occ_route(0)["device"] > 0
    for c in ctxs:
        c.close()


@pytest.mark.parametrize("name", ["tiny", "tinyr"])
def test_paths_sharing_windows_fall_back(name):
    g, ctxs, orc = _pair(name, with_oracle=True)
    walk = synth.genome_walk(g)
    n = len(walk)
    sets = []
    for i in range(1, 5):
        k = (n * i) // 5
        sets.append([list(walk[:k + 4]), list(walk[k:])])  # four nodes in both paths
        sets.append([list(walk[:k]), list(walk[k:])])      # none shared (device route where the paths allow it)
    for s in sets:
        v = _both(ctxs, s)
        w = orc.calc_prob(s, fresh=True)
        assert v[2] == w[2] and abs(v[0] - w[0]) <= 1e-12 * abs(w[0])
    first = ctxs[0].debug_occ_route(0)
    if name == "tiny":
        assert first["fallbacks"] >= 3 and first["device"] == first["fallbacks"]  # (the first set: host route, no resident copy yet; the others are incremental)
    for s in sets:  # again: the first set meets the device route now (once), the others go to the host route directly
        _both(ctxs, s)
    again = ctxs[0].debug_occ_route(0)
    assert again["fallbacks"] - first["fallbacks"] == (1 if name == "tiny" else again["fallbacks"] - first["fallbacks"]) <= 1
    for s in sets:  # every combination known: no fallback any more
        _both(ctxs, s)
    assert ctxs[0].debug_occ_route(0)["fallbacks"] == again["fallbacks"]
    for c in ctxs:
        c.close()


def test_memo_churn_and_pool_compaction():
    g, ctxs, _ = _pair("tiny")
    walk = synth.genome_walk(g)
    n = len(walk)
    rng = np.random.default_rng(11)
    for step in range(170):
        k = int(rng.integers(8, 24))
        cuts = sorted(set(int(x) for x in rng.integers(1, n - 1, size=k - 1)))
        bounds = [0] + cuts + [n]
        paths = [list(walk[a:b]) for a, b in zip(bounds[:-1], bounds[1:]) if b > a]
        if step % 7 == 3:  # a reversed piece: new junction windows, memos that had missed them are invalidated
            j = int(rng.integers(0, len(paths)))
            paths[j] = [x ^ 1 for x in reversed(paths[j])]
        _both(ctxs, paths)
        if step % 10 == 0:
            assert ctxs[0].debug_occ_check(0)["mismatches"] == 0
    r = ctxs[0].debug_occ_route(0)
    assert r["device"] > 100 and r["compactions"] >= 1
    for c in ctxs:
        c.close()
