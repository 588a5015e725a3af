"""GPU window aligner on the inputs of tests/aligner_hard_cases.py -- tandem repeats and a two-letter stretch (one span
holds the same 15-mer code many times: the earliest-seed rule of the span kernels decides), reads with an inserted or
deleted base (extensions that succeed off diagonal 0), reads with several records in one window and windows with
thousands of records (hit ordering and de-duplication), down to 16-base reads -- against the library's host aligner,
which tests/test_aligner_hard_cases_host.py pins against the oracle on the same inputs, and against the oracle's values.
Then the routes no other test enters: a paired small batch the device filing refuses, the general route's retry loop, a
candidate whose seed is not in the read (a run of N codes like G)."""
import numpy as np
import pytest

from aligner_hard_cases import hard_case, junction_moves, n_collision_case

pytestmark = pytest.mark.gpu


def _ctx(gb, go, reads, mean, sd, aligner_route=0, first_cap=0):
    from gaml_amd import api
    ctx = api.Context(device=0)
    ctx.debug_set_knob(api.Knob.ALIGNER_ROUTE, aligner_route)
    ctx.debug_set_knob(api.Knob.ALIGNER_FIRST_CAP, first_cap)
    ctx.set_graph(gb, go)
    ctx.add_paired(api.paired_cfg(mean, sd), *reads)
    return ctx


def _windows(ctx, mate, start=0):
    return [tuple(ctx.debug_window_walk(0, mate, w)) for w in range(start, ctx.window_count(0, mate))]


def _same_records(ctxs):
    """Every window of both mates: the same walks in the same order and byte-identical records in all contexts. Returns
    the number of records of one context."""
    n = 0
    for mate in (0, 1):
        keys = _windows(ctxs[0], mate)
        for other in ctxs[1:]:
            assert _windows(other, mate) == keys
        for key in keys:
            want = ctxs[0].window_records(0, mate, list(key))
            for other in ctxs[1:]:
                got = other.window_records(0, mate, list(key))
                assert got.shape == want.shape and got.tobytes() == want.tobytes(), (mate, key)
            n += len(want)
    return n


def _same_values(results):
    for r in results[1:]:
        assert r[0] == results[0][0] and r[1].tolist() == results[0][1].tolist() and r[2] == results[0][2]


def _most_terms(orc, n_reads):
    """The largest product, over pairs, of the two mates' record counts in the oracle's window cache: the most terms a
    pair's probability can be the sum of."""
    cnt = [np.zeros(n_reads, np.int64), np.zeros(n_reads, np.int64)]
    for mate in (0, 1):
        for key in orc.window_keys(0, mate):
            rec = orc.window_records(0, mate, key)
            if len(rec):
                cnt[mate] += np.bincount(rec[:, 2], minlength=n_reads)
    return int((cnt[0] * cnt[1]).max())


@pytest.mark.parametrize("L", [16, 17, 31, 100, 254, 255, 510])
def test_device_equals_host_aligner_and_oracle_on_hard_cases(L):
    import oracle_py as op
    g, reads, indel, regions, sets = hard_case(L)
    gb, go = g.packed()
    mean, sd = 2.2 * L, 0.2 * L
    from gaml_amd.api import AlignerRoute
    gpu, cpu = _ctx(gb, go, reads, mean, sd, 0), _ctx(gb, go, reads, mean, sd, AlignerRoute.HOST)
    orc = op.Oracle()
    orc.set_graph(gb, go)
    orc.add_paired(*reads, 0.01, op.paired_cfg(mean, sd))
    n_reads = len(reads[1]) - 1
    for paths in sets:
        a, b = gpu.calc_prob(paths), cpu.calc_prob(paths)
        _same_values([a, b])
        want, wzeros, wtl = orc.calc_prob(paths, fresh=True)
        assert abs(a[0] - want) <= 1e-9 * abs(want), (a[0], want)
        assert a[1].tolist() == wzeros.tolist() and a[2] == wtl
        # per-read probabilities: one rounding per addition of a sum of at most n terms, with a factor two of slack
        n = _most_terms(orc, n_reads)
        probs, wprobs = gpu.read_probs(0), orc.paired_probs(0)[0]
        with np.errstate(all="ignore"):
            rel = np.nan_to_num(np.abs(probs - wprobs) / np.abs(wprobs))
        print(f"L = {L}: at most {n} terms per pair, per-read probabilities differ by up to {rel.max():.3e} relative (bound {max(4, n) * 2.3e-16:.3e})")
        np.testing.assert_allclose(probs, wprobs, rtol=max(4, n) * 2.3e-16, atol=0)
    st, routes = gpu.aligner_stats(), gpu.debug_aligner_routes()
    print(f"L = {L}: device aligner {st}, routes {routes}")
    assert st["windows"] > 0 and st["candidates"] > 0 and routes["flushed"] == 0
    assert cpu.aligner_stats()["windows"] == 0 and cpu.aligner_stats()["candidates"] == 0
    n_records = _same_records([gpu, cpu])
    assert n_records > 0
    n_indel = 0
    for mate in (0, 1):  # ... and the oracle's, which also tells whose records they are
        for key in _windows(gpu, mate):
            ref = orc.window_records(0, mate, list(key))
            got = gpu.window_records(0, mate, list(key))
            assert got.shape == ref.shape and (got == ref).all(), (mate, key)
            n_indel += int(indel[mate][ref[:, 2]].sum()) if len(ref) else 0
    print(f"L = {L}: {n_records} records identical, {n_indel} of reads with an inserted or deleted base")
    assert n_indel > 0


@pytest.mark.parametrize("L,n_dense", [(100, 1500), (300, 3500)])
def test_routes_agree_on_junction_windows_in_repeats(L, n_dense):
    """One path per node, then join after join across the planted regions (junction_moves): the paired small batch
    (ALIGNER_ROUTE at 0), the general route (GENERAL), one small pipeline per mate (PER_MATE), window strings through the input
    block (INPUT_BLOCK) and hits filed on the host (HOST_FILING) give bit-equal values and byte-equal records for every window
    after every step, equal to the host aligner's (HOST). n_dense is sized so that one step's junction windows hold more than 2,048 records -- so more
    candidates than that: the device filing refuses the batch after the paired pipeline has run and the per-mate route
    redoes it."""
    g, reads, indel, regions, sets = hard_case(L, n_dense=n_dense)
    gb, go = g.packed()
    from gaml_amd.api import AlignerRoute as R
    held_to = (0, R.GENERAL, R.PER_MATE, R.INPUT_BLOCK, R.HOST_FILING, R.HOST)
    ctxs = [_ctx(gb, go, reads, 2.2 * L, 0.2 * L, k) for k in held_to]
    host = ctxs[-1]
    steps = junction_moves(g, regions)
    assert len(steps) >= 5
    seen, most = [0, 0], 0
    for paths in steps:
        _same_values([c.calc_prob(paths) for c in ctxs])
        _same_records(ctxs)
        new = 0
        for mate in (0, 1):
            new += sum(len(host.window_records(0, mate, list(key))) for key in _windows(host, mate, seen[mate]))
            seen[mate] = host.window_count(0, mate)
        if paths is not steps[0]:
            most = max(most, new)
    routes = {k: c.debug_aligner_routes() for k, c in zip(held_to, ctxs)}
    print(f"L = {L}: {len(steps)} steps, at most {most} records in a step's new windows, routes {routes}")
    assert most > 2048
    for k in (0, R.INPUT_BLOCK):  # the paired pipeline ran, the filing kernel refused, the per-mate route took over
        assert routes[k]["pair_filing"] > 0
    for k in (R.GENERAL, R.PER_MATE, R.HOST_FILING, R.HOST):
        assert routes[k]["pair_filing"] == 0
    assert all(r["flushed"] == 0 for r in routes.values())
    for k, c in zip(held_to, ctxs):
        assert (c.aligner_stats()["windows"] > 0) == (k != R.HOST)


def test_general_route_retry_loop():
    """The general route with room for 4,096, then for 256 spans and candidates at first (ALIGNER_FIRST_CAP): the loop re-reserves and
    runs again; from 256 the spans overflow in the first attempt and the candidates, counted over a truncated span list
    then, in the second: three attempts per mate. Same records and values as the route with its own capacities and as a context without any knob."""
    L = 100
    g, reads, indel, regions, sets = hard_case(L)
    gb, go = g.packed()
    from gaml_amd.api import AlignerRoute
    plain, first, second = (_ctx(gb, go, reads, 2.2 * L, 0.2 * L, AlignerRoute.GENERAL, k) for k in (0, 4096, 256))
    default = _ctx(gb, go, reads, 2.2 * L, 0.2 * L)  # no knob at all: whatever routes its batches take
    for i, paths in enumerate(sets):
        _same_values([c.calc_prob(paths) for c in (plain, first, second, default)])
        if i == 0:  # the cold evaluation: one batch per mate
            routes = [c.debug_aligner_routes() for c in (plain, first, second)]
            print("retries after the cold evaluation:", routes)
            assert routes[0]["retries"] == 0 and routes[1]["retries"] > 0 and routes[2]["retries"] == 4
    assert _same_records([plain, first, second, default]) > 0
    for c in (plain, first, second):
        assert c.debug_aligner_routes()["flushed"] == 0 and c.aligner_stats()["windows"] > 0
    assert plain.aligner_stats()["windows"] == first.aligner_stats()["windows"] == second.aligner_stats()["windows"]


def test_candidates_whose_seed_is_not_in_the_read_are_skipped():
    """A run of N in a node codes like G, so reads with G there are candidates of a window seed they do not hold: both
    device routes skip them as the host aligner does (the reference and the oracle abort there, so no oracle here)."""
    g, reads, collide, node, sets = n_collision_case()
    gb, go = g.packed()
    from gaml_amd.api import AlignerRoute
    ctxs = [_ctx(gb, go, reads, 220.0, 20.0, k) for k in (0, AlignerRoute.GENERAL, AlignerRoute.HOST)]
    for paths in sets:
        _same_values([c.calc_prob(paths) for c in ctxs])
    assert _same_records(ctxs) > 0
    for c in ctxs[:2]:
        assert c.aligner_stats()["windows"] > 0 and c.debug_aligner_routes()["flushed"] == 0
    assert ctxs[2].aligner_stats()["windows"] == 0
    for c in ctxs:
        for walk in ([node], [node ^ 1]):  # the node with the run and its twin
            rec = c.window_records(0, 0, walk)
            assert len(rec) > 0 and not np.isin(rec[:, 2], collide).any()
