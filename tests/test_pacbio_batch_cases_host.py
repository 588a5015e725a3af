"""The inputs of tests/test_gpu_pacbio_batch.py on the oracle: the graph and the record cache are the ones the tests'
comments speak of, and the two families of path sets floor the PacBio reads the module says they floor -- between them
none, some and all of the reads, with sub-walks that do not occur in a set and sub-walks that occur two and three times."""
import pacbio_batch_cases as pc


def test_fixture_a_on_the_oracle(built):
    f = pc.FixtureA()
    assert len(f.walk) == 47 and len(f.pb.walks) == 51 and sum(len(r) for r in f.pb.recs) == 205
    cands, other = f.candidates(), f.unrelated()
    assert len(cands) == 8 and len(other) == 9 and len(f.base()) == 6
    o = f.oracle()
    for sets, floored in ((cands, pc.FLOORED_CANDIDATES), (other, pc.FLOORED_UNRELATED)):
        got = [o.calc_prob(s, fresh=True)[1].tolist() for s in sets]
        assert [z[-1] for z in got] == [[n, pc.N_PACBIO] for n in floored], got
        assert all(z[0][1] == pc.N_PAIRS for z in got)
    counts = pc.FLOORED_CANDIDATES + pc.FLOORED_UNRELATED
    assert 0 in counts and pc.N_PACBIO in counts and any(0 < n < pc.N_PACBIO for n in counts)
    # occurrence counts above 1: a cached sub-walk inside the stretch that two paths of candidate 4 share, and inside the
    # path the sixth unrelated set holds three times
    cached = {tuple(w) for w in f.pb.walks}
    assert any(tuple(f.walk[k:k + n]) in cached for k in range(10, 14) for n in range(1, 14 - k + 1))
    assert any(tuple(f.walk[k:k + n]) in cached for k in range(3, 9) for n in range(1, 9 - k + 1))
