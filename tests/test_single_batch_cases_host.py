"""The inputs of tests/single_batch_cases.py on the CPU oracle: the floored counts recorded there are the oracle's, both
branches of the floor are hit in every set but the empty one, windows that occur several times are scored."""
import numpy as np

import single_batch_cases as sc


def test_the_oracle_floors_the_recorded_counts(built):
    fx = sc.Fixture()
    o, rs = fx.oracle_single()
    for sets, floored in ((fx.candidates(), sc.FLOORED_CANDIDATES), (fx.unrelated(), sc.FLOORED_UNRELATED)):
        got = []
        for s in sets:
            v, probs, o3 = o.single_detail(rs, s)
            z = o.calc_prob(s, fresh=True)[1]
            assert z.tolist() == [[int(o3[0]), sc.N_SINGLE]]
            assert int((probs > 0).sum()) >= sc.N_SINGLE - int(o3[0])  # the reads that are not floored have a value above 0
            got.append(int(o3[0]))
        print(got)
        assert got == floored
    assert sc.FLOORED_UNRELATED[4] == sc.N_SINGLE and fx.unrelated()[4] == []  # the empty set floors every read
    for k, z in enumerate(sc.FLOORED_CANDIDATES + sc.FLOORED_UNRELATED):
        assert 0 < z < sc.N_SINGLE or k == len(sc.FLOORED_CANDIDATES) + 4, (k, z)


def test_windows_with_occurrence_lists_are_scored(built):
    fx = sc.Fixture()
    o, rs = fx.oracle_single()
    w = fx.walk
    assert fx.unrelated()[5] == [w[3:9]] * 3 and fx.candidates()[4][-1] == w[10:14]
    for s in (fx.unrelated()[5], fx.candidates()[4]):
        _, probs, o3 = o.single_detail(rs, s)
        assert (probs > 0).any() and int(o3[0]) < sc.N_SINGLE
    _, once, _ = o.single_detail(rs, [w[3:9]])
    _, thrice, _ = o.single_detail(rs, [w[3:9]] * 3)
    hit = once > 0
    assert hit.any()
    assert (thrice[hit] == 3 * once[hit]).any(), (thrice[hit][:5], once[hit][:5])
    # the stretch two paths hold: reads inside it count twice
    _, base, _ = o.single_detail(rs, fx.candidates()[0])
    _, twice, _ = o.single_detail(rs, fx.candidates()[4])
    assert (twice > base).any() and np.array_equal(twice[twice == base], base[twice == base])
