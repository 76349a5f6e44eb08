"""The action selection's Python model (tests/decide_model.py) and the action table
(aigar_amd/actions.py) against the reference's own decideMove and createDiscreteActions*
recorded in tests/golden/decide_*.npz (tools/golden/gen_decide_golden.py): tolerance 0,
bit patterns equal.  CPU only."""
import os

import numpy as np
import pytest

import decide_model as dm


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def cases(golden_dir):
    return np.load(os.path.join(golden_dir, "decide_cases.npz"))


def test_tables_are_the_references(golden_dir):
    from aigar_amd import actions
    z = np.load(os.path.join(golden_dir, "decide_tables.npz"))
    seen = set()
    for k in range(len(z["t_num"])):
        num, sq, sp, ej = (int(z[n][k]) for n in ("t_num", "t_square", "t_split", "t_eject"))
        want = z["rows"][z["t_off"][k]:z["t_off"][k + 1]]
        got = actions.discrete_actions(num, bool(sq), bool(sp), bool(ej))
        assert got.shape == want.shape == (num * (1 + sp + ej), 4)
        assert np.array_equal(bits(got), bits(want)), (num, sq, sp, ej)
        seen.add((num, sq))
    # every count on the circle; the square ones the reference can build (it quits on 8
    # and its is_square(1) divides by zero)
    assert {(n, 0) for n in (1, 4, 8, 25, 100)} | {(n, 1) for n in (4, 25, 100)} == seen
    with pytest.raises(ValueError):
        actions.discrete_actions(8, True)
    assert actions.discrete_actions(1, True).tolist() == [[0.5, 0.5, 0.0, 0.0]]
    # the order: base, split, eject per direction
    t = actions.discrete_actions(4, True, True, True)
    assert t[:, 2].tolist() == [0, 1, 0] * 4 and t[:, 3].tolist() == [0, 0, 1] * 4
    assert np.array_equal(t[0, :2], t[1, :2]) and np.array_equal(t[0, :2], t[2, :2])


def test_from_parameters_reads_the_four_settings():
    import types

    from aigar_amd import actions
    p = types.SimpleNamespace(NUM_ACTIONS=9, SQUARE_ACTIONS=False, ENABLE_SPLIT=True, ENABLE_EJECT=False)
    assert np.array_equal(actions.from_parameters(p), actions.discrete_actions(9, False, True, False))
    assert actions.from_parameters(types.SimpleNamespace()).shape == (25, 4)


def test_model_replays_every_golden_case(cases):
    z = cases
    n = len(z["idx"])
    kinds = set()
    for k in range(n):
        q = z["q"][z["off"][k]:z["off"][k + 1]].tolist()
        idx, val, bad = dm.decide_row(q, int(z["strategy"][k]), float(z["epsilon"][k]), float(z["temperature"][k]),
                                      z["u"][k].tolist())
        assert not bad
        assert idx == z["idx"][k], k
        want = float(z["value"][k])
        assert (np.isnan(val) and np.isnan(want)) or bits([val])[0] == bits([want])[0], k
        kinds.add((int(z["strategy"][k]), len(q), float(z["temperature"][k]), float(z["epsilon"][k])))
    # what the file was recorded for
    for m in (1, 7, 8, 9, 25, 75, 128, 129, 300):
        for t in (7.0, 0.5, 0.05, 0.0):
            assert (1, m, t, 0.0) in kinds
    for e in (0.0, 1.0, 0.5):
        assert any(k[0] == 0 and k[3] == e for k in kinds)


def test_golden_cases_cover_ties_explore_and_the_draw_edges(cases):
    z = cases
    st, u, idx = z["strategy"], z["u"], z["idx"]
    boltz = (st == 1) & (z["temperature"] != 0)
    assert (u[boltz, 2] == 0.0).any() and (u[boltz, 2] == 1.0 - 2.0 ** -53).any()
    moved = cdf_hit = 0
    for k in np.nonzero(boltz)[0]:
        q = z["q"][z["off"][k]:z["off"][k + 1]].tolist()
        p = dm.boltzmann_dist(q, float(z["temperature"][k]))
        cdf = dm.boltzmann_cdf(p)
        kk = min(int(np.searchsorted(cdf, u[k, 2], side="right")), len(q) - 1)
        moved += int(idx[k] != kk)  # the fold onto the first equal probability changed the index
        cdf_hit += int(z["forced"][k] and (cdf == u[k, 2]).any())
    assert moved >= 1 and cdf_hit >= 1
    eg = st == 0
    half = eg & (z["epsilon"] == 0.5)
    assert np.isnan(z["value"][half]).any() and (~np.isnan(z["value"][half])).any()
    assert np.isnan(z["value"][eg & (z["epsilon"] == 1.0)]).all()
    assert not np.isnan(z["value"][eg & (z["epsilon"] == 0.0)]).any()


def test_own_draws_are_philox_words():
    a = dm.own_draws(5, 12, 99, [3, 4])
    assert a == dm.own_draws(5, 12, 99, [3, 4]) and all(0.0 <= v < 1.0 for v in a)
    assert a != dm.own_draws(5, 13, 99, [3, 4]) and a != dm.own_draws(5, 12, 98, [3, 4]) and a != dm.own_draws(6, 12, 99, [3, 4])
    assert dm.own_draws(0, 0, 0, [1, 2]) != dm.own_draws(0, 0, 0, [1, 3])  # (counter word 0 wraps below zero)


def test_dead_and_nonfinite_rows():
    table = np.arange(12.0).reshape(3, 4)
    q = np.array([[1.0, 3.0, 3.0], [0.0, float("nan"), 1.0], [5.0, 1.0, 1.0], [float("inf"), 0.0, 0.0]])
    idx, val, act, bad = dm.decide(q, table, dm.BOLTZMANN, 0.0, 0.0, [True, True, False, True], u=np.zeros((4, 3)))
    assert idx.tolist() == [1, 0, -1, 0] and bad.tolist() == [False, True, False, True]
    assert val[0] == 3.0 and val[1] == 0.0 and np.isnan(val[2]) and val[3] == float("inf")
    assert np.array_equal(act[0], table[1]) and np.isnan(act[2]).all()
