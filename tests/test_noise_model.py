"""tests/noise_model.py, the specification of the exploration noise, against the records of
the reference's own applyNoise / decideMove (tests/golden/noise_cases.npz, written by
tools/golden/gen_noise_golden.py) and against numpy.random.RandomState.normal itself.
CPU only; everything is compared by bit pattern."""
import os

import numpy as np

import noise_model as nm

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "noise_cases.npz")


def _cases():
    return dict(np.load(GOLD))


def test_golden_set_holds_every_rejection_count_and_both_clips():
    g = _cases()
    cnt = g["cnt"][g["cnt"] > 0] - 1  # rejections per drawn pair
    assert {0, 1, 2} <= set(cnt.tolist()) and (cnt >= 3).any()
    assert set(g["n"].tolist()) == {2, 3, 4} and set(g["kind"].tolist()) == {0, 1}
    assert set(g["std"].tolist()) == {0.0, 0.02, 1.0}
    vals = g["out"][~np.isnan(g["out"])]
    assert (vals == 0.0).any() and (vals == 1.0).any() and np.signbit(vals[vals == 0.0]).any()
    chains = g["chain"][g["chain"] >= 0]
    assert len(chains) and min(np.bincount(chains)) >= 20


def test_model_equals_every_recorded_call():
    g = _cases()
    carried = {}
    for k in range(len(g["n"])):
        n, kind = int(g["n"][k]), int(g["kind"][k])
        prev = g["prev"][k][:n] if kind == nm.ORN_UHL else None
        ch = int(g["chain"][k])
        if ch >= 0 and ch in carried:  # a chain's call starts from the state the model itself carried
            assert nm.bits_equal(carried[ch], prev), k
            prev = carried[ch]
        out, state, exhausted, bad = nm.noise_row(g["mu"][k][:n].tolist(), g["std"][k], g["u"][k], kind, prev,
                                                  g["theta"][k], g["ou_mu"][k], g["dt"][k])
        assert exhausted == 0 and not bad
        assert nm.bits_equal(out, g["out"][k][:n]), (k, out, g["out"][k])
        if kind == nm.ORN_UHL:
            assert nm.bits_equal(state, g["post"][k][:n]), (k, state, g["post"][k])
            if ch >= 0:
                carried[ch] = np.array(state)
        # the attempts each pair consumed are the ones the reference's generator consumed
        for pair in range((n + 1) // 2):
            assert nm.normal_pair(g["u"][k][pair].tolist())[2] == g["cnt"][k][pair]


def test_model_equals_numpy_normal_on_fresh_draws():
    """10^5 standard normals of RandomState(seed).normal against the model fed with a twin
    generator's random_sample: numpy's order (f * x2, then the cached f * x1) included."""
    seed, count = 424242, 100000
    want = np.random.RandomState(seed).normal(size=count)
    twin = np.random.RandomState(seed)
    got = []
    while len(got) < count:
        att = []
        while True:
            att.append((float(twin.random_sample()), float(twin.random_sample())))
            z0, z1, used = nm.normal_pair(att[-1:])
            if used:
                break
        got += [z0, z1]
    assert nm.bits_equal(got[:count], want)
    # ... and loc + scale * z, the form applyNoise uses
    w2 = np.random.RandomState(7).normal(np.array([0.25, 0.5, 0.75, 1.0]), 0.02, 4)
    t2 = np.random.RandomState(7)
    z = []
    while len(z) < 4:
        z0, z1, used = nm.normal_pair([(float(t2.random_sample()), float(t2.random_sample()))])
        if used:
            z += [z0, z1]
    assert nm.bits_equal([m + 0.02 * v for m, v in zip([0.25, 0.5, 0.75, 1.0], z)], w2)


def test_crafted_uniforms_reject_at_every_attempt_and_exhaust():
    ok, far, centre = (0.75, 0.5), (1.0 - nm.GRID, 1.0 - nm.GRID), (0.5, 0.5)  # r2 = 0.25, ~2, 0
    want = nm.normal_pair([ok])
    assert want[2] == 1 and want[0] == 0.0 and want[1] > 0  # x2 = 0: f * x2 = 0, f * x1 > 0
    for T in (1, 4, 16):
        for t in range(T):
            for rej in (far, centre):
                z0, z1, used = nm.normal_pair([rej] * t + [ok] + [far] * (T - t - 1))
                assert (z0, z1, used) == (want[0], want[1], t + 1)
        for rej in (far, centre):
            assert nm.normal_pair([rej] * T) == (0.0, 0.0, None)
    # a row: pair 1 exhausted, pair 0 not; the exhausted values are mu itself (clipped)
    u = [[ok] + [far] * 3, [centre] * 4]
    out, state, exhausted, bad = nm.noise_row([0.5, 0.5, 0.25, 1.5], 1.0, u)
    assert exhausted == 1 and not bad and out[2:] == [0.25, 1.0] and out[0] == 0.5 and out[1] == 1.0
    # an odd n drops the leftover normal of its last pair
    o3 = nm.noise_row([0.5, 0.5, 0.5], 0.1, [[ok], [(0.5, 0.75)]])[0]
    assert o3[2] == 0.5 + 0.1 * nm.normal_pair([(0.5, 0.75)])[0]
    # outside the contract: a non-finite mu is taken as 0, a bad std as 0, both flagged
    assert nm.noise_row([float("nan"), 0.5], 0.0, [[ok], []]) == ([0.0, 0.5], None, 0, True)
    assert nm.noise_row([0.25, 0.5], -1.0, [[ok], []]) == ([0.25, 0.5], None, 0, True)
    assert nm.noise_row([0.25, 0.5], float("inf"), [[ok], []])[3]


def test_own_draws_are_on_numpys_grid_and_distinct():
    a = nm.own_draws(5, 0, 17, 3, (11, 12))
    b = nm.own_draws(5, 1, 17, 3, (11, 12))
    assert len(a) == len(b) == nm.OWN_T and a != b and a != nm.own_draws(6, 0, 17, 3, (11, 12))
    assert a != nm.own_draws(5, 0, 18, 3, (11, 12)) and a != nm.own_draws(5, 0, 17, 4, (11, 12))
    for ua, ub in a + b:
        assert 0.0 <= ua < 1.0 and (ua / nm.GRID) == int(ua / nm.GRID) and 0.0 <= ub < 1.0
