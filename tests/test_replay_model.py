"""tests/replay_model.py against the golden scripts recorded from the reference's
ReplayBuffer / PrioritizedReplayBuffer (tools/golden/gen_replay_golden.py), at tolerance
0: indices equal, weights and tree roots by bit pattern.  CPU only."""
import os

import numpy as np
import pytest

from replay_model import ReplayModel, bits, golden_u, load_golden

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("name", ["replay_prio", "replay_uniform"])
def test_model_replays_the_golden_script(name):
    meta, ops = load_golden(os.path.join(GOLDEN, name + ".npz"))
    m = ReplayModel(meta["capacity"], meta["prioritized"], meta["alpha"], meta["beta"])
    assert meta["capacity"] == 10 and m.it_cap == 16
    n_add = n_samp = 0
    for kind, op in ops:
        if kind == "add":
            m.add(op["add_s"], op["add_a"], op["add_r"], op["add_s2"], op["add_done"])
            n_add += len(op["add_r"])
        elif kind == "sample":
            idx, w = m.sample(golden_u(op, meta["prioritized"], m.size))
            assert idx == list(op["samp_idx"])
            assert np.array_equal(bits(w), bits(op["samp_w"]))
            assert np.array_equal(bits([row[2] for row in m.gather(idx)]), bits(op["samp_r"]))
            n_samp += 1
        else:
            m.update(op["upd_idx"], op["upd_prio"])
        assert (m.size, m.next) == (op["size"], op["next_idx"])
        if meta["prioritized"]:
            assert bits(m.total()) == bits(op["total"])
            assert bits(m.minimum()) == bits(op["vmin"])
            assert bits(m.max_priority) == bits(op["max_priority"])
    assert n_add >= 13 and n_samp >= 2 and m.added == n_add  # (the script wraps the ring of 10)


def test_golden_script_has_the_cases_the_memory_must_handle():
    meta, ops = load_golden(os.path.join(GOLDEN, "replay_prio.npz"))
    ups = [op for kind, op in ops if kind == "update"]
    # a repeated index whose last value is not its largest
    assert any(list(u["upd_idx"]).count(i) > 1 and
               u["upd_prio"][np.nonzero(u["upd_idx"] == i)[0][-1]] < u["upd_prio"][u["upd_idx"] == i].max()
               for u in ups for i in set(u["upd_idx"]))
    assert any((u["upd_prio"] > 1).any() for u in ups) and any((u["upd_prio"] == 1e-4).any() for u in ups)
    # max_priority moves, and adds follow that use it
    kinds = [k for k, _ in ops]
    moved = [i for i, (_, op) in enumerate(ops) if op["max_priority"] > 1][0]
    assert "add" in kinds[moved + 1:]
    # a sample before and after the wrap
    added, wrapped_at = 0, None
    for i, (k, op) in enumerate(ops):
        if k == "add":
            added += len(op["add_r"])
            if added > meta["capacity"] and wrapped_at is None:
                wrapped_at = i
    assert "sample" in kinds[:wrapped_at] and "sample" in kinds[wrapped_at + 1:]


def test_too_small_memory_gives_minus_one_and_nan():
    for prio in (False, True):
        m = ReplayModel(5, prio)
        idx, w = m.sample([0.0, 0.5])
        assert idx == [-1, -1] and all(np.isnan(w))
    m = ReplayModel(5, True)
    m.add(np.zeros((1, 2)), np.zeros((1, 4)), [0.0], np.zeros((1, 2)), [0])
    assert m.sample([0.3])[0] == [-1]
    m.add(np.zeros((1, 2)), np.zeros((1, 4)), [0.0], np.zeros((1, 2)), [0])
    assert m.sample([0.3])[0] == [0]  # (the mass spans the leaves [0, size - 2] only)
