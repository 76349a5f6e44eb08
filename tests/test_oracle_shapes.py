"""CPU: the worlds of test_gpu_shapes.py and test_gpu_obs_masks.py, run by the
oracle alone, are worth comparing.  A fresh world only eats pellets for its
first 40 ticks; the matured starts of tests/shapes.py split, eject, eat cells
and blobs, hit viruses, die and respawn in every arena of every shape, and the
mask worlds fill every grid channel the reference can fill.  The GPU tests
assert the same conditions on the logs and rows they compare, so a change of
seed or shape that empties a run fails here first, on a machine without a GPU.

Per-arena minimum counts measured with the seeds of shapes.py, for the record
(the tests assert presence, not these figures):
  synthetic commands, 40 ticks, kinds 4 / 5 / 6 / 7 / 8 / 9 / 10:
    7 x 36: 2 / 2 / 436 / 46 / 76 / 24 / 24, the other shapes higher;
  Greedy, 40 ticks, kinds 4 / 5 / 6 / 8 / 9 / 10: 5 x 67: 2 / 2 / 734 / 65 / 31 / 30.
Merges (kind 1) and virus splits (kind 3) do not happen within 40 ticks of
these starts; the golden-state tests cover them."""
import numpy as np
import pytest

from aigar_amd import _abi
from oracle_lib import Oracle
import shapes as S


@pytest.mark.parametrize("shape", S.SHAPES, ids=S.SHAPE_IDS)
def test_shapes_synthetic_commands(shape):
    A = shape[0]
    o = S.start(Oracle(S.shape_config(shape)), A, S.SHAPE_SEED)
    w, rng, seen = S.Worth(A), S.synthetic_rng(), S.Seen(S.FULL_CH, 11)
    for t in range(S.SHAPE_TICKS):
        o.set_commands(S.synthetic(rng, shape))
        o.step(1)
        w.tick(o)
        if (t + 1) % 5 == 0:
            seen.rows(o.observe())
    w.check_synthetic()
    seen.check()
    o.close()


@pytest.mark.parametrize("shape", S.SHAPES, ids=S.SHAPE_IDS)
def test_shapes_greedy(shape):
    """40 ticks, and the 25 ticks the GPU tests run (5 calls of 5 steps)."""
    A = shape[0]
    o = S.start(Oracle(S.shape_config(shape)), A, S.SHAPE_SEED)
    w = S.Worth(A)
    for t in range(40):
        o.policy_greedy(True)
        o.step(1)
        w.tick(o)
        if t + 1 == S.GREEDY_CALLS * S.GREEDY_STEPS:
            w.check_greedy()
    w.check_greedy()
    o.close()


def test_heavy_cells_eat_beside_the_arena_boundaries():
    o = S.heavy_start(Oracle(S.shape_config(S.HEAVY_SHAPE)))
    A = S.HEAVY_SHAPE[0]
    rng, meals = S.synthetic_rng(), S.HeavyMeals()
    meals.before(o)
    for _ in range(S.HEAVY_TICKS):
        o.set_commands(S.heavy_commands(rng))
        o.step(1)
        meals.after(o, [o.events(a) for a in range(A)])
    meals.check()
    o.close()


def test_mature_is_the_same_world_on_a_second_handle():
    shape = S.SHAPES[5]
    a = S.start(Oracle(S.shape_config(shape)), shape[0], S.SHAPE_SEED)
    b = S.start(Oracle(S.shape_config(shape)), shape[0], S.SHAPE_SEED)
    for k in range(shape[0]):
        sa, sb = a.get_state(k), b.get_state(k)
        assert np.array_equal(sa["cells_f"], sb["cells_f"])
        m = sa["cells_f"][:, 2]
        assert m.min() >= 12 and m.max() <= 900 and np.array_equal(sa["cells_f"][:, 3], np.sqrt(m / np.pi))
    assert not np.array_equal(a.get_state(0)["cells_f"][:, 2], a.get_state(1)["cells_f"][:, 2])


def test_obs_bits_equal_sees_signed_zeros_and_nan_positions():
    x = np.array([[0.0, 1.5, np.nan], [2.0, -0.0, 3.0]])
    assert S.obs_bits_equal(x, x.copy())
    y = x.copy()
    y[0, 0] = -0.0
    assert np.array_equal(np.nan_to_num(x), np.nan_to_num(y)) and not S.obs_bits_equal(x, y)
    y = x.copy()
    y[1, 1] = 0.0
    assert not S.obs_bits_equal(x, y)
    y = x.copy()
    y[0, 2], y[0, 1] = 1.5, np.nan
    assert not S.obs_bits_equal(x, y)
    assert not S.obs_bits_equal(x, x.astype(np.float32))
    x32 = x.astype(np.float32)
    y32 = x32.copy()
    assert S.obs_bits_equal(x32, y32)
    y32[1, 1] = 0.0
    assert not S.obs_bits_equal(x32, y32)
    assert not S.obs_bits_equal(x, x[:1])


def _mask_world(channels, extras, G):
    cfg = S.mask_config(channels, extras, G)
    o = S.start(Oracle(cfg), 1, S.MASK_SEED, hi=S.MASK_HI)
    seen, rng = S.Seen(channels, G), np.random.default_rng(S.MASK_SEED)
    for _ in range(S.MASK_TICKS):
        cmd = S.mask_commands(rng)
        o.set_actions(cmd, 0.5 * cmd)
        o.set_commands(cmd)
        o.step(1)
        seen.rows(o.observe())
    o.close()
    return seen


@pytest.mark.parametrize("G", S.MASK_GRIDS)
@pytest.mark.parametrize("channels,extras", S.MASKS, ids=S.MASK_IDS)
def test_mask_worlds_fill_their_channels(channels, extras, G):
    _mask_world(channels, extras, G).check()


def test_mask_world_events():
    """The mask worlds are one world (the observation does not act on it): it splits,
    ejects, eats cells and respawns within its 20 ticks."""
    o = S.start(Oracle(S.mask_config(S.FULL_CH, S.FULL_EX)), 1, S.MASK_SEED, hi=S.MASK_HI)
    w, rng = S.Worth(1), np.random.default_rng(S.MASK_SEED)
    for _ in range(S.MASK_TICKS):
        o.set_commands(S.mask_commands(rng))
        o.step(1)
        w.tick(o)
    c = w.counts()[0]
    assert all(c.get(k, 0) > 0 for k in (_abi.EV_CELL_EAT_PELLET, _abi.EV_CELL_EAT_BLOB, _abi.EV_CELL_EAT_CELL,
                                         _abi.EV_PLAYER_DEATH, _abi.EV_RESPAWN)), c
    assert w.cells >= 4, w.cells
    o.close()


@pytest.mark.parametrize("shape", S.FALLBACK_SHAPES, ids=["5x67", "1x257"])
@pytest.mark.parametrize("channels,G", S.FALLBACK, ids=S.FALLBACK_IDS)
def test_fallback_rows_are_not_empty(shape, channels, G):
    """The rows of the Greedy-fallback configurations at the two shapes: live bots
    get numbers, every configured grid channel that is fed is filled."""
    A = shape[0]
    o = S.start(Oracle(S.shape_config(shape, channels, 0 if channels & _abi.OBS_SIMPLE else S.FULL_EX, G)), A,
                S.SHAPE_SEED)
    seen = None if channels & _abi.OBS_SIMPLE else S.Seen(channels, G)
    for _ in range(S.GREEDY_CALLS * S.GREEDY_STEPS):
        o.policy_greedy(True)
        o.step(1)
        rows = o.observe()
        if seen:
            seen.rows(rows)
        else:
            assert rows.shape[1] == 12 and (np.nan_to_num(rows) != 0).any()
    if seen:
        seen.check()
    o.close()
