"""GPU: the helpers of aigar_sem.h and the exact integer helpers of aigar_math.h, run one element
per thread through aigar_selftest_sem, against Python's own operation element by element, by
bit pattern, at tolerance 0 and with no element skipped (tests/math_cases.py holds the inputs,
tests/test_math_cases.py what they cover).  The references are the reference project's own
expressions: its model is Python floats, numpy.sum and the math module."""
import math

import numpy as np
import pytest

from aigar_amd import _abi, model
import math_cases as mc
from math_cases import fl, same

pytestmark = pytest.mark.gpu

_lib = pytest.importorskip("aigar_amd._lib")

# aigar_sem.h's parameters.py constants, as the reference computes them
FPS, GAME_SPEED = 30, 1
SPEED_MODIFIER = GAME_SPEED / FPS
CELL_MOVE_SPEED = 90 * SPEED_MODIFIER
BASE_MERGE_TIME, MERGE_TIME_MASS_FACTOR = 25, 0.0233


def test_mod_pos_is_python_float_mod():
    a, b = mc.mod_pos_cases()
    got, = _lib.selftest_sem(_abi.SEM_MOD_POS, a, b)
    same("mod_pos", got, fl([p % q for p, q in zip(a.tolist(), b.tolist())]), a, b)


@pytest.mark.parametrize("family", ["trunc_div_mask_loops", "trunc_div_pow2", "trunc_div_decimal"])
def test_trunc_div_pos_is_int_of_the_quotient(family):
    x, b = getattr(mc, family)()
    got, = _lib.selftest_sem(_abi.SEM_TRUNC_DIV_POS, x, b)
    same("trunc_div_pos", got, fl([int(p / q) for p, q in zip(x.tolist(), b.tolist())]), x, b)


def test_py_mod_is_python_float_mod():
    a, b = mc.py_mod_cases()
    got, = _lib.selftest_sem(_abi.SEM_PY_MOD, a, b)
    same("py_mod", got, fl([p % q for p, q in zip(a.tolist(), b.tolist())]), a, b)


def test_py_round3_is_python_round():
    v = mc.round3_cases()
    got, = _lib.selftest_sem(_abi.SEM_ROUND3, v)
    same("py_round3", got, fl([round(p, 3) for p in v.tolist()]), v)


def test_np_sum_and_npacc_are_numpy_sum():
    terms, cnt = mc.sum_cases()
    got_sum, got_acc = _lib.selftest_sem(_abi.SEM_SUM, *terms, cnt)
    cols = np.ascontiguousarray(terms.T)
    want = fl([np.sum(row[:int(c)]) for row, c in zip(cols, cnt)])
    same("np_sum", got_sum, want, cnt, *terms)
    same("NpAcc", got_acc, want, cnt, *terms)


def test_radii_are_python_sqrt():
    m = mc.radius_cases()
    got_r, got_p = _lib.selftest_sem(_abi.SEM_RADIUS, m)
    want = fl([math.sqrt(p / math.pi) if p > 0 else 0.0 for p in m.tolist()])
    same("radius_of", got_r, want, m)
    same("pellet_radius", got_p, want, m)


def test_buckets_are_python_floor_division():
    c, cols = mc.bucket_cases()
    got_s, got_f, got_c = _lib.selftest_sem(_abi.SEM_BUCKET, c, cols)
    floor = fl([int(p // 20) for p in c.tolist()])  # (the device returns an int: no sign of zero)
    same("bucket_floor_s", got_s, floor, c)
    pos = c >= 0
    same("bucket_floor", got_f, np.where(pos, floor, -1.0), c)
    same("center_bucket_coord", got_c, np.where(pos, np.minimum(floor, cols - 1), -1.0), c, cols)


def test_footprint_is_the_models():
    px, py, rad, size = mc.footprint_cases()
    got = _lib.selftest_sem(_abi.SEM_FOOTPRINT, px, py, rad, size)
    want = [np.zeros(len(px)) for _ in range(4)]
    for s in np.unique(size):
        rows = size == s
        for w, v in zip(want, model._footprint(px[rows], py[rows], rad[rows], int(s))):
            w[rows] = v
    for name, g, w in zip(("x0", "x1", "y0", "y1"), got, want):
        same("footprint " + name, g, w, px, py, rad, size)


def set_move_direction(x, y, m, r, cpx, cpy):
    """cell.py:47-57 (getReducedSpeed: CELL_MOVE_SPEED * mass ** -0.35), Python floats and math."""
    x_diff = cpx - x
    y_diff = cpy - y
    hypotenuse_squared = x_diff * x_diff + y_diff * y_diff
    radius_squared = r * r
    speed_modifier = min(hypotenuse_squared, radius_squared) / radius_squared
    angle = math.atan2(y_diff, x_diff)
    reduced = CELL_MOVE_SPEED * math.pow(m, -0.35)
    return reduced * speed_modifier * math.cos(angle), reduced * speed_modifier * math.sin(angle), math.cos(angle), \
        math.sin(angle)


def test_set_move_direction_is_the_references():
    cols = mc.move_cases()
    got = _lib.selftest_sem(_abi.SEM_MOVE, *cols)
    want = fl([set_move_direction(*row) for row in zip(*(c.tolist() for c in cols))]).T
    for name, g, w in zip(("vx", "vy", "cos", "sin"), got, want):
        same("set_move_direction " + name, g, w, *cols)


def add_momentum(x, y, cpx, cpy, w, h, orig_r):
    """cell.py:96-103, Python floats and math (max(0, ...) keeps a float operand's value: 0 and 0.0
    differ in type only, and -0.0 never reaches it from a coordinate)."""
    checked_x = max(0, min(w, cpx))
    checked_y = max(0, min(h, cpy))
    angle = math.atan2(checked_y - y, checked_x - x)
    speed = 2 + orig_r * 0.05
    return math.cos(angle) * speed, math.sin(angle) * speed


def test_add_momentum_is_the_references():
    cols = mc.momentum_cases()
    got = _lib.selftest_sem(_abi.SEM_MOMENTUM, *cols)
    want = fl([add_momentum(*row) for row in zip(*(c.tolist() for c in cols))]).T
    for name, g, w in zip(("svx", "svy"), got, want):
        same("add_momentum " + name, g, w, *cols)


def test_merge_time_is_the_references():
    f, m = mc.merge_time_cases()
    got, = _lib.selftest_sem(_abi.SEM_MERGE_TIME, f, m)
    want = fl([p * (BASE_MERGE_TIME + q * MERGE_TIME_MASS_FACTOR) * FPS / 2 / GAME_SPEED
               for p, q in zip(f.tolist(), m.tolist())])  # cell.py:154-155
    same("merge_time_for", got, want, f, m)


def test_philox_u01_and_randint():
    c0, c1, c2, c3, k0, k1, lo, hi = mc.philox_cases()
    out = _lib.selftest_sem(_abi.SEM_PHILOX, c0, c1, c2, c3, k0, k1, lo, hi)
    words = np.stack([o.view(np.uint64) for o in out[:4]], axis=1)
    want = np.zeros_like(words)
    for i in range(len(c0)):
        # numpy's generator steps the counter before it draws: hand it the one before (c0 >= 1)
        ctr = np.array([c0[i] - np.uint64(1), c1[i], c2[i], c3[i]], dtype=np.uint64)
        want[i] = np.random.Philox(key=np.array([k0[i], k1[i]], dtype=np.uint64), counter=ctr).random_raw(4)
    bad = np.flatnonzero((words != want).any(axis=1))
    assert not len(bad), "philox: %d of %d differ, first (counter, key) -> device, numpy: %s" % (
        len(bad), len(c0), [([hex(int(v[i])) for v in (c0, c1, c2, c3, k0, k1)], [hex(int(w)) for w in words[i]],
                             [hex(int(w)) for w in want[i]]) for i in bad[:5]])
    u = [int(w) for w in want[:, 0]]
    same("u01", out[4], fl([(w >> 11) * (1.0 / 9007199254740992.0) for w in u]), out[0], lo, hi)
    randint = [int(a) + ((w * (int(b) - int(a))) >> 64) if int(b) > int(a) else int(a)
               for w, a, b in zip(u, lo.tolist(), hi.tolist())]
    same("ph_randint", out[5], fl(randint), out[0], lo, hi)
