"""The Q-learning bots' discrete action table (network.py:26-65).

`discrete_actions` restates createDiscreteActionsSquare / createDiscreteActionsCircle:
one [x, y, split, eject] row per network output, in the order base, split, eject per
direction.  The rows are what `aigar_decide_config` uploads and what the chosen index
is turned into (a 4-value action of `apply_actions`).  Pure Python floats: the values
are the reference's, bit for bit (tests/test_decide_model.py).
"""
import math

import numpy as np


def _is_square(n):
    r = math.isqrt(n)
    return r * r == n


def discrete_actions(num_actions, square=True, enable_split=False, enable_eject=False):
    """[n_out, 4] float64 with n_out = num_actions * (1 + enable_split + enable_eject).
    square: a grid of int(sqrt(num_actions)) points per side at the cell centres
    (num_actions must be a perfect square: ValueError, where the reference quits);
    else num_actions directions on the unit circle, 360 / num_actions degrees apart."""
    n = int(num_actions)
    if n < 1:
        raise ValueError("discrete_actions: NUM_ACTIONS = %d" % n)
    points = []
    if square:
        if not _is_square(n):
            raise ValueError("discrete_actions: NUM_ACTIONS = %d is not a perfect square (SQUARE_ACTIONS)" % n)
        side = int(math.sqrt(n))
        for row in range(side):
            for col in range(side):
                points.append((col / side + 1 / side / 2, row / side + 1 / side / 2))
    else:
        deg_per_action = 360 / n
        for k in range(n):
            degree = math.radians(k * deg_per_action)
            points.append((math.cos(degree), math.sin(degree)))
    rows = []
    for x, y in points:
        rows.append([x, y, 0, 0])
        if enable_split:
            rows.append([x, y, 1, 0])
        if enable_eject:
            rows.append([x, y, 0, 1])
    return np.array(rows, np.float64).reshape(-1, 4)


def from_parameters(parameters):
    """The table of a parameter set: NUM_ACTIONS, SQUARE_ACTIONS, ENABLE_SPLIT, ENABLE_EJECT."""
    g = lambda n, dflt: getattr(parameters, n, dflt)  # noqa: E731
    return discrete_actions(int(g("NUM_ACTIONS", 25)), bool(g("SQUARE_ACTIONS", True)), bool(g("ENABLE_SPLIT", False)),
                            bool(g("ENABLE_EJECT", False)))
