"""Shared world builders of the ragged-shape and observation-mask tests
(test_oracle_shapes.py on the CPU, test_gpu_shapes.py and test_gpu_obs_masks.py
on the device): the shape table, the matured start, the bit-pattern row
comparison and the oracle-side drivers whose event logs say whether a run is
worth comparing (test infrastructure, like parity.py)."""
import math

import numpy as np

from aigar_amd import _abi
from oracle_lib import make_config
import parity

FULL_CH = (_abi.OBS_PELLET | _abi.OBS_SELF | _abi.OBS_WALL | _abi.OBS_ENEMY | _abi.OBS_VIRUS | _abi.OBS_SELF_SLF
           | _abi.OBS_SELF_LF | _abi.OBS_ENEMY_SLF | _abi.OBS_ENEMY_LF)  # 0x3ef
FULL_EX = 0x1F

# (arenas, bots per arena, field size, max_viruses); viruses on.  What each row cuts:
#   1 x 257  second k_players tile holds one player; k_observe grid of 257 blocks (nb & 7 = 1)
#   1 x 300  partial second tile; 75 wave-per-player blocks (nb & 7 = 3)
#   2 x 260  two tiles per arena with the y grid dimension > 1; NP = 520: 3 NP-blocks, the
#            arena boundary inside block 1
#   3 x 100  NP = 300: block 0 holds arenas 0, 1 and part of 2; waves span arenas
#   5 x 67   B odd: a block's four players and a wave's 64 lanes straddle arenas; 84 blocks
#   7 x 36   NP = 252: one partial NP-block with seven arenas in four waves
SHAPES = [(1, 257, 480, 30), (1, 300, 520, 30), (2, 260, 480, 30), (3, 100, 300, 12), (5, 67, 250, 12),
          (7, 36, 180, 8)]
SHAPE_IDS = ["%dx%d" % s[:2] for s in SHAPES]
SHAPE_SEED = 31
SHAPE_TICKS = 40  # separate calls, synthetic commands
RANDOM_TICKS = 20  # graph, random policy
GREEDY_CALLS, GREEDY_STEPS = 5, 5  # graph, Greedy policy: 25 ticks
P_SPLIT = P_EJECT = 0.08

SYNTH_KINDS = (_abi.EV_CELL_EAT_VIRUS, _abi.EV_EXPLODE, _abi.EV_CELL_EAT_PELLET, _abi.EV_CELL_EAT_BLOB,
               _abi.EV_CELL_EAT_CELL, _abi.EV_PLAYER_DEATH, _abi.EV_RESPAWN)
GREEDY_KINDS = (_abi.EV_CELL_EAT_VIRUS, _abi.EV_EXPLODE, _abi.EV_CELL_EAT_PELLET, _abi.EV_CELL_EAT_CELL,
                _abi.EV_PLAYER_DEATH, _abi.EV_RESPAWN)

# the observation-mask worlds
MASK_BOTS, MASK_FIELD, MASK_VIRUSES, MASK_SEED, MASK_TICKS, MASK_HI = 24, 200, 8, 5, 20, 400.0
MASK_GRIDS = (11, 16, 17, 42)  # k_observe up to 16 squares per side, k_observe_wide above
_O, _E = _abi, _abi
MASKS = [
    (_O.OBS_ALL, 0),
    (_O.OBS_PELLET | _O.OBS_WALL | _O.OBS_ALL | _O.OBS_VIRUS, _E.EX_LAST_FOV),
    (_O.OBS_SELF | _O.OBS_ENEMY | _O.OBS_VIRUS, _E.EX_FOV),
    (_O.OBS_WALL, _E.EX_MASS),
    (_O.OBS_SELF_SLF, _E.EX_LAST_ACT),
    (_O.OBS_SELF_LF | _O.OBS_ENEMY_SLF, _E.EX_2LAST_ACT),
    (_O.OBS_SELF | _O.OBS_ENEMY | _O.OBS_SELF_SLF | _O.OBS_ENEMY_LF, _E.EX_LAST_ACT | _E.EX_2LAST_ACT),
    (_O.OBS_VIRUS | _O.OBS_ENEMY_SLF | _O.OBS_ENEMY_LF, _E.EX_LAST_FOV | _E.EX_MASS),
    (_O.OBS_PELLET | _O.OBS_SELF_SLF | _O.OBS_SELF_LF | _O.OBS_ENEMY_SLF | _O.OBS_ENEMY_LF,
     _E.EX_LAST_FOV | _E.EX_FOV | _E.EX_2LAST_ACT),
    (_O.OBS_ENEMY | _O.OBS_ALL, _E.EX_FOV | _E.EX_LAST_ACT),
]
MASK_IDS = ["ch%03x-ex%02x" % m for m in MASKS]
GRID_BITS = (_abi.OBS_PELLET, _abi.OBS_SELF, _abi.OBS_WALL, _abi.OBS_ENEMY, _abi.OBS_ALL, _abi.OBS_VIRUS,
             _abi.OBS_SELF_SLF, _abi.OBS_SELF_LF, _abi.OBS_ENEMY_SLF, _abi.OBS_ENEMY_LF)  # stacking order

# aigar_run's Greedy fallback (the observation does not make the Greedy moves): (channels, grid squares)
FALLBACK = [(_abi.OBS_SELF | _abi.OBS_ENEMY | _abi.OBS_VIRUS, 11), (FULL_CH, 17), (_abi.OBS_SIMPLE, 11)]
FALLBACK_IDS = ["no-pellet-g11", "full-g17", "simple"]
FALLBACK_SHAPES = [SHAPES[4], SHAPES[0]]  # 5 x 67 and 1 x 257


def shape_config(shape, channels=FULL_CH, extras=FULL_EX, G=11):
    A, B, field, mv = shape
    return make_config(n_arenas=A, bots=B, field_size=field, virus=True, max_viruses=mv, channels=channels,
                       extras=extras, grid_squares=G, flags=_abi.FLAG_EVENTS)


def mask_config(channels, extras, G=11):
    return shape_config((1, MASK_BOTS, MASK_FIELD, MASK_VIRUSES), channels, 0 if channels & _abi.OBS_SIMPLE
                        else extras, G)


def mature(x, A, seed, lo=12.0, hi=900.0):
    """Every cell of every arena of the stepper or oracle x gets a mass of
    exp(U(log lo, log hi)) from default_rng(seed) and the radius sqrt(m / pi): a
    world in which cells split, eject, eat each other and hit viruses from the
    first tick (fresh cells are below the split and eject thresholds)."""
    rng = np.random.default_rng(seed)
    for a in range(A):
        d = dict(x.get_state(a))
        cf = np.array(d["cells_f"], copy=True)
        m = np.exp(rng.uniform(math.log(lo), math.log(hi), len(cf)))
        cf[:, 2] = m
        cf[:, 3] = np.sqrt(m / math.pi)
        d["cells_f"] = cf
        x.load_state(d, a)


def start(x, A, seed, hi=900.0):
    x.reset(seed)
    mature(x, A, seed, hi=hi)
    return x


# One arena's extreme beside another's ordinary players.  The matured masses are alike in
# every arena, so per-arena values that a 64-lane wave or a 256-thread block reduces (the
# cell grids' radius bound, queue and scan totals) could leak across an arena boundary
# unseen.  At 3 x 100 the first players of arenas 1 and 2 (global 100 and 200, each in a
# wave and a block that start in the arena before) get a cell near the mass cap: it covers
# a virus at once and explodes to 16 cells (field.py:333-370), eats its neighbours, and
# keeps its arena's biggest radius over 50 while arena 0's stays near 25.  The grid walks
# of the tick and of the observation widen by that bound: with arena 1's or 2's bound
# handed to the arena of the wave's first lane (no per-lane fallback in
# wave_atomic_max_pos), a bot whose view only touches the rim of the heavy cell loses it
# from its enemy grid within a few ticks.
HEAVY_SHAPE, HEAVY_PLAYERS, HEAVY_MASS, HEAVY_TICKS = SHAPES[3], ((1, 0), (2, 0)), 20000.0, 12


def heavy_commands(rng):
    """The shape's synthetic commands; the heavy players neither split nor eject, so
    their cell stays the arena's radius bound."""
    cmd = synthetic(rng, HEAVY_SHAPE)
    for a, p in HEAVY_PLAYERS:
        cmd[a * HEAVY_SHAPE[1] + p, 2:] = 0
    return cmd


def heavy_start(x):
    A = HEAVY_SHAPE[0]
    start(x, A, SHAPE_SEED)
    for a, p in HEAVY_PLAYERS:
        d = dict(x.get_state(a))
        cf = np.array(d["cells_f"], copy=True)
        k = int(np.nonzero(np.asarray(d["cells_i"])[:, 0] == p)[0][0])
        cf[k, 2], cf[k, 3] = HEAVY_MASS, math.sqrt(HEAVY_MASS / math.pi)
        d["cells_f"] = cf
        x.load_state(d, a)
    return x


class HeavyMeals:
    """The cells the heavy players ate (EV_CELL_EAT_CELL rows whose eater is one of
    their cells), per heavy player, from the oracle's states and logs."""

    def __init__(self):
        self.seqs = [set() for _ in HEAVY_PLAYERS]
        self.meals = [0 for _ in HEAVY_PLAYERS]
        self.cells = [0 for _ in HEAVY_PLAYERS]
        self.rmax = [math.inf for _ in HEAVY_PLAYERS]
        self.rmax_light = 0.0  # the biggest radius of an arena without a heavy cell

    def before(self, o):
        for i, (a, p) in enumerate(HEAVY_PLAYERS):
            ci = np.asarray(o.get_state(a)["cells_i"])
            self.seqs[i] |= set(ci[ci[:, 0] == p, 2].tolist())

    def after(self, o, logs):
        self.before(o)
        for i, (a, p) in enumerate(HEAVY_PLAYERS):
            ev = np.asarray(logs[a])
            self.meals[i] += sum(1 for r in ev if r[1] == _abi.EV_CELL_EAT_CELL and int(r[2]) in self.seqs[i])
            self.cells[i] = max(self.cells[i], int(np.asarray(o.get_state(a)["players_i"])[p, 4]))
            self.rmax[i] = min(self.rmax[i], float(np.asarray(o.get_state(a)["cells_f"])[:, 3].max()))
        for a in set(range(HEAVY_SHAPE[0])) - {a for a, _ in HEAVY_PLAYERS}:
            self.rmax_light = max(self.rmax_light, float(np.asarray(o.get_state(a)["cells_f"])[:, 3].max()))

    def check(self):
        assert all(n >= 2 for n in self.meals), self.meals
        assert all(n == 16 for n in self.cells), self.cells
        # the grids are walked ceil((rmax + 1) / 20) + 1 buckets wide (HASH_BUCKET_SIZE 20): the
        # heavy arenas ask for a wider walk than the arena beside them, all the way
        assert all(r > 40 for r in self.rmax) and self.rmax_light < 39, (self.rmax, self.rmax_light)


def obs_bits_equal(x, y):
    """Rows equal bit for bit: NaN at the same positions, everywhere else the
    same bit pattern, so -0.0 != 0.0 here (parity.obs_close lets that through)."""
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    if x.shape != y.shape or x.dtype != y.dtype or x.dtype.kind != "f":
        return False
    nx, ny = np.isnan(x), np.isnan(y)
    if not np.array_equal(nx, ny):
        return False
    it = np.dtype("int%d" % (8 * x.dtype.itemsize))
    return bool(np.array_equal(x.view(it)[~nx], y.view(it)[~ny]))


def bits_diff(x, y):
    """Where obs_bits_equal fails (for the assertion message)."""
    if x.shape != y.shape or x.dtype != y.dtype:
        return "shape / dtype %s %s vs %s %s" % (x.shape, x.dtype, y.shape, y.dtype)
    nx, ny = np.isnan(x), np.isnan(y)
    it = np.dtype("int%d" % (8 * x.dtype.itemsize))
    bad = np.argwhere((nx != ny) | (~nx & ~ny & (np.ascontiguousarray(x).view(it) != np.ascontiguousarray(y).view(it))))
    if not len(bad):
        return "equal"
    i = tuple(bad[0])
    return "%d values differ, first at row %d col %d: %r vs %r" % (len(bad), i[0], i[1], x[i], y[i])


def commands(x, A):
    """Current (x, y, split, eject) of all A * B players."""
    out = []
    for a in range(A):
        st = x.get_state(a)
        pf, pi = np.asarray(st["players_f"]), np.asarray(st["players_i"])
        out.append(np.c_[pf[:, 0], pf[:, 1], pi[:, 2], pi[:, 3]].astype(np.float64))
    return np.concatenate(out)


def most_cells(x, A):
    """Per arena: the cell counts of its players."""
    return [np.asarray(x.get_state(a)["players_i"])[:, 4] for a in range(A)]


def kind_counts(logs):
    """Event rows (tick, code, a, b) of one arena -> {code: count}."""
    out = {}
    for ev in logs:
        for k, n in zip(*np.unique(np.asarray(ev)[:, 1], return_counts=True)):
            out[int(k)] = out.get(int(k), 0) + int(n)
    return out


class Worth:
    """What the oracle's event logs must show for a run to be worth comparing; the
    GPU tests assert it on the very logs they compare, test_oracle_shapes.py on the
    oracle alone."""

    def __init__(self, A):
        self.A = A
        self.logs = [[] for _ in range(A)]
        self.cells = 0
        self.ever = None  # per arena: the players that held several cells at some tick

    def tick(self, o, logs=None):
        for a in range(self.A):
            self.logs[a].append(o.events(a) if logs is None else logs[a])
        n = most_cells(o, self.A)
        self.cells = max(self.cells, max(int(c.max()) for c in n))
        self.ever = [c > 1 for c in n] if self.ever is None else [e | (c > 1) for e, c in zip(self.ever, n)]

    @property
    def multi(self):
        return max(int(e.sum()) for e in self.ever)

    def counts(self):
        return [kind_counts(l) for l in self.logs]

    def check_synthetic(self):
        cnt = self.counts()
        for a, c in enumerate(cnt):
            assert all(c.get(k, 0) > 0 for k in SYNTH_KINDS), "arena %d logged %s" % (a, c)
        assert any(c.get(_abi.EV_VIRUS_EAT_BLOB, 0) > 0 for c in cnt), cnt
        assert self.cells == 16, self.cells

    def check_greedy(self):
        for a, c in enumerate(self.counts()):
            assert all(c.get(k, 0) > 0 for k in GREEDY_KINDS), "arena %d logged %s" % (a, c)
        # in some arena, ten players held several cells at some tick (k_pp_active's shared cells);
        # an arena of 36 bots gets to 7 of them in 25 ticks and 9 in 40
        assert self.multi >= (10 if len(self.ever[0]) >= 67 else 5), self.multi


def synthetic_rng():
    return np.random.default_rng(SHAPE_SEED)


def synthetic(rng, shape):
    A, B, field, _ = shape
    return parity.synthetic_commands(rng, None, A * B, field, P_SPLIT, P_EJECT)


def mask_slices(channels, G):
    """{channel bit: slice of the row} in the reference's stacking order."""
    out, k = {}, 0
    for b in GRID_BITS:
        if channels & b:
            out[b] = slice(k * G * G, (k + 1) * G * G)
            k += 1
    return out


class Seen:
    """Which grid channels of a mask world's rows were ever non-zero.  A world is
    worth comparing when every channel the reference can fill was filled for
    some bot; the second-last-frame grid of a pair whose last-frame grid is not
    configured is never fed (bot.py:480-495) and must stay zero."""

    def __init__(self, channels, G):
        self.ch, self.sl = channels, mask_slices(channels, G)
        self.hit = {b: False for b in self.sl}
        self.all_differs = False
        self.wall_zeros = [False, False]  # a +0.0 and a -0.0 seen in the wall channel

    def rows(self, want):
        live = want[~np.isnan(want).any(axis=1)]
        for b, s in self.sl.items():
            self.hit[b] |= bool((live[:, s] != 0).any())
        if self.ch & _abi.OBS_WALL:  # round(1 - free / gs ** 2, 3) gives zeros of both signs
            z = live[:, self.sl[_abi.OBS_WALL]]
            z = np.signbit(z[z == 0])
            self.wall_zeros[0] |= bool((~z).any())
            self.wall_zeros[1] |= bool(z.any())
        if self.ch & _abi.OBS_ALL and self.ch & _abi.OBS_ENEMY:
            self.all_differs |= bool((live[:, self.sl[_abi.OBS_ALL]] != live[:, self.sl[_abi.OBS_ENEMY]]).any())

    def check(self):
        unfed = {_abi.OBS_SELF_SLF: _abi.OBS_SELF_LF, _abi.OBS_ENEMY_SLF: _abi.OBS_ENEMY_LF}
        for b, hit in self.hit.items():
            fed = b not in unfed or bool(self.ch & unfed[b])
            assert hit == fed, "channel 0x%x of mask 0x%x: non-zero %s, fed %s" % (b, self.ch, hit, fed)
        if self.ch & _abi.OBS_ALL and self.ch & _abi.OBS_ENEMY:
            assert self.all_differs
        if self.ch & _abi.OBS_WALL:
            assert all(self.wall_zeros), self.wall_zeros


def mask_commands(rng):
    return parity.synthetic_commands(rng, None, MASK_BOTS, MASK_FIELD, P_SPLIT, P_EJECT)
