"""Built worlds for the player-eats-player pass (test_pp_worlds.py checks on the
oracle that each case sits where it claims; test_gpu_pp.py steps them on the
device, the oracle and a device forced to the serial pass).

tick.hip's pp_pass runs playerPlayerOverlap either in one wavefront or as up to
PPG_SEEDS independent groups over PPG_WAVES wavefronts; the cases stand on both
sides of every limit of that choice (PPG_MIN 3, PPG_SEEDS 64, PPG_PL 16,
PPG_CELLS 64, PPG_WAVES 16, 12 closure rounds, PP_LOWN_MAX 8192, the dirty-word
bitmap's 2048 occupancy words) and reach the branches inside a group: merged
closures, the table's re-activation walk, the row shift when a turn's own cell
is eaten, deaths from many waves in one tick.

A case is a config and a start state.  Viruses are off and there are no
pellets, so only the pass moves mass.  Every single-cell player is commanded to
its own cell's position and holds still (set_move_direction: hyp = 0); multi-cell
players are made by splitting on the oracle first, then all cells are placed.
Clusters sit on sites 260 units (13 buckets) apart, origins on bucket corners,
so bucket footprints are what the coordinates below say they are.

pending() and closure() restate k_pp_active's predicate and pp_closure's fixed
point in plain Python.  They prove where a case sits; they are no second oracle."""
import math

import numpy as np

from aigar_amd import _abi
from oracle_lib import make_config

CH = (_abi.OBS_PELLET | _abi.OBS_SELF | _abi.OBS_WALL | _abi.OBS_ENEMY | _abi.OBS_SELF_LF | _abi.OBS_ENEMY_LF)
SEED = 31
BUCKET = 20
MAX_MASS = 22500.0
DECAY = 1 - (0.01 * (1.0 / 30))  # CELL_MASS_DECAY_RATE
MOVE_SPEED = 90 * (1.0 / 30)     # CELL_MOVE_SPEED
RESPAWN_DELAY = 1                # stepsUntilRespawn (player.py:110-112)
# a death on tick t: respawn at the end of tick t + RESPAWN_DELAY, observed moving on the tick after
TICKS = RESPAWN_DELAY + 3

# the pass's limits (tick.hip), named here so a test reads as the kernel does
PPG_MIN, PPG_SEEDS, PPG_PL, PPG_CELLS, PPG_WAVES, CLOSURE_ROUNDS = 3, 64, 16, 64, 16, 12
PP_LOWN_MAX, OCC_DIRTY_WORDS = 8192, 2048

PITCH = 260
SITE_X0, SITE_Y0 = 400, 140      # (x < 400 stays free: the corner cluster of "cap")
BIG = 520                        # clusters wider than a site take a square of this side
PARK_MASS = 10.0


def radius_of(m):
    return math.sqrt(m / math.pi) if m > 0 else 0.0


# ---------------------------------------------------------------- the predicates, restated
def footprint(x, y, rad, size):
    """getIdsForArea as a bucket rectangle (x0, x1, y0, y1), inclusive (aigar_sem.h footprint)"""
    cl, ct = max(0.0, x - rad), max(0.0, y - rad)
    kx, ky = int(cl // BUCKET), int(ct // BUCKET)
    lx, ly = int(min(float(size), x + rad + 1)), int(min(float(size), y + rad + 1))
    x1 = (lx - 1) // BUCKET if lx > kx * BUCKET else kx - 1
    y1 = (ly - 1) // BUCKET if ly > ky * BUCKET else ky - 1
    return kx, x1, ky, y1


def rect_hit(a, b):
    return (a[0] <= a[1] and a[2] <= a[3] and b[0] <= b[1] and b[2] <= b[3]
            and a[0] <= b[1] and b[0] <= a[1] and a[2] <= b[3] and b[2] <= a[3])


def at_pass(state, size):
    """The cells as the pass sees them on the next tick: decayed (cell.py:123-126) and moved
    towards their player's command point (cell.py:47-57, 132-141).  No split momentum, no
    pushes between a player's cells: the start states have neither."""
    cf, ci = np.asarray(state["cells_f"]).copy(), np.asarray(state["cells_i"])
    pf = np.asarray(state["players_f"])
    for k in range(len(cf)):
        x, y, m = cf[k, 0], cf[k, 1], cf[k, 2]
        if m >= 4:
            m = m * DECAY
        r = math.sqrt(m / math.pi)
        xd, yd = pf[ci[k, 0], 0] - x, pf[ci[k, 0], 1] - y
        hyp, r2 = xd * xd + yd * yd, r * r
        mod = min(hyp, r2) / r2
        ang = math.atan2(yd, xd)
        sp = MOVE_SPEED * math.pow(m, -0.35)
        vx, vy = sp * mod * math.cos(ang), sp * mod * math.sin(ang)
        cf[k, 0] = min(float(size), max(0.0, x + (vx + cf[k, 6])))
        cf[k, 1] = min(float(size), max(0.0, y + (vy + cf[k, 7])))
        cf[k, 2], cf[k, 3], cf[k, 4], cf[k, 5] = m, r, vx, vy
    out = dict(state)
    out["cells_f"] = cf
    return out


def pending(state):
    """k_pp_active's predicate: the players with a cell that overlaps a live cell of a
    higher-index player while one of the two can eat the other (only the lower index of a
    pair is marked).  Sorted."""
    cf, own = np.asarray(state["cells_f"]), np.asarray(state["cells_i"])[:, 0]
    x, y, m, r = cf[:, 0], cf[:, 1], cf[:, 2], cf[:, 3]
    out = set()
    for k in range(len(cf)):
        hi = own > own[k]
        if not hi.any():
            continue
        big = m[k] > m  # overlap (cell.py:143-152): the strictly heavier cell's radius, else the other's
        rb = np.where(big, r[k], r)
        d2 = (x - x[k]) * (x - x[k]) + (y - y[k]) * (y - y[k])
        hit = hi & (d2 * 1.1 < rb * rb) & ((m[k] > 1.25 * m) | (m > 1.25 * m[k]))
        if hit.any():
            out.add(int(own[k]))
    return sorted(out)


def closure(state, cfg, players):
    """pp_closure's fixed point from the starting players: (players, cells, rounds).  A round
    takes the group's mass M and R = max(radius_of(min(22500, M)), largest radius) * (1 + 1e-9)
    + 1e-9, the bounding rectangle U of the members' footprints at R, and adds every player with
    a cell whose footprint at max(r, R) meets U; the round that adds nobody is counted too.  The
    kernel gives up above 16 players, above 64 cells and after 12 rounds; this goes on."""
    cf, own, size = np.asarray(state["cells_f"]), np.asarray(state["cells_i"])[:, 0], cfg.field_size
    members, rounds = list(players), 0
    while True:
        rounds += 1
        ins = np.isin(own, members)
        M, rr = float(np.sum(cf[ins, 2])), float(np.max(cf[ins, 3]))
        R = max(radius_of(min(MAX_MASS, M)), rr) * (1 + 1e-9) + 1e-9
        fps = [footprint(c[0], c[1], R, size) for c in cf[ins]]
        U = (min(f[0] for f in fps), max(f[1] for f in fps), min(f[2] for f in fps), max(f[3] for f in fps))
        lo, hi = (U[0] - 1) * BUCKET - 2 * R - 2, (U[1] + 2) * BUCKET + 2 * R + 2  # (only near cells can meet U)
        lo_y, hi_y = (U[2] - 1) * BUCKET - 2 * R - 2, (U[3] + 2) * BUCKET + 2 * R + 2
        near = ~ins & (cf[:, 0] + cf[:, 3] >= lo) & (cf[:, 0] - cf[:, 3] <= hi) & (cf[:, 1] + cf[:, 3] >= lo_y) \
            & (cf[:, 1] - cf[:, 3] <= hi_y)
        new = []
        for k in np.nonzero(near)[0]:
            if rect_hit(footprint(cf[k, 0], cf[k, 1], max(cf[k, 3], R), size), U) and int(own[k]) not in new:
                new.append(int(own[k]))
        if not new:
            return sorted(members), int(np.sum(ins)), rounds
        members += new


# ---------------------------------------------------------------- layouts
class Layout:
    """One arena's players in index order: each a list of (x, y, mass) cells, and the clusters
    the checks ask about."""

    def __init__(self, bots, size):
        self.bots, self.size = bots, size
        self.cells = []      # [player] -> [(x, y, m), ...]
        self.clusters = []   # dict(name, seeds, players, cells, settles) -- closure claims
        self._site = 0
        self._big = 0
        self.pending = 0     # pending players at the first tick's pass
        self.eats = 0        # EV_CELL_EAT_CELL events of the first tick
        self.deaths = 0      # deaths of the first tick
        self.order = []      # claims on the first tick's events, checked on the oracle

    def player(self, *cells):
        self.cells.append(list(cells))
        return len(self.cells) - 1

    def site(self):
        g = (self.size - SITE_X0 - PITCH // 2) // PITCH
        k, self._site = self._site, self._site + 1
        x, y = SITE_X0 + PITCH * (k % g), SITE_Y0 + PITCH * (k // g)
        assert y + PITCH <= self.big_y0(), "the sites run into the wide clusters' rows"
        return x, y

    def big_y0(self):
        return self.size - 2 * BIG - 20

    def big(self):
        k, self._big = self._big, self._big + 1
        g = (self.size - SITE_X0) // BIG
        return SITE_X0 + BIG * (k % g), self.big_y0() + BIG * (k // g)

    def claim(self, name, seeds, players, cells, settles=True):
        self.clusters.append(dict(name=name, seeds=list(seeds), players=players, cells=cells, settles=settles))

    def pair(self, victim_first=False, at=None):
        """an eater (100) over a victim (40), both single cells; returns (eater, victim)"""
        x, y = at or self.site()
        if victim_first:
            v = self.player((x + 12, y + 10, 40.0))
            e = self.player((x + 10, y + 10, 100.0))
        else:
            e = self.player((x + 10, y + 10, 100.0))
            v = self.player((x + 12, y + 10, 40.0))
        self.pending += 1
        self.eats += 1
        self.deaths += 1
        self.claim("pair", [min(e, v)], 2, 2)
        return e, v

    def pairs(self, n):
        for k in range(n):
            self.pair(victim_first=bool(k & 1))

    def park(self):
        """the remaining players: inert single cells, one to a site"""
        while len(self.cells) < self.bots:
            x, y = self.site()
            self.player((x + 10, y + 10, PARK_MASS))


def _ring(cx, cy, rad, n, m):
    return [(cx + rad * math.cos(2 * math.pi * k / n), cy + rad * math.sin(2 * math.pi * k / n), m) for k in range(n)]


def _feast(L, victims):
    """one heavy eater of low index with `victims` single-cell victims around it: one long
    turn, `victims` deaths with the eater's keys"""
    x, y = L.site()
    e = L.player((x + 50, y + 50, 2000.0))
    vs = [L.player(c) for c in _ring(x + 50, y + 50, 15.0, victims, 40.0)]
    L.pending += 1
    L.eats += victims
    L.deaths += victims
    L.claim("feast", [e], 1 + victims, 1 + victims)
    return e, vs


def _crowd(L, bystanders):
    """a pair with inert bystanders (equal masses) around it, all in one closure"""
    x, y = L.site()
    e, v = L.pair(at=(x + 20, y + 20))
    L.clusters.pop()
    for c in _ring(x + 30, y + 30, 9.0, bystanders, PARK_MASS):
        L.player(c)
    L.claim("crowd", [e], 2 + bystanders, 2 + bystanders)


def _blocks(L, extra):
    """four 16-cell players (4 x 4 cells of mass 50, 12 apart) in one closure: 64 cells; one cell
    of the first is heavy and lies over a cell of the second.  extra: one more single cell."""
    x, y = L.big()
    ps = []
    for b, (bx, by) in enumerate(((20, 20), (80, 20), (20, 80), (80, 80))):
        cells = [(x + bx + 12 * (k % 4), y + by + 12 * (k // 4), 50.0) for k in range(16)]
        if b == 0:
            cells[15] = (cells[15][0], cells[15][1], 100.0)
        if b == 1:
            cells[0] = (x + 59, y + 56, 50.0)
        ps.append(L.player(*cells))
    n = 64
    if extra:
        ps.append(L.player((x + 68, y + 100, 50.0)))
        n += 1
    L.pending += 1
    L.eats += 1
    L.claim("blocks", [ps[0]], len(ps), n)
    return ps


def _corner(L, x, y, third=None, crowd_in=0, crowd_by=0, far=0, far_pair=False):
    """Two closures that share one player and do not hold each other.  A two-cell player Q with
    its cells on a square's diagonal (its closure's rectangle U spans the square), a light
    bystander S inside the square's corner, and a heavy pair just outside that corner: S is in
    Q's closure because it lies in U, and in the pair's because the pair's R reaches it.
    third: a second heavy pair and bystander at the opposite corner (three seeds).
    crowd_in / crowd_by: inert bystanders inside the square / beside the heavy pair.
    far: bystanders that only the merged group's larger R reaches.
    far_pair: a pair there instead -- a group of its own, which the merged root's closure takes in."""
    v1 = L.player((x + 12, y + 10, 40.0))
    q = L.player((x + 10, y + 10, 100.0), (x + 210, y + 210, 100.0))
    s = L.player((x + 205, y + 15, PARK_MASS))
    e2 = L.player((x + 240, y + 15, 600.0))
    v2 = L.player((x + 242, y + 15, 200.0))
    L.pending += 2
    L.eats += 2
    L.deaths += 2
    own1, own2 = [v1, q, s], [e2, v2, s]
    for k in range(crowd_in):
        own1.append(L.player((x + 90 + 8 * (k % 5), y + 100 + 8 * (k // 5), PARK_MASS)))
    for k in range(crowd_by):
        own2.append(L.player((x + 262 + 6 * (k % 3), y + 6 + 6 * (k // 3), PARK_MASS)))
    fars = [L.player((x + 290, y + 4 + 2.5 * k, PARK_MASS)) for k in range(far)]
    if far_pair:
        fars += L.pair(at=(x + 280, y + 5))
    seeds, union = [v1, e2], set(own1) | set(own2)
    if third:
        s3 = L.player((x + 15, y + 205, PARK_MASS))
        e3 = L.player((x + 15, y + 240, 600.0))
        v3 = L.player((x + 15, y + 242, 200.0))
        L.pending += 1
        L.eats += 1
        L.deaths += 1
        own1.append(s3)
        L.claim("corner-pair3", [e3], 3, 3)
        seeds.append(e3)
        union |= {s3, e3, v3}
    L.claim("corner-q", [v1], len(own1), len(own1) + 1)
    L.claim("corner-pair", [e2], len(own2), len(own2))
    L.claim("corner-merged", seeds, len(union) + len(fars), len(union) + len(fars) + 1)
    return dict(seeds=seeds, union=sorted(union), q=q, s=s, fars=fars)


def _line(L, joiners):
    """a pair and a line of light cells a bucket apart: each joins the closure only after the
    one before it has widened U -- one round each, and one more that adds nobody"""
    x, y = L.big()
    e = L.player((x + 16, y + 10, 100.0))
    v = L.player((x + 18, y + 10, 40.0))
    for j in range(1, joiners + 1):
        L.player((x + 16 + 20 * j, y + 10, PARK_MASS))
    L.pending += 1
    L.eats += 1
    L.deaths += 1
    L.claim("line", [e], 2 + joiners, 2 + joiners, settles=joiners + 1 <= CLOSURE_ROUNDS)
    return joiners + 1


def _chain(L):
    """three clusters, each one pending player at the start:
    (a) A 100 over C 90 and B 40, C made before B: A and C are inert, A eats B, grows past
        1.25 C, and the walk after the growth wakes C, whose own turn feeds it to A;
    (b) M with four cells, X < M < E < W, V: E 100 lies over M's first cell (40), so M's first
        cell is eaten in M's own turn, the list closes up and M's second cell -- over W, which
        it could eat -- is skipped (W is woken: its own turn feeds it to that cell); the turn
        goes on to M's third cell, which eats V; E's growth wakes E (a higher index than M),
        whose turn eats X 90, inert against E before;
    (c) a plain pair."""
    x, y = L.site()
    a = L.player((x + 30, y + 30, 100.0))
    c = L.player((x + 27, y + 30, 90.0))
    b = L.player((x + 33, y + 30, 40.0))
    L.claim("chain-a", [a], 3, 3)
    x, y = L.site()
    xx = L.player((x + 13, y + 30, 90.0))
    m = L.player((x + 20, y + 30, 40.0), (x + 60, y + 30, 60.0), (x + 100, y + 30, 60.0), (x + 140, y + 30, 60.0))
    e = L.player((x + 17, y + 30, 100.0))
    w = L.player((x + 62, y + 30, 30.0))
    v = L.player((x + 102, y + 30, 30.0))
    L.claim("chain-b", [m], 5, 8)
    L.pending += 2
    L.eats += 2 + 4
    L.deaths += 2 + 3
    L.pair()
    # (eater's owner, victim's owner) of the first tick's eats, in order, per cluster
    L.order = [[(a, b), (a, c)], [(e, m), (m, v), (e, xx), (m, w)]]
    return dict(a=a, b=b, c=c, x=xx, m=m, e=e, w=w, v=v)


# ---------------------------------------------------------------- the cases
# name -> dict(arenas, bots, size, build(L, arena), groups: [per arena] does the first tick run the groups)
def _case(bots, size, build, groups, arenas=1, why=""):
    return dict(arenas=arenas, bots=bots, size=size, build=build, groups=groups, why=why)


def _b_pairs(n):
    return lambda L, a: L.pairs(n)


def _b_seeds(n):
    def build(L, a):
        _feast(L, 8)
        L.pairs(n - 1)
    return build


def _b_with_pairs(fn, *args, **kw):
    def build(L, a):
        out = fn(L, *args, **kw)
        L.pairs(3)
        return out
    return build


def _b_cap(L, a):
    """two 12000 cells and a victim in the field's corner: the group's mass passes 22500, R is
    the capped radius, and the footprints clamp at 0"""
    pa = L.player((40.0, 40.0, 12000.0))
    L.player((90.0, 40.0, 12000.0))
    L.player((10.0, 40.0, 100.0))
    L.pending += 1
    L.eats += 1
    L.deaths += 1
    L.claim("cap", [pa], 3, 3)
    L.pairs(3)


def _b_corner(**kw):
    def build(L, a):
        out = _corner(L, *L.big(), **kw)
        L.pairs(2)
        return out
    return build


def _b_big_arena(L, a):
    out = _corner(L, 20, 20, third=True)
    for k in range(3):
        L.pair(victim_first=bool(k & 1), at=(600 + PITCH * k, 140))
    k = 0
    while len(L.cells) < L.bots:  # everybody else: inert single cells three buckets apart, below the clusters
        L.player((30.0 + 60 * (k % 99), 530.0 + 60 * (k // 99), PARK_MASS))
        k += 1
    return out


def _b_batched(L, a):
    if a == 0:
        _feast(L, 5)
        L.pairs(31)
    elif a == 1:
        L.pairs(2)


CASES = {
    "min2": _case(24, 3000, _b_pairs(2), [False], why="below PPG_MIN"),
    "min3": _case(24, 3000, _b_pairs(3), [True], why="at PPG_MIN"),
    "seeds64": _case(140, 4400, _b_seeds(64), [True], why="PPG_SEEDS seeds: four groups a wave, 71 deaths"),
    "seeds65": _case(140, 4400, _b_seeds(65), [False], why="above PPG_SEEDS"),
    "waves17": _case(40, 3000, _b_pairs(17), [True], why="one wave runs two groups"),
    "pl16": _case(30, 3000, _b_with_pairs(_crowd, 14), [True], why="a closure of PPG_PL players"),
    "pl17": _case(30, 3000, _b_with_pairs(_crowd, 15), [False], why="a closure above PPG_PL"),
    "cells64": _case(16, 3000, _b_with_pairs(_blocks, False), [True], why="a closure of PPG_CELLS cells"),
    "cells65": _case(16, 3000, _b_with_pairs(_blocks, True), [False], why="a closure above PPG_CELLS"),
    "merge": _case(20, 3000, _b_corner(third=True), [True], why="three seeds, one merged group"),
    "merge_over": _case(40, 3000, _b_corner(crowd_in=9, crowd_by=9), [False], why="the union is above PPG_PL"),
    "merge_grow": _case(30, 3000, _b_corner(far=12), [False], why="the merged root's closure is above PPG_PL"),
    "merge_conflict": _case(30, 3000, _b_corner(far_pair=True), [False],
                            why="the merged root's closure holds a player of another root"),
    "rounds12": _case(30, 3000, _b_with_pairs(_line, 11), [True], why="the closure settles in its 12th round"),
    "rounds13": _case(30, 3000, _b_with_pairs(_line, 12), [False], why="the closure needs a 13th round"),
    "chain": _case(16, 3000, lambda L, a: _chain(L), [True], why="re-activation and the row shift in a group"),
    "cap": _case(12, 3000, _b_cap, [True], why="R at the mass cap, footprints clamped"),
    "big_arena": _case(8200, 6000, _b_big_arena, [True], why="owners in global memory"),
    "big_field": _case(16, 7400, _b_pairs(4), [False], why="no dirty-word bitmap: serial, immediate occupancy"),
    "batched": _case(70, 4400, _b_batched, [True, False, False], arenas=3, why="three pending sets side by side"),
}


def config(name):
    c = CASES[name]
    return make_config(n_arenas=c["arenas"], bots=c["bots"], field_size=c["size"], virus=False, max_pellets=0.0,
                       channels=CH, extras=0x1F)


_layouts = {}


def layout(name, arena=0):
    if (name, arena) not in _layouts:
        c = CASES[name]
        L = Layout(c["bots"], c["size"])
        L.roles = c["build"](L, arena)
        L.park()
        assert len(L.cells) == c["bots"], "%s: %d players for %d bots" % (name, len(L.cells), c["bots"])
        _layouts[name, arena] = L
    return _layouts[name, arena]


def _prep_xy(p, multi, size):
    """where a player waits while the multi-cell players split: those in a row of their own,
    600 apart, everybody else three buckets apart below them"""
    if p in multi:
        return 300.0 + 600 * multi.index(p), 300.0
    per = (size - 60) // 60
    return 30.0 + 60 * (p % per), 930.0 + 60 * (p // per)


def _splits(n):
    return max(0, int(math.ceil(math.log2(n))))


def _arena_state(src, name, a):
    """arena a's state after reset, its multi-cell players set apart to split (on the stepper src)"""
    c = CASES[name]
    L = layout(name, a)
    B, size = c["bots"], c["size"]
    multi = [p for p in range(B) if len(L.cells[p]) > 1]
    d = dict(src.get_state(a))
    cf, ci = np.asarray(d["cells_f"]).copy(), np.asarray(d["cells_i"]).copy()
    assert len(cf) == B and np.array_equal(ci[:, 0], np.arange(B))
    if multi:  # split first: 80 * 2^s of mass gives 2^s cells of 80
        pf = np.asarray(d["players_f"]).copy()
        for p in range(B):
            x, y = _prep_xy(p, multi, size)
            m = 80.0 * 2 ** _splits(len(L.cells[p])) if p in multi else PARK_MASS
            cf[p, :4] = x, y, m, radius_of(m)
            pf[p] = x, y
        d["cells_f"], d["players_f"] = cf, pf
        src.load_state(d, a)
    return d, multi


def start(name, *steppers):
    """reset(SEED), then the case's start state loaded into every stepper (made on the last
    one, the oracle in every test).  Returns the commands every tick of the case uses."""
    c = CASES[name]
    A, B, size = c["arenas"], c["bots"], c["size"]
    src = steppers[-1]
    for s in steppers:
        s.reset(SEED)
    cmd = np.zeros((A * B, 4))
    multis = []
    for a in range(A):
        d, multi = _arena_state(src, name, a)
        multis.append(multi)
        for p in range(B):
            cmd[a * B + p, :2] = _prep_xy(p, multi, size)
    rounds = max([_splits(len(layout(name, a).cells[p])) for a in range(A) for p in multis[a]] + [0])
    for t in range(rounds):  # a player that needs s splits splits on the last s of these ticks
        step = cmd.copy()
        for a in range(A):
            for p in multis[a]:
                if rounds - t <= _splits(len(layout(name, a).cells[p])):
                    step[a * B + p] = (cmd[a * B + p, 0] + 50, cmd[a * B + p, 1], 1, 0)
        src.set_commands(step)
        src.step(1)
    for a in range(A):
        L = layout(name, a)
        d = dict(src.get_state(a))
        cf, ci = np.asarray(d["cells_f"]).copy(), np.asarray(d["cells_i"]).copy()
        pf, pi = np.asarray(d["players_f"]).copy(), np.asarray(d["players_i"]).copy()
        assert int(d["n_dead"]) == 0
        for p in range(B):
            rows = np.nonzero(ci[:, 0] == p)[0]
            want = L.cells[p]
            assert len(rows) == len(want), "%s: player %d split into %d cells, not %d" % (name, p, len(rows), len(want))
            for k, (x, y, m) in zip(rows, want):
                cf[k] = (x, y, m, radius_of(m), 0, 0, 0, 0, 900.0 if len(want) > 1 else 0.0)
                ci[k, 1] = -1
            tot = sum(m for _, _, m in want)
            pf[p] = (sum(x * m for x, _, m in want) / tot, sum(y * m for _, y, m in want) / tot) \
                if len(want) > 1 else want[0][:2]
            pi[p, 2] = pi[p, 3] = 0
        cmd[a * B:(a + 1) * B, :2] = pf
        d["cells_f"], d["cells_i"], d["players_f"], d["players_i"] = cf, ci, pf, pi
        for s in steppers:
            s.load_state(d, a)
    cmd[:, 2:] = 0
    return cmd
