"""The worlds of test_gpu_multicell.py are worth comparing (oracle only, no GPU).

From the oracle's state before each tick: per player, the pellets whose bucket
footprint (20-unit buckets, spatialHashTable.py:70-83) meets the footprint of
its cells, summed over the cells (a pellet near two of them counts twice) --
what the eat prep's walk keeps for the player.  World A must
hold many multi-cell player-ticks that fit one 128-entry candidate list and some
that do not, and all three eat events (6 pellet, 7 blob, 8 cell); world B must
hold single cells with more than 128 such pellets (the per-cell overflow path)
next to players that fit."""
import numpy as np

from oracle_lib import Oracle
import multicell_worlds as mw

BUCKET = 20


def _rects(x, y, r, size):
    """aigar_sem.h footprint(): inclusive bucket rectangles, empty when x1 < x0 or y1 < y0."""
    cl, ct = np.maximum(0.0, x - r), np.maximum(0.0, y - r)
    kx, ky = np.floor(cl / BUCKET).astype(np.int64), np.floor(ct / BUCKET).astype(np.int64)
    lx = np.minimum(float(size), x + r + 1).astype(np.int64)
    ly = np.minimum(float(size), y + r + 1).astype(np.int64)
    x1 = np.where(lx > kx * BUCKET, (lx - 1) // BUCKET, kx - 1)
    y1 = np.where(ly > ky * BUCKET, (ly - 1) // BUCKET, ky - 1)
    return kx, x1, ky, y1


def _hits(c, p):
    """[cells, pellets] rectangle intersections (rect_hit)."""
    cx0, cx1, cy0, cy1 = (v[:, None] for v in c)
    px0, px1, py0, py1 = (v[None, :] for v in p)
    ok = (cx0 <= cx1) & (cy0 <= cy1) & (px0 <= px1) & (py0 <= py1)
    return ok & (cx0 <= px1) & (px0 <= cx1) & (cy0 <= py1) & (py0 <= cy1)


def _census(name, arena=0):
    w = mw.WORLDS[name]
    o = Oracle(mw.config(name))
    mw.start(name, o)
    fn = mw.command_fn(name)
    fit = over = biggest = 0
    kinds = {}
    for t in range(mw.TICKS):
        st = o.get_state(arena)
        cf, ci, pf = np.asarray(st["cells_f"]), np.asarray(st["cells_i"]), np.asarray(st["pellets_f"])
        hit = _hits(_rects(cf[:, 0], cf[:, 1], cf[:, 3], w["size"]), _rects(pf[:, 0], pf[:, 1], pf[:, 3], w["size"]))
        if hit.size:
            biggest = max(biggest, int(hit.sum(axis=1).max()))
        for p in range(w["bots"]):
            mine = ci[:, 0] == p
            if mine.sum() < 2:
                continue
            n = int(hit[mine].sum())  # (a pellet near two of the cells is kept once for each)
            if n <= 128:
                fit += 1
            else:
                over += 1
        o.set_commands(fn(t))
        o.step(1)
        for e in o.events(arena):
            kinds[int(e[1])] = kinds.get(int(e[1]), 0) + 1
    o.close()
    return fit, over, biggest, kinds


def test_world_a_has_multicell_players_that_fit_and_overflow():
    fit, over, biggest, kinds = _census("A")
    print("world A: fit %d, over %d, largest cell %d, events %s" % (fit, over, biggest, kinds))
    assert fit >= 500
    assert over >= 10
    assert all(kinds.get(k, 0) > 0 for k in (6, 7, 8)), kinds


def test_world_b_has_cells_past_the_candidate_list():
    fit, over, biggest, _ = _census("B")
    print("world B arena 0: fit %d, over %d, largest cell %d" % (fit, over, biggest))
    assert fit >= 30
    assert over >= 100
    assert biggest > 128
