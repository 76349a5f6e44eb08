"""The cases of pp_worlds.py sit where they claim (oracle only, no GPU).

test_gpu_pp.py compares the device's player-eats-player pass -- its parallel
groups and its serial wavefront -- with the oracle on these worlds.  That
comparison says something only if each world reaches the branch it was built
for, so here, on the oracle and with pp_worlds' restatement of the activity
predicate and of the closure: on the first tick every single-cell player holds
still and every cell is where at_pass() puts it; the pending players are as
many as the case names; every cluster's closure has exactly the players, cells
and rounds it names (16 against 17, 64 against 65, 12 against 13); clusters
meant to be apart have disjoint closures; whether the pass would take the
groups, worked out from those numbers and the pass's limits, is what the case
says; and the tick's events are the eats and deaths the case was built for.
These are conditions on the inputs, not measurements of the device."""
import functools

import numpy as np
import pytest

from aigar_amd import _abi
from oracle_lib import Oracle
import pp_worlds as pw

EAT, DEATH, RESPAWN = _abi.EV_CELL_EAT_CELL, _abi.EV_PLAYER_DEATH, _abi.EV_RESPAWN
PARTS = ("corner-q", "corner-pair", "corner-pair3")  # closures that merge into "corner-merged"


@functools.lru_cache(maxsize=None)
def walk(name):
    """per arena: the start state, and per tick (state after, events)"""
    c = pw.CASES[name]
    o = Oracle(pw.config(name))
    cmd = pw.start(name, o)
    out = [dict(start=o.get_state(a), ticks=[]) for a in range(c["arenas"])]
    for _ in range(pw.TICKS):
        o.set_commands(cmd)
        o.step(1)
        for a in range(c["arenas"]):
            out[a]["ticks"].append((o.get_state(a), o.events(a)))
    o.close()
    return out


def arenas():
    return [(n, a) for n in pw.CASES for a in range(pw.CASES[n]["arenas"])]


def seen(name, a):
    """the arena as the first tick's pass sees it"""
    return pw.at_pass(walk(name)[a]["start"], pw.CASES[name]["size"])


def components(name, a):
    """the pending players' closures, united where they share a player: [(seeds, players)]"""
    st, cfg = seen(name, a), pw.config(name)
    comps = []
    for p in pw.pending(st):
        players = set(pw.closure(st, cfg, [p])[0])
        seeds = [p]
        for c in [c for c in comps if c[1] & players]:
            comps.remove(c)
            seeds += c[0]
            players |= c[1]
        comps.append((sorted(seeds), players))
    return comps


@pytest.mark.parametrize("name,a", arenas())
def test_cells_are_where_the_pass_is_told_they_are(name, a):
    w = walk(name)[a]
    L = pw.layout(name, a)
    before, want = w["start"], seen(name, a)
    after = w["ticks"][0][0]
    pos = {int(s): (x, y) for (x, y), s in zip(np.asarray(after["cells_f"])[:, :2], np.asarray(after["cells_i"])[:, 2])}
    cf0, cfw, ci = np.asarray(before["cells_f"]), np.asarray(want["cells_f"]), np.asarray(before["cells_i"])
    n = 0
    for k in range(len(ci)):
        if int(ci[k, 2]) not in pos:
            continue  # (eaten on this tick)
        n += 1
        assert pos[int(ci[k, 2])] == (cfw[k, 0], cfw[k, 1]), "cell %d is not where at_pass puts it" % k
        if len(L.cells[int(ci[k, 0])]) == 1:
            assert pos[int(ci[k, 2])] == (cf0[k, 0], cf0[k, 1]), "single cell %d moved" % k
    assert n == len(ci) - L.eats


@pytest.mark.parametrize("name,a", arenas())
def test_pending_players_and_closures_are_what_the_case_names(name, a):
    c, L = pw.CASES[name], pw.layout(name, a)
    st, size, cfg = seen(name, a), c["size"], pw.config(name)
    pend = pw.pending(st)
    assert len(pend) == L.pending
    merged_ok = True
    for cl in L.clusters:
        start = cl["seeds"]
        if cl["name"] == "corner-merged":  # (as the pass: from the union of the seeds' closures)
            start = sorted(set().union(*[pw.closure(st, cfg, [s])[0] for s in cl["seeds"]]))
            assert len(start) < cl["players"] or name != "merge_grow", "the merged closure has to grow"
            if len(start) > pw.PPG_PL:
                merged_ok = False
                assert name == "merge_over" and len(start) == cl["players"]
                continue
        players, cells, rounds = pw.closure(st, cfg, start)
        assert set(cl["seeds"]) <= set(pend), cl
        assert (len(players), cells) == (cl["players"], cl["cells"]), (cl, players, cells)
        assert (rounds <= pw.CLOSURE_ROUNDS) == cl["settles"], (cl, rounds)
        if cl["name"] == "line":
            assert rounds == pw.CLOSURE_ROUNDS + (0 if cl["settles"] else 1)
        if cl["name"] == "corner-merged" and len(players) > pw.PPG_PL:
            merged_ok = False
    # clusters meant to be apart are apart: one component per cluster (the corner's parts are one)
    comps = components(name, a)
    assert len(comps) == sum(1 for cl in L.clusters if cl["name"] not in PARTS)
    for i, (_, x) in enumerate(comps):
        for _, y in comps[i + 1:]:
            assert not x & y
    # the path, from the pass's limits
    cols = -(-size // pw.BUCKET)
    deferred = (cols * cols + 63) // 64 <= pw.OCC_DIRTY_WORDS
    # (conflict: two roots, each closed from its component's players, that share a player)
    roots = [set(pw.closure(st, cfg, sorted(players))[0]) for _, players in comps]
    conflict = any(x & y for i, x in enumerate(roots) for y in roots[i + 1:])
    assert conflict == (name == "merge_conflict")
    groups = deferred and pw.PPG_MIN <= len(pend) <= pw.PPG_SEEDS and merged_ok and not conflict
    if groups:
        for p in pend:
            players, cells, rounds = pw.closure(st, cfg, [p])
            groups = groups and len(players) <= pw.PPG_PL and cells <= pw.PPG_CELLS and rounds <= pw.CLOSURE_ROUNDS
    assert groups == c["groups"][a], "%s: %s" % (name, c["why"])


def test_the_limits_each_have_a_case_on_either_side():
    n = {name: pw.layout(name).pending for name in pw.CASES}
    assert (n["min2"], n["min3"]) == (pw.PPG_MIN - 1, pw.PPG_MIN)
    assert (n["seeds64"], n["seeds65"]) == (pw.PPG_SEEDS, pw.PPG_SEEDS + 1)
    assert n["waves17"] == pw.PPG_WAVES + 1
    assert pw.CASES["big_arena"]["bots"] > pw.PP_LOWN_MAX and pw.CASES["big_arena"]["groups"] == [True]
    cols = -(-pw.CASES["big_field"]["size"] // pw.BUCKET)
    assert (cols * cols + 63) // 64 > pw.OCC_DIRTY_WORDS
    assert pw.CASES["batched"]["groups"] == [True, False, False] and pw.layout("batched", 2).pending == 0
    # the corner cluster of "cap": the group's mass is past the cap, its footprints clamp at 0
    st = seen("cap", 0)
    players, _, _ = pw.closure(st, pw.config("cap"), [0])
    cf, own = np.asarray(st["cells_f"]), np.asarray(st["cells_i"])[:, 0]
    assert cf[np.isin(own, players), 2].sum() > pw.MAX_MASS
    assert min(cf[np.isin(own, players), 0].min(), cf[np.isin(own, players), 1].min()) < pw.radius_of(pw.MAX_MASS)


@pytest.mark.parametrize("name,a", arenas())
def test_the_first_tick_has_the_eats_and_deaths_and_everybody_respawns(name, a):
    w, L = walk(name)[a], pw.layout(name, a)
    ev = w["ticks"][0][1]
    assert int(np.sum(ev[:, 1] == EAT)) == L.eats
    assert int(np.sum(ev[:, 1] == DEATH)) == L.deaths
    assert set(ev[:, 1].tolist()) <= {EAT, DEATH}
    died = set(ev[ev[:, 1] == DEATH, 2].tolist())
    back = set()
    for _, e in w["ticks"][:pw.TICKS - 1]:  # (a tick is left to observe the respawned cells)
        back |= set(e[e[:, 1] == RESPAWN, 2].tolist())
    assert died <= back
    # the first tick's eats by owner, in order, hold the sequences the case was built for
    ci = np.asarray(w["start"]["cells_i"])
    owner = {int(s): int(p) for p, s in zip(ci[:, 0], ci[:, 2])}
    eats = [(owner[int(e[2])], owner[int(e[3])]) for e in ev if e[1] == EAT]
    for seq in L.order:
        it = iter(eats)
        assert all(x in it for x in seq), (seq, eats)


def test_chain_wakes_a_later_player_and_skips_the_cell_moved_into_the_row():
    w, L = walk("chain")[0], pw.layout("chain")
    r = L.roles
    ci, cf = np.asarray(w["start"]["cells_i"]), np.asarray(w["start"]["cells_f"])
    seq = {p: ci[ci[:, 0] == p, 2] for p in r.values()}
    assert seq[r["c"]][0] < seq[r["b"]][0], "A has to meet C (inert) before B"
    assert pw.pending(seen("chain", 0))[:2] == [r["a"], r["m"]], "C, E, W and X are woken, not pending"
    after = w["ticks"][0][0]
    alive = {int(s): m for s, m in zip(np.asarray(after["cells_i"])[:, 2], np.asarray(after["cells_f"])[:, 2])}
    skipped = int(seq[r["m"]][1])
    assert alive[skipped] > cf[ci[:, 2] == skipped, 2][0], "the skipped cell is alive and has eaten W"
    assert int(seq[r["m"]][0]) not in alive


@pytest.mark.parametrize("name,a", [("seeds64", 0), ("batched", 0)])
def test_deaths_come_from_many_groups_and_the_first_in_turn_order_is_the_longest(name, a):
    """the group of the lowest pending player has the most deaths (its wave finishes last), so
    the order the deaths are made in is not the order of the players' turns"""
    w = walk(name)[a]
    ev = w["ticks"][0][1]
    dead = ev[ev[:, 1] == DEATH, 2].tolist()
    per = sorted((min(s), sum(1 for p in dead if p in players)) for s, players in components(name, a))
    assert len([n for _, n in per if n]) > pw.PPG_WAVES
    assert per[0][1] > max(n for _, n in per[1:]) * 4
