"""The worlds of test_gpu_closing.py are worth comparing (oracle only, no GPU).

World E must hold, in the player-eats-player pass and the respawns behind it:
an eat whose eaten player lives on with fewer cells, an eat by a player of
several cells, a death, a respawn, and a tick with both an eat and a respawn.
World S must hold a tick that spawns more than 64 pellets (more than a tick
draws ahead), a tick that spawns a virus, and a tick on which a stopped blob's
pellet and a spawned pellet join the same bucket row.  These are conditions on
the worlds (seeds and masses chosen so the oracle alone meets them), not
measurements."""
import numpy as np

from oracle_lib import Oracle
import closing_worlds as cw

BUCKET = 20
EV_CELL, EV_DEATH, EV_RESPAWN = 8, 9, 10


def _walk(name, arena=0):
    """per tick: (state before, state after, events) of one arena"""
    w = cw.WORLDS[name]
    o = Oracle(cw.config(name))
    cw.start(name, o)
    fn = cw.command_fn(name)
    out = []
    for t in range(w["ticks"]):
        before = o.get_state(arena)
        o.set_commands(fn(t))
        o.step(1)
        out.append((before, o.get_state(arena), o.events(arena)))
    o.close()
    return out


def census_e():
    c = dict(eaten_survives=0, eater_multicell=0, deaths=0, respawns=0, eat_and_respawn=0)
    for before, after, ev in _walk("E"):
        owner = {int(r[2]): int(r[0]) for r in np.asarray(after["cells_i"])}  # seq -> owner, the cells left
        owner0 = {int(r[2]): int(r[0]) for r in np.asarray(before["cells_i"])}
        ncells = np.asarray(after["players_i"])[:, 4]
        died = {int(e[2]) for e in ev if e[1] == EV_DEATH}
        eats = [e for e in ev if e[1] == EV_CELL]
        for e in eats:
            victim = owner0.get(int(e[3]))  # (a cell made by this tick's split: not counted)
            if victim is not None and victim not in died and ncells[victim] >= 1:
                c["eaten_survives"] += 1
            eater = owner.get(int(e[2]))
            if eater is not None and ncells[eater] >= 2:
                c["eater_multicell"] += 1
        resp = sum(1 for e in ev if e[1] == EV_RESPAWN)
        c["deaths"] += len(died)
        c["respawns"] += resp
        c["eat_and_respawn"] += 1 if eats and resp else 0
    return c


def census_s():
    w = cw.WORLDS["S"]
    c = dict(most_pellet_spawns=0, virus_spawn_ticks=0, shared_row_ticks=0)
    for a in range(w["arenas"]):
        for before, after, ev in _walk("S", a):
            c["most_pellet_spawns"] = max(c["most_pellet_spawns"], int(after["ctr_pellet"]) - int(before["ctr_pellet"]))
            c["virus_spawn_ticks"] += 1 if int(after["ctr_virus"]) > int(before["ctr_virus"]) else 0
            had = set(np.asarray(before["pellets_seq"]).tolist())
            blobs = set(np.asarray(before["blobs_i"])[:, 1].tolist()) if len(before["blobs_i"]) else set()
            rows_conv, rows_spawn = set(), set()
            for sq, rec in zip(np.asarray(after["pellets_seq"]).tolist(), np.asarray(after["pellets_f"])):
                if sq in had:
                    continue
                row = min(int(rec[1] // BUCKET), w["size"] // BUCKET - 1)
                (rows_conv if sq in blobs else rows_spawn).add(row)
            c["shared_row_ticks"] += 1 if rows_conv & rows_spawn else 0
    return c


def test_world_e_has_partial_eats_multicell_eaters_deaths_and_respawns():
    c = census_e()
    print("world E:", c)
    assert c["eaten_survives"] >= 1
    assert c["eater_multicell"] >= 1
    assert c["deaths"] >= 1
    assert c["respawns"] >= 1
    assert c["eat_and_respawn"] >= 1


def test_world_s_has_a_spawn_burst_a_virus_spawn_and_a_shared_row():
    c = census_s()
    print("world S:", c)
    assert c["most_pellet_spawns"] > 64
    assert c["virus_spawn_ticks"] >= 1
    assert c["shared_row_ticks"] >= 1
