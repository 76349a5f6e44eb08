"""World L of test_gpu_lists.py is worth comparing (oracle only, no GPU).

Per tick and arena, from the oracle's events and states: virus deaths, virus
spawns, player deaths, respawns, blobs created and blobs alive.  The device keeps
dead blobs' slots in its list until a rule says compact (tick.hip,
blob_compact_due); the rule is replayed here on those counts.  World L must
hold: a heavy cell that eats a virus (the virus list is compacted, its grid
rebuilt) and a virus spawn, at least two blob compactions, deaths and respawns
in the player-eats-player pass, and a tick with a compaction, a respawn and a
death at once.  World M must hold eats and respawns among more players than the
FOV marks have bits.  These are conditions on the worlds (seeds and masses
chosen so the oracle alone meets them), not measurements."""
import numpy as np

from oracle_lib import Oracle
import lists_worlds as lw

EV_VIRUS_EAT_BLOB, EV_EAT_VIRUS, EV_EAT_BLOB, EV_CELL, EV_DEATH, EV_RESPAWN = 2, 4, 7, 8, 9, 10
MAX_CELLS = 16


def _walk(name):
    """per tick: per arena (state before, state after, events)"""
    w = lw.WORLDS[name]
    o = Oracle(lw.config(name))
    lw.start(name, o)
    fn = lw.command_fn(name)
    out = []
    for t in range(w["ticks"]):
        before = [o.get_state(a) for a in range(w["arenas"])]
        o.set_commands(fn(t))
        o.step(1)
        out.append([(before[a], o.get_state(a), o.events(a)) for a in range(w["arenas"])])
    o.close()
    return out


def _blob_seqs(st):
    return set(np.asarray(st["blobs_i"])[:, 1].tolist()) if len(st["blobs_i"]) else set()


def tick_counts(before, after, ev):
    """one arena's tick: the counts the device's end-of-tick plan turns on"""
    had, have = _blob_seqs(before), _blob_seqs(after)
    eaten = {int(e[3]) for e in ev if e[1] in (EV_VIRUS_EAT_BLOB, EV_EAT_BLOB)}
    return dict(virus_deaths=sum(1 for e in ev if e[1] == EV_EAT_VIRUS),
                virus_spawns=int(after["ctr_virus"]) - int(before["ctr_virus"]),
                deaths=sum(1 for e in ev if e[1] == EV_DEATH),
                respawns=sum(1 for e in ev if e[1] == EV_RESPAWN),
                pp_eats=sum(1 for e in ev if e[1] == EV_CELL),
                blobs_created=len(have - had) + len(eaten - had),  # (the second: made and eaten in one tick)
                blobs_died=len(had - have) + len(eaten - had),
                blobs_alive=len(have),
                cells=len(np.asarray(after["cells_i"])))


def blob_compactions(ticks, bots, cap=lw.BLOB_CAP):
    """the device's rule on one arena's counts: the ticks on which the blob list is compacted, for
    the least and the most the rule's cell total can be (it only ever adds compactions)"""
    out = []
    for ncell in (0, MAX_CELLS * bots):
        n_list, fired = 0, []
        for t, c in enumerate(ticks):
            n_list += c["blobs_created"]
            live = c["blobs_alive"]
            if c["blobs_died"]:  # (DIRTY_BLOB)
                skip = n_list < 2 * live + 256 and n_list < cap // 2 and n_list + min(2 * ncell, MAX_CELLS * bots) <= cap
                if not skip:
                    n_list = live
                    fired.append(t)
            assert n_list <= cap, "tick %d: the blob list overflows its %d slots" % (t, cap)
        out.append(fired)
    return out


def census_l():
    w = lw.WORLDS["L"]
    walk = _walk("L")
    c = dict(virus_deaths=0, virus_spawns=0, deaths=0, respawns=0, blob_compactions=0, all_at_once=0)
    for a in range(w["arenas"]):
        ticks = [tick_counts(*walk[t][a]) for t in range(w["ticks"])]
        least, _most = blob_compactions(ticks, w["bots"])
        for k in ("virus_deaths", "virus_spawns", "deaths", "respawns"):
            c[k] += sum(tc[k] for tc in ticks)
        c["blob_compactions"] += len(least)
        c["all_at_once"] += sum(1 for t, tc in enumerate(ticks)
                                if (t in least or tc["virus_deaths"]) and tc["respawns"] and tc["deaths"])
    return c


def census_m():
    w = lw.WORLDS["M"]
    c = dict(pp_eats=0, deaths=0, respawns=0, respawn_and_eat=0, bots=w["bots"])
    for tick in _walk("M"):
        tc = tick_counts(*tick[0])
        for k in ("pp_eats", "deaths", "respawns"):
            c[k] += tc[k]
        c["respawn_and_eat"] += 1 if tc["respawns"] and tc["pp_eats"] else 0
    return c


def test_world_l_has_compactions_virus_spawns_deaths_and_respawns():
    c = census_l()
    print("world L:", c)
    assert c["virus_deaths"] >= 1
    assert c["virus_spawns"] >= 1
    assert c["blob_compactions"] >= 2
    assert c["deaths"] >= 1
    assert c["respawns"] >= 1
    assert c["all_at_once"] >= 1


def test_world_m_has_eats_and_respawns_past_the_mark_bits():
    c = census_m()
    print("world M:", c)
    assert c["bots"] > 8192
    assert c["pp_eats"] >= 1
    assert c["deaths"] >= 1
    assert c["respawns"] >= 1
    assert c["respawn_and_eat"] >= 1
