"""GPU vs oracle for what the untiled tick settles ahead of its player-eats-player
pass (lists_worlds.py): in the launch of the activity test one block per arena
compacts the virus and blob lists, partitions the dead list -- waiters to the
front, respawners to the respawn list -- and takes every spawn count; the last
launch then only runs the pass, spawns the viruses, stores the FOV entries of
the players the pass marked and respawns the listed players.  Events exact,
states at tolerance 0, every bot observed every tick, and player_stats (alive,
mass, FOV x / y / size) equal.  World L once through separate step / observe
calls and once through the run graphs (random and Greedy, five steps a call);
world M -- one arena of more players than the FOV marks have bits -- stepped.
test_lists_worlds.py checks without a GPU that the worlds hold what these runs
need."""
import numpy as np
import pytest

from oracle_lib import Oracle
import lists_worlds as lw
import parity

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
_lib = pytest.importorskip("aigar_amd._lib")


def _same_world(g, o, name, what):
    for a in range(lw.WORLDS[name]["arenas"]):
        dif = parity.diff_states(g.get_state(a), o.get_state(a), ftol=0.0)
        assert dif == [], "%s, arena %d: %s" % (what, a, dif[:3])


def _same_stats(g, o, what):
    sg, so = g.player_stats(), o.player_stats()
    assert np.array_equal(sg, so, equal_nan=True), "%s: player_stats differ at bots %s" % (
        what, np.argwhere(~((sg == so) | (np.isnan(sg) & np.isnan(so))))[:4].tolist())


def _pair(name):
    cfg = lw.config(name)
    g, o = _lib.Stepper(cfg), Oracle(cfg)
    lw.start(name, g, o)
    _same_world(g, o, name, "start")
    return g, o


def _tick(g, o, name, fn, t):
    """one tick of run_pair (arena 0's events and state, every bot's row), then the other arenas and the stats"""
    err, _ = parity.run_pair(g, o, 1, lambda _t: fn(t), obs=True, ftol=0.0)
    assert err is None, "tick %d: %s" % (t, err)
    for a in range(1, lw.WORLDS[name]["arenas"]):
        assert np.array_equal(g.events(a), o.events(a)), "tick %d, arena %d: event logs differ" % (t, a)
    _same_world(g, o, name, "tick %d" % t)
    _same_stats(g, o, "tick %d" % t)


def _stepped(name):
    g, o = _pair(name)
    fn = lw.command_fn(name)
    for t in range(lw.WORLDS[name]["ticks"]):
        _tick(g, o, name, fn, t)
    g.sync()
    g.close()
    o.close()


def test_world_l_stepped():
    _stepped("L")


def test_world_m_more_players_than_mark_bits():
    _stepped("M")


def _drawn_commands(twin, arenas):
    """the commands a stepper holds (after policy_random): x, y, split, eject per bot"""
    rows = []
    for a in range(arenas):
        st = twin.get_state(a)
        rows.append(np.column_stack([np.asarray(st["players_f"])[:, :2], np.asarray(st["players_i"])[:, 2:4]]))
    return np.concatenate(rows).astype(np.float64)


@pytest.mark.parametrize("policy", ["random", "greedy"])
def test_world_l_run_graphs(policy):
    """World L through the aigar_run graphs, five steps a call.  Greedy: against the oracle's
    Greedy moves (as test_gpu_closing.py's world E).  Random: the oracle has no such policy, so a
    twin stepper draws the same commands through separate policy_random / step calls; the oracle
    is given what the twin drew, and the graph's world must equal the oracle's after the call."""
    w = lw.WORLDS["L"]
    g, o = _pair("L")
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    twin = None
    if policy == "random":
        twin = _lib.Stepper(lw.config("L"))
        lw.start("L", twin, o)
    fn = lw.command_fn("L")
    for t in range(w["split_ticks"]):  # the forced splits first
        cmd = fn(t)
        if twin is not None:
            twin.set_commands(cmd)
            twin.step(1)
        g.set_commands(cmd)
        o.set_commands(cmd)
        g.step(1)
        o.step(1)
    _same_world(g, o, "L", "after the splits")
    obs = torch.full((g.NP, g.obs_len), -7.0, dtype=torch.float64, device="cuda")
    for c in range((w["ticks"] - w["split_ticks"]) // 5):
        if policy == "greedy":
            g.run(5, "greedy", obs, greedy_split=True)
        else:
            g.run(5, "random", obs, p_split=0.05, p_eject=w["p_eject"], seed=17)
        torch.cuda.synchronize()
        logs = [[] for _ in range(w["arenas"])]
        for _ in range(5):
            if policy == "greedy":
                o.policy_greedy(True)
            else:
                twin.policy_random(0.05, w["p_eject"], 17)
                o.set_commands(_drawn_commands(twin, w["arenas"]))
                twin.step(1)
            o.step(1)
            want = o.observe()
            for a in range(w["arenas"]):
                logs[a].append(o.events(a))
        for a in range(w["arenas"]):
            assert np.array_equal(g.events(a), np.concatenate(logs[a])), "call %d, arena %d: event logs differ" % (c, a)
        _same_world(g, o, "L", "call %d" % c)
        if twin is not None:
            _same_world(twin, o, "L", "call %d, the twin" % c)
        assert parity.obs_close(obs.cpu().numpy(), want, 0.0), "call %d: observation rows differ" % c
        _same_stats(g, o, "call %d" % c)
    g.sync()
    g.close()
    if twin is not None:
        twin.close()
    o.close()
