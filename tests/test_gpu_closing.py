"""GPU vs oracle at the end of the tick (closing_worlds.py): the untiled tick ends
in two launches -- the activity test, beside which the pellet bookkeeping closes
and the FOV cache is stored, then the player-eats-player pass with the pellet
rows beside it, the respawns, the virus spawns and the FOV cache entries of the
players the pass changed.  Events exact, states at
tolerance 0, every bot observed every tick, and player_stats (alive, mass, FOV
x / y / size) equal: the FOV cache is the one output the state diff does not
carry.  test_closing_worlds.py checks without a GPU that the worlds hold what
these runs need."""
import numpy as np
import pytest

from oracle_lib import Oracle
import closing_worlds as cw
import parity

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
_lib = pytest.importorskip("aigar_amd._lib")


def _pair(name):
    cfg = cw.config(name)
    g, o = _lib.Stepper(cfg), Oracle(cfg)
    cw.start(name, g, o)
    _same_world(g, o, name, "start")
    return g, o


def _same_world(g, o, name, what):
    for a in range(cw.WORLDS[name]["arenas"]):
        dif = parity.diff_states(g.get_state(a), o.get_state(a), ftol=0.0)
        assert dif == [], "%s, arena %d: %s" % (what, a, dif[:3])


def _same_stats(g, o, what):
    sg, so = g.player_stats(), o.player_stats()
    assert np.array_equal(sg, so, equal_nan=True), "%s: player_stats differ at bots %s" % (
        what, np.argwhere(~((sg == so) | (np.isnan(sg) & np.isnan(so))))[:4].tolist())


def _tick(g, o, name, fn, t):
    """one tick of run_pair (arena 0's events and state, every bot's row), then the other arenas and the stats"""
    err, _ = parity.run_pair(g, o, 1, lambda _t: fn(t), obs=True, ftol=0.0)
    assert err is None, "tick %d: %s" % (t, err)
    for a in range(1, cw.WORLDS[name]["arenas"]):
        assert np.array_equal(g.events(a), o.events(a)), "tick %d, arena %d: event logs differ" % (t, a)
    _same_world(g, o, name, "tick %d" % t)
    _same_stats(g, o, "tick %d" % t)


def _stepped(name):
    g, o = _pair(name)
    fn = cw.command_fn(name)
    for t in range(cw.WORLDS[name]["ticks"]):
        _tick(g, o, name, fn, t)
    g.sync()
    g.close()
    o.close()


def test_world_e_pp_eats_and_respawns():
    _stepped("E")


def test_world_s_spawn_burst_ragged_arenas():
    _stepped("S")


def test_world_e_greedy_graph():
    """World E through the aigar_run graph with the Greedy policy, five steps a call,
    against the oracle's Greedy moves (as test_gpu_multicell.py's world A)."""
    g, o = _pair("E")
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    fn = cw.command_fn("E")
    for t in range(cw.WORLDS["E"]["split_ticks"]):  # the forced splits first
        _tick(g, o, "E", fn, t)
    obs = torch.full((g.NP, g.obs_len), -7.0, dtype=torch.float64, device="cuda")
    for c in range(4):
        g.run(5, "greedy", obs, greedy_split=True)
        torch.cuda.synchronize()
        logs = []
        for _ in range(5):
            o.policy_greedy(True)
            o.step(1)
            want = o.observe()
            logs.append(o.events())
        assert np.array_equal(g.events(), np.concatenate(logs)), "call %d: event logs differ" % c
        _same_world(g, o, "E", "call %d" % c)
        assert parity.obs_close(obs.cpu().numpy(), want, 0.0), "call %d: observation rows differ" % c
        _same_stats(g, o, "call %d" % c)
    g.sync()
    g.close()
    o.close()


def test_observe_twice_after_one_tick():
    """The observe epoch now moves in the tick's last launch: two observes after one
    tick both give the oracle's rows (the second with the first's frame as its history)."""
    g, o = _pair("E")
    fn = cw.command_fn("E")
    for t in range(cw.WORLDS["E"]["split_ticks"] + 2):
        cmd = fn(t)
        g.set_commands(cmd)
        o.set_commands(cmd)
        g.step(1)
        o.step(1)
        for k in range(2):
            assert parity.obs_close(g.observe(), o.observe(), 0.0), "tick %d, observe %d: rows differ" % (t, k)
    g.sync()
    g.close()
    o.close()
