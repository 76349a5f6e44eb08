"""GPU vs oracle where most players hold many cells (multicell_worlds.py): the
eat prep's and the activity test's path that walks all of a player's cells at
once, next to the per-cell loop it falls back to.  Events exact, states at
tolerance 0, every bot observed every tick.  test_multicell_worlds.py checks
without a GPU that the worlds hold what these runs need."""
import numpy as np
import pytest

from oracle_lib import Oracle
import multicell_worlds as mw
import parity

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
_lib = pytest.importorskip("aigar_amd._lib")


def _pair(name):
    cfg = mw.config(name)
    g, o = _lib.Stepper(cfg), Oracle(cfg)
    mw.start(name, g, o)
    _same_world(g, o, name, "start")
    return g, o


def _same_world(g, o, name, what):
    for a in range(mw.WORLDS[name]["arenas"]):
        dif = parity.diff_states(g.get_state(a), o.get_state(a), ftol=0.0)
        assert dif == [], "%s, arena %d: %s" % (what, a, dif[:3])


def _stepped(name):
    g, o = _pair(name)
    A = mw.WORLDS[name]["arenas"]
    fn = mw.command_fn(name)
    most = 0
    for t in range(mw.TICKS):
        # one tick of run_pair (arena 0's events and state, every bot's row), then the other arenas
        err, _ = parity.run_pair(g, o, 1, lambda _t: fn(t), obs=True, ftol=0.0)
        assert err is None, "tick %d: %s" % (t, err)
        for a in range(1, A):
            assert np.array_equal(g.events(a), o.events(a)), "tick %d, arena %d: event logs differ" % (t, a)
        _same_world(g, o, name, "tick %d" % t)
        most = max(most, int(np.max(g.get_state()["players_i"][:, 4])))
    g.sync()
    g.close()
    o.close()
    return most


def test_world_a_sixteen_cells_merge_and_eject():
    assert _stepped("A") == 16


def test_world_b_ragged_arenas_and_overflowing_cells():
    assert _stepped("B") >= 8


def test_world_a_greedy_graph():
    """World A through the aigar_run graph with the Greedy policy (whichever eat-prep /
    activity kernels that graph launches), five steps a call, against the oracle's Greedy moves."""
    g, o = _pair("A")
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    fn = mw.command_fn("A")
    for t in range(mw.SPLIT_TICKS):  # every player to 16 cells first
        err, _ = parity.run_pair(g, o, 1, lambda _t: fn(t), obs=True, ftol=0.0)
        assert err is None, "tick %d: %s" % (t, err)
    obs = torch.full((g.NP, g.obs_len), -7.0, dtype=torch.float64, device="cuda")
    for c in range(5):
        g.run(5, "greedy", obs, greedy_split=True)
        torch.cuda.synchronize()
        logs = []
        for _ in range(5):
            o.policy_greedy(True)
            o.step(1)
            want = o.observe()
            logs.append(o.events())
        assert np.array_equal(g.events(), np.concatenate(logs)), "call %d: event logs differ" % c
        _same_world(g, o, "A", "call %d" % c)
        assert parity.obs_close(obs.cpu().numpy(), want, 0.0), "call %d: observation rows differ" % c
    g.sync()
    g.close()
    o.close()
