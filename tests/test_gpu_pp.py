"""GPU vs oracle for the player-eats-player pass on built worlds (pp_worlds.py):
tick.hip's pp_pass as independent groups and as one serial wavefront, on both
sides of each of its limits -- fewer than 3 and more than 64 pending players, 16
against 17 players and 64 against 65 cells in a closure, a closure's 12th
against a 13th round, more groups than wavefronts, merged closures (kept, over
the player cap by their union, over it once closed again, in conflict with
another root once closed again), re-activation and the row shift inside a
group, R at the mass cap in the field's corner, owners in global memory (more
than 8192 players), immediate occupancy on a field too large for the dirty-word
bitmap, and three arenas with different pending sets.

Every case runs on three steppers: the device, the oracle, and a second device
handle forced to the serial pass (AIGAR_PP_SERIAL).  Every tick: the event logs
of every arena equal, states at tolerance 0, every bot's observation row and
player_stats equal; and the pass took the path the case names, by the handles'
counters (pp_serial_players counts the pending players on either path,
pp_parallel_ticks the ticks run as groups).  A raised candidate- or work-cap
error bit fails get_state.  test_pp_worlds.py checks without a GPU that each
world holds what its case claims."""
import os

import numpy as np
import pytest

from oracle_lib import Oracle
import pp_worlds as pw
import parity

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
_lib = pytest.importorskip("aigar_amd._lib")


def _three(name):
    """(device, forced-serial device, oracle), all in the case's start state; the commands"""
    cfg = pw.config(name)
    g = _lib.Stepper(cfg)
    os.environ["AIGAR_PP_SERIAL"] = "1"
    try:
        s = _lib.Stepper(cfg)
    finally:
        del os.environ["AIGAR_PP_SERIAL"]
    o = Oracle(cfg)
    cmd = pw.start(name, g, s, o)
    return g, s, o, cmd


def _same(x, o, name, what, want_obs):
    for a in range(pw.CASES[name]["arenas"]):
        ex, eo = x.events(a), o.events(a)
        assert np.array_equal(ex, eo), "%s, arena %d: event logs differ: %s vs the oracle's %s" % (
            what, a, ex[:6].tolist(), eo[:6].tolist())
        dif = parity.diff_states(x.get_state(a), o.get_state(a), ftol=0.0)
        assert dif == [], "%s, arena %d: %s" % (what, a, dif[:3])
    assert parity.obs_close(x.observe(), want_obs, 0.0), "%s: observation rows differ" % what
    sx, so = x.player_stats(), o.player_stats()
    assert np.array_equal(sx, so, equal_nan=True), "%s: player_stats differ" % what


def _path(x, before, name, forced):
    """the first tick's pass by the counters: every arena's pending players, and the path"""
    for a, groups in enumerate(pw.CASES[name]["groups"]):
        c = x.counters(a)
        who = "%s, arena %d%s" % (name, a, ", forced serial" if forced else "")
        assert c["pp_serial_players"] - before[a]["pp_serial_players"] == pw.layout(name, a).pending, who
        assert c["pp_parallel_ticks"] - before[a]["pp_parallel_ticks"] == (1 if groups and not forced else 0), who


@pytest.mark.parametrize("name", list(pw.CASES))
def test_pass_matches_the_oracle_and_takes_the_path_the_case_names(name):
    g, s, o, cmd = _three(name)
    A = pw.CASES[name]["arenas"]
    before = [[x.counters(a) for a in range(A)] for x in (g, s)]
    for t in range(pw.TICKS):
        for x in (g, s, o):
            x.set_commands(cmd)
            x.step(1)
        want = o.observe()
        _same(g, o, name, "%s, tick %d, groups" % (name, t), want)
        _same(s, o, name, "%s, tick %d, forced serial" % (name, t), want)
        if t == 0:
            _path(g, before[0], name, False)
            _path(s, before[1], name, True)
    for x in (g, s):
        x.sync()  # (raises on any device error bit)
        x.close()
    o.close()


def test_seeds64_through_the_run_graph():
    """the 64 groups of seeds64 under graph replay: aigar_run with the held commands (policy
    "none"), all of the case's ticks in one call, observation rows included"""
    name = "seeds64"
    cfg = pw.config(name)
    g, o = _lib.Stepper(cfg), Oracle(cfg)
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    cmd = pw.start(name, g, o)
    before = g.counters()
    obs = torch.full((g.NP, g.obs_len), -7.0, dtype=torch.float64, device="cuda")
    g.set_commands(cmd)
    g.run(pw.TICKS, "none", obs)
    torch.cuda.synchronize()
    o.set_commands(cmd)
    log = []
    for _ in range(pw.TICKS):
        o.step(1)
        want = o.observe()
        log.append(o.events())
    assert np.array_equal(g.events(), np.concatenate(log)), "event logs differ"
    assert parity.diff_states(g.get_state(), o.get_state(), ftol=0.0) == []
    assert parity.obs_close(obs.cpu().numpy(), want, 0.0), "observation rows differ"
    after = g.counters()
    assert after["pp_serial_players"] - before["pp_serial_players"] >= pw.layout(name).pending
    assert after["pp_parallel_ticks"] - before["pp_parallel_ticks"] >= 1
    g.sync()
    g.close()
    o.close()
