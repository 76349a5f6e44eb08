"""The two worlds of the tick-closing tests (test_closing_worlds.py checks on the
oracle that they hold what the GPU tests need; test_gpu_closing.py steps them on
the device).  They aim at the end of the tick: the player-eats-player pass, the
respawns, the spawns and the FOV cache, which the untiled tick finishes in its last
two launches.

World E (pp eats and respawns): 1 arena, 12 bots on a 300 field with viruses.
The players' cells are set to three masses in turn -- 3000, 600, 40 -- so big
cells meet small ones; everybody splits on the first ticks (the big and the
middle players become multi-cell) and then steers at the middle of the field.
World S (spawn burst): 3 arenas of 13 bots on a 400 field, so arena boundaries
fall inside a block of players and the last block is partial.  The start state
lacks 150 of its pellets and two of its viruses: the first tick spawns more
pellets than were drawn ahead (the staging path) and the missing viruses; with
p_eject > 0 the stopped blobs turn into pellets that join the rows next to the
spawns."""
import math

import numpy as np

from aigar_amd import _abi
from oracle_lib import make_config
import parity

CH = (_abi.OBS_PELLET | _abi.OBS_SELF | _abi.OBS_WALL | _abi.OBS_ENEMY | _abi.OBS_VIRUS | _abi.OBS_SELF_LF
      | _abi.OBS_ENEMY_LF)

WORLDS = {
    "E": dict(arenas=1, bots=12, size=300, ticks=25, seed=11, split_ticks=3,
              cfg=dict(bots=12, field_size=300, virus=True, max_pellets=600.0, max_viruses=4.0, blob_cap=1024)),
    "S": dict(arenas=3, bots=13, size=400, ticks=15, seed=23, split_ticks=0,
              cfg=dict(n_arenas=3, bots=13, field_size=400, virus=True, max_pellets=1200.0, max_viruses=6.0,
                       blob_cap=2048)),
}
E_MASSES = (3000.0, 600.0, 40.0)
S_MASS = 400.0          # heavy enough to eject
S_PELLETS_GONE = 150    # more than the 64 spawns a tick draws ahead
S_VIRUSES_GONE = 2
S_WARM_TICKS = 30       # a blob flies for about that long before it stops and turns into a pellet


def config(name):
    return make_config(channels=CH, extras=0x1F, **WORLDS[name]["cfg"])


def _without(d, key_f, key_i, keep, extra=()):
    """state d with only the first `keep` entities of a kind (its float rows, int rows / seqs, extra columns)"""
    d[key_f] = np.asarray(d[key_f])[:keep].copy()
    d[key_i] = np.asarray(d[key_i])[:keep].copy()
    for k in extra:
        if k in d:
            d[k] = np.asarray(d[k])[:keep].copy()


def _with_masses(d, masses):
    """state d with every cell's mass set by its owner's index (masses in turn)"""
    d = dict(d)
    cf = np.asarray(d["cells_f"]).copy()
    m = np.array([masses[int(p) % len(masses)] for p in np.asarray(d["cells_i"])[:, 0]])
    cf[:, 2] = m
    cf[:, 3] = np.sqrt(m / math.pi)
    d["cells_f"] = cf
    return d


def start(name, *steppers):
    """reset(seed), then the world's start state loaded into every stepper (made on the last one)."""
    w = WORLDS[name]
    src = steppers[-1]
    n = w["arenas"] * w["bots"]
    for s in steppers:
        s.reset(w["seed"])
    if name == "E":
        for a in range(w["arenas"]):
            d = _with_masses(src.get_state(a), E_MASSES)
            for s in steppers:
                s.load_state(d, a)
        return
    # S: the source alone ejects for a while, so blobs are in flight at the start
    # and stop during the test; then pellets and viruses are taken out
    for a in range(w["arenas"]):
        src.load_state(_with_masses(src.get_state(a), (S_MASS,)), a)
    rng = np.random.default_rng(9)
    for _ in range(S_WARM_TICKS):
        src.set_commands(parity.synthetic_commands(rng, None, n, w["size"], 0.0, 0.3))
        src.step(1)
    for a in range(w["arenas"]):
        d = dict(src.get_state(a))
        npel, nvir = len(np.asarray(d["pellets_seq"])), len(np.asarray(d["viruses_i"]))
        _without(d, "pellets_f", "pellets_seq", npel - S_PELLETS_GONE, ("pellets_col",))
        _without(d, "viruses_f", "viruses_i", nvir - S_VIRUSES_GONE)
        for s in steppers:
            s.load_state(d, a)


def command_fn(name):
    """t -> commands.  E: everybody splits for the first ticks, then steers at the middle
    third of the field.  S: random points, p_eject 0.3."""
    w = WORLDS[name]
    rng = np.random.default_rng(5)
    n = w["arenas"] * w["bots"]

    def fn(t):
        if name == "S":
            return parity.synthetic_commands(rng, None, n, w["size"], 0.0, 0.3)
        cmd = parity.synthetic_commands(rng, None, n, w["size"] / 3.0, 1.0 if t < w["split_ticks"] else 0.0, 0.0)
        cmd[:, :2] += w["size"] / 3.0
        return cmd
    return fn
