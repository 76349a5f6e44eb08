"""World L of the list-and-plan tests (test_lists_worlds.py checks on the oracle
that it holds what the GPU test needs; test_gpu_lists.py steps it on the device).
It aims at what the untiled tick settles before its player-eats-player pass: the
compaction of the virus and blob lists, the dead list's partition and the spawn
counts -- and at the respawns and spawns that follow the pass.

World L: 2 arenas of 13 bots on a 300 field (the arena boundary falls inside a
block of players, the last block is partial), viruses on with max_viruses 4, a
blob list of 256 slots.  The players' cells are set to three masses in turn --
3000, 600, 40 -- as in closing_worlds' world E, and two of each arena's viruses
are moved onto a heavy cell: they are eaten on the first tick (the virus list is
compacted, its grid rebuilt, the eaters burst) and spawned anew.  Everybody
splits on the first ticks and then steers at the middle of the field, ejecting
all the while: the blob list fills past half its slots while blobs are eaten, so
the device's compaction rule fires again and again.  Its second case is a
single arena of 8200 bots for the FOV marks' aliases (more players than mark bits)."""
import math

import numpy as np

from aigar_amd import _abi
from oracle_lib import make_config
import parity

CH = (_abi.OBS_PELLET | _abi.OBS_SELF | _abi.OBS_WALL | _abi.OBS_ENEMY | _abi.OBS_VIRUS | _abi.OBS_SELF_LF
      | _abi.OBS_ENEMY_LF)

WORLDS = {
    "L": dict(arenas=2, bots=13, size=300, ticks=28, seed=22, split_ticks=3, p_eject=0.5, masses=(3000.0, 600.0, 40.0),
              viruses_moved=2,
              cfg=dict(n_arenas=2, bots=13, field_size=300, virus=True, max_pellets=600.0, max_viruses=4.0,
                       blob_cap=256)),
    # more players than FOVM_BITS (8192) in one arena: light cells crowded around heavy ones
    "M": dict(arenas=1, bots=8200, size=2000, ticks=5, seed=7, split_ticks=0, p_eject=0.0,
              masses=(2000.0,) + (25.0,) * 15, viruses_moved=0,
              cfg=dict(n_arenas=1, bots=8200, field_size=2000, virus=True, max_pellets=2000.0, max_viruses=8.0)),
}
BLOB_CAP = 256
HEAVY = 3000.0


def config(name):
    return make_config(channels=CH, extras=0x1F, **WORLDS[name]["cfg"])


def _with_masses(d, masses):
    """state d with every cell's mass set by its owner's index (masses in turn)"""
    d = dict(d)
    cf = np.asarray(d["cells_f"]).copy()
    m = np.array([masses[int(p) % len(masses)] for p in np.asarray(d["cells_i"])[:, 0]])
    cf[:, 2] = m
    cf[:, 3] = np.sqrt(m / math.pi)
    d["cells_f"] = cf
    return d


def _viruses_onto_heavy(d, k):
    """state d with its first k viruses moved onto the first k heaviest cells"""
    d = dict(d)
    cf, vf = np.asarray(d["cells_f"]), np.asarray(d["viruses_f"]).copy()
    heavy = np.nonzero(cf[:, 2] >= HEAVY)[0]
    for i in range(min(k, len(vf), len(heavy))):
        vf[i, 0], vf[i, 1] = cf[heavy[i], 0], cf[heavy[i], 1]
    d["viruses_f"] = vf
    return d


def start(name, *steppers):
    """reset(seed), then the world's start state loaded into every stepper (made on the last one)."""
    w = WORLDS[name]
    src = steppers[-1]
    for s in steppers:
        s.reset(w["seed"])
    for a in range(w["arenas"]):
        d = _viruses_onto_heavy(_with_masses(src.get_state(a), w["masses"]), w["viruses_moved"])
        for s in steppers:
            s.load_state(d, a)


def command_fn(name):
    """t -> commands: everybody splits for the first ticks, then steers at the middle
    third of the field; ejections with the world's probability on every tick."""
    w = WORLDS[name]
    rng = np.random.default_rng(5)
    n = w["arenas"] * w["bots"]

    def fn(t):
        cmd = parity.synthetic_commands(rng, None, n, w["size"] / 3.0, 1.0 if t < w["split_ticks"] else 0.0,
                                        w["p_eject"])
        cmd[:, :2] += w["size"] / 3.0
        return cmd
    return fn
