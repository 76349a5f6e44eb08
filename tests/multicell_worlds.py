"""The two worlds of the multi-cell eat-prep / activity tests (test_multicell_worlds.py
checks on the oracle that they hold what the GPU tests need; test_gpu_multicell.py
steps them on the device).

World A: 40 bots on a 600 field, every cell set to mass 1500; all split for five
ticks (every player reaches the 16-cell cap), then merge and eject.
World B: 3 arenas of 13 bots on a 400 field dense with pellets, every cell set to
mass 3000: 13 bots per arena put arena boundaries inside a block of four players
and leave the last block partial, and the cells' boxes hold up to ~200 pellets."""
import math

import numpy as np

from aigar_amd import _abi
from oracle_lib import make_config
import parity

CH = (_abi.OBS_PELLET | _abi.OBS_SELF | _abi.OBS_WALL | _abi.OBS_ENEMY | _abi.OBS_SELF_LF | _abi.OBS_ENEMY_LF)
SEED = 35
TICKS = 30
SPLIT_TICKS = 5

WORLDS = {
    "A": dict(arenas=1, bots=40, size=600, mass=1500.0,
              cfg=dict(bots=40, field_size=600, max_pellets=3000.0, blob_cap=2048)),
    "B": dict(arenas=3, bots=13, size=400, mass=3000.0,
              cfg=dict(n_arenas=3, bots=13, field_size=400, max_pellets=4000.0, blob_cap=2048)),
}


def config(name):
    return make_config(channels=CH, extras=0x1F, **WORLDS[name]["cfg"])


def start(name, *steppers):
    """reset(SEED), then every cell of every arena set to the world's mass (loaded into all steppers)."""
    w = WORLDS[name]
    src = steppers[-1]
    for s in steppers:
        s.reset(SEED)
    for a in range(w["arenas"]):
        d = dict(src.get_state(a))
        cf = d["cells_f"].copy()
        cf[:, 2] = w["mass"]
        cf[:, 3] = math.sqrt(w["mass"] / math.pi)
        d["cells_f"] = cf
        for s in steppers:
            s.load_state(d, a)


def command_fn(name):
    """t -> commands: p_split 1.0 for the first SPLIT_TICKS ticks, then p_split 0 and p_eject 0.1."""
    w = WORLDS[name]
    rng = np.random.default_rng(5)
    n = w["arenas"] * w["bots"]

    def fn(t):
        if t < SPLIT_TICKS:
            return parity.synthetic_commands(rng, None, n, w["size"], 1.0, 0.0)
        return parity.synthetic_commands(rng, None, n, w["size"], 0.0, 0.1)
    return fn
