"""The Philox worlds of the learner-glue tests and their oracle-side driver (test
infrastructure, like shapes.py): NN players among Greedy and Random bots on the CPU
oracle, every role steered by the reference's rules, so that the oracle supplies the
(alive, mass, fov) stream tests/learner_model.py needs and the states to compare with.
test_gpu_learner.py runs the device beside it; test_learner_model.py counts, on the
oracle alone, that these worlds hold what the GPU tests are for.

Roles per tick (Model.takeBotActions): the NN players' commands come from the caller (the
model); the Greedy players' from the oracle's own Greedy bots (bot.py:579-633); a Random
player holds a Philox-drawn action for max(1, FRAME_SKIP_RATE) of its moves (bot.py:243-249
with the device's keying: player, stream 9, move counter, salt); a dead player keeps its
command."""
import ctypes as C

import numpy as np

from aigar_amd import _abi
from oracle_lib import Oracle, lib as oracle_c, make_config
import learner_model as lm
import shapes

# (arenas, players per arena, field size, max_viruses, rounds): arena boundaries inside the one
# 256-thread block of the per-player kernels, which is partial (12, 39 and 128 of 256 threads);
# the six learners of 1 x 12 play three times as many decisions to meet as many deaths
SHAPES = [(1, 12, 90, 3, 3), (3, 13, 115, 4, 1), (2, 64, 260, 12, 1)]
SHAPE_IDS = ["%dx%d" % s[:2] for s in SHAPES]
SEED = 11
G = 5
CHANNELS = _abi.OBS_PELLET | _abi.OBS_SELF | _abi.OBS_ENEMY | _abi.OBS_VIRUS | _abi.OBS_SELF_LF | _abi.OBS_ENEMY_LF
EXTRAS = 0x1F  # last fov size, fov size, mass, last and second-last action
REWARD = dict(reward_term=0.3, reward_scale=0.3, death_factor=1.7, death_term=-40.5)  # nothing dyadic
# the decision matrix of the environment tests: (frame skip, width, enable_split, enable_eject, mass_as_reward)
MATRIX = [(0, 2, False, False, False), (3, 4, True, True, False), (7, 3, True, False, True), (3, 3, False, False, True),
          (7, 4, True, True, False)]
MATRIX_IDS = ["s%d-w%d-split%d-eject%d-mar%d" % tuple(int(v) for v in m) for m in MATRIX]
DECISIONS = {0: 60, 3: 24, 7: 12}  # per frame skip and round: 60 .. 96 ticks


def n_decisions(shape, p):
    return DECISIONS[p.frame_skip] * shape[4]


def roles_of(B):
    """Every second player a learner, the others Greedy with every third of those Random."""
    out = []
    for i in range(B):
        out.append("NN" if i % 2 == 0 else ("Random" if i % 6 == 5 else "Greedy"))
    return out


def model_params(m):
    skip, width, split, eject, mar = m
    return lm.params(skip, width, split, eject, mar, **REWARD)


def env_parameters(p, **kw):
    """The reference-style parameter set of AgarVecEnv / the facade for the model's p."""
    import types
    base = dict(VIRUS_SPAWN=True, ENABLE_SPLIT=p.enable_split, ENABLE_EJECT=p.enable_eject, ENABLE_GREEDY_SPLIT=True,
                PELLET_GRID=True, SELF_GRID=True, WALL_GRID=False, ENEMY_GRID=True, VIRUS_GRID=True, SELF_GRID_LF=True,
                ENEMY_GRID_LF=True, USE_FOVSIZE=True, USE_TOTALMASS=True, USE_LAST_ACTION=True,
                USE_SECOND_LAST_ACTION=True, USE_LAST_FOVSIZE=True, GRID_SQUARES_PER_FOV=G, EXTRA_INPUT=True,
                GRID_VIEW_ENABLED=True, FRAME_SKIP_RATE=p.frame_skip, RESET_LIMIT=0, GATHER_EXP=True,
                **vars(lm.reward_namespace(p)))
    base.update(kw)
    return types.SimpleNamespace(**base)


def config(shape):
    A, B, field, mv = shape[:4]
    return make_config(n_arenas=A, bots=B, field_size=field, virus=True, max_viruses=mv, channels=CHANNELS,
                       extras=EXTRAS, grid_squares=G, flags=_abi.FLAG_EVENTS)


def action_table(seed, NP, decisions, width):
    """Uniform actions with about a tenth of the values exactly 0, 0.5 or 1 - 2^-53."""
    rng = np.random.default_rng(seed)
    tab = rng.random((decisions, NP, width))
    edge = rng.random(tab.shape) < 0.1
    tab[edge] = rng.choice((0.0, 0.5, 1.0 - 2.0 ** -53), int(edge.sum()))
    return tab


def mature(x, A, seed):
    """Masses 12 .. 400 from the first tick: the big eat the small at once, and the eaten
    respawn small beside them."""
    shapes.mature(x, A, seed, lo=12.0, hi=400.0)


class World:
    """The oracle and the non-NN roles' policies."""

    def __init__(self, shape, p, seed=SEED, salt=SEED):
        self.A, self.B = shape[:2]
        self.NP = self.A * self.B
        self.p, self.salt = p, salt
        self.roles = np.array([_abi.ROLES[r] for r in roles_of(self.B)] * self.A, np.uint8)
        self.nn = np.nonzero(self.roles == _abi.ROLE_NN)[0]
        self.o = Oracle(config(shape))
        self.o.reset(seed)
        mature(self.o, self.A, seed)
        self.keys = [np.array(self.o.get_state(a)["philox_key"], np.uint64) for a in range(self.A)]
        self.held, self.moves = np.zeros((self.NP, 4)), np.zeros(self.NP, np.int64)
        self.t = 0
        self.log = [[] for _ in range(self.A)]  # per arena: the event rows of every tick since new_window()
        self.was_alive = self.stats()[:, 0] > 0
        self.deaths, self.respawns = [], []  # (tick at which makeMove first sees it, player)

    def close(self):
        self.o.close()

    def stats(self):
        return self.o.player_stats()

    def new_window(self):
        self.log = [[] for _ in range(self.A)]

    def window_events(self, a):
        """The event rows of arena a over the ticks since new_window()."""
        return np.concatenate(self.log[a]) if self.log[a] else np.zeros((0, 4), np.int64)

    def _random_action(self, i):
        rs = max(1, self.p.frame_skip)
        if self.moves[i] % rs == 0:
            ctr = np.array([i, 9, self.moves[i], self.salt], np.uint64)
            u = np.zeros(4, np.uint64)
            oracle_c().oracle_philox(ctr.ctypes.data_as(C.POINTER(C.c_uint64)),
                                     self.keys[i // self.B].ctypes.data_as(C.POINTER(C.c_uint64)),
                                     u.ctypes.data_as(C.POINTER(C.c_uint64)))
            h = [(int(v) >> 11) * (1.0 / 9007199254740992.0) for v in u]
            self.held[i] = (h[0], h[1], h[2] if self.p.enable_split else 0.0, h[3] if self.p.enable_eject else 0.0)
        self.moves[i] += 1
        return self.held[i]

    def tick(self, stats, nn_cmds):
        """One Model.update: the commands of every role (nn_cmds {player: command} for the
        live NN players), then Field.update.  Returns the commands played."""
        prev = shapes.commands(self.o, self.A)
        self.o.policy_greedy(True)
        cmd = shapes.commands(self.o, self.A)
        four = lm.params(width=4)
        for i in range(self.NP):
            alive = stats[i, 0] > 0
            if self.roles[i] == _abi.ROLE_GREEDY and alive:
                continue
            cmd[i] = prev[i]
            if not alive:
                continue
            if self.roles[i] == _abi.ROLE_NN:
                cmd[i] = nn_cmds[i]
            else:
                cmd[i] = lm.set_command_point(stats[i], list(self._random_action(i)), four)
        self.o.set_commands(cmd)
        self.o.step(1)
        self.t += 1
        for a in range(self.A):
            self.log[a].append(self.o.events(a))
        alive = self.stats()[:, 0] > 0
        for i in self.nn:
            if self.was_alive[i] and not alive[i]:
                self.deaths.append((self.t, int(i)))
            if alive[i] and not self.was_alive[i]:
                self.respawns.append((self.t, int(i)))
        self.was_alive = alive
        return cmd

    def state_rows(self, players, cur, prev):
        """getStateRepresentation of the given players with the action extras cur / prev
        [NP, 4]: NaN rows for dead players, whose history does not advance."""
        self.o.set_actions(cur, prev)
        alive = self.stats()[:, 0] > 0
        out = np.full((self.NP, self.o.obs_len), np.nan)
        for i in players:
            if alive[i]:
                out[i] = self.o.observe_one(int(i) % self.B, int(i) // self.B)
        return out


class Need:
    """What a world must hold for the decision tests, counted over its windows on the
    oracle's stream."""

    def __init__(self, skip):
        self.skip = skip
        self.inside = self.on_decision = self.respawn_reward = self.dead_window = 0

    def window(self, rows, nn, known):
        """rows [skip + 2, NP]: alive at the window's decision tick and after each of its
        ticks (the last row is the observation's, the next decision tick); known [NP]:
        the player has a lastMass in this window."""
        last = len(rows) - 1
        for i in nn:
            a = rows[:, i]
            for k in range(1, last + 1):
                if a[k - 1] and not a[k]:
                    if k < last:
                        self.inside += 1  # first seen dead on a skipped frame
                    else:
                        self.on_decision += 1  # first seen dead at the decision's observation
                if a[k] and not a[k - 1] and known[i]:
                    self.respawn_reward += 1  # alive again, rewarded against the lastMass from before its death
            if not a.any():
                self.dead_window += 1

    def check(self):
        if self.skip > 0:
            assert self.inside >= 5, "deaths inside a skip window: %d" % self.inside
        assert self.on_decision >= 1, "deaths on a decision tick: %d" % self.on_decision
        assert self.respawn_reward >= 5, "respawns rewarded against the old lastMass: %d" % self.respawn_reward


def decisions(w, b, table, need=None):
    """Drive the world w through len(table) decisions of the batched model b (learner_model.Batched
    over all players, NN = w.nn).  Yields, after each decision, (d, stats, obs, reward, alive,
    transitions): the oracle's stats and NN state rows at the observation's tick and what
    Batched.end returns.  w.obs_at[tick] keeps every observation for the transitions' states."""
    skip = b.p.frame_skip
    for d in range(len(table)):
        rows = []
        w.new_window()
        for k in range(skip + 1):
            st = w.stats()
            rows.append(st[:, 0] > 0)
            w.tick(st, b.commands(k, st, table[d] if k == 0 else None))
        st = w.stats()
        rows.append(st[:, 0] > 0)
        if need is not None:
            need.window(np.array(rows), w.nn, [m is not None for m in b.last_mass])
        obs = w.state_rows(w.nn, b.cur, b.prev)
        w.obs_at[w.t] = obs
        reward, alive, tr = b.end(w.t, st)
        yield d, st, obs, reward, alive, tr


def begin(w, b):
    """The first observation (AgarVecEnv.reset's): every NN player's first state."""
    st = w.stats()
    obs = w.state_rows(w.nn, b.cur, b.prev)
    w.obs_at = {0: obs}
    b.reset_players(w.nn, 0, st)
    return obs
