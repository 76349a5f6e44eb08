"""Plain-Python model of the learner glue (test infrastructure, like decide_model.py and
replay_model.py): what the reference's NN bot does between "the world after a tick" and
"what a learner is handed" -- set_command_point for its action (bot.py:550-577), getReward
and updateRewards (bot.py:654-667, 166-168), frame skipping (bot.py:171-178), the action
extras (bot.py:313-322) and the experience tuples of move_NN (bot.py:195-230).

It never sees a world: its inputs are every tick's (alive, total mass, fov x, fov y, fov
size) of the bot's player as makeMove reads them (the rows of Oracle.player_stats), the
action table its learner answers from and the ticks after which Model.resetBots ran.  A
state is named by the tick whose observation it is.  test_learner_model.py pins it to the
reference's own bots (tests/golden/learner_*.npz) bit for bit; the GPU tests use it as
their oracle.

Two views:
  BotModel / run_bots   one reference bot, tick by tick, with all its quirks: a bot that
                        dies inside a skip window stops skipping, emits an experience
                        with no new state at every tick it is dead, keeps its cumulative
                        reward, adds the death reward every dead tick and, respawned,
                        rewards against the lastMass from before its death.
  Batched               one transition per player and decision window, as
                        AgarVecEnv.step_calls defines it (DESIGN.md section 4b says where
                        this differs from the bots and why).
"""
import math
import types

import numpy as np


def params(frame_skip=0, width=4, enable_split=True, enable_eject=True, mass_as_reward=False, reward_term=0.0,
           reward_scale=1.0, death_factor=1.0, death_term=0.0):
    return types.SimpleNamespace(frame_skip=int(frame_skip), width=int(width), enable_split=bool(enable_split),
                                 enable_eject=bool(enable_eject), mass_as_reward=bool(mass_as_reward),
                                 reward_term=float(reward_term), reward_scale=float(reward_scale),
                                 death_factor=float(death_factor), death_term=float(death_term))


def params_of(z):
    """The parameters of a learner_*.npz fixture."""
    return params(*(z[k][()] for k in ("frame_skip", "width", "enable_split", "enable_eject", "mass_as_reward",
                                       "reward_term", "reward_scale", "death_factor", "death_term")))


def reward_namespace(p):
    """The same parameters under the reference's names (RewardParams.from_parameters, the facade)."""
    return types.SimpleNamespace(REWARD_TERM=p.reward_term, REWARD_SCALE=p.reward_scale, DEATH_FACTOR=p.death_factor,
                                 DEATH_TERM=p.death_term, MASS_AS_REWARD=p.mass_as_reward)


def set_command_point(stat, action, p):
    """bot.py:550-577: (x, y, split, eject) for an action of 2, 3 or 4 values."""
    x, y, size = int(stat[2]), int(stat[3]), float(stat[4])
    left, top = x - int(size / 2), y - int(size / 2)
    size = int(size)
    split = eject = False
    if len(action) == 3:
        if p.enable_split:
            split = action[2] > 0.5
        elif p.enable_eject:  # bot.py:568 evaluates `[3] > 0.5`
            raise TypeError("the reference does not define 3 values with ENABLE_SPLIT off and ENABLE_EJECT on")
    elif len(action) == 4:
        split, eject = action[2] > 0.5, action[3] > 0.5
    return (left + action[0] * size, top + action[1] * size, float(bool(split)), float(bool(eject)))


def get_reward(alive, mass, last_mass, p):
    """bot.py:654-667; last_mass None -> None unless the mass is the reward."""
    if p.mass_as_reward:
        return mass - p.reward_term if alive else p.death_term - p.reward_term
    if last_mass is None:
        return None
    if not alive:
        reward = -1 * last_mass * p.death_factor + p.death_term
    else:
        reward = mass - last_mass
    return reward * p.reward_scale - p.reward_term


def reward_term_of_tick(alive, mass, last_mass, p):
    """What updateRewards adds (bot.py:167): getReward() if lastMass else 0."""
    return get_reward(alive, mass, last_mass, p) if last_mass else 0


class BotModel:
    """One NN bot (bot.py:125-233, 252-269)."""

    def __init__(self, p, rows):
        self.p, self.rows, self.k = p, rows, 0
        self.last_action = None  # (Bot.reset leaves lastAction alone)
        self.experiences = []  # (emit tick, old tick, action, reward, new tick or None)
        self.reset()

    def reset(self):
        self.last_mass = self.old = self.memory = self.action = None
        self.skip_frames, self.cum, self.last_reward, self.skipping = 0, 0, 0, False

    def move(self, t, stat):
        """makeMove at tick t -> (command or None for a dead player, computed, state):
        computed says whether getStateRepresentation ran, state is t or None."""
        p = self.p
        alive, mass = bool(stat[0] > 0), float(stat[1])
        self.skipping = False
        if self.action is not None:
            self.cum += reward_term_of_tick(alive, mass, self.last_mass, p)
            self.last_reward = self.cum
            if self.skip_frames > 0:
                self.skip_frames -= 1
                self.skipping = alive
        computed, state = not self.skipping, None
        if computed:
            state = t if alive else None
            self.extras = (self.action, self.last_action)  # what the state's action extras show
            if self.old is not None:
                self.experiences.append((t, self.old, self.action, self.last_reward, state))
                self.memory = (self.old, self.action, self.last_reward, state, state is not None)
            if alive:
                row = [float(v) for v in self.rows[self.k]]
                self.k += 1
                self.cum, self.skip_frames, self.old = 0, p.frame_skip, t
                self.last_action, self.action = self.action, row
                self.last_mass = mass
        if not alive:
            return None, computed, state
        act = list(self.action)
        if self.skipping:
            act[2:] = [0, 0]
        return set_command_point(stat, act, p), computed, state


def pad4(a, fill=math.nan):
    out = np.full(4, fill)
    if a is not None:
        out[:len(a)] = a
    return out


def run_bots(p, stats, table, reset_after):
    """stats [T, nn, 5], table [nn, T, width], reset_after [T] -> the record of a
    learner_*.npz fixture under its names, plus cmds [T, nn, 4] (NaN rows for dead bots)
    and the states' extras ext_cur / ext_last [K, 4] (zeros for None, as the state shows them)."""
    T, nn = stats.shape[:2]
    bots = [BotModel(p, table[k]) for k in range(nn)]
    f = {k: np.full((T, nn), np.nan) for k in ("last_mass", "cum_reward", "last_reward", "mem_reward")}
    out = dict(f, skip_frames=np.zeros((T, nn), np.int64), skipping=np.zeros((T, nn), np.uint8),
               mem_old=np.full((T, nn), -2, np.int64), mem_new=np.full((T, nn), -2, np.int64),
               mem_flag=np.zeros((T, nn), np.uint8), cmds=np.full((T, nn, 4), np.nan),
               **{k: np.full((T, nn, 4), np.nan) for k in ("cur_action", "last_action", "mem_action")})
    state_bot, state_tick, none_bot, none_tick, ext_cur, ext_last = [], [], [], [], [], []
    exp, n_exp = [], [0] * nn
    for t in range(T):
        for k, b in enumerate(bots):
            cmd, computed, state = b.move(t, stats[t, k])
            if cmd is not None:
                out["cmds"][t, k] = cmd
            if computed and state is None:
                none_bot.append(k)
                none_tick.append(t)
            elif computed:
                state_bot.append(k)
                state_tick.append(t)
                ext_cur.append(pad4(b.extras[0], 0.0))
                ext_last.append(pad4(b.extras[1], 0.0))
            out["last_mass"][t, k] = np.nan if b.last_mass is None else b.last_mass
            out["cum_reward"][t, k], out["last_reward"][t, k] = float(b.cum), float(b.last_reward)
            out["skip_frames"][t, k], out["skipping"][t, k] = b.skip_frames, b.skipping
            out["cur_action"][t, k], out["last_action"][t, k] = pad4(b.action), pad4(b.last_action)
            for e in b.experiences[n_exp[k]:]:
                exp.append((k,) + e)
            n_exp[k] = len(b.experiences)
            if b.memory is not None:
                m = b.memory
                out["mem_old"][t, k], out["mem_new"][t, k] = m[0], -1 if m[3] is None else m[3]
                out["mem_flag"][t, k], out["mem_reward"][t, k], out["mem_action"][t, k] = m[4], float(m[2]), pad4(m[1])
        if reset_after[t]:
            for b in bots:
                b.reset()
                b.experiences = []
            n_exp = [0] * nn
    out.update(state_bot=np.array(state_bot, np.int64), state_tick=np.array(state_tick, np.int64),
               none_bot=np.array(none_bot, np.int64), none_tick=np.array(none_tick, np.int64),
               ext_cur=np.array(ext_cur).reshape(-1, 4), ext_last=np.array(ext_last).reshape(-1, 4),
               exp_bot=np.array([e[0] for e in exp], np.int64), exp_tick=np.array([e[1] for e in exp], np.int64),
               exp_old=np.array([e[2] for e in exp], np.int64),
               exp_new=np.array([-1 if e[5] is None else e[5] for e in exp], np.int64),
               exp_action=np.array([pad4(e[3]) for e in exp]).reshape(-1, 4),
               exp_reward=np.array([float(e[4]) for e in exp]))
    return out


class Batched:
    """One decision of AgarVecEnv for n players (env.py step_calls), `nn` the indices of
    the NN players: at the window's first tick the action of every live NN player goes
    through set_command_point, is recorded (current -> last action) and the player's mass
    becomes its lastMass; on the skip further ticks the same action with split / eject
    dropped; after every tick the term updateRewards adds; then lastMass for the players
    alive at the end.  An NN player's window is one transition (old tick, the action row
    padded to 4, the summed reward, new tick or None, dead) if it had an old state.

    Against the reference's bots: a player alive at every tick of
    its window gives the bot's experience exactly.  A player that dies in the window and
    is still dead at its end gives the *last* of the experiences the bot emits in that
    window (the one of the window's last tick: same old state, action and cumulative
    reward, no new state); the bot's earlier ones, one per dead tick, are not emitted.
    The reward of every window starts at 0, where a bot that is dead when it would decide
    goes on adding to its cumulative reward; and a player dead at the start of a window
    has no old state, so that window emits nothing."""

    def __init__(self, p, n, nn=None):
        self.p, self.n = p, n
        self.nn = list(range(n)) if nn is None else [int(i) for i in nn]
        self.last_mass = [None] * n
        self.cur, self.prev = np.zeros((n, 4)), np.zeros((n, 4))
        self.old = [None] * n
        self.reward = np.zeros(n)
        self.act, self.terms = None, 0

    def reset_players(self, idx, t, stats):
        """Bot.reset for the players idx and their first states, observed at tick t."""
        for i in idx:
            self.last_mass[i], self.old[i] = None, (t if stats[i, 0] > 0 else None)
            self.cur[i] = 0

    def commands(self, k, stats, act=None):
        """Tick k of the window (0: the decision with the actions act [n, width]; > 0: a
        skipped frame) -> {player: command} of the live NN players."""
        p, out = self.p, {}
        if k == 0:
            self.act = np.array(act, np.float64)
            self.terms = 0
        else:  # updateRewards on a skipped frame
            self._rewards(stats)
        for i in self.nn:
            if not stats[i, 0] > 0:
                continue
            a = [float(v) for v in self.act[i]]
            if k > 0:
                a[2:] = [0, 0]
            out[i] = set_command_point(stats[i], a, p)
            if k == 0:
                self.prev[i] = self.cur[i]
                self.cur[i] = pad4(self.act[i], 0.0)
                self.last_mass[i] = float(stats[i, 1])
        return out

    def _rewards(self, stats):
        for i in range(self.n):
            r = float(reward_term_of_tick(bool(stats[i, 0] > 0), float(stats[i, 1]), self.last_mass[i], self.p))
            self.reward[i] = r if self.terms == 0 else self.reward[i] + r
        self.terms += 1

    def end(self, t, stats):
        """After the window's last tick (the observation's tick t) -> (reward [n], alive [n],
        transitions [(player, old tick, action row [4], reward, new tick or None, dead)] in
        ascending player order)."""
        self._rewards(stats)
        alive = stats[:, 0] > 0
        for i in range(self.n):
            if alive[i]:
                self.last_mass[i] = float(stats[i, 1])
        tr = []
        for i in self.nn:
            if self.old[i] is not None:
                tr.append((i, self.old[i], pad4(self.act[i], 0.0), float(self.reward[i]), t if alive[i] else None,
                           not alive[i]))
            self.old[i] = t if alive[i] else None
        return self.reward.copy(), alive.copy(), tr
