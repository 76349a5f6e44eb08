#!/usr/bin/env python3
"""Golden vectors for the learner glue: what a learner is handed after a tick.

CPU-ONLY TEST INFRASTRUCTURE, on the model of gen_golden.py (whose reference import,
pygame stub, canonical-order shims, parameter copy and snapshot it reuses): this script
imports the read-only reference and drives its own `Model` with its own NN `Bot`s among
Greedy and Random bots.  It writes `tests/golden/learner_*.npz`, numbers only.

The NN bots carry a stub learning algorithm (`discrete`, `__str__`, `reset`,
`decideMove`) whose decideMove returns the rows of a pre-drawn action table indexed by
(bot, decision number); the table is in the fixture, so no action depends on the bits of
an observation.  About a tenth of the table's values are exactly 0, 0.5 or 1 - 2^-53.

Cadence (aigar.py:795-887): `Model.initialize`, then `windows` collector windows of
FRAME_SKIP_RATE + 2 updates each followed by `Model.resetBots`, then one long run without
resetBots, in which skip windows cross deaths and respawns.  `Model.update` is issued as
its two halves (`takeBotActions`, `field.update`; model.py:100-106 with the GUI off and no
humans) so that the commands and numpy's stream position can be recorded between them.

Not recorded: the width-3 branch of set_command_point with ENABLE_SPLIT off.  It cannot
run in the reference -- bot.py:568 compares the list `[3]` with a float, a TypeError in
Python 3.  And the reference's Random bots divide by FRAME_SKIP_RATE (bot.py:244), so the
scenario with FRAME_SKIP_RATE 0 has Greedy bots only beside the NN bots.

File layout (T ticks, n players, nn NN bots, L values per state; tick t is the t-th
update, counted from 0: its makeMove sees the world after t field updates):
  the gen_golden.py layout: n_players, size, max_pellets, max_viruses, virus_enabled,
  obs_channels, obs_extras, obs_len, obs_grids, grid_squares, ticks, init/*, ck<t>/*,
  ck_ticks, cmds [T, n, 4], mt_keys, mt_pos, events, events_off, digest_i
  roles [n]              0 NN, 1 Greedy, 2 Random;  nn_players [nn] their player indices
  frame_skip, width, enable_split, enable_eject, mass_as_reward, reward_term,
  reward_scale, death_factor, death_term        scalars
  table [nn, T, width]   the action table (row k: the bot's k-th decision)
  reset_after [T]        1 where Model.resetBots followed the tick's field update
  stats [T, n, 5]        alive, total mass, fov x, fov y, fov size of every player as the
                         tick's makeMove read them (fov NaN for a dead player)
  after the tick's makeMove, per NN bot:
  last_mass [T, nn]      NaN for None;   cum_reward, last_reward [T, nn]
  skip_frames [T, nn]    int;   skipping [T, nn]   currentlySkipping
  cur_action, last_action [T, nn, 4]     NaN for None and past the width
  states [K, L], state_bot [K], state_tick [K]   every state a bot computed, once each
  none_bot [K0], none_tick [K0]          getStateRepresentation calls that returned None
  exp_bot, exp_tick, exp_old, exp_new [E]   the experiences in order of emission: the
                         bot, the tick it was appended at, the ticks of its old and new
                         state (new -1: None);  exp_action [E, 4], exp_reward [E]
  mem_old, mem_new [T, nn]   lastMemory's states as ticks (-2: lastMemory is None, new -1:
                         None); mem_flag [T, nn] its last field (`newState is not None`),
                         mem_reward [T, nn] (NaN for None), mem_action [T, nn, 4]

Usage:  python tools/golden/gen_learner_golden.py [--out tests/golden] [--only NAME]
"""
import argparse
import os
import random
import sys
import tracemalloc

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg  # noqa: E402

ROLE = {"NN": 0, "Greedy": 1, "Random": 2}
EDGES = (0.0, 0.5, 1.0 - 2.0 ** -53)

_MIX = ["NN", "Greedy", "NN", "Random", "NN", "Greedy", "NN", "Greedy", "NN", "Random", "NN", "Greedy", "Greedy", "NN",
        "Random", "NN"]
_NO_RANDOM = ["NN", "Greedy"] * 8
_REWARD = dict(REWARD_TERM=0.3, REWARD_SCALE=0.3, DEATH_FACTOR=1.7, DEATH_TERM=-40.5)
_BOOST = (300.0, 220.0, 160.0, 120.0, 90.0)  # masses of the first Greedy bots: they hunt from the first tick

# 16 players on a field of 152 with viruses; the seeds were chosen among 20 .. 39 for NN bots that die in the
# collector windows and in the long run
SCENARIOS = {
    # width 4, 3 skipped frames, mass differences as reward, both action extras
    "learner_w4_s3": dict(roles=_MIX, skip=3, width=4, split=True, eject=True, mar=False, last=True, second=True,
                          windows=6, ticks=110, seed=23),
    # width 3 (ENABLE_SPLIT on), 7 skipped frames, the mass as reward, the last action only
    "learner_w3_s7": dict(roles=_MIX, skip=7, width=3, split=True, eject=False, mar=True, last=True, second=False,
                          windows=4, ticks=120, seed=30),
    # width 2, no frame skip (no Random bots: bot.py:244), mass differences, both action extras
    "learner_w2_s0": dict(roles=_NO_RANDOM, skip=0, width=2, split=False, eject=False, mar=False, last=True,
                          second=True, windows=10, ticks=70, seed=24),
    # width 4, 7 skipped frames, the mass as reward, no action extras
    "learner_w4_s7_mass": dict(roles=_MIX, skip=7, width=4, split=True, eject=True, mar=True, last=False,
                               second=False, windows=4, ticks=120, seed=33),
}


class TableLearner:
    """The stub learning algorithm: the k-th decision is row k of the bot's table."""
    discrete = False

    def __init__(self, rows):
        self.rows, self.k = rows, 0

    def __str__(self):
        return "AC"

    def reset(self):
        pass

    def decideMove(self, state):
        row = [float(v) for v in self.rows[self.k]]
        self.k += 1
        return None, row


def action_table(rng, nn, T, width):
    tab = rng.random((nn, T, width))
    edge = rng.random(tab.shape) < 0.1
    tab[edge] = rng.choice(EDGES, int(edge.sum()))
    return tab


def pad4(a):
    out = np.full(4, np.nan)
    if a is not None:
        out[:len(a)] = [float(v) for v in a]
    return out


def run_scenario(ref, rec, sc):
    roles = sc["roles"]
    n, T = len(roles), sc["ticks"]
    mf = ref.field
    mf.SIZE_INCREASE_PER_PLAYER = 38
    mf.MAX_COLLECTIBLE_DENSITY = 0.015
    mf.MAX_VIRUS_DENSITY = 4e-4
    over = dict(GRID_SQUARES_PER_FOV=5, SELF_GRID=True, SELF_GRID_LF=True, ENEMY_GRID_LF=True,
                USE_LAST_FOVSIZE=True, USE_LAST_ACTION=sc["last"], USE_SECOND_LAST_ACTION=sc["second"],
                FRAME_SKIP_RATE=sc["skip"], MASS_AS_REWARD=sc["mar"], GATHER_EXP=True, **_REWARD)
    params = gg.make_params(ref, n, True, sc["split"], sc["eject"], over)
    params.ENABLE_GREEDY_SPLIT = False
    model = ref.model.Model(False, False, params)
    tracemalloc.stop()
    np.random.seed(sc["seed"])
    random.seed(sc["seed"])
    rec.seq = 0
    nn_players = [i for i, r in enumerate(roles) if r == "NN"]
    nn = len(nn_players)
    table = action_table(np.random.default_rng(2000 + sc["seed"]), nn, T, sc["width"])
    for i, r in enumerate(roles):
        model.createBot(r, TableLearner(table[nn_players.index(i)]) if r == "NN" else None, params)
    model.initialize()
    field = model.field
    for pi, m in zip([i for i, r in enumerate(roles) if r == "Greedy"], _BOOST):
        field.players[pi].cells[0].setMass(m)
    bots = [b for b in model.bots if b.type == "NN"]
    assert [field.players.index(b.player) for b in bots] == nn_players
    bot_of = {id(b): k for k, b in enumerate(bots)}

    ch_mask, ex_mask = gg.obs_masks(params)
    L = params.STATE_REPR_LEN
    out = {
        "n_players": np.int64(n), "size": np.int64(field.size),
        "max_pellets": np.float64(field.maxCollectibleCount), "max_viruses": np.float64(field.maxVirusCount),
        "virus_enabled": np.int64(int(field.virusEnabled)),
        "obs_channels": np.int64(ch_mask), "obs_extras": np.int64(ex_mask), "obs_len": np.int64(L),
        "obs_grids": np.int64(params.NUM_OF_GRIDS), "grid_squares": np.int64(params.GRID_SQUARES_PER_FOV),
        "ticks": np.int64(T),
        "roles": np.array([ROLE[r] for r in roles], np.uint8), "nn_players": np.array(nn_players, np.int64),
        "frame_skip": np.int64(sc["skip"]), "width": np.int64(sc["width"]),
        "enable_split": np.int64(sc["split"]), "enable_eject": np.int64(sc["eject"]),
        "mass_as_reward": np.int64(sc["mar"]), "reward_term": np.float64(params.REWARD_TERM),
        "reward_scale": np.float64(params.REWARD_SCALE), "death_factor": np.float64(params.DEATH_FACTOR),
        "death_term": np.float64(params.DEATH_TERM), "table": table,
    }
    for k, v in gg.snapshot(field).items():
        out["init/" + k] = v
    out["init/seq_next"] = np.int64(rec.seq)
    out["init/mt_key"], pos = gg.mt_state()
    out["init/mt_pos"] = np.int64(pos)

    # every state a bot computes, through the bot's own call in move_NN
    Bot = ref.bot.Bot
    tick = [0]
    states, state_bot, state_tick, none_bot, none_tick, tick_of, keep = [], [], [], [], [], {}, []
    orig_state = Bot.getStateRepresentation

    def get_state(self):
        s = orig_state(self)
        if s is None:
            none_bot.append(bot_of[id(self)])
            none_tick.append(tick[0])
        else:
            states.append(np.asarray(s, np.float64).reshape(-1).copy())
            state_bot.append(bot_of[id(self)])
            state_tick.append(tick[0])
            tick_of[id(s)] = tick[0]
            keep.append(s)  # (the id stays this object's)
        return s
    Bot.getStateRepresentation = get_state

    def when(s):
        return -1 if s is None else tick_of[id(s)]

    cmds = np.zeros((T, n, 4))
    mt_keys, mt_pos = np.zeros((T, 624), np.uint32), np.zeros(T, np.int64)
    stats = np.zeros((T, n, 5))
    f2 = {k: np.full((T, nn), np.nan) for k in ("last_mass", "cum_reward", "last_reward", "mem_reward")}
    skip_frames, skipping = np.zeros((T, nn), np.int64), np.zeros((T, nn), np.uint8)
    mem_old, mem_new = np.full((T, nn), -2, np.int64), np.full((T, nn), -2, np.int64)
    mem_flag = np.zeros((T, nn), np.uint8)
    cur_a, last_a, mem_a = (np.full((T, nn, 4), np.nan) for _ in range(3))
    exp = {k: [] for k in ("bot", "tick", "old", "new", "action", "reward")}
    n_exp = [0] * nn
    reset_after = np.zeros(T, np.uint8)
    window = sc["skip"] + 2
    ev_rows, ev_off, dig_i, ck_ticks = [], [0], [], []
    try:
        for t in range(T):
            tick[0] = t
            for i, p in enumerate(field.players):
                alive = p.getIsAlive()
                stats[t, i, :2] = (float(alive), float(p.getTotalMass()))
                if alive:
                    fp = p.getFovPos()
                    stats[t, i, 2:] = (float(fp[0]), float(fp[1]), float(p.getFovSize()))
                else:
                    stats[t, i, 2:] = np.nan
            model.counter += 1
            model.takeBotActions()
            for i, p in enumerate(field.players):
                cmds[t, i] = (float(p.commandPoint[0]), float(p.commandPoint[1]), float(bool(p.doSplit)),
                              float(bool(p.doEject)))
            for k, b in enumerate(bots):
                f2["last_mass"][t, k] = np.nan if b.lastMass is None else float(b.lastMass)
                f2["cum_reward"][t, k], f2["last_reward"][t, k] = float(b.cumulativeReward), float(b.lastReward)
                skip_frames[t, k], skipping[t, k] = b.skipFrames, bool(b.currentlySkipping)
                cur_a[t, k], last_a[t, k] = pad4(b.currentAction), pad4(b.lastAction)
                for e in b.experiences[n_exp[k]:]:
                    exp["bot"].append(k)
                    exp["tick"].append(t)
                    exp["old"].append(when(e[0]))
                    exp["new"].append(when(e[3]))
                    exp["action"].append(pad4(e[1]))
                    exp["reward"].append(float(e[2]))
                n_exp[k] = len(b.experiences)
                m = b.lastMemory
                if m is not None:
                    mem_old[t, k], mem_new[t, k], mem_flag[t, k] = when(m[0][0]), when(m[3][0]), bool(m[4][0])
                    f2["mem_reward"][t, k], mem_a[t, k] = float(m[2][0]), pad4(m[1][0])
            mt_keys[t], mt_pos[t] = gg.mt_state()
            rec.events = []
            field.update()
            ev_rows.extend(rec.events)
            ev_off.append(len(ev_rows))
            dig_i.append(gg.digest(field)[0])
            if t + 1 <= sc["windows"] * window and (t + 1) % window == 0:
                model.resetBots()
                reset_after[t] = 1
                n_exp = [0] * nn
            if t + 1 == sc["windows"] * window or t == T - 1:
                ck_ticks.append(t + 1)
                for k, v in gg.snapshot(field).items():
                    out["ck%d/%s" % (t + 1, k)] = v
                out["ck%d/seq_next" % (t + 1)] = np.int64(rec.seq)
                kk, pp = gg.mt_state()
                out["ck%d/mt_key" % (t + 1)], out["ck%d/mt_pos" % (t + 1)] = kk, np.int64(pp)
    finally:
        Bot.getStateRepresentation = orig_state
    out.update(cmds=cmds, mt_keys=mt_keys, mt_pos=mt_pos, events=np.array(ev_rows, np.int64).reshape(-1, 3),
               events_off=np.array(ev_off, np.int64), digest_i=np.array(dig_i, np.int64),
               ck_ticks=np.array(ck_ticks, np.int64), reset_after=reset_after, stats=stats, skip_frames=skip_frames,
               skipping=skipping, cur_action=cur_a, last_action=last_a, mem_old=mem_old, mem_new=mem_new,
               mem_flag=mem_flag, mem_action=mem_a, **f2)
    out.update(states=np.array(states, np.float64).reshape(-1, L), state_bot=np.array(state_bot, np.int64),
               state_tick=np.array(state_tick, np.int64), none_bot=np.array(none_bot, np.int64),
               none_tick=np.array(none_tick, np.int64))
    out.update(exp_bot=np.array(exp["bot"], np.int64), exp_tick=np.array(exp["tick"], np.int64),
               exp_old=np.array(exp["old"], np.int64), exp_new=np.array(exp["new"], np.int64),
               exp_action=np.array(exp["action"], np.float64).reshape(-1, 4), exp_reward=np.array(exp["reward"]))
    alive_nn = stats[:, nn_players, 0] > 0
    info = dict(deaths=int((alive_nn[:-1] & ~alive_nn[1:]).sum()), states=len(states), experiences=len(exp["bot"]),
                terminal=int((out["exp_new"] < 0).sum()), skipped=int(skipping.sum()))
    return out, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests",
                                                  "golden"))
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    ref = gg.import_reference()
    rec = gg.Recorder()
    gg.install_shims(ref, rec)
    for name, sc in SCENARIOS.items():
        if args.only not in (None, name):
            continue
        out, info = run_scenario(ref, rec, sc)
        path = os.path.join(args.out, name + ".npz")
        np.savez_compressed(path, **out)
        print(name, os.path.getsize(path), "bytes;", info, flush=True)


if __name__ == "__main__":
    main()
