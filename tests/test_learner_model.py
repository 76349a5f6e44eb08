"""Pin the learner-glue model (tests/learner_model.py) to the reference's own NN bots.

The fixtures tests/golden/learner_*.npz were recorded from the reference's Model and Bot
objects (tools/golden/gen_learner_golden.py: a stub learner answering from an action
table, the collector's windows with resetBots, then a long run across deaths).  Here:
  * the per-bot model, fed the recorded (alive, mass, fov) stream, equals every recorded
    value bit for bit: commands, lastMass, the cumulative and last reward, skipFrames,
    currentlySkipping, both actions, which states were computed, the experience list and
    lastMemory;
  * the MT-mode oracle, replaying the recorded commands from the recorded start, gives
    that stream, and observe_one at the recorded ticks gives the recorded states -- which
    ties when a state is computed to the history frames it carries;
  * the batched view (one transition per decision window) is derived from the same record:
    equal to the bot's experience at the end of every window it decided at the start of,
    deaths included; the bot's extra experiences are exactly the ones DESIGN.md section 4b
    lists as not emitted;
  * the Philox worlds of tests/test_gpu_learner.py hold, on the oracle alone, the deaths
    and respawns those tests are about.
"""
import os

import numpy as np
import pytest

from aigar_amd import _abi
from oracle_lib import golden_state
import learner_model as lm
import learner_worlds as lw
from shapes import bits_diff, obs_bits_equal
from test_oracle_golden import _same, oracle_for

FIXTURES = ["learner_w4_s3", "learner_w3_s7", "learner_w2_s0", "learner_w4_s7_mass"]
FLOATS = ("last_mass", "cum_reward", "last_reward", "cur_action", "last_action", "exp_action", "exp_reward",
          "mem_reward", "mem_action")
INTS = ("skip_frames", "skipping", "state_bot", "state_tick", "none_bot", "none_tick", "exp_bot", "exp_tick", "exp_old",
        "exp_new", "mem_old", "mem_new", "mem_flag")


def load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + ".npz"), allow_pickle=False)


def model_record(z):
    return lm.run_bots(lm.params_of(z), z["stats"][:, z["nn_players"]], z["table"], z["reset_after"])


@pytest.mark.parametrize("name", FIXTURES)
def test_bot_model_equals_the_reference_bots(name, golden_dir):
    z = load(golden_dir, name)
    got = model_record(z)
    for k in FLOATS:
        assert obs_bits_equal(got[k], z[k]), "%s: %s" % (k, bits_diff(got[k].reshape(len(got[k]), -1),
                                                                       z[k].reshape(len(z[k]), -1)))
    for k in INTS:
        assert np.array_equal(got[k], z[k]), k
    # the commands the bots set (bot.py:550-577); a dead bot sets none
    want = z["cmds"][:, z["nn_players"]]
    live = ~np.isnan(got["cmds"][:, :, 0])
    assert np.array_equal(live, z["stats"][:, z["nn_players"], 0] > 0)
    assert obs_bits_equal(got["cmds"][live], want[live]), bits_diff(got["cmds"][live], want[live])


def test_fixtures_cover_the_parameter_matrix(golden_dir):
    """Frame skip 0 / 3 / 7, widths 2 / 3 / 4, both reward modes, the action extras with and
    without the second-last action, no exact reward arithmetic; and the reference's quirks."""
    zs = [load(golden_dir, n) for n in FIXTURES]
    assert {int(z["frame_skip"]) for z in zs} == {0, 3, 7}
    assert {int(z["width"]) for z in zs} == {2, 3, 4}
    assert {int(z["mass_as_reward"]) for z in zs} == {0, 1}
    extras = {int(z["obs_extras"]) & (_abi.EX_LAST_ACT | _abi.EX_2LAST_ACT) for z in zs}
    assert extras >= {_abi.EX_LAST_ACT, _abi.EX_LAST_ACT | _abi.EX_2LAST_ACT}
    for z in zs:
        assert int(z["grid_squares"]) == 5 and 12 <= int(z["n_players"]) <= 16 and 150 <= int(z["size"]) <= 300
        assert int(z["ticks"]) <= 120 and int(z["virus_enabled"]) == 1
        for k in ("reward_term", "reward_scale", "death_factor"):
            m, _ = np.frexp(float(z[k]))
            assert float(z[k]) != 0 and m * 2 ** 20 != int(m * 2 ** 20), k  # no short binary fraction
        assert float(z["death_term"]) % 1 != 0  # (added to lastMass * DEATH_FACTOR: that sum rounds)
        tab = z["table"]
        assert all((tab == e).any() for e in (0.0, 0.5, 1.0 - 2.0 ** -53))
        alive = z["stats"][:, z["nn_players"], 0] > 0
        skipping = z["skipping"].astype(bool)
        # a bot that is dead does not skip, and emits an experience without a new state
        assert not (skipping & ~alive).any()
        assert (z["exp_new"] < 0).sum() >= 5
        if int(z["frame_skip"]) > 0:
            # deaths inside a skip window: skipFrames still counting at a dead tick
            assert ((z["skip_frames"] > 0) & ~alive).any()
        # rewarded alive against the lastMass from before the death: lastMass unchanged over a respawn
        back = alive[1:] & ~alive[:-1]
        assert back.sum() >= 5


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_gives_the_recorded_stream_and_states(name, golden_dir):
    z = load(golden_dir, name)
    got = model_record(z)
    nn = z["nn_players"]
    n = int(z["n_players"])
    o = oracle_for(z)
    o.load_state(golden_state(z, "init"))
    cks = set(int(t) for t in z["ck_ticks"])
    by_tick = {}
    for k, (b, t) in enumerate(zip(z["state_bot"], z["state_tick"])):
        by_tick.setdefault(int(t), []).append((k, int(b)))
    ev, off = z["events"], z["events_off"]
    checked = 0
    for t in range(int(z["ticks"])):
        assert obs_bits_equal(o.player_stats(), z["stats"][t]), "tick %d: %s" % (t, bits_diff(o.player_stats(),
                                                                                             z["stats"][t]))
        for k, b in by_tick.get(t, []):
            cur, prev = np.zeros((n, 4)), np.zeros((n, 4))
            cur[nn[b]], prev[nn[b]] = got["ext_cur"][k], got["ext_last"][k]
            o.set_actions(cur, prev)
            row = o.observe_one(int(nn[b]))
            assert obs_bits_equal(row, z["states"][k]), "state of bot %d at tick %d: %s" % (
                b, t, bits_diff(row[None], z["states"][k][None]))
            checked += 1
        o.set_commands(z["cmds"][t])
        o.set_mt(z["mt_keys"][t], z["mt_pos"][t])
        o.step(1)
        assert _same(o.events()[:, 1:], ev[off[t]:off[t + 1]]), "event log differs at tick %d" % t
        if z["reset_after"][t]:
            mask = np.zeros(n, np.uint8)
            mask[nn] = 1
            o.reset_bots(mask)
        if (t + 1) in cks:
            st = o.get_state()
            for k in _abi.LAYOUT:
                if k in _abi.OPTIONAL and "ck%d/%s" % (t + 1, k) not in z.files:
                    continue
                assert _same(st[k], z["ck%d/%s" % (t + 1, k)]), "%s differs at tick %d" % (k, t + 1)
    assert checked == len(z["states"]) > 100
    o.close()


def batched_window(p, stats, act, t0):
    """The batched view of one player's window starting at tick t0 of the recorded stream
    stats [T, 5] -> (commands per tick, reward, transition)."""
    b = lm.Batched(p, 1)
    b.reset_players([0], t0, stats[t0:t0 + 1])
    cmds = [b.commands(k, stats[t0 + k:t0 + k + 1], act[None] if k == 0 else None).get(0)
            for k in range(p.frame_skip + 1)]
    te = t0 + p.frame_skip + 1
    reward, alive, tr = b.end(te, stats[te:te + 1])
    return cmds, reward[0], tr[0]


@pytest.mark.parametrize("name", FIXTURES)
def test_batched_view_against_the_reference_experiences(name, golden_dir):
    """Every experience of the record is one of: the one at the end of a window the bot decided
    at the start of -- the batched transition, exactly, deaths and respawns inside included; one
    without a new state from a dead tick inside such a window; or one from a bot that was dead
    when its window ended, until it decides again.  The last two kinds are not emitted by the
    batched path."""
    z = load(golden_dir, name)
    p = lm.params_of(z)
    nn, T, W = z["nn_players"], int(z["ticks"]), int(z["frame_skip"]) + 1
    resets = np.nonzero(z["reset_after"])[0]
    exp = {(int(b), int(t)): k for k, (b, t) in enumerate(zip(z["exp_bot"], z["exp_tick"]))}
    assert len(exp) == len(z["exp_bot"])  # (a bot emits at most one per tick)
    kinds = {"end": 0, "end_dead": 0, "end_after_death": 0, "inside": 0, "late": 0}
    matched = set()
    decisions = np.zeros((T, len(nn)), bool)
    decisions[z["state_tick"], z["state_bot"]] = True  # a live bot that computes a state decides
    for b in range(len(nn)):
        stats = z["stats"][:, nn[b]]
        n_dec = 0
        for t0 in range(T):
            if not decisions[t0, b]:
                continue
            act = z["table"][b, n_dec]
            n_dec += 1
            te = t0 + W
            if te >= T or ((resets >= t0) & (resets < te)).any():
                continue
            cmds, reward, tr = batched_window(p, stats, act, t0)
            k = exp[(b, te)]
            matched.add(k)
            alive = stats[t0:te + 1, 0] > 0
            assert int(z["exp_old"][k]) == t0 == tr[1]
            assert int(z["exp_new"][k]) == (te if alive[-1] else -1) == (-1 if tr[4] is None else tr[4])
            assert tr[5] == (not alive[-1])
            assert obs_bits_equal(np.array([reward, tr[3]]), np.array([z["exp_reward"][k]] * 2)), (b, t0, reward,
                                                                                                z["exp_reward"][k])
            assert obs_bits_equal(tr[2], np.nan_to_num(z["exp_action"][k], nan=0.0))
            for j, c in enumerate(cmds):  # the window's commands are the bot's
                if c is not None:
                    assert obs_bits_equal(np.array(c), z["cmds"][t0 + j, nn[b]]), (b, t0, j)
            kinds["end_dead" if not alive[-1] else "end" if alive.all() else "end_after_death"] += 1
    old, tick, new = z["exp_old"], z["exp_tick"], z["exp_new"]
    for k in range(len(old)):
        if k in matched:
            continue
        d = int(tick[k] - old[k])
        t_reset = ((resets >= old[k]) & (resets < tick[k])).any()
        assert not t_reset  # (resetBots clears the old state)
        if d < W:
            assert new[k] == -1  # a dead tick inside the window
            kinds["inside"] += 1
        elif d > W:
            b = int(z["exp_bot"][k])
            assert not z["stats"][old[k] + W, nn[b], 0] > 0  # dead when the window ended
            kinds["late"] += 1
        else:
            raise AssertionError("experience %d at the end of a window was not compared" % k)
    print(name, kinds)
    # (a bot is dead for one tick, so without skipped frames every death is seen at a window's end)
    assert kinds["end"] >= 50 and kinds["end_dead"] >= 1, kinds
    if W > 1:
        assert kinds["inside"] >= 5 and kinds["end_after_death"] >= 5, kinds
    else:
        assert kinds["late"] >= 1, kinds


@pytest.mark.parametrize("m", lw.MATRIX, ids=lw.MATRIX_IDS)
@pytest.mark.parametrize("shape", lw.SHAPES, ids=lw.SHAPE_IDS)
def test_gpu_test_worlds_hold_what_they_need(shape, m):
    """On the oracle alone: the worlds of test_gpu_learner.py's decision tests see at least 5
    deaths inside skip windows, a death on a decision tick, and 5 respawns rewarded against the
    old lastMass (Need.check).  No world can hold a bot dead for a whole window: a player
    respawns one tick after its death (Player.stepsUntilRespawn = 1), so makeMove sees it dead
    once, and a window has at least two ticks' views."""
    p = lw.model_params(m)
    w = lw.World(shape, p)
    b = lm.Batched(p, w.NP, w.nn)
    lw.begin(w, b)
    need = lw.Need(p.frame_skip)
    table = lw.action_table(lw.SEED, w.NP, lw.n_decisions(shape, p), p.width)
    n_tr = n_dead = 0
    for d, st, obs, reward, alive, tr in lw.decisions(w, b, table, need):
        n_tr += len(tr)
        n_dead += sum(1 for x in tr if x[5])
    need.check()
    assert need.dead_window == 0
    assert n_dead >= 1 and n_tr > 100, (n_tr, n_dead)
    w.close()


def test_gpu_test_worlds_cover_every_width_and_mode():
    assert {m[0] for m in lw.MATRIX} == {0, 3, 7} and {m[1] for m in lw.MATRIX} == {2, 3, 4}
    assert {m[4] for m in lw.MATRIX} == {False, True}
    assert (3, False) in {(m[1], m[2]) for m in lw.MATRIX}  # 3 values with ENABLE_SPLIT (and ENABLE_EJECT) off
