"""GPU: the learner glue against tests/learner_model.py, bit for bit.

learner_model.py is pinned to the reference's own NN bots on the CPU
(test_learner_model.py); here it is the oracle of `aigar_apply_actions`, `aigar_rewards`,
the decision graph (`aigar_env_step`, `AgarVecEnv.step`, with the replay memory's rows) and
the facade's NN bots.  The worlds are Philox worlds of learner_worlds.py -- NN players
among Greedy and Random bots, matured so that players die from the first ticks -- with
the CPU oracle in lockstep: it supplies every tick's (alive, mass, fov) stream and the
states, and its event logs and final world must equal the device's.  Every comparison of
floats is by bit pattern (shapes.obs_bits_equal: NaN where NaN, signed zeros apart)."""
import numpy as np
import pytest

from aigar_amd import _abi
from oracle_lib import Oracle
import learner_model as lm
import learner_worlds as lw
import parity
import shapes
from shapes import bits_diff, obs_bits_equal

pytestmark = pytest.mark.gpu
_lib = pytest.importorskip("aigar_amd._lib")

EDGES = (0.0, 0.5, 1.0 - 2.0 ** -53)


def device(shape, w, p):
    """A stepper in the world w's start state with its roles and the Random bots' keying."""
    g = _lib.Stepper(lw.config(shape))
    g.reset(lw.SEED)
    lw.mature(g, w.A, lw.SEED)
    configure(g, w, p)
    return g


def configure(g, w, p):
    g.set_roles(w.roles)
    g.env_config(greedy_split=True, random_skip=max(1, p.frame_skip), random_split=p.enable_split,
                 random_eject=p.enable_eject, salt=w.salt)
    for a in range(w.A):
        assert parity.diff_states(g.get_state(a), w.o.get_state(a), ftol=0.0) == []


def same(got, want, what):
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert obs_bits_equal(got, want), "%s: %s" % (what, bits_diff(got.reshape(len(got), -1),
                                                                   want.reshape(len(want), -1)))


def other_roles_move(g, w):
    g.policy_greedy(True, (w.roles == _abi.ROLE_GREEDY).astype(np.uint8))
    g.policy_random_bots()


def same_events(g, w, what):
    for a in range(w.A):
        assert np.array_equal(g.events(a), w.o.events(a)), "%s: events of arena %d differ" % (what, a)


def same_worlds(g, w):
    for a in range(w.A):
        assert parity.diff_states(g.get_state(a), w.o.get_state(a), ftol=0.0) == [], "arena %d" % a


# (width, ENABLE_SPLIT, ENABLE_EJECT): every width, 3 values where the reference defines them
WIDTHS = [(2, False, False), (3, True, False), (3, False, False), (4, True, True), (4, False, False)]


@pytest.mark.parametrize("width,split,eject", WIDTHS, ids=["w%d-split%d" % (w, s) for w, s, _ in WIDTHS])
@pytest.mark.parametrize("shape", lw.SHAPES, ids=lw.SHAPE_IDS)
def test_apply_actions(shape, width, split, eject):
    """aigar_apply_actions against set_command_point and updateValues (bot.py:550-577, 180-193,
    266-267): skipping and record both ways, the commands of the live NN players, everybody
    else's command untouched (dead players, Greedy and Random bots), both action extras in the
    next observation -- with actions exactly 0, 0.5 and 1 - 2^-53 among them."""
    p = lm.params(3, width, split, eject, **lw.REWARD)
    w = lw.World(shape, p)
    g = device(shape, w, p)
    ticks = 12 * shape[4]
    table = lw.action_table(lw.SEED + width, w.NP, ticks, width)
    cur, prev = np.zeros((w.NP, 4)), np.zeros((w.NP, 4))
    L = g.obs_len
    edges = {e: 0 for e in EDGES}
    n_dead = n_split = n_dropped = 0
    for t in range(ticks):
        skipping, record = bool(t & 1), bool(t & 2)
        stats = w.stats()
        act = table[t]
        want = shapes.commands(g, w.A)
        nn_cmds = {}
        for i in w.nn:
            if not stats[i, 0] > 0:
                n_dead += 1
                continue
            a = [float(v) for v in act[i]]
            for e in EDGES:
                edges[e] += a.count(e)
            if skipping:
                n_dropped += sum(v > 0.5 for v in a[2:])
                a[2:] = [0, 0]
            want[i] = nn_cmds[i] = lm.set_command_point(stats[i], a, p)
            n_split += int(want[i][2] + want[i][3])
            if record:
                prev[i] = cur[i]
                cur[i] = lm.pad4(act[i], 0.0)
        g.apply_actions(act, enable_split=split, skipping=skipping, record=record)
        same(shapes.commands(g, w.A), want, "commands at tick %d" % t)
        obs = g.observe()
        live = [i for i in w.nn if stats[i, 0] > 0]
        same(obs[live, L - 8:L - 4], cur[live], "last action at tick %d" % t)
        same(obs[live, L - 4:], prev[live], "second-last action at tick %d" % t)
        other_roles_move(g, w)
        played = w.tick(stats, nn_cmds)
        same(shapes.commands(g, w.A), played, "every role's commands at tick %d" % t)
        g.step(1)
        same_events(g, w, "tick %d" % t)
    same_worlds(g, w)
    assert all(n > 0 for n in edges.values()), edges
    assert n_dead >= 1, "no NN player was dead when the actions came"
    if width > 2 and (split or width == 4):
        assert n_split >= 5 and n_dropped >= 5, (n_split, n_dropped)
    else:
        assert n_split == 0
    g.close()
    w.close()


@pytest.mark.parametrize("mar", [False, True], ids=["mass-difference", "mass-as-reward"])
@pytest.mark.parametrize("shape", lw.SHAPES, ids=lw.SHAPE_IDS)
def test_rewards(shape, mar):
    """aigar_rewards against Bot.getReward (bot.py:654-667) for every player, with and without
    update_last, with no exact operation in it (REWARD_TERM 0.3, REWARD_SCALE 0.3, DEATH_FACTOR
    1.7, DEATH_TERM -40.5): NaN where the reference has None, the death branch, and lastMass set
    by a decision (aigar_apply_actions with record) and by update_last."""
    p = lm.params(0, 4, True, True, mar, **lw.REWARD)
    prm = lm.reward_namespace(p)
    w = lw.World(shape, p)
    g = device(shape, w, p)
    ticks = 60 * shape[4]
    table = lw.action_table(lw.SEED, w.NP, ticks, 4)
    last = [None] * w.NP
    n_none = n_death = n_alive = n_stale = 0
    for t in range(ticks):
        record = t >= 3 and t % 3 == 0  # a decision: the live NN players get a lastMass
        stats = w.stats()
        nn_cmds = {}
        for i in w.nn:
            if stats[i, 0] > 0:
                a = [float(v) for v in table[t, i]]
                if not record:
                    a[2:] = [0, 0]
                nn_cmds[i] = lm.set_command_point(stats[i], a, p)
                if record:
                    last[i] = float(stats[i, 1])
        g.apply_actions(table[t], enable_split=True, skipping=not record, record=record)
        other_roles_move(g, w)
        w.tick(stats, nn_cmds)
        g.step(1)
        same_events(g, w, "tick %d" % t)
        st = w.stats()
        update = t >= 6 and t % 4 == 1
        want = np.full(w.NP, np.nan)
        for i in range(w.NP):
            alive = bool(st[i, 0] > 0)
            r = lm.get_reward(alive, float(st[i, 1]), last[i], p)
            if r is None:
                n_none += 1
            else:
                want[i] = r
            if last[i] is not None:
                n_death += not alive
                n_alive += alive
                n_stale += alive and not stats[i, 0] > 0  # alive again, against the lastMass from before
            if update and alive:
                last[i] = float(st[i, 1])
        same(g.rewards(prm, update_last=update), want, "rewards at tick %d (update_last %s)" % (t, update))
    same_worlds(g, w)
    assert (n_none == 0) if mar else (n_none > w.NP), n_none
    assert n_death >= 5 and n_stale >= 5 and n_alive > 10 * w.NP, (n_death, n_stale, n_alive)
    g.close()
    w.close()


def gather(stepper, n, row_shape, dtype):
    """The first n rows of the replay ring as numpy (s, a, r, s2, done)."""
    import torch
    s = torch.zeros((n,) + tuple(row_shape), dtype=dtype, device="cuda")
    s2 = torch.zeros_like(s)
    a = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    r = torch.zeros(n, dtype=torch.float64, device="cuda")
    dn = torch.zeros(n, dtype=torch.uint8, device="cuda")
    stepper.exp_gather(torch.arange(n, device="cuda"), s=s, a=a, r=r, s2=s2, done=dn)
    return [x.cpu().numpy() for x in (s, a, r, s2, dn)]


@pytest.mark.parametrize("via", ["env-float64", "abi-float32"])
@pytest.mark.parametrize("m", lw.MATRIX, ids=lw.MATRIX_IDS)
@pytest.mark.parametrize("shape", lw.SHAPES, ids=lw.SHAPE_IDS)
def test_decisions(shape, m, via):
    """One graph replay per decision against the batched view (learner_model.Batched): the
    window's reward, who is alive, the state rows with their action extras, and the
    (s, a, r, s2, done) rows the decision appends to the replay memory.  env-float64:
    AgarVecEnv.step with memory=; abi-float32: Stepper.env_step (aigar_env_step) writing
    float32 states into a float32 memory."""
    torch = pytest.importorskip("torch")
    from aigar_amd.env import AgarVecEnv
    p = lw.model_params(m)
    w = lw.World(shape, p)
    b = lm.Batched(p, w.NP, w.nn)
    n_dec = lw.n_decisions(shape, p)
    table = lw.action_table(lw.SEED, w.NP, n_dec, p.width)
    capacity = n_dec * len(w.nn)  # (no wrap: the ring is test_gpu_replay.py's subject)
    f32 = via == "abi-float32"
    nn_t = torch.as_tensor(w.roles == _abi.ROLE_NN, device="cuda")
    if f32:
        g = device(shape, w, p)
        g.set_stream(torch.cuda.current_stream().cuda_stream)  # (ordered with the tensor copies below)
        g.exp_config(capacity, dtype="float32")
        obs_buf = torch.zeros((w.NP, g.obs_len), dtype=torch.float32, device="cuda")
        r_buf = torch.zeros(w.NP, dtype=torch.float64, device="cuda")
        act_buf = torch.zeros((w.NP, p.width), dtype=torch.float64, device="cuda")
        prm = _abi.RewardParams.from_parameters(lm.reward_namespace(p))
        g.observe(obs_buf, mask=nn_t.to(torch.uint8))
        first = obs_buf.cpu().numpy()
        env = None
    else:
        A, B, field, mv = shape[:4]
        env = AgarVecEnv(B, lw.env_parameters(p), n_arenas=A, field_size=field, max_viruses=mv, roles=lw.roles_of(B),
                         seed=lw.SEED, memory=dict(capacity=capacity))
        env.reset(lw.SEED)
        g = env.stepper
        lw.mature(g, A, lw.SEED)  # (load_state: the bots start over, as after Model.resetBots)
        for a in range(w.A):
            assert parity.diff_states(g.get_state(a), w.o.get_state(a), ftol=0.0) == []
        first = env.observe().cpu().numpy()
    cast = (lambda x: x.astype(np.float32)) if f32 else (lambda x: x)
    want0 = lw.begin(w, b)
    assert obs_bits_equal(first[w.nn], cast(want0[w.nn])), bits_diff(first[w.nn], cast(want0[w.nn]))
    need = lw.Need(p.frame_skip)
    want_rows = []
    for d, st, obs, reward, alive, tr in lw.decisions(w, b, table, need):
        if f32:
            act_buf.copy_(torch.as_tensor(table[d]))
            g.env_step(act_buf, r_buf, obs_buf, enable_split=p.enable_split, skip=p.frame_skip, params=prm)
            got_obs, got_r = obs_buf.cpu().numpy(), r_buf.cpu().numpy()
            got_alive = ~np.isnan(got_obs[:, 0]) & (w.roles == _abi.ROLE_NN)
        else:
            out = env.step(torch.as_tensor(table[d], device="cuda"))
            got_obs, got_r, got_alive, done = [x.cpu().numpy() for x in out]
            assert not done.any()
        for k in range(w.A if f32 else 0):  # (the log holds the window's ticks; AgarVecEnv keeps none)
            assert np.array_equal(g.events(k), w.window_events(k)), "decision %d: events of arena %d differ" % (d, k)
        assert obs_bits_equal(got_r, reward), "reward of decision %d: %s" % (d, bits_diff(got_r[:, None],
                                                                                       reward[:, None]))
        assert np.array_equal(got_alive, alive & (w.roles == _abi.ROLE_NN)), d
        assert obs_bits_equal(got_obs[w.nn], cast(obs[w.nn])), "states of decision %d: %s" % (
            d, bits_diff(got_obs[w.nn], cast(obs[w.nn])))
        L = obs.shape[1]  # the extras in the row are the action just taken and the one before it
        live = [i for i in w.nn if alive[i]]
        assert obs_bits_equal(got_obs[live, L - 8:L - 4], cast(b.cur[live]))
        assert obs_bits_equal(got_obs[live, L - 4:], cast(b.prev[live]))
        want_rows.extend(tr)
    need.check()
    same_worlds(g, w)
    # the memory: one row per NN player and window that began with a state, in order
    info = g.exp_info()
    assert info["added"] == info["size"] == len(want_rows) <= capacity
    s, a, r, s2, dn = gather(g, len(want_rows), first.shape[1:], torch.float32 if f32 else torch.float64)
    want_s = np.array([w.obs_at[x[1]][x[0]] for x in want_rows])
    none = np.full(first.shape[1], np.nan)
    want_s2 = np.array([w.obs_at[x[4]][x[0]] if x[4] is not None else none for x in want_rows])
    assert obs_bits_equal(s, cast(want_s)), bits_diff(s, cast(want_s))
    assert obs_bits_equal(s2, cast(want_s2)), bits_diff(s2, cast(want_s2))
    assert obs_bits_equal(a, np.array([x[2] for x in want_rows]))
    assert obs_bits_equal(r, np.array([x[3] for x in want_rows]))
    assert np.array_equal(dn.astype(bool), np.array([x[5] for x in want_rows]))
    assert dn.sum() >= 1 and not np.isnan(s).any()
    (env or g).close()
    w.close()


def test_separate_calls_follow_the_graph_with_the_mass_as_reward():
    """AgarVecEnv.step_calls, the decision as separate calls, against the graph with
    MASS_AS_REWARD: aigar_rewards is Bot.getReward, which then ignores lastMass, and the
    window's sum must still leave out who has none (bot.py:167) -- here the Greedy and Random
    bots during the first window, and the NN players that are dead at a decision after the
    bots started over."""
    torch = pytest.importorskip("torch")
    from aigar_amd.env import AgarVecEnv
    shape, p = lw.SHAPES[1], lw.model_params(lw.MATRIX[2])
    A, B, field, mv = shape[:4]
    envs = []
    for _ in range(2):
        e = AgarVecEnv(B, lw.env_parameters(p), n_arenas=A, field_size=field, max_viruses=mv, roles=lw.roles_of(B),
                       seed=lw.SEED)
        e.obs.zero_()
        e.reset(lw.SEED)
        envs.append(e)
    a, c = envs
    table = lw.action_table(lw.SEED, A * B, 8, p.width)
    not_nn = ~a.nn.cpu().numpy()
    for d in range(8):
        if d in (0, 4):  # the bots start over (load_state: lastMass None), some of them dead from the last window
            for e in envs:
                lw.mature(e.stepper, A, lw.SEED + d)
                e.observe()
        act = torch.as_tensor(table[d], device="cuda")
        oa, ra, la, _ = a.step(act)
        oc, rc, lc = c.step_calls(act)
        ra, rc = ra.cpu().numpy(), rc.cpu().numpy()
        assert obs_bits_equal(ra, rc), "decision %d: %s" % (d, bits_diff(ra[:, None], rc[:, None]))
        assert obs_bits_equal(oa.cpu().numpy(), oc.cpu().numpy()) and torch.equal(la, lc), d
        if d in (0, 4):
            assert not ra[not_nn].any()  # no lastMass during this window: nothing added
        else:
            assert (ra[not_nn] != 0).any()
    for k in range(A):
        assert parity.diff_states(a.stepper.get_state(k), c.stepper.get_state(k), ftol=0.0) == []
    a.close()
    c.close()


class TableLearner:
    """The stub learner of the fixtures: the k-th decideMove answers row k of a table."""
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


FACADE = [lw.MATRIX[0], lw.MATRIX[1], lw.MATRIX[2]]  # skip 0 / 3 / 7, widths 2 / 4 / 3, both reward modes


@pytest.mark.parametrize("m", FACADE, ids=lw.MATRIX_IDS[:3])
def test_facade_bots(m):
    """aigar_amd.model's NN bots through Model.takeBotActions against the per-bot model, after
    every tick: lastMass, cumulativeReward, lastReward, skipFrames, currentlySkipping, the
    command, the new experiences (reward, action, which states) and the states themselves
    against the oracle -- through the collector's windows with resetBots and then a long run in
    which bots die inside skip windows and come back."""
    model = pytest.importorskip("aigar_amd.model")
    p = lw.model_params(m)
    W = p.frame_skip + 2
    ticks, windows, B = 144, 4, 16
    # (the Random bots divide by FRAME_SKIP_RATE, bot.py:244: none without frame skip)
    kinds = [k if (k != "Random" or p.frame_skip) else "Greedy" for k in lw.roles_of(B)]
    np.random.seed(lw.SEED)
    fm = model.Model(False, False, lw.env_parameters(p, ALGORITHM="AC", RESET_LIMIT=20000), seed=lw.SEED,
                     field_size=100, max_viruses=3, record_events=True)
    nn_idx = [i for i, k in enumerate(kinds) if k == "NN"]
    table = lw.action_table(lw.SEED, len(nn_idx), ticks, p.width).transpose(1, 0, 2)  # [bot, decision, width]
    bots = [fm.createBot(k, TableLearner(table[nn_idx.index(i)]) if k == "NN" else None) for i, k in enumerate(kinds)]
    fm.initialize()
    lw.mature(fm.field.stepper, 1, lw.SEED)
    fm.field._cache = {}
    o = Oracle(fm.field.stepper.cfg)
    o.load_state(fm.field.stepper.get_state())
    nn = [bt for bt in bots if bt.type == "NN"]
    ref = [lm.BotModel(p, table[k]) for k in range(len(nn))]
    tick_of = {}
    n_exp = [0] * len(nn)
    n_inside = n_terminal = n_back = 0
    was_alive = [True] * len(nn)
    for t in range(ticks):
        stats = o.player_stats()
        fm.field._set_actions(nn)  # (Model.update does this before takeBotActions)
        cur, prev = np.zeros((B, 4)), np.zeros((B, 4))
        for bt in nn:
            cur[bt.player.index], prev[bt.player.index] = lm.pad4(bt.currentAction, 0.0), lm.pad4(bt.lastAction, 0.0)
        o.set_actions(cur, prev)
        before = [bt.oldState for bt in nn]
        fm.takeBotActions()
        cmd = fm.field._cmd.copy()
        for k, (bt, rb) in enumerate(zip(nn, ref)):
            i = bt.player.index
            want_cmd, computed, state = rb.move(t, stats[i])
            what = "tick %d bot %d" % (t, k)
            alive = stats[i, 0] > 0
            n_inside += (not alive) and rb.skip_frames > 0
            n_back += alive and not was_alive[k] and rb.last_mass is not None
            was_alive[k] = alive
            same(np.array([np.nan if bt.lastMass is None else bt.lastMass, bt.cumulativeReward, bt.lastReward]),
                 np.array([np.nan if rb.last_mass is None else rb.last_mass, rb.cum, rb.last_reward]), what)
            assert (bt.skipFrames, bool(bt.currentlySkipping)) == (rb.skip_frames, rb.skipping), what
            same(np.array([lm.pad4(bt.currentAction), lm.pad4(bt.lastAction)]),
                 np.array([lm.pad4(rb.action), lm.pad4(rb.last_action)]), what)
            if want_cmd is not None:
                same(cmd[i], np.array(want_cmd), what + " command")
            if bt.oldState is not None and bt.oldState is not before[k]:  # a state was computed and kept
                assert computed and state == t, what
                tick_of[id(bt.oldState)] = t
                same(bt.oldState.reshape(-1), o.observe_one(i), what + " state")
            new = bt.experiences[n_exp[k]:]
            want_new = rb.experiences[n_exp[k]:]
            assert len(new) == len(want_new) <= 1, what
            for (s, a, r, s2, _), (te, told, wa, wr, tnew) in zip(new, want_new):
                assert te == t and tick_of[id(s)] == told and (s2 is None) == (tnew is None), what
                assert s2 is None or tick_of[id(s2)] == tnew, what
                same(np.array([r]), np.array([float(wr)]), what + " experience reward")
                same(lm.pad4(a), lm.pad4(wa), what + " experience action")
                n_terminal += s2 is None
            n_exp[k] = len(bt.experiences)
        fm.field.update()
        o.set_commands(cmd)
        o.step(1)
        assert np.array_equal(fm.field.events(), o.events()), "tick %d: events differ" % t
        if t + 1 <= windows * W and (t + 1) % W == 0:  # the collector's resetBots (aigar.py:845-852)
            fm.resetBots()
            mask = np.zeros(B, np.uint8)
            mask[nn_idx] = 1
            o.reset_bots(mask)
            for rb in ref:
                rb.reset()
                rb.experiences = []
            n_exp = [0] * len(nn)
    assert parity.diff_states(fm.field.stepper.get_state(), o.get_state(), ftol=0.0) == []
    assert n_terminal >= 5 and n_back >= 5, (n_terminal, n_back)
    if p.frame_skip:
        assert n_inside >= 5, n_inside
    o.close()
