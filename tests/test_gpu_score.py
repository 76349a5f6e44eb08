"""GPU: AIGAR_FLAG_SCORE -- every bot's mass history (Bot.makeMove's
totalMasses.append(player.getTotalMass()), bot.py:253) sampled on the device at the
start of every tick: against the oracle tick by tick, under the step graphs, with a
trace buffer, across every kind of reset, and through AgarVecEnv's episodes."""
import types

import numpy as np
import pytest

from aigar_amd import _abi
from oracle_lib import Oracle, make_config
import parity

pytestmark = pytest.mark.gpu
_lib = pytest.importorskip("aigar_amd._lib")

A, B, SIZE = 3, 24, 250  # NP = 72: no multiple of the wave or of the sampler's 256-thread block
NP = A * B
CH, EX = _abi.OBS_PELLET, _abi.EX_FOV | _abi.EX_MASS


def config(arenas=A, score=True, **kw):
    flags = _abi.FLAG_EVENTS | (_abi.FLAG_SCORE if score else 0)
    return make_config(n_arenas=arenas, bots=B, field_size=SIZE, virus=True, max_viruses=6, channels=CH, extras=EX,
                       flags=flags, **kw)


def fatten(g, base=200.0, step=40.0):
    """Fresh players weigh 10 and cannot split: give them base .. base + 7 * step, heavy
    enough to split down to 8 and more cells (np_sum's unrolled branch in getTotalMass)."""
    for a in range(g.A):
        st = g.get_state(a)
        cf = np.array(st["cells_f"], np.float64).reshape(-1, 9)
        owner = np.asarray(st["cells_i"]).reshape(-1, 4)[:, 0]
        cf[:, 2] = base + step * (owner % 8)
        cf[:, 3] = np.sqrt(cf[:, 2] / np.pi)
        st["cells_f"] = cf.reshape(np.asarray(st["cells_f"]).shape)
        g.load_state(st, a)


def on_torch_stream(g):
    """The handle's work on torch's stream: ordered with the fills and reads of the trace tensors."""
    import torch
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    return g


def heavy_handle(seed=3, score=True, arenas=A):
    g = on_torch_stream(_lib.Stepper(config(arenas=arenas, score=score)))
    g.reset(seed)
    fatten(g)
    return g


def rows(a):
    return slice(a * B, (a + 1) * B)


def stats_of(lists):
    """samples, sum, max, dead of the lists [T, players] as aigar_score defines them: the sum
    one Python float add per sample in tick order."""
    lists = np.asarray(lists, np.float64).reshape(len(lists), -1)
    out = np.zeros((lists.shape[1], 4))
    for i in range(lists.shape[1]):
        s = 0.0
        for x in lists[:, i].tolist():
            s += x
        out[i] = (len(lists), s, lists[:, i].max() if len(lists) else 0.0, int((lists[:, i] == 0).sum()))
    return out


def masses(h):
    """Player.getTotalMass() of every player as the reference's bots see it: 0 when dead."""
    st = h.player_stats()
    assert not st[st[:, 0] == 0, 1].any()
    return st[:, 1].copy()


def trace_buffer(cap, fill=-7.0, guard=0):
    import torch
    return torch.full((cap + guard, NP), fill, dtype=torch.float64, device="cuda")


def test_samples_match_the_oracle_tick_by_tick():
    T = 40
    g = heavy_handle()
    tr = trace_buffer(T + 8)
    g.score_trace(tr)
    orc = []
    for a in range(A):
        o = Oracle(config(arenas=1))
        o.load_state(g.get_state(a))
        orc.append(o)
    rng = np.random.default_rng(11)
    want = np.zeros((T, NP))
    many_cells = 0
    for t in range(T):
        cmd = parity.synthetic_commands(rng, None, NP, SIZE, 0.2, 0.1)
        for a, o in enumerate(orc):
            want[t, rows(a)] = o.player_stats()[:, 1]
            owner = np.asarray(o.get_state()["cells_i"]).reshape(-1, 4)[:, 0].astype(int)
            many_cells += int((np.bincount(owner, minlength=B) >= 8).sum())
            o.set_commands(cmd[rows(a)])
            o.step(1)
        g.set_commands(cmd)
        g.step(1)
    # the input exercises what it should (properties of the oracle's run, not of the sampler)
    assert many_cells > 0, "no sample of a player with >= 8 cells"
    assert (want == 0).any(), "no death"
    assert ((want[:-1] == 0) & (want[1:] > 0)).any(), "no respawn"
    got = tr.cpu().numpy()
    assert np.array_equal(got[:T], want)
    assert (got[T:] == -7.0).all()
    sc, exp = g.score(), stats_of(want)
    assert (sc[:, 0] == T).all()
    assert np.array_equal(sc[:, 2], want.max(axis=0))
    assert np.array_equal(sc[:, 3], (want == 0).sum(axis=0))
    assert np.array_equal(sc[:, 1], exp[:, 1])
    for i in range(NP):  # any two summation orders of non-negative terms
        tot = np.sum(want[:, i])
        assert abs(sc[i, 1] - tot) <= 2 * T * 2.0 ** -53 * tot, i
    assert np.array_equal(sc, exp)
    for h in [g] + orc:
        h.close()


@pytest.mark.parametrize("policy", ["greedy", "random"])
def test_graphed_run_samples_every_tick(policy):
    import torch
    T = 41  # ten replays of the 4-step graph and one of the one-step graph
    g, twin = heavy_handle(), heavy_handle()
    tr = trace_buffer(T + 3)
    g.score_trace(tr)
    obs = torch.empty((NP, g.obs_len), dtype=torch.float64, device="cuda")
    if policy == "greedy":
        g.run(T, policy="greedy", greedy_split=True, out=obs)
    else:
        g.run(T, policy="random", p_split=0.2, p_eject=0.1, seed=5, out=obs)
    want = np.zeros((T, NP))
    for t in range(T):
        want[t] = masses(twin)
        if policy == "greedy":
            twin.policy_greedy(True)
        else:
            twin.policy_random(0.2, 0.1, 5)
        twin.step(1)
    got = tr.cpu().numpy()
    print("samples that differ (tick, player):", np.argwhere(got[:T] != want)[:8].tolist())
    assert np.array_equal(got[:T], want)
    assert (got[T:] == -7.0).all()
    assert np.array_equal(g.score(), stats_of(want))
    assert np.array_equal(twin.score(), stats_of(want))
    assert len(np.unique(want, axis=0)) > T // 2  # (the masses do move)
    g.close()
    twin.close()


def test_trace_capacity_reattachment_and_detachment():
    import torch
    g, twin = heavy_handle(), heavy_handle()
    prm = dict(policy="random", p_split=0.2, p_eject=0.1, seed=5)
    want = []
    def twin_ticks(n):
        for t in range(n):
            want.append(masses(twin))
            twin.policy_random(0.2, 0.1, 5)
            twin.step(1)
    store = trace_buffer(8, fill=-7.0, guard=1)  # 9 rows, the last one a guard behind the buffer
    g.score_trace(store[:8])
    for k in range(3):
        g.run(4, **prm)  # (the 4-step graph, captured by the first call)
    twin_ticks(12)
    got = store.cpu().numpy()
    assert np.array_equal(got[:8], np.array(want[:8]))
    assert (got[8] == -7.0).all()
    assert (g.score()[:, 0] == 12).all()
    # a second buffer under the same graphs: the samples go on at their own indices
    second = trace_buffer(20, fill=-3.0)
    g.score_trace(second)
    g.run(5, **prm)  # (both graphs replayed)
    twin_ticks(5)
    got2 = second.cpu().numpy()
    assert np.array_equal(got2[12:17], np.array(want[12:17]))
    assert (got2[:12] == -3.0).all() and (got2[17:] == -3.0).all()
    assert np.array_equal(store.cpu().numpy(), got)
    # detached: nothing is written, the statistics go on
    g.score_trace(None)
    g.run(4, **prm)
    twin_ticks(4)
    assert np.array_equal(second.cpu().numpy(), got2) and np.array_equal(store.cpu().numpy(), got)
    assert np.array_equal(g.score(), stats_of(want))
    with pytest.raises(ValueError, match="score_trace"):
        g.score_trace(torch.zeros((4, NP + 1), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="score_trace"):
        g.score_trace(torch.zeros((4, NP), dtype=torch.float32, device="cuda"))
    g.close()
    twin.close()


def test_every_reset_clears_what_it_restarts_and_nothing_else():
    s = 9
    g, twin = heavy_handle(), heavy_handle()
    tr = trace_buffer(32)
    g.score_trace(tr)
    def ticks(n):
        for t in range(n):
            for h in (g, twin):
                h.policy_random(0.2, 0.1, 5)
                h.step(1)
    ticks(20)
    assert np.array_equal(g.score(), twin.score()) and (g.score()[:, 0] == 20).all()
    g.reset_arenas([1], [s])
    sg, st = g.score(), twin.score()
    assert not sg[rows(1)].any()
    assert np.array_equal(sg[rows(0)], st[rows(0)]) and np.array_equal(sg[rows(2)], st[rows(2)])
    ticks(5)
    sg, st = g.score(), twin.score()
    assert (sg[rows(1), 0] == 5).all() and (sg[rows(0), 0] == 25).all() and (sg[rows(2), 0] == 25).all()
    assert np.array_equal(sg[rows(0)], st[rows(0)]) and np.array_equal(sg[rows(2)], st[rows(2)])
    one = _lib.Stepper(config(arenas=1))
    one.reset(s)
    fresh = masses(one)
    assert (fresh > 0).all()
    assert np.array_equal(tr.cpu().numpy()[0, rows(1)], fresh)  # the new episode's sample 0: the fresh world
    one.close()
    # Bot.resetMassList for a mask
    mask = (np.arange(NP) % 3 == 1).astype(np.uint8)
    before = g.score()
    g.score_reset(mask)
    after = g.score()
    assert not after[mask == 1].any() and np.array_equal(after[mask == 0], before[mask == 0])
    # a snapshot carries no score
    before = after
    g.load_state(g.get_state(2), 2)
    after = g.score()
    assert not after[rows(2)].any()
    assert np.array_equal(after[rows(0)], before[rows(0)]) and np.array_equal(after[rows(1)], before[rows(1)])
    assert after[rows(0)].any()
    # Bot.reset keeps totalMasses
    g.reset_bots()
    assert np.array_equal(g.score(), after)
    g.score_reset()
    assert not g.score().any()
    ticks(2)
    assert (g.score()[:, 0] == 2).all()
    g.reset(4)
    assert not g.score().any()
    g.close()
    twin.close()


def test_without_the_flag_nothing_changes_and_the_calls_say_so():
    import torch
    g, plain = heavy_handle(), heavy_handle(score=False)
    for call in (plain.score, plain.score_reset, lambda: plain.score_trace(None),
                 lambda: plain.score_trace(trace_buffer(4))):
        with pytest.raises(RuntimeError, match="AIGAR_FLAG_SCORE"):
            call()
    obs = [torch.empty((NP, g.obs_len), dtype=torch.float64, device="cuda") for h in range(2)]
    for h, o in ((g, obs[0]), (plain, obs[1])):
        for t in range(3):
            h.policy_random(0.2, 0.1, 5)
            h.step(1)
        h.run(9, policy="random", p_split=0.2, p_eject=0.1, seed=5, out=o)
    for a in range(A):
        x, y = g.get_state(a), plain.get_state(a)
        assert parity.diff_states(x, y, ftol=0.0) == [] and np.array_equal(x["philox_key"], y["philox_key"]), a
    assert torch.equal(torch.nan_to_num(obs[0]), torch.nan_to_num(obs[1]))
    assert (g.score()[:, 0] == 12).all()
    g.close()
    plain.close()


def test_env_scores_every_episode():
    import torch
    from aigar_amd.env import AgarVecEnv
    p = types.SimpleNamespace(VIRUS_SPAWN=True, ENABLE_SPLIT=True, ENABLE_EJECT=False, ENABLE_GREEDY_SPLIT=True,
                              PELLET_GRID=True, SELF_GRID=True, WALL_GRID=True, ENEMY_GRID=True, VIRUS_GRID=True,
                              SELF_GRID_LF=True, ENEMY_GRID_LF=True, USE_FOVSIZE=True, USE_TOTALMASS=True,
                              USE_LAST_ACTION=True, USE_LAST_FOVSIZE=True, GRID_SQUARES_PER_FOV=11, EXTRA_INPUT=True,
                              FRAME_SKIP_RATE=1, RESET_LIMIT=16)
    roles = ["NN"] * 16 + ["Greedy"] * 8 + ["Random"] * 8
    EA, EB = 4, 32
    kw = dict(n_arenas=EA, field_size=250, max_viruses=6, roles=roles, seed=1)
    env = AgarVecEnv(EB, p, score=True, **kw)
    plain = AgarVecEnv(EB, p, **kw)
    tw_env = AgarVecEnv(EB, p, **kw)  # the twin Stepper, brought to the same start (reset + warm-up)
    for e in (plain, tw_env):
        assert not hasattr(e, "last_score") and not hasattr(e, "last_return")
        with pytest.raises(RuntimeError, match="score=True"):
            e.score()
    o_env, o_plain = env.reset(2), plain.reset(2)
    tw_env.reset(2)
    nn = np.array([r == "NN" for r in roles] * EA)
    nn_t = torch.as_tensor(nn, device="cuda")  # (the rows of the other players are never written)
    assert torch.equal(torch.nan_to_num(o_env[nn_t]), torch.nan_to_num(o_plain[nn_t]))
    assert torch.isnan(env.last_score).all() and torch.isnan(env.last_return).all()
    assert not env.score().any()  # the warm-up is not scored
    tw = tw_env.stepper
    greedy = torch.as_tensor(tw_env.roles == _abi.ROLE_GREEDY, device="cuda").to(torch.uint8)
    lists = [[] for a in range(EA)]  # the twin's mass lists of the running episodes
    ret = np.zeros(EA * EB)
    er = lambda a: slice(a * EB, (a + 1) * EB)
    k = n_done = 0
    gen = torch.Generator(device="cuda").manual_seed(2)
    for t in range(20):
        act = torch.rand((EA * EB, 4), dtype=torch.float64, device="cuda", generator=gen)
        obs, rew, alive, done = env.step(act)
        obs_p, rew_p, alive_p, done_p = plain.step(act)
        assert torch.equal(torch.nan_to_num(obs[nn_t]), torch.nan_to_num(obs_p[nn_t])) and torch.equal(rew, rew_p)
        assert torch.equal(alive, alive_p) and torch.equal(done, done_p)
        ret += np.where(nn, rew.cpu().numpy(), 0.0)
        for j in range(env.skip + 1):  # the decision as step_calls makes it
            tw.apply_actions(act, env.enable_split, skipping=j > 0, record=j == 0)
            tw.policy_greedy(True, greedy)
            tw.policy_random_bots()
            m = masses(tw)
            for a in range(EA):
                lists[a].append(m[er(a)])
            tw.step(1)
        ended = sorted(set((done.nonzero().flatten() // EB).tolist()))
        last, last_ret = env.last_score.cpu().numpy(), env.last_return.cpu().numpy()
        seeds = []
        for a in ended:
            k += 1
            n_done += 1
            seeds.append(env.seed + 7919 * k)
            exp = stats_of(lists[a])
            assert np.array_equal(last[er(a)], exp), (t, a)
            assert (last[er(a), 0] == len(lists[a])).all() and len(lists[a]) in (6, 10, 14, 18), (t, a, len(lists[a]))
            assert np.array_equal(last_ret[er(a)][nn[er(a)]], ret[er(a)][nn[er(a)]]), (t, a)
            assert np.isnan(last_ret[er(a)][~nn[er(a)]]).all()
            # performAgarioTest's reduction (aigar.py:533-535) of the twin's lists
            mo = np.array(lists[a]).T  # massOverTime[bot][time]
            mean_mass = np.mean([np.mean(bm) for bm in mo])
            max_mass = np.max([np.max(bm) for bm in mo])
            gm, gx = (x.cpu().numpy() for x in env.test_score())
            assert abs(gm[a] - mean_mass) <= 2 * mo.size * 2.0 ** -53 * mean_mass, (t, a, gm[a], mean_mass)
            assert gx[a] == max_mass, (t, a)
            lists[a] = []
            ret[er(a)] = 0.0
        if ended:
            tw.reset_arenas(ended, seeds)
        running = env.score().cpu().numpy()
        for a in range(EA):
            assert np.array_equal(running[er(a)], stats_of(lists[a]) if lists[a] else np.zeros((EB, 4))), (t, a)
    assert n_done >= 8  # every arena ended at least twice
    gm, gx = env.test_score(arena_mask=[True, False, True, False])
    assert torch.isnan(gm[[1, 3]]).all() and torch.isnan(gx[[1, 3]]).all() and not torch.isnan(gm[[0, 2]]).any()
    for e in (env, plain, tw_env):
        e.close()
