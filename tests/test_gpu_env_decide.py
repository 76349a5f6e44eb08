"""GPU: AgarVecEnv(discrete=...) -- `step_q` (the selection inside the decision graph)
against a twin env without `discrete` that steps with the table rows of the Python
model's indices (tests/decide_model.py), and against `step_q_calls`; the replay memory's
action rows hold the indices; the observation's last-action extras hold the table rows.

The world is tests/test_gpu_env_memory.py's (2 arenas of 12 players, NN among Greedy and
Random bots on a field of 120, 2 ticks per decision, RESET_LIMIT 80; arena 1 starts 40
ticks old, so it is reset after 21 decisions): within 40 decisions NN players die, one is
dead at decision time and an arena is reset -- asserted below."""
import types

import numpy as np
import pytest

import decide_model as dm
import parity

pytestmark = pytest.mark.gpu
_lib = pytest.importorskip("aigar_amd._lib")

A, B, FIELD, SEED, DECISIONS, CAPACITY = 2, 12, 120, 2, 40, 512
ROLES = ["NN", "Greedy"] * 5 + ["NN", "Random"]


def parameters(strategy):
    return types.SimpleNamespace(PELLET_GRID=True, SELF_GRID=True, WALL_GRID=True, ENEMY_GRID=True, SELF_GRID_LF=True,
                                 USE_FOVSIZE=True, USE_TOTALMASS=True, USE_LAST_ACTION=True, GRID_SQUARES_PER_FOV=5,
                                 EXTRA_INPUT=True, GRID_VIEW_ENABLED=True, ENABLE_SPLIT=True, FRAME_SKIP_RATE=1,
                                 RESET_LIMIT=80, VIRUS_SPAWN=False, NUM_ACTIONS=16, SQUARE_ACTIONS=True,
                                 EXPLORATION_STRATEGY=strategy, EPSILON=0.3, TEMPERATURE=0.5)


def same(x, y):
    """Bit patterns equal, NaN equal to NaN."""
    x, y = x.cpu().numpy(), y.cpu().numpy()
    if x.dtype.kind != "f":
        return x.shape == y.shape and np.array_equal(x, y)
    nx, ny = np.isnan(x), np.isnan(y)
    v = np.uint64 if x.dtype.itemsize == 8 else np.uint32
    return x.shape == y.shape and np.array_equal(nx, ny) and np.array_equal(np.where(nx, 0, x).view(v),
                                                                            np.where(ny, 0, y).view(v))


@pytest.mark.parametrize("strategy,pixels,q_dtype", [("Boltzmann", None, "float32"), ("e-Greedy", None, "float64"),
                                                     ("e-Greedy", (12, False, True), "float32")])
def test_step_q_is_the_models_choice_stepped(strategy, pixels, q_dtype):
    torch = pytest.importorskip("torch")
    from aigar_amd import actions
    from aigar_amd.env import AgarVecEnv
    p = parameters(strategy)
    kw = dict(n_arenas=A, field_size=FIELD, roles=ROLES, seed=SEED, pixels=pixels)
    if pixels is not None:
        kw["pixel_dtype"] = torch.float32
    a = AgarVecEnv(B, p, discrete=True, memory=dict(capacity=CAPACITY), **kw)
    b = AgarVecEnv(B, p, **kw)                  # the twin: plain actions
    c = AgarVecEnv(B, p, discrete=True, **kw)   # the same decision as separate calls
    NP = A * B
    table = actions.discrete_actions(16, True, True, False)
    assert a.discrete["n_out"] == 32 and np.array_equal(a.actions.cpu().numpy(), table)
    assert a.explore.tolist() == [0.3, 0.5] and b.discrete is None
    code = dm.BOLTZMANN if strategy == "Boltzmann" else dm.E_GREEDY
    nn = np.array([r == "NN" for r in ROLES] * A)
    for env in (a, b, c):
        env.obs.zero_()  # (the Greedy and Random bots' rows are never written)
    oa, ob, oc = a.reset(), b.reset(), c.reset()
    assert same(oa, ob) and same(oa, oc)
    deciding = ~np.isnan(ob.cpu().numpy().reshape(NP, -1)[:, 0]) & nn
    gen = torch.Generator(device="cuda").manual_seed(SEED)
    want_a = []
    held = np.zeros((NP, 4))  # a player that does not decide keeps its last chosen row (zeros before the first)
    n_died = n_silent = n_resets = n_explored = 0
    for t in range(DECISIONS):
        q = (torch.randn((NP, 32), dtype=torch.float64, device="cuda", generator=gen) * 2).to(getattr(torch, q_dtype))
        u = torch.rand((NP, 3), dtype=torch.float64, device="cuda", generator=gen)
        if t == DECISIONS // 2:  # the schedule is the caller's: a write, no re-capture
            for env in (a, c):
                env.set_exploration(epsilon=0.6, temperature=0.05)
        eps, temp = (0.3, 0.5) if t < DECISIONS // 2 else (0.6, 0.05)
        idx, val, rows, bad = dm.decide(q.cpu().numpy(), table, code, eps, temp, deciding, u=u.cpu().numpy())
        assert not bad.any()
        held = np.where(deciding[:, None], rows, held)
        act = torch.as_tensor(held, device="cuda")
        ra, rb = a.step_q(q, u), b.step(act)
        obs_c, rew_c, _ = c.step_q_calls(q, u)
        done_c = c._episode_ends()  # (step_calls leaves the episode bookkeeping out)
        for x, y in zip(ra, rb):
            assert same(x, y), t
        assert same(c.obs, ra[0]) and same(rew_c, ra[1]) and same(done_c, ra[3]), t
        for env in (a, c):
            assert np.array_equal(env.action_idx.cpu().numpy(), idx), t
            got = env.action_value.cpu().numpy()
            assert np.array_equal(np.isnan(got), np.isnan(val)) and np.array_equal(np.nan_to_num(got), np.nan_to_num(val)), t
        want_a.append(idx[deciding].astype(np.float64))
        n_silent += int((nn & ~deciding).sum())
        n_explored += int((np.isnan(val) & deciding).sum())
        obs, reward, alive, done = [x.cpu().numpy() for x in rb]
        alive_now = ~np.isnan(obs.reshape(NP, -1)[:, 0]) & nn
        assert np.array_equal(alive, alive_now)
        n_died += int((deciding & ~alive_now & ~done).sum())
        n_resets += len(set((np.nonzero(done)[0] // B).tolist()))
        if pixels is None:  # updateValues: the chosen row is the bot's currentAction (the row's last four values)
            kept = deciding & alive_now & ~done
            assert kept.any() and np.array_equal(obs[kept][:, -4:], table[idx[kept]]), t
        deciding = alive_now
    # the run met what it was chosen for
    assert n_died >= 1, "no NN player died"
    assert n_silent >= 1, "no NN player was dead at decision time"
    assert n_resets >= 1, "no arena was reset"
    assert (n_explored >= 1) == (strategy == "e-Greedy")
    # the replay memory's action rows: [index, 0, 0, 0] of every deciding player, in order
    want_a = np.concatenate(want_a)
    info = a.stepper.exp_info()
    assert info["added"] == len(want_a) <= CAPACITY
    ac = torch.full((CAPACITY, 4), -3.0, dtype=torch.float64, device="cuda")
    a.stepper.exp_gather(torch.arange(CAPACITY, device="cuda"), a=ac)
    ac = ac.cpu().numpy()[:len(want_a)]
    assert np.array_equal(ac[:, 0], want_a) and (ac[:, 1:] == 0.0).all() and (want_a >= 0).all()
    for k in range(A):
        assert parity.diff_states(a.stepper.get_state(k), b.stepper.get_state(k), ftol=0.0) == []
        assert parity.diff_states(c.stepper.get_state(k), b.stepper.get_state(k), ftol=0.0) == []
    for env in (a, b, c):
        env.close()


def test_discrete_is_off_unless_asked_for_and_reads_its_parameters():
    torch = pytest.importorskip("torch")
    from aigar_amd.env import AgarVecEnv
    p = parameters("Boltzmann")
    off = AgarVecEnv(4, p, field_size=100)
    assert off.discrete is None and off.stepper.dec is None
    q = torch.zeros((4, 32), dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError, match="discrete"):
        off.step_q(q)
    with pytest.raises(RuntimeError, match="discrete"):
        off.set_exploration(epsilon=0.1)
    off.reset()
    out = off.step(torch.rand((4, 4), dtype=torch.float64, device="cuda"))  # step is as it was
    assert len(out) == 4 and out[0].shape == (4, off.stepper.obs_len)
    off.close()
    env = AgarVecEnv(4, p, field_size=100, discrete=True)
    assert env.discrete == {"num_actions": 16, "square": True, "strategy": "Boltzmann", "seed": 0, "n_out": 32}
    assert env.explore.tolist() == [0.3, 0.5] and env.actions.shape == (32, 4)
    env.reset()
    obs, reward, alive, done = env.step_q(q)  # the device's own draws
    assert obs.shape == (4, env.stepper.obs_len) and env.action_idx.dtype == torch.int32
    assert ((env.action_idx >= 0) & (env.action_idx < 32)).all()
    env.step_q(q.double())  # the other dtype: its own buffer, the selection configured anew
    assert set(env._q) == {torch.float32, torch.float64}
    with pytest.raises(ValueError):
        env.step_q(torch.zeros((4, 31), dtype=torch.float32, device="cuda"))
    env.close()
    circle = AgarVecEnv(4, p, field_size=100, discrete=dict(num_actions=7, square=False, strategy="e-Greedy", seed=3))
    assert circle.discrete["n_out"] == 14 and circle.actions.shape == (14, 4)
    circle.close()
    with pytest.raises(ValueError, match="unknown keys"):
        AgarVecEnv(4, p, field_size=100, discrete=dict(actions=5))
    with pytest.raises(ValueError, match="perfect square"):
        AgarVecEnv(4, p, field_size=100, discrete=dict(num_actions=8))
