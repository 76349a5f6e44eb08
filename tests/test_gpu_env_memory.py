"""GPU: AgarVecEnv(memory=...) -- the transitions the decision graph appends to the replay
memory against the list built in Python from a second env's (obs, reward, alive, done),
with the rules of include/aigar.h: every NN player that had an old state emits (old
state, action padded to 4, window reward, new row -- NaN if dead, done = dead) in
ascending player order; a dead player, a reset arena and the first decision emit nothing;
Greedy and Random players never do.  The memory must not disturb the step.

The world (2 arenas of 12 players, NN among Greedy and Random bots on a field of 120,
2 ticks per decision, RESET_LIMIT 80, 100 decisions) was chosen on the CPU oracle: 12
players on a field of 120 with every second one on random commands among Greedy bots lose
22 .. 27 of those players in 200 ticks (seeds 1 .. 3), about half of them on the last tick
of a 2-tick window, where the decision's observation sees the death; arena 1 starts 40
ticks old (the desynchronising warm-up), so it is reset after 21 decisions and arena 0
after 41; 12 NN players emit up to 12 transitions per decision into a ring of 256."""
import types

import numpy as np
import pytest

import parity

pytestmark = pytest.mark.gpu
_lib = pytest.importorskip("aigar_amd._lib")

A, B, FIELD, SEED, DECISIONS, CAPACITY = 2, 12, 120, 2, 100, 256
ROLES = ["NN", "Greedy"] * 5 + ["NN", "Random"]


def parameters():
    return types.SimpleNamespace(PELLET_GRID=True, SELF_GRID=True, WALL_GRID=True, ENEMY_GRID=True, SELF_GRID_LF=True,
                                 USE_FOVSIZE=True, USE_TOTALMASS=True, USE_LAST_ACTION=True, GRID_SQUARES_PER_FOV=5,
                                 EXTRA_INPUT=True, GRID_VIEW_ENABLED=True, ENABLE_SPLIT=True, FRAME_SKIP_RATE=1,
                                 RESET_LIMIT=80, VIRUS_SPAWN=False)


def same_rows(a, b):
    """Bit patterns equal, NaN rows equal to NaN rows."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    na, nb = np.isnan(a), np.isnan(b)
    v = np.uint64 if a.dtype.itemsize == 8 else np.uint32
    return np.array_equal(na, nb) and np.array_equal(np.where(na, 0, a).view(v), np.where(nb, 0, b).view(v))


@pytest.mark.parametrize("pixels,dtype", [(None, "float64"), ((12, False, True), "float64"), ((12, False, True), "float32")])
def test_decisions_fill_the_memory_with_the_bots_transitions(pixels, dtype):
    torch = pytest.importorskip("torch")
    from aigar_amd.env import AgarVecEnv
    kw = dict(n_arenas=A, field_size=FIELD, roles=ROLES, seed=SEED, pixels=pixels)
    if pixels is not None:
        kw["pixel_dtype"] = getattr(torch, dtype)
    a = AgarVecEnv(B, parameters(), memory=dict(capacity=CAPACITY), **kw)
    b = AgarVecEnv(B, parameters(), **kw)
    NP = A * B
    nn = np.array([r == "NN" for r in ROLES] * A)
    assert str(a.obs.dtype) == "torch." + dtype and a.memory["capacity"] == CAPACITY and not a.memory["prioritized"]
    assert a.memory_size() == 0

    seen = {}
    ends = b._episode_ends

    def ends_after_a_look():  # the decision's observation, before an ended arena's reset overwrites its rows
        seen["obs"] = b.obs.clone()
        return ends()
    b._episode_ends = ends_after_a_look

    for env in (a, b):
        env.obs.zero_()  # (the Greedy and Random bots' rows are never written)
    oa, ob = a.reset(), b.reset()
    assert same_rows(oa.cpu().numpy(), ob.cpu().numpy())
    first = ob.cpu().numpy().reshape(NP, -1)
    old = [first[i].copy() if nn[i] and not np.isnan(first[i, 0]) else None for i in range(NP)]
    died = np.zeros(NP, bool)  # no old state because the player was dead at the last observation
    want = []
    n_done = n_silent = n_resets = 0
    gen = torch.Generator(device="cuda").manual_seed(SEED)
    for t in range(DECISIONS):
        act = torch.rand((NP, 4 if t < DECISIONS // 2 else 3), dtype=torch.float64, device="cuda", generator=gen)
        ra, rb = a.step(act), b.step(act)
        for x, y in zip(ra, rb):  # the memory does not disturb the step
            assert same_rows(x.cpu().numpy(), y.cpu().numpy()), t
        obs, reward, alive, done = [x.cpu().numpy() for x in rb]
        new = seen["obs"].cpu().numpy().reshape(NP, -1)
        act_h = np.zeros((NP, 4))
        act_h[:, :act.shape[1]] = act.cpu().numpy()
        for i in np.nonzero(nn)[0]:
            dead = bool(np.isnan(new[i, 0]))
            if old[i] is not None:
                want.append((old[i], act_h[i].copy(), float(reward[i]), new[i].copy(), dead))
                n_done += dead
            elif died[i]:
                n_silent += 1
            old[i], died[i] = (None, True) if dead else (new[i].copy(), False)
        ended = sorted(set((np.nonzero(done)[0] // B).tolist()))
        n_resets += len(ended)
        for k in ended:  # no transition bridges the reset: the fresh world's first states are the old states
            rows = obs.reshape(NP, -1)
            for i in range(k * B, (k + 1) * B):
                if nn[i]:
                    assert not np.isnan(rows[i, 0])
                    old[i], died[i] = rows[i].copy(), False
    # the run met what it was chosen for
    assert n_done >= 1, "no NN player died at a decision's observation"
    assert n_silent >= 1, "no NN player was dead at decision time"
    assert n_resets >= 1, "no arena was reset"
    assert len(want) > CAPACITY, "the ring did not wrap"
    info = a.stepper.exp_info()
    assert info["added"] == len(want) and info["size"] == CAPACITY == a.memory_size()
    assert info["next_idx"] == len(want) % CAPACITY
    ring = [None] * CAPACITY
    for k, tr in enumerate(want):
        ring[k % CAPACITY] = tr
    row = tuple(a.obs.shape[1:])
    s = torch.zeros((CAPACITY,) + row, dtype=a.obs.dtype, device="cuda")
    s2 = torch.zeros_like(s)
    ac = torch.zeros((CAPACITY, 4), dtype=torch.float64, device="cuda")
    r = torch.zeros(CAPACITY, dtype=torch.float64, device="cuda")
    dn = torch.zeros(CAPACITY, dtype=torch.uint8, device="cuda")
    a.stepper.exp_gather(torch.arange(CAPACITY, device="cuda"), s=s, a=ac, r=r, s2=s2, done=dn)
    s, s2 = s.cpu().numpy().reshape(CAPACITY, -1), s2.cpu().numpy().reshape(CAPACITY, -1)
    ac, r, dn = ac.cpu().numpy(), r.cpu().numpy(), dn.cpu().numpy()
    for k, (ws, wa, wr, ws2, wd) in enumerate(ring):
        assert same_rows(s[k], ws), k
        assert same_rows(s2[k], ws2), k
        assert np.array_equal(ac[k], wa) and r[k] == wr and bool(dn[k]) == wd, k
        assert wd == bool(np.isnan(ws2).all()) and not np.isnan(ws).any()
    # a uniform mini-batch through the env: rows of the ring, weights 1
    u = np.linspace(0, 0.999, 32)
    batch = a.sample(32, u=torch.as_tensor(u))
    idx = batch.idx.cpu().numpy()
    assert np.array_equal(idx, np.floor(u * CAPACITY).astype(np.int64))
    assert same_rows(batch.s.cpu().numpy().reshape(32, -1), s[idx]) and np.array_equal(batch.r.cpu().numpy(), r[idx])
    assert np.array_equal(batch.done.cpu().numpy(), dn[idx].astype(bool)) and (batch.w == 1.0).all()
    a.update_priorities(batch.idx, batch.r)  # (uniform: nothing happens)
    assert a.memory_size() == CAPACITY
    # and the worlds went the same way
    for k in range(A):
        assert not parity.diff_states(a.stepper.get_state(k), b.stepper.get_state(k))
    a.close()
    b.close()


def test_memory_is_off_unless_asked_for_and_reads_its_parameters():
    torch = pytest.importorskip("torch")
    from aigar_amd.env import AgarVecEnv
    p = parameters()
    p.MEMORY_CAPACITY, p.PRIORITIZED_EXP_REPLAY_ENABLED, p.MEMORY_ALPHA, p.MEMORY_BETA, p.MEMORY_BATCH_LEN = 50, True, 0.5, 0.3, 8
    off = AgarVecEnv(4, p, field_size=100)
    assert off.memory is None and off.stepper.exp is None
    with pytest.raises(RuntimeError):
        off.sample()
    off.close()
    env = AgarVecEnv(4, p, field_size=100, memory=True)
    assert env.memory == {"capacity": 50, "prioritized": True, "alpha": 0.5, "beta": 0.3, "batch": 8, "seed": 0}
    env.reset()
    empty = env.sample()
    assert empty.idx.tolist() == [-1] * 8 and torch.isnan(empty.w).all()  # nothing to draw from yet
    act = torch.rand((4, 4), dtype=torch.float64, device="cuda")
    env.step(act)
    env.step(act)
    assert env.memory_size() >= 2  # (enough for a prioritized draw)
    b = env.sample()
    assert b.s.shape == (8, env.stepper.obs_len) and ((b.idx >= 0) & (b.idx < env.memory_size())).all()
    assert torch.isfinite(b.w).all() and b.w.max() <= 1.0
    env.update_priorities(b.idx, torch.arange(8, dtype=torch.float64, device="cuda") - 3.0)
    b2 = env.sample(64)
    assert ((b2.idx >= 0) & (b2.idx < env.memory_size())).all() and torch.isfinite(b2.w).all()
    with pytest.raises(RuntimeError, match="state_dtype"):  # the memory stores float64 states
        env.stepper.env_step(env._act[4], env._r, torch.empty((4, env.stepper.obs_len), dtype=torch.float32,
                                                             device="cuda"), True, env.skip, env.reward_params)
    env.close()
