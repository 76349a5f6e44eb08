"""GPU: AgarVecEnv(continuous=...) -- `step_ac` (the exploration noise inside the decision
graph) against a twin env without `continuous` that steps with the Python model's noisy rows
(tests/noise_model.py), and against `step_ac_calls`; the replay ring's action rows and fifth
field across a ring wrap, deaths and an arena reset; the observation's last-action extras.

The worlds are tests/learner_worlds.py's (1 x 12, 3 x 13 and 2 x 64 players, NN among Greedy
and Random bots, matured so that players die from the first ticks); every arena's episode
ends once within the 40 decisions, and before decision 6 an NN player of arena 0 is taken
out of the world for two decisions (a dead player as the tick leaves it, respawnTime set; loading
that state restarts its arena's bots).  That an NN player is dead at decision time and
decides again afterwards, that the arenas are reset, that the ring wraps and (one tick per
decision) that deciding players die is asserted below."""
import numpy as np
import pytest

import learner_worlds as lw
import noise_model as nm
import parity

pytestmark = pytest.mark.gpu
from aigar_amd import _abi, _lib  # noqa: E402

DECISIONS, T = 40, 4
# (shape, decision matrix row, noise, mu dtype, algorithm, ring capacity)
CASES = [(lw.SHAPES[0], lw.MATRIX[1], "Orn-Uhl", "float32", "CACLA", 40),   # 4 values, 4 ticks per decision
         (lw.SHAPES[1], lw.MATRIX[2], "Gaussian", "float64", "SPG", 120),   # 3 values, 8 ticks
         (lw.SHAPES[2], lw.MATRIX[0], "Orn-Uhl", "float32", "CACLA", 400)]  # 2 values, 1 tick
OU = dict(ORN_UHL_THETA=0.3, ORN_UHL_MU=0.25, ORN_UHL_DT=0.5)


def same(x, y):
    """Bit patterns equal, NaN equal to NaN."""
    x, y = x.cpu().numpy(), y.cpu().numpy()
    if x.dtype.kind != "f":
        return x.shape == y.shape and np.array_equal(x, y)
    nx, ny = np.isnan(x), np.isnan(y)
    v = np.uint64 if x.dtype.itemsize == 8 else np.uint32
    return x.shape == y.shape and np.array_equal(nx, ny) and np.array_equal(np.where(nx, 0, x).view(v),
                                                                            np.where(ny, 0, y).view(v))


def make_envs(shape, m, noise, algorithm, capacity, kinds):
    """Envs on one matured world: "ac" continuous with a memory, "plain" neither, "calls"
    continuous without a memory."""
    from aigar_amd.env import AgarVecEnv
    p = lw.model_params(m)
    A, B, field, mv = shape[:4]
    prm = lw.env_parameters(p, NOISE_TYPE=noise, GAUSSIAN_NOISE=0.3, ALGORITHM=algorithm, **OU)
    kw = dict(n_arenas=A, field_size=field, max_viruses=mv, roles=lw.roles_of(B), seed=lw.SEED, desync=False,
              reset_limit=24 * (p.frame_skip + 1))
    opts = {"ac": dict(continuous=True, memory=dict(capacity=capacity)), "plain": {}, "calls": dict(continuous=True),
            "plain-memory": dict(memory=dict(capacity=capacity)),
            "ac-memory-unused": dict(continuous=True, memory=dict(capacity=capacity))}
    envs = []
    for k in kinds:
        e = AgarVecEnv(B, prm, **kw, **opts[k])
        e.obs.zero_()  # (the Greedy and Random bots' rows are never written)
        e.reset(lw.SEED)
        lw.mature(e.stepper, A, lw.SEED)  # (load_state: the bots start over)
        envs.append(e)
    return p, envs


def take_out(env, p, respawn):
    """Player p of arena 0 as the tick leaves a dead player: no cells, on the dead list."""
    st = env.stepper.get_state(0)
    keep = st["cells_i"][:, 0] != p
    st["cells_f"], st["cells_i"] = st["cells_f"][keep], st["cells_i"][keep]
    st["players_i"][p, 0], st["players_i"][p, 1], st["players_i"][p, 4] = 0, respawn, 0
    st["dead"] = np.concatenate([st["dead"], np.array([p], np.int64)])
    env.stepper.load_state(st, 0)


def grid_draws(rng, NP):
    return rng.integers(0, 2 ** 53, (NP, 2, T, 2)) * nm.GRID


@pytest.mark.parametrize("shape,m,noise,dtype,algorithm,capacity", CASES, ids=lw.SHAPE_IDS)
def test_step_ac_is_the_models_noise_stepped(shape, m, noise, dtype, algorithm, capacity):
    import torch
    p, (a, b, c) = make_envs(shape, m, noise, algorithm, capacity, ("ac", "plain", "calls"))
    A, B = shape[:2]
    NP, n = A * B, p.width
    kind = nm.ORN_UHL if noise == "Orn-Uhl" else nm.GAUSSIAN
    cc = a.continuous
    assert cc["n_act"] == n and cc["noise"] == noise and cc["store_raw"] == (algorithm == "CACLA")
    assert (cc["theta"], cc["mu"], cc["dt"], cc["std"]) == (0.3, 0.25, 0.5, 0.3) and a.noise_std.tolist() == [0.3]
    assert b.continuous is None and b.stepper.noi is None
    nn = np.array([r == "NN" for r in lw.roles_of(B)] * A)
    oa, ob, oc = a.observe(), b.observe(), c.observe()
    assert same(oa, ob) and same(oa, oc)
    deciding = ~np.isnan(ob.cpu().numpy()[:, 0]) & nn
    rng = np.random.default_rng(lw.SEED)
    held = np.zeros((NP, n))   # a player that does not decide keeps its last noisy row (zeros before the first)
    state = np.zeros((NP, n))  # ... and its Orn-Uhl state
    ring = {"a": np.zeros((capacity, 4)), "x": np.full((capacity, 4), np.nan), "v": np.zeros(capacity, bool)}
    nxt = size = added = added_at_update = 0
    silent_since_reset = np.zeros(NP, bool)
    n_died = n_silent = n_resets = n_resumed = n_clipped = 0
    L = a.stepper.obs_len
    for t in range(DECISIONS):
        mu = rng.random((NP, n)).astype(dtype)
        u = grid_draws(rng, NP)
        std = 0.3 if t < DECISIONS // 2 else 0.05
        if t == 6:  # arena 0's first deciding player is dead at the next two decisions; its bots start over
            out = int(np.nonzero(deciding[:B])[0][0])
            for env in (a, b, c):
                take_out(env, out, 2 * (p.frame_skip + 1) + 1)
            oa, ob = a.observe(), b.observe()
            assert same(oa, ob) and same(oa, c.observe())
            deciding = ~np.isnan(ob.cpu().numpy()[:, 0]) & nn
            assert not deciding[out]
            state[:B] = 0.0  # aigar_load_state clears the arena's Orn-Uhl state
            c._ou_ac[:B] = 0.0  # (a direct stepper call: the separate-calls path's own state follows by hand)
            silent_since_reset[:B] = False
        if t == DECISIONS // 2:  # the schedule is the caller's: a write, no re-capture
            a.set_noise(0.05)
            c.set_noise(0.05)
            # ... and the trainer's write-back of best actions: a duplicate (the last wins), a
            # negative index and one just past the ring's size are skipped
            assert 8 < size
            added_at_update = added
            idx = np.array([3, 5, 3, -1, size, 7, capacity + 2], np.int64)
            rows = rng.random((len(idx), n))
            a.update_actions(torch.as_tensor(idx, device="cuda"), torch.as_tensor(rows, device="cuda"))
            for j, i in enumerate(idx):
                if 0 <= i < size:
                    ring["x"][i], ring["v"][i] = np.concatenate([rows[j], np.zeros(4 - n)]), True
            # read back at once: the written slots hold the last row given, the others are as they were
            x_now, v_now = a.sample_extra(torch.arange(capacity, device="cuda"))
            assert nm.bits_equal(x_now.cpu().numpy(), ring["x"]) and np.array_equal(v_now.cpu().numpy(), ring["v"])
            assert ring["v"][[3, 5, 7]].all() and nm.bits_equal(ring["x"][3, :n], rows[2])
        want, new_state, exh, bad = nm.noise(mu, std, deciding, u, kind, state, cc["theta"], cc["mu"], cc["dt"])
        assert not bad.any()
        if kind == nm.ORN_UHL:
            state = new_state
        held = np.where(deciding[:, None], want, held)
        n_clipped += int(((want == 0.0) | (want == 1.0)).sum())
        n_resumed += int((deciding & silent_since_reset).sum())
        mu_t, u_t = torch.as_tensor(mu, device="cuda"), torch.as_tensor(u, device="cuda")
        ra, rb = a.step_ac(mu_t, u_t), b.step(torch.as_tensor(held, device="cuda"))
        obs_c, rew_c, _ = c.step_ac_calls(mu_t, u_t)
        done_c = c._episode_ends()  # (step_calls leaves the episode bookkeeping out)
        for x, y in zip(ra, rb):
            assert same(x, y), t
        assert same(c.obs, ra[0]) and same(rew_c, ra[1]) and same(done_c, ra[3]), t
        for env in (a, c):
            assert nm.bits_equal(env.noisy_action.cpu().numpy(), want), t
        # the decision's transitions: every deciding player's, in ascending order
        for i in np.nonzero(deciding)[0]:
            ring["a"][nxt] = np.concatenate([want[i], np.zeros(4 - n)])
            if cc["store_raw"]:
                ring["x"][nxt], ring["v"][nxt] = np.concatenate([mu[i].astype(np.float64), np.zeros(4 - n)]), True
            else:
                ring["x"][nxt], ring["v"][nxt] = np.nan, False
            nxt, size, added = (nxt + 1) % capacity, min(size + 1, capacity), added + 1
        obs, reward, alive, done = [x.cpu().numpy() for x in rb]
        alive_now = ~np.isnan(obs[:, 0]) & nn
        assert np.array_equal(alive, alive_now)
        n_silent += int((nn & ~deciding).sum())
        silent_since_reset |= nn & ~deciding
        n_died += int((deciding & ~alive_now & ~done).sum())
        n_resets += len(set((np.nonzero(done)[0] // B).tolist()))
        state[done] = 0.0  # aigar_reset_arenas clears the Orn-Uhl state
        silent_since_reset[done] = False
        kept = deciding & alive_now & ~done  # updateValues: the noisy row is the bot's currentAction
        assert kept.any() or done.any(), t
        assert nm.bits_equal(obs[kept][:, L - 8:L - 4], ring_pad(want[kept], n)), t
        deciding = alive_now
    # the run met what it was chosen for
    assert n_died >= 1 or p.frame_skip > 0, "no deciding NN player was dead at its observation"
    assert n_silent >= 2, "no NN player was dead at decision time"
    assert n_resumed >= 1, "no NN player decided again after it was dead at decision time"
    assert n_resets == A, "not every arena was reset once"
    assert n_clipped >= 1 and added - added_at_update >= capacity, "no clipped value / no ring wrap after the write-back"
    # the ring: the action rows and the fifth field of every slot
    info = a.stepper.exp_info()
    assert (info["added"], info["size"], info["next_idx"]) == (added, capacity, nxt)
    every = torch.arange(capacity, device="cuda")
    ac = torch.full((capacity, 4), -3.0, dtype=torch.float64, device="cuda")
    a.stepper.exp_gather(every, a=ac)
    assert nm.bits_equal(ac.cpu().numpy(), ring["a"])
    extra, valid = a.sample_extra(every)
    assert nm.bits_equal(extra.cpu().numpy(), ring["x"]) and np.array_equal(valid.cpu().numpy(), ring["v"])
    assert ring["v"].all() if cc["store_raw"] else not ring["v"].any()  # (the wrap overwrote the write-backs)
    # indices outside [0, size) leave the caller's rows as they are
    e2, v2 = a.sample_extra(torch.as_tensor([-1, capacity, 2], device="cuda"))
    assert np.isnan(e2.cpu().numpy()[:2]).all() and not v2.cpu().numpy()[:2].any()
    assert nm.bits_equal(e2.cpu().numpy()[2], ring["x"][2])
    for k in range(A):
        assert parity.diff_states(a.stepper.get_state(k), b.stepper.get_state(k), ftol=0.0) == []
        assert parity.diff_states(c.stepper.get_state(k), b.stepper.get_state(k), ftol=0.0) == []
    for env in (a, b, c):
        env.close()


def ring_pad(rows, n):
    return np.concatenate([rows, np.zeros((len(rows), 4 - n))], axis=1)


def test_update_actions_last_wins_and_out_of_range_is_skipped():
    """exp_extra_set on a memory filled by aigar_exp_add (whose slots start invalid)."""
    import torch
    from oracle_lib import make_config
    g = _lib.Stepper(make_config(n_arenas=1, bots=2, field_size=100, flags=0))
    g.reset(1)
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    g.exp_config(16, extra=True)
    Lr = g.obs_len
    s = torch.zeros((10, Lr), dtype=torch.float64, device="cuda")
    g.exp_add(s, torch.ones((10, 4), dtype=torch.float64, device="cuda"), torch.zeros(10, dtype=torch.float64, device="cuda"),
              s, torch.zeros(10, dtype=torch.uint8, device="cuda"))
    every = torch.arange(16, device="cuda")
    out = torch.full((16, 4), -5.0, dtype=torch.float64, device="cuda")
    val = torch.full((16,), 9, dtype=torch.uint8, device="cuda")
    g.exp_extra_get(every, out, val)
    o, v = out.cpu().numpy(), val.cpu().numpy()
    assert np.isnan(o[:10]).all() and (v[:10] == 0).all()       # aigar_exp_add leaves the extra invalid
    assert (o[10:] == -5.0).all() and (v[10:] == 9).all()       # beyond size: untouched
    rng = np.random.default_rng(0)
    idx = np.array([4, 9, 4, 10, -3, 0, 4, 9, 15], np.int64)     # size is 10: 10, -3 and 15 are skipped
    rows = rng.random((len(idx), 4))
    g.exp_extra_set(torch.as_tensor(idx, device="cuda"), torch.as_tensor(rows, device="cuda"))
    g.exp_extra_get(every, out, val)
    o, v = out.cpu().numpy(), val.cpu().numpy()
    want = np.full((10, 4), np.nan)
    want[4], want[9], want[0] = rows[6], rows[7], rows[5]
    assert nm.bits_equal(o[:10], want) and v[:10].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 0, 1]
    assert (o[10:] == -5.0).all() and (v[10:] == 9).all()
    # the scratch is clean again: a second write-back of other slots behaves the same
    g.exp_extra_set(torch.as_tensor([1, 1], device="cuda"), torch.as_tensor(rows[:2], device="cuda"))
    g.exp_extra_get(every, out, val)
    assert nm.bits_equal(out.cpu().numpy()[1], rows[1]) and val.cpu().numpy()[:10].tolist() == [1, 1, 0, 0, 1, 0, 0, 0, 0, 1]
    # resetting the memory clears the extras
    g.exp_config(16, extra=True)
    g.exp_add(s, torch.ones((10, 4), dtype=torch.float64, device="cuda"), torch.zeros(10, dtype=torch.float64, device="cuda"),
              s, torch.zeros(10, dtype=torch.uint8, device="cuda"))
    g.exp_extra_get(every, out, val)
    assert np.isnan(out.cpu().numpy()[:10]).all() and not val.cpu().numpy()[:10].any()
    g.close()


def test_reset_bots_and_reset_arenas_clear_the_orn_uhl_state():
    import torch
    p, (a,) = make_envs(lw.SHAPES[1], lw.MATRIX[0], "Orn-Uhl", "CACLA", 64, ("calls",))
    A, B = lw.SHAPES[1][:2]
    NP, n = A * B, 2
    nn = np.array([r == "NN" for r in lw.roles_of(B)] * A)
    cc = a.continuous
    rng = np.random.default_rng(3)
    state = np.zeros((NP, n))
    deciding = ~np.isnan(a.observe().cpu().numpy()[:, 0]) & nn
    mask = np.zeros(NP, np.uint8)
    mask[0:B:2] = 1  # the reset bots: every second player of arena 0
    for t in range(6):
        mu, u = rng.random((NP, n)), grid_draws(rng, NP)
        want, state, _, _ = nm.noise(mu, 0.3, deciding, u, nm.ORN_UHL, state, cc["theta"], cc["mu"], cc["dt"])
        obs = a.step_ac(torch.as_tensor(mu, device="cuda"), torch.as_tensor(u, device="cuda"))[0].cpu().numpy()
        assert nm.bits_equal(a.noisy_action.cpu().numpy(), want), t
        deciding = ~np.isnan(obs[:, 0]) & nn
        if t == 1:
            a.stepper.reset_bots(mask)
            state[mask.astype(bool)] = 0.0
        if t == 3:
            a.stepper.reset_arenas([2], [77])
            state[2 * B:3 * B] = 0.0
            deciding = ~np.isnan(a.observe().cpu().numpy()[:, 0]) & nn
    a.close()


def test_mixed_dtypes_and_perturb_leave_the_decision_alone():
    """step_ac(float32), perturb(float64), step_ac(float32), step_ac(float64) on an Orn-Uhl env:
    the players' state chain continues through all of it (every noisy row equals the model's,
    which carries the state), and the handle's noise is never configured again -- a
    reconfiguration is what would restart the state and drop the captured graph."""
    import torch
    p, (a,) = make_envs(lw.SHAPES[0], lw.MATRIX[0], "Orn-Uhl", "CACLA", 64, ("ac",))
    A, B = lw.SHAPES[0][:2]
    NP, n = A * B, 2
    nn = np.array([r == "NN" for r in lw.roles_of(B)] * A)
    cc = a.continuous

    def refuse(*args, **kw):
        raise AssertionError("the noise was configured again")
    a.stepper.noise_config = refuse
    mu_buf, noi = a._mu.data_ptr(), a.stepper.noi
    rng = np.random.default_rng(9)
    state = np.zeros((NP, n))
    deciding = ~np.isnan(a.observe().cpu().numpy()[:, 0]) & nn
    for t, dtype in enumerate(("float32", "float32", "float64", "float32", "float64", "float32")):
        mu, u = rng.random((NP, n)).astype(dtype), grid_draws(rng, NP)
        want, state, _, _ = nm.noise(mu, 0.3, deciding, u, nm.ORN_UHL, state, cc["theta"], cc["mu"], cc["dt"])
        obs = a.step_ac(torch.as_tensor(mu, device="cuda"), torch.as_tensor(u, device="cuda"))[0].cpu().numpy()
        assert nm.bits_equal(a.noisy_action.cpu().numpy(), want), t
        deciding = ~np.isnan(obs[:, 0]) & nn
        # the trainer's side between two decisions: the best actions read back as float64, perturbed
        # on the caller's own state, with the caller's draws, then with the device's, in either dtype
        best = rng.random((37, n))
        prev = rng.standard_normal((37, n)) * 0.1
        pu = rng.integers(0, 2 ** 53, (37, 2, T, 2)) * nm.GRID
        w2, s2, _, _ = nm.noise(best, 0.5, None, pu, nm.ORN_UHL, prev, cc["theta"], cc["mu"], cc["dt"])
        pt = torch.as_tensor(prev, device="cuda")
        got = a.perturb(torch.as_tensor(best, device="cuda"), std=0.5, u=torch.as_tensor(pu, device="cuda"), prev=pt)
        assert nm.bits_equal(got.cpu().numpy(), w2) and nm.bits_equal(pt.cpu().numpy(), s2), t
        a.perturb(torch.as_tensor(best.astype(np.float32), device="cuda"), prev=pt)
    assert (np.abs(state[nn]) > 0).any()
    assert a._mu.data_ptr() == mu_buf and a.stepper.noi == noi and a._mu.dtype == torch.float64
    a.close()


def test_without_the_feature_the_decision_is_as_it_was():
    """A memory without the flag on a handle without a noise config, beside a continuous env
    whose noise is never used: `step` gives the same outputs, worlds and memory rows bit for
    bit, and the unused fifth field stays invalid."""
    import torch
    shape, cap = lw.SHAPES[0], 48
    p, (x, y) = make_envs(shape, lw.MATRIX[1], "Gaussian", "CACLA", cap, ("plain-memory", "ac-memory-unused"))
    NP = shape[0] * shape[1]
    assert x.stepper.noi is None and y.stepper.noi is not None
    table = lw.action_table(lw.SEED, NP, 12, p.width)
    assert same(x.observe(), y.observe())
    for d in range(12):
        act = torch.as_tensor(table[d], device="cuda")
        for u, v in zip(x.step(act), y.step(act)):
            assert same(u, v), d
    bx, by = x.stepper.exp_info(), y.stepper.exp_info()
    assert bx == by and bx["added"] > cap
    every = torch.arange(cap, device="cuda")
    rows = []
    for e in (x, y):
        s = torch.zeros((cap, e.stepper.obs_len), dtype=torch.float64, device="cuda")
        s2, ac = torch.zeros_like(s), torch.zeros((cap, 4), dtype=torch.float64, device="cuda")
        r, dn = torch.zeros(cap, dtype=torch.float64, device="cuda"), torch.zeros(cap, dtype=torch.bool, device="cuda")
        e.stepper.exp_gather(every, s=s, a=ac, r=r, s2=s2, done=dn)
        rows.append((s, ac, r, s2, dn))
    for u, v in zip(*rows):
        assert same(u, v)
    extra, valid = y.sample_extra(every)
    assert torch.isnan(extra).all() and not valid.any()
    with pytest.raises(RuntimeError, match="continuous"):
        x.sample_extra(every)
    with pytest.raises(RuntimeError, match="continuous"):
        x.step_ac(torch.zeros((NP, 4), device="cuda"))
    for k in range(shape[0]):
        assert parity.diff_states(x.stepper.get_state(k), y.stepper.get_state(k), ftol=0.0) == []
    x.close()
    y.close()


def test_continuous_reads_its_parameters_and_excludes_discrete():
    import torch
    from aigar_amd.env import AgarVecEnv
    p = lw.env_parameters(lw.model_params(lw.MATRIX[2]), NOISE_TYPE="Gaussian", GAUSSIAN_NOISE=0.7, ALGORITHM="DPG")
    with pytest.raises(ValueError, match="exclude"):
        AgarVecEnv(4, p, field_size=100, continuous=True, discrete=True)
    with pytest.raises(ValueError, match="unknown keys"):
        AgarVecEnv(4, p, field_size=100, continuous=dict(sigma=1.0))
    with pytest.raises(ValueError, match="noise must be"):
        AgarVecEnv(4, p, field_size=100, continuous=dict(noise="Uniform"))
    env = AgarVecEnv(4, p, field_size=100, continuous=dict(seed=3))
    assert env.continuous == {"noise": "Gaussian", "theta": 0.15, "mu": 0.0, "dt": 0.01, "std": 0.7, "store_raw": False,
                              "seed": 3, "n_act": 3}
    env.reset()
    mu = torch.rand((4, 3), dtype=torch.float32, device="cuda")
    obs, reward, alive, done = env.step_ac(mu)  # the device's own draws
    assert obs.shape == (4, env.stepper.obs_len) and env.noisy_action.shape == (4, 3)
    na = env.noisy_action
    assert ((na >= 0) & (na <= 1)).all() and not torch.equal(na, mu.double())
    env.set_noise(0.0)
    env.step_ac(mu)
    assert torch.equal(env.noisy_action, mu.double())  # std 0: the actor's own output
    # perturb: any rows, an explicit std, its own draws; std 0 is the identity on [0, 1]
    many = torch.rand((37, 3), dtype=torch.float64, device="cuda")
    assert torch.equal(env.perturb(many), many) and not torch.equal(env.perturb(many, std=0.5), many)
    with pytest.raises(ValueError):
        env.step_ac(torch.zeros((4, 2), dtype=torch.float32, device="cuda"))
    for a in range(1):
        assert env.stepper.warnings(a) & (_abi.WARN_NOISE_NONFINITE | _abi.WARN_NOISE_EXHAUSTED) == 0
    env.close()
