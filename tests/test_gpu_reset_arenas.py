"""GPU: aigar_reset_arenas -- Field.reset of single arenas of a batched handle on
the device.  A reset arena must be the world of a one-arena handle after
reset(seed) (state, later ticks, observations, bot state), every other arena must
not notice; the vectorised environment's episode ends go through it.

aigar_reset (every arena), aigar_reset_arenas (the listed ones) and aigar_load_state
(the bots of one arena) share one restart path on the device: the last four tests
pin what the three calls have in common -- a reset dirty handle is a fresh handle,
a loaded arena's bots restart and its neighbours do not notice, the learners' side
buffers (pixel history, old states, Orn-Uhl state) restart with their arena, and a
tiled handle resets like a new one."""
import ctypes as C
import types

import numpy as np
import pytest

from aigar_amd import _abi
from oracle_lib import Oracle, make_config
import parity

pytestmark = pytest.mark.gpu
_lib = pytest.importorskip("aigar_amd._lib")

A, B, SIZE = 3, 32, 250
# every channel a handle may combine (ALL_PLAYER_GRID excludes the last-frame grids) and every extra
CH = (_abi.OBS_PELLET | _abi.OBS_SELF | _abi.OBS_WALL | _abi.OBS_ENEMY | _abi.OBS_VIRUS | _abi.OBS_SELF_SLF |
      _abi.OBS_SELF_LF | _abi.OBS_ENEMY_SLF | _abi.OBS_ENEMY_LF)
EX = 0x1F
GG = 121
HIST = slice(5 * GG, 9 * GG)  # the four last-frame grids (channel order: P S W E V | SSLF SLF ESLF ELF)
LAST_FOV = 9 * GG             # extras: lastFov, fov, mass, lastAction[4], secondLastAction[4]
ACT_PREV = slice(9 * GG + 7, 9 * GG + 11)


def config(arenas=A, **kw):
    return make_config(n_arenas=arenas, bots=B, field_size=SIZE, virus=True, max_viruses=6, channels=CH, extras=EX,
                       **kw)


def fatten(g):
    """Fresh players weigh 10 and can neither split (> 36) nor eject (>= 35): give them
    40 .. 82, so that the random policy below leaves blobs, split players and deaths."""
    for a in range(g.A):
        st = g.get_state(a)
        cf = np.array(st["cells_f"], np.float64).reshape(-1, 9)
        owner = np.asarray(st["cells_i"]).reshape(-1, 4)[:, 0]
        cf[:, 2] = 40.0 + 6.0 * (owner % 8)
        cf[:, 3] = np.sqrt(cf[:, 2] / np.pi)
        st["cells_f"] = cf.reshape(np.asarray(st["cells_f"]).shape)
        g.load_state(st, a)


def dirty_handle(seed=3, decisions=0):
    """A 3-arena world 40 ticks into a game of heavy players: blobs, multi-cell players,
    stale flags, owners, epochs and grids everywhere (asserted).  decisions: learner-style
    decisions on top, so that lastMass, the history grids and lastFovSize are non-trivial."""
    g = _lib.Stepper(config())
    g.reset(seed)
    fatten(g)
    for t in range(40):
        g.policy_random(p_split=0.05, p_eject=0.05, seed=seed)
        g.step(1)
    rng = np.random.default_rng(seed)
    for t in range(decisions):
        g.apply_actions(rng.random((A * B, 4)), enable_split=True, skipping=False, record=True)
        g.step(1)
        g.rewards(update_last=True)
        g.observe()
    return g


def assert_dirty(g):
    for a in range(A):
        st = g.get_state(a)
        ncells = np.bincount(np.asarray(st["cells_i"]).reshape(-1, 4)[:, 0].astype(int), minlength=B)
        assert int(st["n_blobs"]) > 0 and ncells.max() > 1, (a, int(st["n_blobs"]), ncells.max())


def fresh_one(seed):
    """The reference of a reset arena: a one-arena handle of the same config after reset(seed)."""
    r = _lib.Stepper(config(arenas=1))
    r.reset(seed)
    return r


def same_state(x, y):
    return parity.diff_states(x, y, ftol=0.0) == [] and np.array_equal(x["philox_key"], y["philox_key"])


def rows(a):
    return slice(a * B, (a + 1) * B)


def test_fresh_world_and_untouched_neighbour():
    s0, s2 = 5, 22
    g, twin = dirty_handle(), dirty_handle()
    assert_dirty(g)
    before = [g.get_state(a) for a in range(A)]
    g.reset_arenas([2, 0], [s2, s0])  # non-contiguous, unsorted
    r0, r2 = fresh_one(s0), fresh_one(s2)
    for a, ref in ((0, r0), (2, r2)):
        st = g.get_state(a)
        assert parity.diff_states(st, ref.get_state()) == [], a
        assert np.array_equal(st["philox_key"], ref.get_state()["philox_key"]), a  # the one-arena world's key
    assert same_state(g.get_state(1), before[1])
    assert same_state(g.get_state(1), twin.get_state(1))
    og, ot = g.observe(), twin.observe()
    assert parity.obs_close(og[rows(0)], r0.observe(), 0.0)
    assert parity.obs_close(og[rows(2)], r2.observe(), 0.0)
    assert parity.obs_close(og[rows(1)], ot[rows(1)], 0.0)
    for h in (g, twin, r0, r2):
        h.close()


def test_trajectory_after_the_reset_matches_oracle():
    s0, s2 = 5, 22  # (with the commands below both arenas see a kill and a respawn within 30 ticks)
    g, twin = dirty_handle(), dirty_handle()
    g.reset_arenas([2, 0], [s2, s0])
    orc = {0: Oracle(config(arenas=1)), 2: Oracle(config(arenas=1))}
    orc[0].reset(s0)
    orc[2].reset(s2)
    rng = np.random.default_rng(11)
    kinds = set()
    for t in range(30):
        cmd = parity.synthetic_commands(rng, None, A * B, SIZE, 0.1, 0.1)
        for h in (g, twin):
            h.set_commands(cmd)
            h.step(1)
        og, ot = g.observe(), twin.observe()
        for a, o in orc.items():
            o.set_commands(cmd[rows(a)])
            o.step(1)
            eg, eo = g.events(a), o.events()
            assert np.array_equal(eg, eo), "tick %d arena %d: events" % (t, a)
            kinds |= set(eo[:, 1].tolist())
            assert parity.diff_states(g.get_state(a), o.get_state()) == [], "tick %d arena %d" % (t, a)
            assert parity.obs_close(og[rows(a)], o.observe()), "tick %d arena %d: observation" % (t, a)
        assert np.array_equal(g.events(1), twin.events(1)), t
        assert same_state(g.get_state(1), twin.get_state(1)), t
        assert parity.obs_close(og[rows(1)], ot[rows(1)], 0.0), t
    assert {6, 8, 10} <= kinds, kinds  # pellets eaten, a cell eaten, a respawn
    for h in (g, twin, orc[0], orc[2]):
        h.close()


def test_bot_state_restarts():
    s = 9
    g, twin = dirty_handle(decisions=4), dirty_handle(decisions=4)
    o_before = g.observe()
    twin.observe()
    assert np.abs(np.nan_to_num(o_before[rows(1), HIST])).max() > 0 and np.nanmax(o_before[rows(1), LAST_FOV]) > 0
    g.reset_arenas([1], [s])
    rg, rt = g.rewards(update_last=False), twin.rewards(update_last=False)
    assert np.isnan(rg[rows(1)]).all()  # lastMass is None
    for a in (0, 2):
        assert np.isfinite(rg[rows(a)]).all() and np.array_equal(rg[rows(a)], rt[rows(a)])
    og, ot = g.observe(), twin.observe()
    assert not np.isnan(og[rows(1)]).any()  # every player lives again
    assert not og[rows(1), HIST].any() and not og[rows(1), LAST_FOV].any()
    ref = fresh_one(s)
    # all of a fresh bot's row, but the previous action: load_state leaves that buffer alone, so does this call
    keep = np.ones(og.shape[1], bool)
    keep[ACT_PREV] = False
    assert parity.obs_close(og[rows(1)][:, keep], ref.observe()[:, keep], 0.0)
    was_alive = ~np.isnan(o_before[rows(1), 0])  # (a dead player's row is NaN)
    assert was_alive.any()
    assert np.array_equal(og[rows(1), ACT_PREV][was_alive], o_before[rows(1), ACT_PREV][was_alive])
    for a in (0, 2):
        assert parity.obs_close(og[rows(a)], ot[rows(a)], 0.0)
    for h in (g, twin, ref):
        h.close()


def test_twice_in_a_row_all_at_once_and_single_arena_handles():
    s = 13
    g = dirty_handle()
    g.reset_arenas([1], [s])
    first = g.get_state(1)
    g.reset_arenas([1], [s])
    assert same_state(g.get_state(1), first)
    g.reset_arenas([0, 1, 2], [s, s, s])
    w = [g.get_state(a) for a in range(A)]
    assert same_state(w[0], first) and same_state(w[1], first) and same_state(w[2], first)
    o3 = g.observe()
    assert parity.obs_close(o3[rows(0)], o3[rows(1)], 0.0) and parity.obs_close(o3[rows(0)], o3[rows(2)], 0.0)
    # aigar_reset keys arena a's world by (seed, a): its arena 0 is that world; the key's
    # arena word is what differs for arenas 1 and 2, by design, so it is compared on its own
    g.reset(s)
    z = g.get_state(0)
    for a in range(A):
        assert parity.diff_states(w[a], z, ftol=0.0) == [], a
        assert w[a]["philox_key"].tolist() == [s, 0x9E3779B9], a
        assert g.get_state(a)["philox_key"].tolist() == [s, (a << 32) | 0x9E3779B9], a
    g.close()
    # one arena: reset_arena(0, s) is reset(s)
    one, ref = _lib.Stepper(config(arenas=1)), fresh_one(s)
    one.reset(4)
    fatten(one)
    for t in range(20):
        one.policy_random(0.05, 0.05, 4)
        one.step(1)
    one.observe()
    one.reset_arena(0, s)
    assert same_state(one.get_state(), ref.get_state())
    assert parity.obs_close(one.observe(), ref.observe(), 0.0)
    one.close()
    ref.close()


def test_env_episode_ends_on_the_device_and_graphs_survive():
    import torch
    from aigar_amd.env import AgarVecEnv
    p = types.SimpleNamespace(VIRUS_SPAWN=True, ENABLE_SPLIT=True, ENABLE_EJECT=False, ENABLE_GREEDY_SPLIT=True,
                              PELLET_GRID=True, SELF_GRID=True, WALL_GRID=True, ENEMY_GRID=True, VIRUS_GRID=True,
                              SELF_GRID_LF=True, ENEMY_GRID_LF=True, USE_FOVSIZE=True, USE_TOTALMASS=True,
                              USE_LAST_ACTION=True, USE_LAST_FOVSIZE=True, GRID_SQUARES_PER_FOV=11, EXTRA_INPUT=True,
                              FRAME_SKIP_RATE=1, RESET_LIMIT=16)
    roles = ["NN"] * 16 + ["Greedy"] * 8 + ["Random"] * 8
    env = AgarVecEnv(32, p, n_arenas=4, field_size=250, max_viruses=6, roles=roles, seed=1)
    env.reset(2)
    assert getattr(env.stepper, "_one", None) is None
    c1 = _abi.Config()
    C.memmove(C.byref(c1), C.byref(env.stepper.cfg), C.sizeof(_abi.Config))
    c1.n_arenas = 1
    ref = _lib.Stepper(c1)
    nn = np.array([r == "NN" for r in roles] * 4)
    k = n_done = 0
    gen = torch.Generator(device="cuda").manual_seed(2)
    for t in range(20):
        act = torch.rand((128, 4), dtype=torch.float64, device="cuda", generator=gen)
        obs, rew, alive, done = env.step(act)  # (the same decision graph throughout)
        for a in sorted(set((done.nonzero().flatten() // 32).tolist())):
            k += 1
            n_done += 1
            ref.reset(env.seed + 7919 * k)
            assert same_state(env.stepper.get_state(a), ref.get_state()), (t, a, k)
            first = obs[a * 32:(a + 1) * 32][torch.as_tensor(nn[a * 32:(a + 1) * 32], device=obs.device)]
            assert not torch.isnan(first).any(), (t, a)
    assert n_done >= 8  # every arena ended at least twice
    assert getattr(env.stepper, "_one", None) is None
    env.close()
    ref.close()


def test_bad_lists_are_refused_on_the_host():
    g = _lib.Stepper(config())
    g.reset(3)
    for t in range(3):
        g.policy_random(0.0, 0.0, 3)
        g.step(1)
    before = [g.get_state(a) for a in range(A)]
    for arenas, msg in (([A], "out of range"), ([-1], "out of range"), ([0, 2, 0], "duplicate"),
                        ([0, 1, 2, 1], "4 arenas listed")):
        with pytest.raises(RuntimeError, match=msg):
            g.reset_arenas(arenas, [7] * len(arenas))
    g.reset_arenas([], [])  # n == 0: nothing happens
    for a in range(A):
        assert same_state(g.get_state(a), before[a]), a
    g.close()
    tiled = _lib.Stepper(make_config(bots=B, field_size=SIZE, channels=_abi.OBS_PELLET, extras=0x3, tile_x=2,
                                     tile_y=1, tile_id=0))
    with pytest.raises(RuntimeError, match="tiled"):
        tiled.reset_arenas([0], [7])
    tiled.close()


def test_reset_of_a_dirty_handle_is_a_fresh_handle():
    """Every arena's state, key, observation row (history channels and extras) and reward equal
    a newly created handle's after the same reset, and stay so over later ticks.  One extra is
    compared on its own: Bot.reset leaves lastAction alone (bot.py:125-164 resets currentAction
    only), so the row's secondLastAction is the bot's from before the reset, as
    test_bot_state_restarts pins for reset_arenas; a new handle's is zero."""
    s = 17
    g, f = dirty_handle(decisions=4), _lib.Stepper(config())
    assert_dirty(g)
    o_before = g.observe()
    was_alive = ~np.isnan(o_before[:, 0])  # (a dead player's row is NaN)
    assert was_alive.any() and o_before[was_alive][:, ACT_PREV].any()
    keep = np.ones(o_before.shape[1], bool)
    keep[ACT_PREV] = False

    def same_rows(t):
        og, of = g.observe(), f.observe()
        assert parity.obs_close(og[:, keep], of[:, keep], 0.0), t
        live = ~np.isnan(of[:, 0])
        assert live.all() if t == "reset" else live.any(), t
        assert np.array_equal(og[was_alive & live][:, ACT_PREV], o_before[was_alive & live][:, ACT_PREV]), t
        assert not of[live][:, ACT_PREV].any(), t

    g.reset(s)
    f.reset(s)
    for a in range(A):
        sg, sf = g.get_state(a), f.get_state(a)
        assert parity.diff_states(sg, sf, ftol=0.0) == [], a
        assert sg["philox_key"].tolist() == [s, (a << 32) | 0x9E3779B9] == sf["philox_key"].tolist(), a
    same_rows("reset")
    assert np.isnan(g.rewards(update_last=False)).all() and np.isnan(f.rewards(update_last=False)).all()
    rng = np.random.default_rng(s)
    for t in range(10):
        cmd = parity.synthetic_commands(rng, None, A * B, SIZE, 0.1, 0.1)
        for h in (g, f):
            h.set_commands(cmd)
            h.step(1)
        for a in range(A):
            assert np.array_equal(g.events(a), f.events(a)), (t, a)
            assert same_state(g.get_state(a), f.get_state(a)), (t, a)
        same_rows(t)
    g.close()
    f.close()


def test_load_state_restarts_the_arenas_bots_and_spares_its_neighbours():
    s = 19
    g, twin = dirty_handle(decisions=4), dirty_handle(decisions=4)
    ref = fresh_one(s)
    loaded = ref.get_state()
    g.load_state(loaded, 1)
    assert same_state(g.get_state(1), loaded)
    rg, rt = g.rewards(update_last=False), twin.rewards(update_last=False)
    assert np.isnan(rg[rows(1)]).all()  # lastMass is None
    og, ot = g.observe(), twin.observe()
    assert not np.isnan(og[rows(1)]).any()
    assert not og[rows(1), HIST].any() and not og[rows(1), LAST_FOV].any()
    assert np.abs(np.nan_to_num(ot[rows(1), HIST])).max() > 0  # (the twin's bots kept theirs)
    for a in (0, 2):
        assert same_state(g.get_state(a), twin.get_state(a)), a
        assert np.isfinite(rg[rows(a)]).any() and np.array_equal(rg[rows(a)], rt[rows(a)], equal_nan=True), a
        assert parity.obs_close(og[rows(a)], ot[rows(a)], 0.0), a
    rng = np.random.default_rng(s)
    for t in range(5):
        cmd = parity.synthetic_commands(rng, None, A * B, SIZE, 0.1, 0.1)
        for h in (g, twin):
            h.set_commands(cmd)
            h.step(1)
        og, ot = g.observe(), twin.observe()
        for a in (0, 2):
            assert np.array_equal(g.events(a), twin.events(a)), (t, a)
            assert same_state(g.get_state(a), twin.get_state(a)), (t, a)
            assert parity.obs_close(og[rows(a)], ot[rows(a)], 0.0), (t, a)
    for h in (g, twin, ref):
        h.close()


SIDE = 12  # pixel state: SIDE x SIDE x [current | previous frame]


def learner_handle(draws):
    """The 3-arena world with a pixel history (AIGAR_PIX_LAST), a replay memory and
    Orn-Uhl noise, after one actor-critic decision per entry of draws."""
    g = _lib.Stepper(config())
    g.reset(3)
    g.pixel_config(SIDE, last=True, color_seed=1)
    g.exp_config(1024, dtype="float32")
    g.noise_config(2, "Orn-Uhl", mu_dtype="float64", seed=5)
    last = None
    for d in draws:
        last = decide(g, d)
    return g, last


def decide(g, draw):
    """One env_step_ac with the caller's mu rows and uniforms: (noisy actions, pixel states,
    transitions the decision added to the memory)."""
    import torch
    dev = lambda x: torch.as_tensor(np.ascontiguousarray(x), device="cuda")  # noqa: E731
    mu, u = draw
    reward = torch.zeros(A * B, dtype=torch.float64, device="cuda")
    obs = torch.zeros(g.pixel_state_shape, dtype=torch.float32, device="cuda")
    noisy = torch.full((A * B, 2), -7.0, dtype=torch.float64, device="cuda")
    before = g.exp_info()["added"]
    g.env_step_ac(dev(mu), dev(np.array([0.3])), reward, obs, u=dev(u), noisy=noisy)
    g.sync()
    return noisy.cpu().numpy(), obs.cpu().numpy(), g.exp_info()["added"] - before


@pytest.mark.parametrize("call", ("reset", "reset_arenas", "load_state"))
def test_side_buffers_restart_with_their_arena(call):
    """has_old, the Orn-Uhl state and the pixel history of the restarted arenas read as on a
    fresh handle at the next decision (no transition, the noise of a zero state, a zero
    previous frame); the other arenas' go on as the twin's."""
    s = 23
    rng = np.random.default_rng(s)
    draws = [(rng.random((A * B, 2)), rng.integers(0, 2 ** 53, (A * B, 2, 4, 2)) * 2.0 ** -53) for t in range(4)]
    (g, _), (twin, last) = learner_handle(draws[:3]), learner_handle(draws[:3])
    fresh, _ = learner_handle([])
    had_old = ~np.isnan(last[1][:, 0, 0, 0])  # the bots alive at the last decision hold an old state
    assert last[2] > 0 and had_old[rows(0)].any() and had_old[rows(2)].any()
    if call == "reset":
        g.reset(s)
    elif call == "reset_arenas":
        g.reset_arenas([1], [s])
    else:
        ref = fresh_one(s)
        g.load_state(ref.get_state(), 1)
        ref.close()
    restarted = (0, 1, 2) if call == "reset" else (1,)
    (ng, og, added_g), (nt, ot, added_t), (nf, of, added_f) = (decide(h, draws[3]) for h in (g, twin, fresh))
    assert added_f == 0 and added_t == int(had_old.sum())
    assert added_g == sum(int(had_old[rows(a)].sum()) for a in range(A) if a not in restarted)
    for a in range(A):
        r = rows(a)
        if a in restarted:
            assert not np.isnan(nf[r]).any() and np.array_equal(ng[r].view(np.uint64), nf[r].view(np.uint64)), a
            assert not np.isnan(og[r]).any() and not og[r][..., 1].any() and not of[r][..., 1].any(), a
        else:
            assert np.array_equal(ng[r].view(np.uint64), nt[r].view(np.uint64)), a
            assert np.array_equal(og[r], ot[r], equal_nan=True), a
            live = ~np.isnan(nt[r][:, 0])
            assert (nt[r][live] != nf[r][live]).any() and np.nan_to_num(ot[r][..., 1]).any(), a  # (not a fresh bot's)
    for h in (g, twin, fresh):
        h.close()


def test_reset_of_a_dirty_tiled_handle_is_a_fresh_tiled_handle():
    from aigar_amd.tiles import TiledArena
    s = 29
    cfg = make_config(bots=B, field_size=SIZE, virus=True, max_viruses=6, channels=CH, extras=EX)
    ta, tf = TiledArena(cfg, 2, 1), TiledArena(cfg, 2, 1)
    ta.reset(3)
    rng = np.random.default_rng(s)
    for t in range(12):
        ta.set_commands(parity.synthetic_commands(rng, None, B, SIZE, 0.1, 0.1))
        ta.tick()
        ta.observe()  # (history grids, observers and hand-offs to restart)
    ta.reset(s)
    tf.reset(s)
    assert parity.diff_states(ta.get_state(), tf.get_state(), ftol=0.0) == []
    for x, y in zip(ta.tiles, tf.tiles):
        assert same_state(x.get_state(), y.get_state())
    og, of = ta.observe(), tf.observe()
    assert not np.isnan(of).any() and parity.obs_close(og, of, 0.0)
    assert np.array_equal(ta.last_observers, tf.last_observers)
    ta.close()
    tf.close()
