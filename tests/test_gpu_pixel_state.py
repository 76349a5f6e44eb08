"""GPU: the learner's pixel state (CNN_P_REPR, bot.py:276-282) -- aigar_observe_pixel_state
and aigar_env_step under aigar_pixel_config -- against the reference's expression applied in
numpy to the CPU oracle's raw RGB frames (the oracle has no state mode).  Tolerance 0.

  gray  = numpy.average(rgb as float64, weights 0.298 0.587 0.114)   (test_gpu_pixels pins it)
  state = (gray - 255) / 100;  RGB: the uint8 subtraction wraps, ((b + 1) & 255) / 100
  float32 = the float64 state rounded once

The frame history (AIGAR_PIX_LAST) is modelled here per bot: the previous channels are the
current channels of the bot's last observation at which it was alive and observed, zeros
before the first one and after everything that resets the bot.
"""
import ctypes as C

import numpy as np
import pytest

from aigar_amd import _abi
from oracle_lib import Oracle, make_config
import parity
from test_facade import reference_like_parameters

pytestmark = pytest.mark.gpu

_lib = pytest.importorskip("aigar_amd._lib")

CH = _abi.OBS_PELLET | _abi.OBS_SELF | _abi.OBS_WALL | _abi.OBS_ENEMY
W = [0.298, 0.587, 0.114]
SENTINEL = -7.0


def state_of(frames, rgb):
    """float64 [N, side, side, C] pixel state of uint8 [N, side, side, 3] frames."""
    if rgb:
        return ((frames.astype(np.int64) + 1) & 255) / 100.0
    gray = np.average(frames.astype(np.float64), axis=-1, weights=W)
    return ((gray - 255) / 100)[..., None]


class Expect:
    """The expected rows, with the per-bot frame history."""

    def __init__(self, n, side, rgb, last, dtype):
        self.rgb, self.last, self.dtype = rgb, last, dtype
        self.prev = np.zeros((n, side, side, 3 if rgb else 1))

    def clear(self, mask=None):
        self.prev[slice(None) if mask is None else np.asarray(mask, bool)] = 0.0

    def observe(self, frames, alive, out, mask=None):
        """Writes the rows of the observed players into out (the others stay)."""
        cur = state_of(frames, self.rgb)
        for i in range(len(cur)):
            if mask is not None and not mask[i]:
                continue
            if not alive[i]:
                out[i] = np.nan  # (the history stays)
                continue
            row = np.concatenate([cur[i], self.prev[i]], axis=2) if self.last else cur[i]
            out[i] = row.astype(self.dtype)
            self.prev[i] = cur[i]
        return out


def same(x, y):
    return x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y, equal_nan=True)


def first_diff(x, y):
    bad = np.argwhere(~((x == y) | (np.isnan(x) & np.isnan(y))))
    return "no difference" if not len(bad) else "%d differ, first %s: %r != %r" % (
        len(bad), tuple(bad[0]), x[tuple(bad[0])], y[tuple(bad[0])])


def pair(cfg, seed):
    g, o = _lib.Stepper(cfg), Oracle(cfg)
    g.reset(seed)
    o.reset(seed)
    return g, o


def stepper_of(rng, g, o, bots, ps=0.0, pe=0.0):
    size = g.get_state()["field_size"]

    def go(ticks):
        err, _ = parity.run_pair(g, o, ticks, lambda t: parity.synthetic_commands(rng, None, bots, size, ps, pe))
        assert err is None, err
    return go


def alive_of(o):
    return o.player_stats()[:, 0] > 0


# ------------------------------------------------------------------ 1. values and layout
@pytest.mark.parametrize("seed,side,kw", [
    (2, 42, dict()),
    (2, 41, dict()),                                   # odd side
    (3, 84, dict(virus=True, max_viruses=40)),
])
def test_state_values_and_layout(seed, side, kw):
    torch = pytest.importorskip("torch")
    bots = 32
    g, o = pair(make_config(bots=bots, channels=CH, extras=0, **kw), seed)
    stepper_of(np.random.default_rng(seed), g, o, bots, 0.05, 0.05)(60)
    alive = alive_of(o)
    assert alive.any()
    for cseed in (0, 12345):
        frames = o.pixels(side, cseed)
        assert np.any(frames[alive] != 255)
        for rgb in (False, True):
            g.pixel_config(side, rgb=rgb, color_seed=cseed)
            c = 3 if rgb else 1
            assert g.pixel_state_shape == (bots, side, side, c)
            for dtype in (np.float64, np.float32):
                want = Expect(bots, side, rgb, False, dtype).observe(frames, alive, np.zeros((bots, side, side, c), dtype))
                got = g.observe_pixel_state(dtype=dtype)
                assert got.shape == (bots, side, side, c) and got.dtype == dtype
                assert same(got, want), (cseed, rgb, dtype, first_diff(got, want))
                dev = torch.full((bots, side, side, c), SENTINEL, device="cuda",
                                 dtype=torch.float64 if dtype == np.float64 else torch.float32)
                g.observe_pixel_state(out=dev)
                g.sync()
                assert same(dev.cpu().numpy(), got), (cseed, rgb, dtype)
    assert np.all(np.isnan(got[~alive]))
    g.pixel_config(None)
    assert g.pixel_state_shape is None
    g.close()
    o.close()


# ------------------------------------------------------------------ 2. both passes under a mask
def in_view_counts(o):
    """Per player: pellet centres inside its view, and an upper bound of the objects of any
    kind that can touch it (centre within the view grown by the object's radius + 1)."""
    st, ps = o.get_state(), o.player_stats()
    pel = np.asarray(st["pellets_f"]).reshape(-1, 4)
    objs = np.concatenate([pel, np.asarray(st["cells_f"]).reshape(-1, 9)[:, :4],
                           np.asarray(st["blobs_f"]).reshape(-1, 8)[:, :4],
                           np.asarray(st["viruses_f"]).reshape(-1, 8)[:, :4]])
    pellets, total = [], []
    for alive, _, fx, fy, fs in ps:
        h = fs / 2
        pellets.append(int(np.sum((np.abs(pel[:, 0] - fx) < h) & (np.abs(pel[:, 1] - fy) < h))))
        r = objs[:, 3] + 1
        total.append(int(np.sum((np.abs(objs[:, 0] - fx) <= h + r) & (np.abs(objs[:, 1] - fy) <= h + r))))
    return np.array(pellets), np.array(total), ps[:, 0] > 0


@pytest.mark.parametrize("field,seed,rgb,dtype,mixed", [
    (130, 7, False, np.float32, True),    # players on both sides of the 256-object first-pass list
    (130, 7, True, np.float64, True),
    (100, 6, False, np.float64, False),   # every frame goes to the second pass
])
def test_mask_holds_in_both_passes(field, seed, rgb, dtype, mixed):
    bots, side = 8, 42
    g, o = pair(make_config(bots=bots, channels=CH, extras=0, field_size=field, max_pellets=1500), seed)
    go = stepper_of(np.random.default_rng(seed), g, o, bots)
    go(30)
    pellets, total, alive = in_view_counts(o)
    print("pellet centres in view", pellets.tolist(), "objects near the view", total.tolist())
    if mixed:
        assert np.any(alive & (pellets >= 300)) and np.any(alive & (total <= 200)), (pellets, total, alive)
    else:
        assert np.all(pellets[alive] > 256) and alive.all(), (pellets, alive)
    g.pixel_config(side, rgb=rgb, last=True, color_seed=seed)
    c = 6 if rgb else 2
    exp = Expect(bots, side, rgb, True, dtype)
    odd = (np.arange(bots) % 2).astype(np.uint8)  # every player is masked in once and out once
    for step, mask in enumerate([None, odd, 1 - odd, None]):
        if step:
            go(2)
        frames, alive = o.pixels(side, seed), alive_of(o)
        got = np.full((bots, side, side, c), SENTINEL, dtype)
        want = exp.observe(frames, alive, got.copy(), mask)
        g.observe_pixel_state(out=got, mask=mask)
        assert same(got, want), (step, first_diff(got, want))
        if mask is not None:  # the masked-out rows were not written
            assert np.all(got[mask == 0] == dtype(SENTINEL))
    # (step 2 showed the players masked out at step 1 their step-0 frame as the previous
    # one; step 3 shows the players masked out at step 2 their step-1 frame)
    g.close()
    o.close()


# ------------------------------------------------------------------ 3. history and death
def test_history_follows_the_bot_and_its_resets():
    bots, side, seed = 16, 42, 4
    g, o = pair(make_config(bots=bots, channels=CH, extras=0, field_size=80), seed)
    go = stepper_of(np.random.default_rng(seed), g, o, bots, 0.05, 0.05)
    g.pixel_config(side, last=True, color_seed=seed)
    exp = Expect(bots, side, False, True, np.float32)

    def check(tag, mask=None):
        frames, alive = o.pixels(side, seed), alive_of(o)
        want = exp.observe(frames, alive, np.zeros((bots, side, side, 2), np.float32), mask)
        got = g.observe_pixel_state()
        assert same(got, want), (tag, first_diff(got, want))
        return got, alive

    go(96)
    got, alive = check(96)
    assert alive.any() and np.all(got[alive][..., 1] == 0.0) and np.any(got[alive][..., 0] != 0.0)
    dead_rows = 0
    for t in range(100, 141, 4):
        go(4)
        got, alive = check(t)
        dead_rows += int((~alive).sum())
        assert np.all(np.isnan(got[~alive]))
        assert np.any(got[alive][..., 1] != 0.0)
    assert dead_rows > 0, "no player was dead at an observation: the NaN rule went untested"
    # Bot.reset for half of the bots: their previous frame is cleared, the others' is kept
    half = (np.arange(bots) < bots // 2).astype(np.uint8)
    g.reset_bots(half)
    exp.clear(half)
    go(1)
    got, alive = check("reset_bots")
    assert np.all(got[alive & (half == 1)][..., 1] == 0.0) and np.any(got[alive & (half == 0)][..., 1] != 0.0)
    # a loaded world restarts its bots
    st = g.get_state()
    g.load_state(st)
    o.load_state(st)
    exp.clear()
    got, alive = check("load_state")
    assert np.all(got[alive][..., 1] == 0.0)
    got, alive = check("after load_state")
    assert np.any(got[alive][..., 1] != 0.0)
    # and so does a reset
    g.reset(seed + 1)
    o.reset(seed + 1)
    exp.clear()
    got, alive = check("reset")
    assert alive.all() and np.all(got[..., 1] == 0.0)
    g.close()
    o.close()


# ------------------------------------------------------------------ 4. decision graph and env
def cnn_parameters(**kw):
    p = reference_like_parameters(False, True, False, 6)
    p.GRID_VIEW_ENABLED = True
    p.CNN_REPR = p.CNN_P_REPR = True
    p.CNN_USE_L1, p.CNN_INPUT_DIM_1 = True, 42
    p.CNN_P_RGB, p.CNN_LAST_GRID = False, True
    p.FRAME_SKIP_RATE, p.RESET_LIMIT = 1, 12
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_env_decisions_carry_the_pixel_state():
    torch = pytest.importorskip("torch")
    from aigar_amd.env import AgarVecEnv
    A, B, side, seed = 3, 6, 42, 5
    roles = ["NN", "Greedy", "NN", "Random", "NN", "Greedy"]
    p = cnn_parameters()
    a = AgarVecEnv(B, p, n_arenas=A, field_size=150, roles=roles, seed=seed)
    b = AgarVecEnv(B, p, n_arenas=A, field_size=150, roles=roles, seed=seed)
    assert a.pixels == (side, False, True) and tuple(a.obs.shape) == (A * B, side, side, 2)
    assert a.obs.dtype == torch.float32
    nn = np.array([r == "NN" for r in roles] * A)
    c1 = _abi.Config()
    C.memmove(C.byref(c1), C.byref(a.stepper.cfg), C.sizeof(_abi.Config))
    c1.n_arenas = 1
    orc = Oracle(c1)
    exp = Expect(A * B, side, False, True, np.float32)

    def expected(into):
        """The NN rows after an observation of the worlds as they are now."""
        for k in range(A):
            orc.load_state(a.stepper.get_state(k))
            sl = slice(k * B, (k + 1) * B)
            sub = Expect(B, side, False, True, np.float32)
            sub.prev = exp.prev[sl]  # (a view: the arena's bots)
            sub.observe(orc.pixels(side, seed), alive_of(orc), into[sl], nn[sl])
        return into

    def check(tag, obs, other):
        got = obs.cpu().numpy()
        assert np.all(got[~nn] == np.float32(SENTINEL)), tag  # rows of the Greedy and Random bots: never written
        want = expected(np.full(got.shape, SENTINEL, np.float32))
        assert same(got, want), (tag, first_diff(got, want))
        assert same(other.cpu().numpy(), got), (tag, "graph != separate calls")

    for env in (a, b):
        env.obs.fill_(SENTINEL)
    oa, ob = a.reset(seed), b.reset(seed)
    check("reset", oa, ob)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    n_done = 0
    for t in range(7):
        act = torch.rand((A * B, 4), dtype=torch.float64, device="cuda", generator=gen)
        oa, ra, la, done = a.step(act)
        ob, rb, lb = b.step_calls(act)
        done_b = b._episode_ends()  # (step_calls leaves the episode bookkeeping out)
        ob = b.obs.clone()
        torch.cuda.synchronize()
        assert torch.equal(done, done_b) and torch.equal(ra, rb), t
        ended = sorted(set((done.nonzero().flatten() // B).tolist()))
        m = np.zeros(A * B, bool)
        for k in ended:
            m[k * B:(k + 1) * B] = True
        # an ended arena was reset after the decision's observation: its bots' history is
        # cleared and their rows are the fresh world's first states
        exp.clear(m)
        check(t, oa, ob)
        if ended:
            n_done += len(ended)
            got = oa.cpu().numpy()
            first = got[m & nn]
            assert not np.isnan(first).any() and np.all(first[..., 1] == 0.0) and np.any(first[..., 0] != 0.0), t
            assert np.any(np.nan_to_num(got[~m & nn][..., 1]) != 0.0), t  # the other arenas' history goes on
        assert torch.equal(la, ~torch.isnan(oa.view(A * B, -1)[:, 0]) & a.nn)
    assert n_done >= 1
    # the pixel state off and on again: the decision graph is captured anew each time
    grid = torch.full((A * B, a.stepper.obs_len), SENTINEL, dtype=torch.float64, device="cuda")
    for env in (a, b):
        env.stepper.pixel_config(None)
    act = torch.rand((A * B, 4), dtype=torch.float64, device="cuda", generator=gen)
    buf = a._act[4]
    buf.copy_(act)
    a.stepper.env_step(buf, a._r, grid, a.enable_split, a.skip, a.reward_params)
    want_grid = torch.full_like(grid, SENTINEL)
    greedy = torch.as_tensor(b.roles == _abi.ROLE_GREEDY, device="cuda").to(torch.uint8)
    for k in range(b.skip + 1):  # (the decision as step_calls makes it)
        b.stepper.apply_actions(act, b.enable_split, skipping=k > 0, record=k == 0)
        b.stepper.policy_greedy(False, greedy)
        b.stepper.policy_random_bots()
        b.stepper.step(1)
    b.stepper.observe(want_grid, mask=b._nn_u8)
    torch.cuda.synchronize()
    assert torch.equal(torch.nan_to_num(grid, nan=-9.0), torch.nan_to_num(want_grid, nan=-9.0))
    for env in (a, b):
        env.stepper.pixel_config(side, rgb=False, last=True, color_seed=seed)
        env.age[:] = 0  # (no episode ends in the decisions below)
    exp.clear()
    for t in range(2):
        act = torch.rand((A * B, 4), dtype=torch.float64, device="cuda", generator=gen)
        oa = a.step(act)[0]
        ob = b.step_calls(act)[0]
        check("again %d" % t, oa, ob)
    orc.close()
    a.close()
    b.close()


# ------------------------------------------------------------------ 5. refusals
def test_refusals_are_made_on_the_host():
    torch = pytest.importorskip("torch")
    g = _lib.Stepper(make_config(bots=2, channels=CH, extras=0))
    g.reset(0)
    with pytest.raises(RuntimeError, match="configured"):
        g.observe_pixel_state()
    with pytest.raises(RuntimeError, match="configured"):
        g._chk(g.L.aigar_observe_pixel_state(g.h, C.c_void_p(1), 1, 0, None, 0))
    assert g.L.aigar_pixel_state_len(g.h) == 0
    for side in (85, -1):
        with pytest.raises(RuntimeError, match="side"):
            g.pixel_config(side)
    with pytest.raises(RuntimeError, match="flags"):
        g._chk(g.L.aigar_pixel_config(g.h, C.byref(_abi.PixelParams(42, 4, 0))))
    assert g.pixel_state_shape is None and g.L.aigar_pixel_state_len(g.h) == 0
    g.pixel_config(42, rgb=True, last=True)
    assert g.L.aigar_pixel_state_len(g.h) == 42 * 42 * 6
    for bad in (np.zeros((2, 42, 42, 3), np.float32), np.zeros((2, 42, 42, 6), np.uint8),
                np.zeros((2, 6, 42, 42), np.float64), np.zeros((2, 42, 42, 12), np.float32)[..., ::2]):
        with pytest.raises(ValueError):
            g.observe_pixel_state(out=bad)
    act = torch.zeros((2, 4), dtype=torch.float64, device="cuda")
    rew = torch.zeros(2, dtype=torch.float64, device="cuda")
    for bad in (torch.zeros((2, g.obs_len), dtype=torch.float64, device="cuda"),
                torch.zeros((2, 42, 42, 3), dtype=torch.float32, device="cuda"),
                torch.zeros((2, 42, 42, 6), dtype=torch.float16, device="cuda")):
        with pytest.raises(ValueError):
            g.env_step(act, rew, bad)
    g.pixel_config(None)
    with pytest.raises(ValueError):  # and the grid row's check is as it was
        g.env_step(act, rew, torch.zeros((2, 42, 42, 6), dtype=torch.float32, device="cuda"))
    g.close()
    tiled = _lib.Stepper(make_config(bots=4, channels=CH, extras=0, tile_flags=_abi.TILE_FORCE))
    with pytest.raises(RuntimeError, match="tiled"):
        tiled.pixel_config(42)
    tiled.close()
