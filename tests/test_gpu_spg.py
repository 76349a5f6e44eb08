"""GPU: aigar_spg_step (spg.inc) against the Python model (tests/spg_model.py), bit pattern for bit
pattern after every step: the actor's and the critic's weights, both targets, both networks' Adam
m and v, the counters, the TD errors, the drawn indices, the prioritized memory's trees (through a
sample with given draws), the memory's fifth field and its valid bytes, the noise double and the
pad checks.  No tolerance anywhere.  The worlds are tests/spg_worlds.py's; tests/test_spg_model.py
checks on the CPU that each of them is worth comparing."""
import ctypes as C

import numpy as np
import pytest

import net_model as M
import spg_model as SM
import spg_worlds as W
from oracle_lib import make_config

pytestmark = pytest.mark.gpu
from aigar_amd import _abi, _lib  # noqa: E402

F32 = np.float32
CH7 = (_abi.OBS_PELLET | _abi.OBS_SELF | _abi.OBS_WALL | _abi.OBS_ENEMY | _abi.OBS_VIRUS | _abi.OBS_SELF_LF
       | _abi.OBS_ENEMY_LF)
CH6 = CH7 & ~_abi.OBS_ENEMY_LF
CH5 = _abi.OBS_PELLET | _abi.OBS_SELF | _abi.OBS_WALL | _abi.OBS_ENEMY | _abi.OBS_VIRUS
# state width -> (grid_squares, channels, extras) of a handle whose observation row has it
WIDTHS = {3: (1, _abi.OBS_PELLET | _abi.OBS_SELF | _abi.OBS_WALL, 0),
          61: (3, CH6, _abi.EX_LAST_FOV | _abi.EX_FOV | _abi.EX_MASS | _abi.EX_LAST_ACT),
          62: (3, CH6, _abi.EX_LAST_ACT | _abi.EX_2LAST_ACT), 64: (3, CH7, _abi.EX_FOV),
          130: (5, CH5, _abi.EX_FOV | _abi.EX_LAST_ACT)}
FUSED = [0, 1]  # the search as a composition of launches, and fused into k_spg_search: both equal the model
_G = {}


@pytest.fixture(scope="module", autouse=True)
def close_handles():
    yield
    for g in _G.values():
        g.close()
    _G.clear()


def handle(width):
    if width not in _G:
        import torch
        g, ch, ex = WIDTHS[width]
        st = _lib.Stepper(make_config(n_arenas=2, bots=5, field_size=100, grid_squares=g, channels=ch, extras=ex,
                                      virus=bool(ch & _abi.OBS_VIRUS), flags=0))
        assert st.obs_len == width
        st.set_stream(torch.cuda.current_stream().cuda_stream)  # (ordered with the tensors torch makes and reads)
        st.reset(11)
        _G[width] = st
    return _G[width]


def dev(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    v = np.uint64 if a.dtype.itemsize == 8 else np.uint32
    return np.array_equal(a.view(v), b.view(v))


def noise_tensor(st):
    """The device double of the search noise as a one-element tensor (no copy)."""
    import torch

    class Ptr:
        __cuda_array_interface__ = {"shape": (1,), "typestr": "<f8", "data": (st.spg_noise_ptr(), False), "version": 2}
    return torch.as_tensor(Ptr(), device="cuda")


class Case:
    """A handle configured as the world says, and the model's run beside it."""

    def __init__(self, fused=0, seed_own=0, **kw):
        self.w = w = W.World(**kw)
        self.st = st = handle(w.n_in)
        self.run = W.ModelRun(w)
        self.tr = self.run.tr
        st.exp_config(W.CAP, prioritized=w.prio, dtype=w.dtype, seed=3, extra=True)
        st.net_config((w.n_in, w.actor, w.ha, "sigmoid"), x_dtype=w.dtype)
        st.qcritic_config((w.n_in + w.n_act, w.critic, w.hc, "linear"), x_dtype=w.dtype)
        st.net_set_weights(w.a0)
        st.critic_set_weights(w.c0)
        if w.rows is not None:
            st.exp_add(*w.rows)
            v = np.flatnonzero(w.valid)
            if len(v):
                st.exp_extra_set(dev(v.astype(np.int64)), dev(w.extra[v]))
        st.spg_config(batch=w.batch, fused=fused, seed=seed_own, **w.kw)

    def steps(self, n, u=None, zu=None, calls=1):
        """n steps on both sides from the same draws; the device's in `calls` calls."""
        if u is None or zu is None:
            du, dzu = self.w.draws(n)
            u, zu = du if u is None else u, dzu if zu is None else zu
        for part in np.split(np.arange(n), calls):
            self.st.spg_step(len(part), dev(u[part]), dev(zu[part]) if self.tr.K else None)
        self.run.run(u, zu)

    def check(self, what):
        import torch
        st, tr, run, w = self.st, self.tr, self.run, self.w
        info = st.spg_info()
        got = tuple(info[k] for k in ("steps", "skipped", "since_target", "actor_steps", "actor_skipped", "actor_empty",
                                      "selected")) + (0,)
        assert got == tr.info(), (what, got, tr.info())
        sets = [("actor " + k, st.net_get_weights(k), x, st.net_pad_check(k))
                for k, x in (("online", tr.a.theta), ("target", tr.target_a), ("m", tr.a.m), ("v", tr.a.v))]
        sets += [("critic " + k, st.critic_get_weights(k), x, st.critic_pad_check(k))
                 for k, x in (("online", tr.c.theta), ("target", tr.target_c), ("m", tr.c.m), ("v", tr.c.v))]
        for name, got, want, pad in sets:
            for l, ((Wg, b), (Ww, bw)) in enumerate(zip(got, want)):
                assert np.isfinite(Ww).all() and np.isfinite(bw).all(), (what, name, l)
                assert same_bits(Wg, Ww), (what, name, l, int((Wg.view(np.uint32) != Ww.view(np.uint32)).sum()), Wg.size)
                assert same_bits(b, bw), (what, name, l, b, bw)
            assert pad == 0, (what, name)
        assert same_bits(noise_tensor(st).cpu().numpy(), np.array([tr.noise])), (what, "noise")
        if run.last_idx is not None:
            B = w.batch
            td = torch.full((B + 1,), -7.25, dtype=torch.float64, device="cuda")
            idx = torch.full((B + 1,), -7, dtype=torch.int64, device="cuda")
            st.spg_td(td[:B], idx[:B])
            td, idx = td.cpu().numpy(), idx.cpu().numpy()
            assert td[-1] == -7.25 and idx[-1] == -7, "the entry behind the last one was written"
            assert idx[:-1].tolist() == list(run.last_idx), what
            if tr.td is not None and tr.can_draw(run.rm.size):
                fin = np.isfinite(tr.td)
                assert same_bits(td[:-1][fin], tr.td[fin]), what
                assert np.array_equal(np.isfinite(td[:-1]), fin), what
        if w.prio and run.rm.size >= 2:  # the trees: a sample's indices and weights are functions of their sums
            u = np.linspace(0.0, 0.999, 23)
            wt = torch.zeros(23, dtype=torch.float64, device="cuda")
            i = torch.zeros(23, dtype=torch.int64, device="cuda")
            st.exp_sample(wt, i, u=dev(u))
            wi, ww = run.rm.sample(list(u))
            assert i.cpu().numpy().tolist() == list(wi), what
            assert same_bits(wt.cpu().numpy(), np.asarray(ww, np.float64)), what
        if run.rm.size:  # the fifth field of every held slot
            n = run.rm.size
            out = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
            val = torch.zeros(n, dtype=torch.uint8, device="cuda")
            st.exp_extra_get(dev(np.arange(n, dtype=np.int64)), out, val)
            assert val.cpu().numpy().tolist() == run.valid[:n].tolist(), what
            v = run.valid[:n].astype(bool)
            assert same_bits(out.cpu().numpy()[v], run.extra[:n][v]), (what, "extras")


def moved(now, start):
    return sum(int((Wn.view(np.uint32) != W0.view(np.uint32)).sum()) for (Wn, _), (W0, _) in zip(now, start))


@pytest.mark.parametrize("fused", FUSED)
@pytest.mark.parametrize("name", list(W.CASES))
def test_worlds_step_by_step(name, fused):
    kw, n = W.CASES[name]
    c = Case(fused=fused, **kw)
    u, zu = c.w.draws(n)
    for k in range(n):
        c.steps(1, u[k:k + 1], zu[k:k + 1])
        c.check((name, k))
    assert c.tr.c.t == n and c.run.worth_comparing(sources=c.w.batch > 1)
    assert moved(c.tr.c.theta, c.w.c0) > 0 and moved(c.tr.a.theta, c.w.a0) > 0, "a network did not move"
    assert moved(c.tr.target_c, c.w.c0) > 0 and moved(c.tr.target_a, c.w.a0) > 0, "a target did not move"


@pytest.mark.parametrize("fused", FUSED)
def test_done_rows_and_duplicate_indices_under_replace(fused):
    n = 40
    done = np.zeros(n, bool)
    done[[0, 15, 16, 17, 31, 32]] = True
    c = Case(fused=fused, n_in=61, actor=(16, 16, 3), critic=(17, 25, 1), batch=33, done=done, seed=5)
    u = (np.arange(33)[None, :] + 0.5) / n * np.ones((3, 1))  # slot k in row k: the done rows sit at the tile edges
    u[:, 20:] = u[:, 3:16]  # ... and slots 3..15 are drawn twice: the last entry's row is written back
    _, zu = c.w.draws(3)
    for k in range(3):
        c.steps(1, u[k:k + 1], zu[k:k + 1])
        assert len(set(c.run.last_idx)) < 33
        c.check(("edges", k))
    assert c.tr.c.t == 3 and c.run.worth_comparing()
    # the two entries of a slot searched with other draws: the case tells the last from the first
    i = np.asarray(c.run.last_idx)
    assert any(not same_bits(c.tr.best[j], c.tr.best[j + 17]) for j in range(3, 16) if i[j] == i[j + 17])


def crafted_zu(B, K, rng):
    """Uniforms whose first accepted attempt sits at 0, 1, 7 and 15, and one pair with none: an
    attempt at (0.99, 0.99) lies outside the unit circle, one at (0.5, 0.5) is r2 = 0."""
    zu = rng.random((1, B, K, 2, 16, 2))
    ok = zu[0, 0, 0, 0, 0].copy()
    assert (2 * ok[0] - 1) ** 2 + (2 * ok[1] - 1) ** 2 < 1
    for r in range(B):
        first = (0, 1, 7, 15)[r % 4]
        for x in range(K):
            for pair in range(2):
                zu[0, r, x, pair, :first] = 0.99 if (r + x) % 2 else 0.5
                zu[0, r, x, pair, first] = ok
    zu[0, 1, 0, 0, :, :] = 0.99  # row 1, sample 0, pair 0: exhausted
    return zu


@pytest.mark.parametrize("fused", FUSED)
def test_rejected_attempts_and_an_exhausted_pair(fused):
    c = Case(fused=fused, n_in=62, actor=(15, 4), critic=(25, 1), batch=17, samples=2, seed=7)
    c.st.reset(11)  # (the warn bits are sticky since the last reset)
    u, _ = c.w.draws(2)
    rng = np.random.default_rng(5)
    c.steps(1, u[:1], rng.random((1, 17, 2, 2, 16, 2)))
    c.check("plain")
    assert c.st.warnings(0) & _abi.WARN_NOISE_EXHAUSTED == 0 and c.tr.exhausted == 0
    c.steps(1, u[1:], crafted_zu(17, 2, rng))
    assert c.tr.exhausted == 1
    c.check("crafted")
    assert c.st.warnings(0) & _abi.WARN_NOISE_EXHAUSTED


@pytest.mark.parametrize("fused", FUSED)
def test_own_draws_are_the_models_philox(fused):
    """zu NULL: Philox under arena 0's key at (row, 12 | pair << 8 | b << 16 | x << 24, the step's
    ordinal, seed): two seeds, three steps, and the ordinal starting over at aigar_spg_reset."""
    kw = dict(n_in=62, actor=(15, 3), critic=(25, 1), batch=17, samples=5, seed=8)
    firsts = []
    for seed in (9, 10):
        c = Case(fused=fused, seed_own=seed, **kw)
        key = c.st.get_state(0)["philox_key"]
        u, _ = c.w.draws(4)
        for k in range(4):
            if k == 3:
                c.st.spg_reset()
                c.tr.reset()
            zu = SM.own_zu(17, 5, c.tr.ordinal, seed, key)
            if k == 0:
                firsts.append(zu)
            if k == 3:
                assert c.tr.ordinal == 0 and np.array_equal(zu, firsts[-1])
            c.st.spg_step(1, dev(u[k:k + 1]), None)
            c.run.run(u[k:k + 1], zu[None])
            c.check(("own", seed, k))
        assert c.run.worth_comparing()
    assert not np.array_equal(firsts[0], firsts[1])


@pytest.mark.parametrize("fused", FUSED)
def test_a_step_without_a_selected_row(fused):
    """A noise of 0 and K = 1 around mu: the candidate is mu, nothing beats qmu except a stored
    action or an extra; on a batch of one row that the actor's action wins, no row is selected:
    t_a stays, the half is counted as empty, the critic and the targets still move."""
    c = Case(fused=fused, n_in=62, actor=(15, 2), critic=(25, 1), batch=1, samples=1, moving=False, noise=0.0, seed=9)
    u, zu = c.w.draws(12)
    for k in range(12):
        c.steps(1, u[k:k + 1], zu[k:k + 1])
        c.check(("empty", k))
    assert c.tr.aempty > 0 and c.tr.a.t > 0 and c.tr.a.t + c.tr.aempty == c.tr.c.t == 12


@pytest.mark.parametrize("fused", FUSED)
def test_noise_written_by_the_caller_takes_effect(fused):
    c = Case(fused=fused, n_in=62, actor=(15, 2), critic=(25, 1), batch=17, seed=10)
    c.steps(1)
    c.check("before")
    noise_tensor(c.st).fill_(0.0625)
    c.tr.noise = 0.0625
    c.steps(2)
    c.check("after")
    assert c.tr.noise == 0.0625 * c.tr.noise_decay ** 2


@pytest.mark.parametrize("fused", FUSED)
@pytest.mark.parametrize("prio", [False, True])
def test_memory_below_min_size_changes_nothing(prio, fused):
    kw = dict(n_in=64, actor=(15, 2), critic=(25, 1), batch=16, prio=prio, seed=11)
    c = Case(fused=fused, min_size=41, **kw)
    c.steps(1)
    assert (c.tr.c.t, c.tr.a.t, c.tr.skipped, c.tr.askipped, c.tr.aempty) == (0, 0, 1, 0, 0) and c.tr.noise == 0.3
    c.check("below min_size")
    c = Case(fused=fused, n_mem=12, **kw)  # fewer than a batch
    c.steps(2)
    assert (c.tr.c.t, c.tr.skipped) == (0, 2)
    c.check("below the batch")
    c = Case(fused=fused, n_mem=0, **kw)  # empty
    c.steps(1)
    assert (c.tr.c.t, c.tr.skipped) == (0, 1)
    c.check("empty")


@pytest.mark.parametrize("fused", FUSED)
def test_inf_reward_sets_the_warn_bit_and_changes_nothing(fused):
    r = np.linspace(-1, 1, 40)
    r[5] = np.inf
    c = Case(fused=fused, n_in=64, actor=(15, 2), critic=(25, 1), batch=16, prio=True, rewards=r, seed=12)
    c.st.reset(11)  # (the warn bits are sticky since the last reset)
    assert c.st.warnings(0) & _abi.WARN_TRAIN_NONFINITE == 0
    # a fresh prioritized memory's leaves are all 1.0: u maps to floor(39 u); one row of the batch draws slot 5
    u = (np.arange(16)[None, :] + 20.5) / 39
    u[0, 15] = 5.5 / 39
    _, zu = c.w.draws(2)
    c.steps(1, u, zu[:1])
    assert c.run.last_idx[15] == 5 and c.tr.nonfinite
    assert (c.tr.c.t, c.tr.a.t, c.tr.skipped, c.tr.askipped, c.tr.ordinal) == (0, 0, 1, 0, 1) and c.tr.noise == 0.3
    assert c.st.warnings(0) & _abi.WARN_TRAIN_NONFINITE
    c.check("inf")
    u[0, 15] = 6.5 / 39
    c.steps(1, u, zu[1:])
    assert c.tr.c.t == 1
    c.check("after inf")


@pytest.mark.parametrize("fused", FUSED)
def test_nonfinite_actor_delta_skips_the_actor_half_only(fused):
    """Every slot's extra holds 1e300 as its first value.  It enters a critic without a hidden layer
    as float32's +inf on a positive weight, so Q is +inf and the extra wins its row; td (on the
    stored action) is finite and the critic is updated; the actor's delta towards 1e300 is not a
    float32: the actor, its Adam state and t_a stay, the half is counted, the warn bit is set, the
    write-back and the targets still apply."""
    n = 40
    kw = dict(n_in=64, actor=(15, 2), critic=(1,), batch=16, prio=True, seed=14, samples=1)
    cw = M.make_weights(np.random.default_rng(21), 66, (1,), hi=2)
    cw[0][0][64, 0] = F32(1.0)
    c = Case(fused=fused, critic_weights=cw, **kw)
    big = np.zeros((n, 4))
    big[:, 0], big[:, 1] = 1e300, 0.25
    c.st.exp_extra_set(dev(np.arange(n, dtype=np.int64)), dev(big))
    c.run.extra[:n], c.run.valid[:n] = big, 1
    c.st.reset(11)  # (the warn bits are sticky since the last reset)
    assert c.st.warnings(0) & _abi.WARN_TRAIN_NONFINITE == 0
    c.steps(1)
    assert np.isfinite(c.tr.td).all() and (c.tr.src == SM.SRC_EXTRA).all() and not np.isfinite(c.tr.delta_a).all()
    assert (c.tr.c.t, c.tr.a.t, c.tr.skipped, c.tr.askipped, c.tr.aempty) == (1, 0, 0, 1, 0) and c.tr.nonfinite
    assert moved(c.tr.a.theta, c.w.a0) == 0 and moved(c.tr.c.theta, cw) > 0 and moved(c.tr.target_c, cw) > 0
    assert c.st.warnings(0) & _abi.WARN_TRAIN_NONFINITE
    c.check("overflow")
    for which in ("m", "v"):
        for Wg, b in c.st.net_get_weights(which):
            assert not Wg.view(np.uint32).any() and not b.view(np.uint32).any()
    c.steps(2)
    assert (c.tr.c.t, c.tr.a.t, c.tr.askipped) == (3, 0, 3)
    c.check("overflow 3")


@pytest.mark.parametrize("fused", FUSED)
def test_n_steps_in_one_call_equal_n_calls(fused):
    got = []
    for calls in (1, 3):
        c = Case(fused=fused, n_in=61, actor=(16, 2), critic=(15, 25, 1), batch=17, prio=True, seed=16)
        c.steps(3, calls=calls)
        c.check(("calls", calls))
        got.append((c.st.net_get_weights("online"), c.st.critic_get_weights("target")))
    assert moved(got[1][0], got[0][0]) == 0 and moved(got[1][1], got[0][1]) == 0


@pytest.mark.parametrize("fused", FUSED)
def test_sync_target_reset_and_hard_copy(fused):
    c = Case(fused=fused, n_in=61, actor=(16, 2), critic=(15, 25, 1), batch=17, tau=0.0, target_steps=2, prio=True, seed=10)
    c.steps(1)
    c.check("t1")
    assert same_bits(c.tr.target_a[0][0], c.w.a0[0][0]) and c.tr.since == 1
    c.steps(1)
    c.check("t2")
    assert same_bits(c.tr.target_a[0][0], c.tr.a.theta[0][0]) and c.tr.since == 0
    c.steps(1)
    c.st.spg_sync_target()
    c.tr.sync_target()
    c.check("synced")
    c.st.spg_reset()
    c.tr.reset()
    assert (c.tr.c.t, c.tr.a.t, c.tr.ordinal) == (0, 0, 0)
    c.check("reset")
    c.steps(1)
    c.check("after reset")


def test_configuration_exclusions_and_drops():
    st = handle(64)
    st.exp_config(W.CAP, extra=True)
    st.net_config((64, (15, 2), "relu", "sigmoid"))
    crit = (66, (15, 1), "relu", "linear")
    with pytest.raises(RuntimeError, match="spg_config: no critic is configured"):
        st.spg_config(batch=16)
    st.critic_config((64, (15, 1), "relu", "linear"))
    with pytest.raises(RuntimeError, match=r"spg_config: the critic is V\(s\)"):
        st.spg_config(batch=16)
    st.qcritic_config(crit)
    st.spg_config(batch=16)
    v = C.c_int64()
    for which in range(8):  # every copy is there, as under a DPG configuration
        assert st.L.aigar_net_pad_check(st.h, which, C.byref(v)) == 0 and v.value == 0
    assert st.L.aigar_dpg_step(st.h, 1, None) < 0 and b"no DPG training is configured" in st.L.aigar_last_error()
    st.dpg_config(None)  # (a null turns off its own trainer, not another)
    st.spg_step(1)
    st.dpg_config(batch=16)  # configuring one drops the other
    assert st.L.aigar_spg_step(st.h, 1, None, None) < 0 and b"no SPG training is configured" in st.L.aigar_last_error()
    st.dpg_step(1)
    st.spg_config(batch=16)
    assert st.L.aigar_dpg_step(st.h, 1, None) < 0 and b"no DPG training is configured" in st.L.aigar_last_error()
    st.spg_step(1)
    assert st.spg_info()["skipped"] == 1  # (an empty memory)
    drops = [lambda: st.qcritic_config(crit), lambda: st.exp_config(W.CAP, extra=True), lambda: st.critic_config(None),
             lambda: st.net_config((64, (15, 2), "relu", "sigmoid")), lambda: st.spg_config(None)]
    for k, drop in enumerate(drops):
        drop()
        assert st.L.aigar_spg_info(st.h, (C.c_int64 * 8)()) < 0, k
        assert b"no SPG training is configured" in st.L.aigar_last_error(), k
        assert st.L.aigar_net_pad_check(st.h, 5, C.byref(v)) < 0, k
        st.qcritic_config(crit)
        st.spg_config(batch=16)
    st.exp_config(W.CAP)  # a memory without the fifth field
    with pytest.raises(RuntimeError, match="spg_config: replace needs a replay memory with the extra field"):
        st.spg_config(batch=16)
    st.spg_config(batch=16, replace=False)
    st.spg_step(1)
    with pytest.raises(RuntimeError, match="n_steps = 0"):
        st.spg_step(0)


@pytest.mark.parametrize("fused", FUSED)
@pytest.mark.parametrize("n_act,K", [(2, 1), (2, 5), (3, 1), (3, 5), (4, 1), (4, 5)])
def test_the_golden_cases_uniforms_as_zu(n_act, K, fused, golden_dir):
    """The uniforms the reference's own searches consumed (tests/golden/spg_cases.npz), rejected
    attempts included, as the search's zu: the four recorded cases of (n_act, K), six rows each,
    are the four steps of a batch of six."""
    import os
    g = W.load_golden(os.path.join(golden_dir, "spg_cases.npz"))
    cases = [c for c in range(len(g["K"])) if g["n_act"][c] == n_act and g["K"][c] == K]
    assert len(cases) == 4 and g["B"] == 6
    zu = np.stack([g["zu"][c * 6:(c + 1) * 6, :K] for c in cases])
    assert (zu[:, :, :, 0, 1] != 0.5).any(), "no pair with a rejected first attempt"
    c = Case(fused=fused, n_in=3, actor=(15, n_act), critic=(25, 1), batch=6, samples=K, seed=20 + n_act)
    u, _ = c.w.draws(4)
    for k in range(4):
        c.steps(1, u[k:k + 1], zu[k:k + 1])
        c.check(("golden", k))
    assert c.tr.c.t == 4 and c.tr.seen[1] > 0
