"""GPU: aigar_dpg_step (dpg.inc) against the Python model (tests/dpg_model.py, checked by
tests/test_dpg_model.py), bit pattern for bit pattern: the actor's and the critic's weights, both
targets, both networks' Adam m and v, the TD errors, the drawn indices, the counters, the pad
checks and the prioritized memory's trees (through a sample with given draws).  No tolerance
anywhere.

Shapes: batches 1 / 15 / 16 / 17 / 33; state widths 1 / 63 / 64 / 65 / 130 with 1..4 actions, so
that the action columns of the critic's input straddle the first layer's 64-chunk and a 16-row
weight tile (63 + 2, 63 + 4, 64 + 1); both memory dtypes; relu and linear hidden layers; actor and
critic layer sets that differ; a critic without a hidden layer; first-layer widths 1 / 16 / 17 /
256.  Magnitudes as tests/test_gpu_actrain.py's: states and weights 2^-30 .. 2^2 with subnormals
and signed zeros, rewards 2^-10 .. 2^5 of both signs, stored actions in [0, 1)."""
import numpy as np
import pytest

import dpg_model as DM
import net_model as M
from oracle_lib import make_config
from replay_model import ReplayModel

pytestmark = pytest.mark.gpu
from aigar_amd import _abi, _lib  # noqa: E402

F32 = np.float32
CH7 = (_abi.OBS_PELLET | _abi.OBS_SELF | _abi.OBS_WALL | _abi.OBS_ENEMY | _abi.OBS_VIRUS | _abi.OBS_SELF_LF
       | _abi.OBS_ENEMY_LF)
CH5 = _abi.OBS_PELLET | _abi.OBS_SELF | _abi.OBS_WALL | _abi.OBS_ENEMY | _abi.OBS_VIRUS
# state width -> (grid_squares, channels, extras) of a handle whose observation row has it
WIDTHS = {1: (1, _abi.OBS_PELLET, 0), 63: (3, CH7, 0), 64: (3, CH7, _abi.EX_FOV), 65: (3, CH7, _abi.EX_FOV | _abi.EX_MASS),
          130: (5, CH5, _abi.EX_FOV | _abi.EX_LAST_ACT)}
CAP = 64
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


def overflow_critic(rng, n_s, n_act):
    """A critic (17, 1) whose action row 0 of the first layer is 2^58 on units 0..15 and whose head
    weights there are +-2^30 in turn: the pairs cancel exactly in Q, so td stays small, while
    delta_0 W_0 on that row overflows float32 once the combined model's delta is large."""
    w = M.make_weights(rng, n_s + n_act, (17, 1), hi=2)
    w[0][0][n_s, :16] = F32(2.0 ** 58)
    w[1][0][:16, 0] = F32(2.0 ** 30) * np.where(np.arange(16) % 2 == 0, 1, -1).astype(F32)
    return w


class Case:
    """A handle with a filled memory, an actor, a Q(s, a) critic and a DPG train configuration, and
    its model twin."""

    def __init__(self, n_in, actor, critic, batch, ha="relu", hc="relu", dtype="float64", prio=False, n_mem=40, hi=2,
                 seed=0, target_steps=0, min_size=0, done=None, rewards=None, tau=0.25, q_increase=2.0, lr=1e-2,
                 critic_weights=None, extra=False):
        self.st = st = handle(n_in)
        self.rng = rng = np.random.default_rng(1000 * n_in + 10 * batch + seed)
        self.n_in, self.batch, self.dtype, self.prio = n_in, batch, dtype, prio
        self.actor, self.critic = tuple(actor), tuple(critic)
        n_act = self.actor[-1]
        np_dt = np.float64 if dtype == "float64" else np.float32
        self.a0 = M.make_weights(rng, n_in, self.actor, hi=hi)
        self.c0 = M.make_weights(rng, n_in + n_act, self.critic, hi=hi) if critic_weights is None else critic_weights
        st.exp_config(CAP, prioritized=prio, dtype=dtype, seed=3, extra=extra)
        st.net_config((n_in, self.actor, ha, "sigmoid"), x_dtype=dtype)
        st.qcritic_config((n_in + n_act, self.critic, hc, "linear"), x_dtype=dtype)
        st.net_set_weights(self.a0)
        st.critic_set_weights(self.c0)
        self.rm = ReplayModel(CAP, prio)
        if n_mem:
            s = M.mixed(rng, (n_mem, n_in), hi=3)
            s2 = M.mixed(rng, (n_mem, n_in), hi=3)
            if dtype == "float64":  # float64 rows that are not float32 values: one rounding each
                s, s2 = (np.where(x == 0, x, x.astype(np.float64) * (1 + 2.0 ** -30)) for x in (s, s2))
            a = np.zeros((n_mem, 4))
            a[:, :n_act] = rng.random((n_mem, n_act))  # (float64 values that are not float32 values)
            r = M.mixed(rng, (n_mem,), lo=-10, hi=5).astype(np.float64) if rewards is None else rewards
            d = (rng.random(n_mem) < 0.25) if done is None else done
            d = np.asarray(d, bool)
            s2 = s2.astype(np_dt)
            s2[d] = np.nan  # (the decision's transitions: a dead player's new state is the NaN row)
            args = (s.astype(np_dt), a, np.asarray(r, np.float64), s2, d.astype(np.uint8))
            st.exp_add(*args)
            self.rm.add(*args)
        self.kw = dict(critic_lr=lr, actor_lr=lr / 2, beta1=0.9, beta2=0.999, epsilon=1e-7, discount=0.85,
                       target_steps=target_steps, min_size=min_size, tau=tau, q_increase=q_increase)
        st.dpg_config(batch=batch, **self.kw)
        self.tr = DM.Trainer(self.a0, self.c0, batch, hidden_actor=ha, hidden_critic=hc, **self.kw)
        self.last_idx = None

    def model_step(self, u):
        idx, w = self.rm.sample(list(u))
        if not self.tr.can_draw(self.rm.size) or idx[0] < 0:
            self.tr.skipped += 1
            return idx
        rows = self.rm.gather(idx)
        s, a, r, s2, d = (np.array([row[k] for row in rows]) for k in range(5))
        prio = self.tr.step(s, a, r, s2, d, np.asarray(w))
        if prio is not None:
            self.rm.update(idx, prio)
        return idx

    def steps(self, n, u=None, calls=1):
        """n steps on both sides from the same draws; the device's in `calls` calls."""
        u = self.rng.random((n, self.batch)) if u is None else u
        for part in np.split(np.arange(n), calls):
            self.st.dpg_step(len(part), dev(u[part]))
        for k in range(n):
            self.last_idx = self.model_step(u[k])

    def check(self, what):
        import torch
        st, tr = self.st, self.tr
        info = st.dpg_info()
        got = tuple(info[k] for k in ("steps", "skipped", "since_target", "actor_steps", "actor_skipped")) + (0, 0, 0)
        assert got == tr.info(), (what, got, tr.info())
        sets = [("actor " + w, st.net_get_weights(w), x, st.net_pad_check(w))
                for w, x in (("online", tr.a.theta), ("target", tr.target_a), ("m", tr.a.m), ("v", tr.a.v))]
        sets += [("critic " + w, st.critic_get_weights(w), x, st.critic_pad_check(w))
                 for w, x in (("online", tr.c.theta), ("target", tr.target_c), ("m", tr.c.m), ("v", tr.c.v))]
        for name, got, want, pad in sets:
            for l, ((W, b), (Ww, bw)) in enumerate(zip(got, want)):
                assert np.isfinite(Ww).all() and np.isfinite(bw).all(), (what, name, l)
                assert same_bits(W, Ww), (what, name, l, int((W.view(np.uint32) != Ww.view(np.uint32)).sum()), W.size)
                assert same_bits(b, bw), (what, name, l, b, bw)
            assert pad == 0, (what, name)
        if self.last_idx is not None:
            B = self.batch
            td = torch.full((B + 1,), -7.25, dtype=torch.float64, device="cuda")
            idx = torch.full((B + 1,), -7, dtype=torch.int64, device="cuda")
            st.dpg_td(td[:B], idx[:B])
            td, idx = td.cpu().numpy(), idx.cpu().numpy()
            assert td[-1] == -7.25 and idx[-1] == -7, "the entry behind the last one was written"
            assert idx[:-1].tolist() == list(self.last_idx), what
            if tr.td is not None and self.tr.can_draw(self.rm.size):
                fin = np.isfinite(tr.td)
                assert same_bits(td[:-1][fin], tr.td[fin]), what
                assert np.array_equal(np.isfinite(td[:-1]), fin), what
        if self.prio and self.rm.size >= 2:  # the trees: a sample's indices and weights are functions of their sums
            u = np.linspace(0.0, 0.999, 23)
            w = torch.zeros(23, dtype=torch.float64, device="cuda")
            i = torch.zeros(23, dtype=torch.int64, device="cuda")
            st.exp_sample(w, i, u=dev(u))
            wi, ww = self.rm.sample(list(u))
            assert i.cpu().numpy().tolist() == list(wi), what
            assert same_bits(w.cpu().numpy(), np.asarray(ww, np.float64)), what


def moved(now, start):
    return sum(int((W.view(np.uint32) != W0.view(np.uint32)).sum()) for (W, _), (W0, _) in zip(now, start))


def one_and_three(c, what):
    c.steps(1)
    assert c.tr.c.t == 1 and c.tr.a.t == 1, "the model skipped a step or a half the case means to apply"
    c.check((what, 1))
    c.steps(2)
    assert c.tr.c.t == 3 and c.tr.a.t == 3
    c.check((what, 3))
    assert moved(c.tr.c.theta, c.c0) > 0 and moved(c.tr.a.theta, c.a0) > 0, "a network did not move: the case checks nothing"
    assert moved(c.tr.target_c, c.c0) > 0 and moved(c.tr.target_a, c.a0) > 0, "a target did not move"


@pytest.mark.parametrize("batch", [1, 15, 16, 17, 33])
def test_batches(batch):
    one_and_three(Case(65, (16, 16, 3), (17, 25, 1), batch, prio=True, seed=1), batch)


@pytest.mark.parametrize("n_in,n_act", [(1, 1), (63, 1), (63, 2), (63, 4), (64, 1), (64, 4), (65, 3), (130, 2)])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_state_and_action_widths_and_dtypes(n_in, n_act, dtype):
    one_and_three(Case(n_in, (15, n_act), (25, 1), 17, dtype=dtype, prio=(n_in % 2 == 1), seed=2), (n_in, n_act, dtype))


# (actor, critic, hi): a critic without a hidden layer; first-layer widths 1 / 16 / 17 / 256; five layers
LAYERS = [((2,), (1,), 2), ((16, 3), (1, 1), 2), ((16, 16, 3), (16, 1), 2), ((16, 16, 3), (17, 25, 1), 2),
          ((33, 100, 4), (256, 1), 2), ((100, 100, 1), (15, 1), 2), ((17, 64, 33, 20, 4), (33, 256, 17, 64, 1), 0)]


@pytest.mark.parametrize("actor,critic,hi", LAYERS, ids=["-".join(map(str, a)) + "_" + "-".join(map(str, c))
                                                        for a, c, _ in LAYERS])
@pytest.mark.parametrize("hidden", ["relu", "linear"])
def test_layer_sets(actor, critic, hi, hidden):
    other = "linear" if hidden == "relu" else "relu"  # (the two networks' hidden activations differ too)
    one_and_three(Case(63, actor, critic, 18, ha=hidden, hc=other if len(critic) > 1 else hidden, prio=True, hi=hi, seed=3),
                  (actor, critic, hidden))


def test_done_rows_at_tile_edges_and_a_batch_of_only_done_rows():
    n = 40
    done = np.zeros(n, bool)
    done[[0, 15, 16, 17, 31, 32]] = True
    c = Case(65, (16, 16, 3), (17, 25, 1), 33, done=done, seed=5)
    u = (np.arange(33)[None, :] + 0.5) / n * np.ones((3, 1))  # slot k in row k: the done rows sit at the tile edges
    c.steps(1, u[:1])
    c.check("edges 1")
    c.steps(2, u[1:])
    c.check("edges 3")
    assert c.tr.c.t == 3 and c.tr.a.t == 3
    one_and_three(Case(65, (16, 16, 3), (17, 25, 1), 17, done=np.ones(n, bool), prio=True, seed=6), "all done")
    one_and_three(Case(65, (16, 16, 3), (17, 25, 1), 17, done=np.zeros(n, bool), prio=True, seed=6), "none done")


@pytest.mark.parametrize("tau", [0.001, 0.25, 1.0])
def test_soft_update(tau):
    c = Case(65, (16, 2), (15, 25, 1), 17, tau=tau, target_steps=2, prio=True, seed=10)
    one_and_three(c, ("tau", tau))
    assert c.tr.since == 3  # (no hard copy under tau > 0)
    if tau == 1.0:  # the targets are the online networks, up to the sign of a zero
        assert all(np.array_equal(W, Wt) for (W, _), (Wt, _) in zip(c.tr.c.theta, c.tr.target_c))
    else:
        assert not same_bits(c.tr.target_a[0][0], c.tr.a.theta[0][0])


@pytest.mark.parametrize("target_steps", [1, 3, 0])
def test_hard_copy(target_steps):
    c = Case(65, (16, 2), (15, 25, 1), 17, tau=0.0, target_steps=target_steps, prio=True, seed=10)
    c.steps(1)
    c.check("t1")
    copied = target_steps == 1
    assert same_bits(c.tr.target_c[0][0], c.tr.c.theta[0][0] if copied else c.c0[0][0])
    assert same_bits(c.tr.target_a[0][0], c.tr.a.theta[0][0] if copied else c.a0[0][0])
    c.steps(3)
    c.check("t4")
    assert c.tr.c.t == 4 and c.tr.since == {1: 0, 3: 1, 0: 4}[target_steps]
    if target_steps == 3:  # step 3's weights, not step 4's
        assert not same_bits(c.tr.target_a[0][0], c.tr.a.theta[0][0]) and not same_bits(c.tr.target_a[0][0], c.a0[0][0])


@pytest.mark.parametrize("q_increase", [0.0, -3.5, 2.0])
def test_q_increase(q_increase):
    one_and_three(Case(64, (15, 2), (25, 1), 16, q_increase=q_increase, seed=8), ("q_increase", q_increase))


def test_q_increase_changes_the_actor_only():
    u = np.random.default_rng(5).random((1, 16))
    res = []  # (the two cases share one handle: run and read them one after the other)
    for q in (0.0, 2.0):
        c = Case(64, (15, 2), (25, 1), 16, q_increase=q, seed=8)
        c.steps(1, u)
        c.check(q)
        res.append((c.st.net_get_weights("online"), c.st.critic_get_weights("online")))
    assert moved(res[0][0], res[1][0]) > 0 and moved(res[0][1], res[1][1]) == 0


@pytest.mark.parametrize("prio", [False, True])
def test_memory_below_min_size_changes_nothing(prio):
    c = Case(64, (15, 2), (25, 1), 16, prio=prio, min_size=41, seed=11)
    c.steps(1)
    assert (c.tr.c.t, c.tr.a.t, c.tr.skipped, c.tr.askipped) == (0, 0, 1, 0)
    c.check("below min_size")
    c = Case(64, (15, 2), (25, 1), 16, prio=prio, n_mem=12, seed=11)  # fewer than a batch
    c.steps(2)
    assert (c.tr.c.t, c.tr.skipped) == (0, 2)
    c.check("below the batch")
    c = Case(64, (15, 2), (25, 1), 16, prio=prio, n_mem=0, seed=11)  # empty
    c.steps(1)
    assert (c.tr.c.t, c.tr.skipped) == (0, 1)
    c.check("empty")


def test_inf_reward_sets_the_warn_bit_and_changes_nothing():
    r = np.linspace(-1, 1, 40)
    r[5] = np.inf
    c = Case(64, (15, 2), (25, 1), 16, prio=True, rewards=r, seed=12)
    c.st.reset(11)  # (the warn bits are sticky since the last reset)
    assert c.st.warnings(0) & _abi.WARN_TRAIN_NONFINITE == 0
    # a fresh prioritized memory's leaves are all 1.0: u maps to floor(39 u); one row of the batch draws slot 5
    u = (np.arange(16)[None, :] + 20.5) / 39
    u[0, 15] = 5.5 / 39
    c.steps(1, u)
    assert c.last_idx[15] == 5 and c.tr.nonfinite and (c.tr.c.t, c.tr.a.t, c.tr.skipped, c.tr.askipped) == (0, 0, 1, 0)
    assert c.st.warnings(0) & _abi.WARN_TRAIN_NONFINITE
    c.check("inf")
    u[0, 15] = 6.5 / 39
    c.steps(1, u)
    assert (c.tr.c.t, c.tr.a.t) == (1, 1)
    c.check("after inf")


@pytest.mark.parametrize("n_in,n_act,batch", [(63, 2, 16), (64, 1, 33)])
def test_nonfinite_actor_delta_skips_the_actor_half_only(n_in, n_act, batch):
    """td is finite and the critic is updated; delta_0 W_0 overflows on action 0, so the actor, its
    Adam state and t_a stay, the half is counted and the warn bit is set; the targets still move."""
    rng = np.random.default_rng(21)
    c = Case(n_in, (15, n_act), (17, 1), batch, prio=True, q_increase=2.0 ** 50, seed=14, rewards=np.linspace(-0.25, 0.25, 40),
             critic_weights=overflow_critic(rng, n_in, n_act))
    c.st.reset(11)
    assert c.st.warnings(0) & _abi.WARN_TRAIN_NONFINITE == 0
    c.steps(1)
    assert np.isfinite(c.tr.td).all() and not np.isfinite(c.tr.ea).all()
    assert (c.tr.c.t, c.tr.a.t, c.tr.skipped, c.tr.askipped) == (1, 0, 0, 1) and c.tr.nonfinite
    assert moved(c.tr.c.theta, c.c0) > 0 and moved(c.tr.a.theta, c.a0) == 0 and moved(c.tr.target_c, c.c0) > 0
    assert c.st.warnings(0) & _abi.WARN_TRAIN_NONFINITE
    c.check("overflow 1")
    for which in ("m", "v"):
        for W, b in c.st.net_get_weights(which):
            assert not W.view(np.uint32).any() and not b.view(np.uint32).any()
    c.steps(2)
    assert (c.tr.c.t, c.tr.a.t, c.tr.askipped) == (3, 0, 3)
    c.check("overflow 3")
    # an ordinary critic from here on: the half applies with the actor's own counter, t_a = 1 beside t_c = 4
    wc = M.make_weights(rng, n_in + n_act, (17, 1), hi=2)
    c.st.critic_set_weights(wc)
    c.tr.c.theta = [(W.copy(), b.copy()) for W, b in wc]
    c.st.dpg_sync_target()
    c.tr.sync_target()
    c.steps(1)
    assert (c.tr.c.t, c.tr.a.t, c.tr.askipped) == (4, 1, 3) and moved(c.tr.a.theta, c.a0) > 0
    c.check("applied after the skipped halves")


def test_nonfinite_combined_delta_skips_the_actor_half_only():
    c = Case(64, (15, 2), (25, 1), 16, prio=True, q_increase=1e300, seed=15)  # (finite, but not as a float32 delta)
    c.st.reset(11)
    c.steps(2)
    assert (c.tr.c.t, c.tr.a.t, c.tr.skipped, c.tr.askipped) == (2, 0, 0, 2)
    assert c.st.warnings(0) & _abi.WARN_TRAIN_NONFINITE
    c.check("inf delta")


def test_n_steps_in_one_call_equal_n_calls():
    u = np.random.default_rng(9).random((4, 17))
    got = []
    for calls in (1, 4, 2):
        c = Case(65, (16, 2), (15, 25, 1), 17, prio=True, seed=16)
        c.steps(4, u, calls=calls)
        c.check(("calls", calls))
        got.append((c.st.net_get_weights("online"), c.st.critic_get_weights("target")))
    for g in got[1:]:
        assert moved(g[0], got[0][0]) == 0 and moved(g[1], got[0][1]) == 0


def test_sync_target_and_reset():
    c = Case(65, (16, 2), (15, 25, 1), 17, tau=0.0, target_steps=0, prio=True, seed=10)
    c.steps(2)
    c.check("t2")
    assert same_bits(c.tr.target_a[0][0], c.a0[0][0]) and c.tr.since == 2
    c.st.dpg_sync_target()
    c.tr.sync_target()
    assert c.tr.since == 0 and same_bits(c.tr.target_a[0][0], c.tr.a.theta[0][0])
    c.check("synced")
    c.st.dpg_reset()
    c.tr.reset()
    assert (c.tr.c.t, c.tr.a.t) == (0, 0)
    c.check("reset")
    c.steps(1)
    c.check("after reset")


def test_set_weights_between_steps():
    c = Case(65, (16, 2), (15, 1), 17, prio=True, seed=13)
    c.steps(2)
    rng = np.random.default_rng(77)
    wa, wc = M.make_weights(rng, 65, (16, 2), hi=2), M.make_weights(rng, 67, (15, 1), hi=2)
    c.st.net_set_weights(wa)
    c.st.critic_set_weights(wc)
    c.tr.a.theta = [(W.copy(), b.copy()) for W, b in wa]
    c.tr.c.theta = [(W.copy(), b.copy()) for W, b in wc]
    c.check("pushed")  # (the targets, m, v and the counters are as they were)
    c.steps(2)
    c.check("after push")


def test_reconfiguration_drops_the_graph():
    """The same case before and after another configuration of the same handle ran its own graph."""
    u = np.random.default_rng(3).random((2, 17))
    first = None
    for k in range(2):
        c = Case(65, (16, 2), (15, 25, 1), 17, prio=True, seed=17)
        c.steps(2, u)
        c.check(("A", k))
        now = (c.st.net_get_weights("online"), c.st.critic_get_weights("online"))
        if first is None:
            first = now
            one_and_three(Case(65, (8, 3), (9, 1), 33, dtype="float32", seed=18), "B")  # other shapes, batch and dtype
    assert moved(now[0], first[0]) == 0 and moved(now[1], first[1]) == 0


def test_cacla_runs_on_the_handle_after_dpg_was_dropped():
    import test_gpu_actrain as TA
    c = Case(65, (16, 16, 3), (17, 25, 1), 17, prio=True, seed=19)
    c.steps(1)
    c.check("dpg")
    TA._G[65] = handle(65)  # (its Case configures this module's handle: a V(s) critic drops the DPG configuration)
    try:
        ca = TA.Case(65, (16, 16, 3), (17, 25, 1), 17, prio=True, E=4, seed=1)
        assert ca.st is c.st
        assert c.st.L.aigar_dpg_step(c.st.h, 1, None) < 0 and b"no DPG training is configured" in c.st.L.aigar_last_error()
        TA.one_and_three(ca, "cacla after dpg")
    finally:
        TA._G.pop(65)
    one_and_three(Case(65, (16, 16, 3), (17, 25, 1), 17, prio=True, seed=19), "dpg after cacla")


@pytest.mark.parametrize("rows", [1, 17])
def test_qcritic_forward_equals_the_model(rows):
    import torch
    st = handle(65)
    rng = np.random.default_rng(rows)
    st.net_config((65, (4, 2), "relu", "sigmoid"))
    for hidden, units in (("relu", (17, 25, 1)), ("linear", (1,))):
        w = M.make_weights(rng, 67, units, hi=2)
        st.qcritic_config((67, units, hidden, "linear"))
        st.critic_set_weights(w)
        for dt in (np.float64, np.float32):
            x = M.mixed(rng, (rows, 67), hi=3).astype(dt)
            out = torch.full((rows + 1,), -7.25, dtype=torch.float64, device="cuda")
            st.critic_forward(dev(x), out[:rows])
            out = out.cpu().numpy()
            assert out[-1] == -7.25
            assert same_bits(out[:-1], M.forward(x, w, hidden, "linear")[:, 0])
        got = st.critic_get_weights("online")  # (needs only a critic)
        assert all(same_bits(W, Ww) and same_bits(b, bw) for (W, b), (Ww, bw) in zip(got, w))


def test_own_draws_follow_the_memorys_stream():
    import torch
    c = Case(64, (15, 2), (25, 1), 16, prio=False, seed=15)
    w = torch.zeros(16, dtype=torch.float64, device="cuda")
    i0 = torch.zeros(16, dtype=torch.int64, device="cuda")
    c.st.exp_sample(w, i0)  # call 0 of the stream
    c2 = Case(64, (15, 2), (25, 1), 16, prio=False, seed=15)
    c2.st.dpg_step(1)
    idx = torch.zeros(16, dtype=torch.int64, device="cuda")
    c2.st.dpg_td(None, idx)
    assert idx.cpu().numpy().tolist() == i0.cpu().numpy().tolist()
    assert c2.st.dpg_info()["steps"] == 1


def test_live_handle_refusals():
    import ctypes as C
    st = handle(64)
    st.net_config(None)
    st.exp_config(CAP)
    crit = (66, (15, 1), "relu", "linear")
    with pytest.raises(RuntimeError, match="qcritic_config: no acting network"):
        st.qcritic_config(crit)
    with pytest.raises(RuntimeError, match="dpg_config: no acting network"):
        st.dpg_config(batch=16)
    st.net_config((64, (15, 2), "relu", "sigmoid"))
    with pytest.raises(RuntimeError, match="no critic is configured"):
        st.dpg_config(batch=16)
    with pytest.raises(RuntimeError, match=r"n_in = 64 differs from the acting network's n_in \+ n_out = 64 \+ 2"):
        st.qcritic_config((64, (15, 1), "relu", "linear"))
    with pytest.raises(RuntimeError, match=r"Q\(s, a\) is one linear unit"):
        st.qcritic_config((66, (15, 2), "relu", "linear"))
    st.critic_config((64, (15, 1), "relu", "linear"))
    with pytest.raises(RuntimeError, match=r"dpg_config: the critic is V\(s\)"):
        st.dpg_config(batch=16)
    st.qcritic_config(crit)
    with pytest.raises(RuntimeError, match=r"actrain_config: the critic is Q\(s, a\)"):
        st.actrain_config(batch=16)
    st.exp_config(None)
    with pytest.raises(RuntimeError, match="no replay memory"):
        st.dpg_config(batch=16)
    st.exp_config(CAP)
    st.net_config((64, (15, 2), "relu", "linear"))
    with pytest.raises(RuntimeError, match="qcritic_config: the network's head is linear, the DPG actor needs a sigmoid head"):
        st.qcritic_config(crit)
    st.net_config((64, (15, 5), "relu", "sigmoid"))
    with pytest.raises(RuntimeError, match="5 outputs"):
        st.qcritic_config((69, (15, 1), "relu", "linear"))
    st.net_config((64, (15, 2), "relu", "sigmoid"))
    st.qcritic_config(crit)
    st.dpg_config(batch=16)
    with pytest.raises(RuntimeError, match="n_steps = 0"):
        st.dpg_step(0)
    v = C.c_int64()
    for which in range(8):  # every copy is there under a DPG configuration
        assert st.L.aigar_net_pad_check(st.h, which, C.byref(v)) == 0 and v.value == 0
    st.qcritic_config(crit)  # reconfiguring the critic drops the train configuration
    assert st.L.aigar_dpg_step(st.h, 1, None) < 0 and b"no DPG training is configured" in st.L.aigar_last_error()
    assert st.L.aigar_net_pad_check(st.h, 5, C.byref(v)) < 0 and b"no CACLA training" in st.L.aigar_last_error()
    st.dpg_config(batch=16)
    st.exp_config(CAP)  # ... and so does the memory
    assert st.L.aigar_dpg_step(st.h, 1, None) < 0 and b"no DPG training is configured" in st.L.aigar_last_error()
    st.dpg_config(batch=16)
    st.critic_config(None)  # ... and turning the critic off
    assert st.L.aigar_dpg_info(st.h, (C.c_int64 * 8)()) < 0 and b"no DPG training is configured" in st.L.aigar_last_error()
    st.qcritic_config(crit)
    st.dpg_config(batch=16)
    st.net_config((64, (15, 2), "relu", "sigmoid"))  # ... and the network, with the critic
    assert st.L.aigar_dpg_step(st.h, 1, None) < 0 and b"no DPG training is configured" in st.L.aigar_last_error()
    from aigar_amd import net as N
    px = _lib.Stepper(make_config(n_arenas=1, bots=2, field_size=100, flags=0))
    try:
        px.pixel_config(8)
        px.exp_config(CAP, dtype="float32")
        px.net_config(N.CnnSpec(8, 1, ((3, 1, 4),), 6 * 6 * 4, (2,), "relu", "sigmoid"), x_dtype="float32")
        with pytest.raises(RuntimeError, match="qcritic_config: the acting network has a conv part"):
            px.qcritic_config((6 * 6 * 4 + 2, (1,), "relu", "linear"))
        with pytest.raises(RuntimeError, match="dpg_config: a network with a conv part"):
            px.dpg_config(batch=4)
    finally:
        px.close()


def test_tiled_handle_is_refused():
    import ctypes as C
    st = _lib.Stepper(make_config(n_arenas=1, bots=4, field_size=100, flags=0, tile_x=1, tile_y=1, tile_id=0,
                                  tile_flags=_abi.TILE_FORCE))
    try:
        prm = _abi.DpgParams(16, 0, 0, 0, 1e-4, 1e-4, 0.9, 0.999, 1e-7, 0.85, 0.001, 2.0)
        assert st.L.aigar_dpg_config(st.h, C.byref(prm)) < 0
        assert b"dpg_config: a tiled handle" in st.L.aigar_last_error()
    finally:
        st.close()
