"""GPU: aigar_actrain_step (actrain.inc) against the Python model (tests/cacla_model.py, checked
by tests/test_cacla_model.py), bit pattern for bit pattern: the actor's and the critic's weights,
the critic's target, both networks' Adam m and v, the TD errors, the drawn indices, the per-row
epoch counts, the running variance, all eight counters and the prioritized memory's trees
(through a sample with given draws).  No tolerance anywhere.

Shapes as tests/test_gpu_train.py's: batches 1 / 15 / 16 / 17 / 33, state widths 1 / 63 / 64 /
65 / 130 with both memory dtypes, critic and actor layer sets that differ from each other.
Magnitudes: states and weights 2^-30 .. 2^2 with subnormals and signed zeros, rewards
2^-10 .. 2^5 of both signs, stored actions in [0, 1)."""
import numpy as np
import pytest

import cacla_model as CM
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


class Case:
    """A handle with a filled memory, an actor, a critic and a CACLA train configuration, and its
    model twin."""

    def __init__(self, n_in, actor, critic, batch, ha="relu", hc="relu", dtype="float64", prio=False, n_mem=40, hi=2,
                 seed=0, target_steps=0, min_size=0, done=None, rewards=None, E=0, var_start=1.0, beta=0.001, lr=1e-2,
                 critic_weights=None):
        self.st = st = handle(n_in)
        self.rng = rng = np.random.default_rng(1000 * n_in + 10 * batch + seed)
        self.n_in, self.batch, self.dtype, self.prio = n_in, batch, dtype, prio
        self.actor, self.critic = tuple(actor), tuple(critic)
        np_dt = np.float64 if dtype == "float64" else np.float32
        self.a0 = M.make_weights(rng, n_in, self.actor, hi=hi)
        self.c0 = M.make_weights(rng, n_in, self.critic, hi=hi) if critic_weights is None else critic_weights
        st.exp_config(CAP, prioritized=prio, dtype=dtype, seed=3)
        st.net_config((n_in, self.actor, ha, "sigmoid"), x_dtype=dtype)
        st.critic_config((n_in, self.critic, hc, "linear"), x_dtype=dtype)
        st.net_set_weights(self.a0)
        st.critic_set_weights(self.c0)
        self.rm = ReplayModel(CAP, prio)
        if n_mem:
            s = M.mixed(rng, (n_mem, n_in), hi=3)
            s2 = M.mixed(rng, (n_mem, n_in), hi=3)
            if dtype == "float64":  # float64 rows that are not float32 values: one rounding each
                s, s2 = (np.where(x == 0, x, x.astype(np.float64) * (1 + 2.0 ** -30)) for x in (s, s2))
            a = np.zeros((n_mem, 4))
            a[:, :self.actor[-1]] = rng.random((n_mem, self.actor[-1]))
            r = M.mixed(rng, (n_mem,), lo=-10, hi=5).astype(np.float64) if rewards is None else rewards
            d = (rng.random(n_mem) < 0.25) if done is None else done
            d = np.asarray(d, bool)
            s2 = s2.astype(np_dt)
            s2[d] = np.nan  # (the decision's transitions: a dead player's new state is the NaN row)
            args = (s.astype(np_dt), a, np.asarray(r, np.float64), s2, d.astype(np.uint8))
            st.exp_add(*args)
            self.rm.add(*args)
        self.kw = dict(critic_lr=lr, actor_lr=lr / 2, beta1=0.9, beta2=0.999, epsilon=1e-7, discount=0.85,
                       target_steps=target_steps, min_size=min_size, var_epochs=E, var_start=var_start, var_beta=beta)
        st.actrain_config(batch=batch, **self.kw)
        self.tr = CM.Trainer(self.a0, self.c0, batch, hidden_actor=ha, hidden_critic=hc, **self.kw)
        self.last_idx = None
        self.counts = []  # every applied step's per-row epoch counts

    def model_step(self, u):
        idx, w = self.rm.sample(list(u))
        if not self.tr.can_draw(self.rm.size) or idx[0] < 0:
            self.tr.skip()
            return idx
        rows = self.rm.gather(idx)
        s, a, r, s2, d = (np.array([row[k] for row in rows]) for k in range(5))
        prio = self.tr.step(s, a, r, s2, d, np.asarray(w))
        if prio is not None:
            self.rm.update(idx, prio)
            self.counts.append(self.tr.count.copy())
        return idx

    def steps(self, n, u=None):
        """n steps on both sides from the same draws."""
        u = self.rng.random((n, self.batch)) if u is None else u
        self.st.actrain_step(n, dev(u))
        for k in range(n):
            self.last_idx = self.model_step(u[k])

    def check(self, what):
        import torch
        st, tr = self.st, self.tr
        info = st.actrain_info()
        got = tuple(info[k] for k in ("steps", "skipped", "since_target", "actor_epochs", "selected", "epochs", "cut",
                                      "epochs_skipped"))
        assert got == tr.info(), (what, got, tr.info())
        sets = [("actor", st.net_get_weights(w), x, st.net_pad_check(w))
                for w, x in (("online", tr.a.theta), ("m", tr.a.m), ("v", tr.a.v))]
        sets += [("critic " + w, st.critic_get_weights(w), x, st.critic_pad_check(w))
                 for w, x in (("online", tr.c.theta), ("target", tr.target), ("m", tr.c.m), ("v", tr.c.v))]
        for k, (name, got, want, pad) in enumerate(sets):
            for l, ((W, b), (Ww, bw)) in enumerate(zip(got, want)):
                assert np.isfinite(Ww).all() and np.isfinite(bw).all(), (what, name, k, l)
                assert same_bits(W, Ww), (what, name, k, l, int((W.view(np.uint32) != Ww.view(np.uint32)).sum()), W.size)
                assert same_bits(b, bw), (what, name, k, l, b, bw)
            assert pad == 0, (what, name, k)
        assert same_bits(np.float64(st.actrain_var()), np.float64(tr.var)), (what, st.actrain_var(), tr.var)
        if tr.count is not None:
            B = self.batch
            td = torch.full((B + 1,), -7.25, dtype=torch.float64, device="cuda")
            idx = torch.full((B + 1,), -7, dtype=torch.int64, device="cuda")
            cnt = torch.full((B + 1,), -7, dtype=torch.int32, device="cuda")
            st.actrain_td(td[:B], idx[:B], cnt[:B])
            td, idx, cnt = td.cpu().numpy(), idx.cpu().numpy(), cnt.cpu().numpy()
            assert td[-1] == -7.25 and idx[-1] == -7 and cnt[-1] == -7, "the entry behind the last one was written"
            assert idx[:-1].tolist() == list(self.last_idx), what
            assert cnt[:-1].tolist() == tr.count.tolist(), (what, cnt[:-1], tr.count)
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


def one_and_three(c, what, selection=True):
    c.steps(1)
    assert c.tr.c.t == 1, "the model skipped a step the case means to apply"
    c.check((what, 1))
    c.steps(2)
    assert c.tr.c.t == 3
    c.check((what, 3))
    assert moved(c.tr.c.theta, c.c0) > 0 and moved(c.tr.a.theta, c.a0) > 0, "a network did not move: the case checks nothing"
    if selection:
        cnt = np.concatenate(c.counts)
        assert (cnt > 0).any() and (cnt == 0).any(), "the selection has one kind of row only"


@pytest.mark.parametrize("batch", [1, 15, 16, 17, 33])
def test_batches(batch):
    # batch 1: every reward is large, so the one row's td is positive and the actor is trained
    r = np.full(40, 100.0) if batch == 1 else None
    one_and_three(Case(65, (16, 16, 3), (17, 25, 1), batch, prio=True, rewards=r, E=4, seed=1), batch, selection=batch > 1)


@pytest.mark.parametrize("n_in", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_state_widths_and_dtypes(n_in, dtype):
    one_and_three(Case(n_in, (15, 2), (25, 1), 17, dtype=dtype, prio=(n_in % 2 == 1), E=1, seed=2), (n_in, dtype))


# (actor, critic, var_epochs, hi): the five-layer and the 256-unit sets at one epoch
LAYERS = [((2,), (1,), 4, 2), ((16, 16, 3), (17, 25, 1), 4, 2), ((33, 100, 4), (256, 1), 1, 2), ((100, 100, 1), (15, 1), 4, 2),
          ((17, 64, 33, 20, 4), (33, 256, 17, 64, 1), 1, 0)]


@pytest.mark.parametrize("actor,critic,E,hi", LAYERS, ids=["-".join(map(str, a)) + "_" + "-".join(map(str, c))
                                                          for a, c, _, _ in LAYERS])
@pytest.mark.parametrize("hidden", ["relu", "linear"])
def test_layer_sets_and_action_widths(actor, critic, E, hi, hidden):
    other = "linear" if hidden == "relu" else "relu"  # (the two networks' hidden activations differ too)
    one_and_three(Case(64, actor, critic, 18, ha=hidden, hc=other if len(critic) > 1 else hidden, prio=True, E=E, hi=hi,
                       seed=3), (actor, critic, hidden))


@pytest.mark.parametrize("E", [0, 1, 4])
def test_var_epochs(E):
    c = Case(65, (16, 16, 3), (17, 25, 1), 33, prio=True, E=E, seed=4)
    one_and_three(c, ("E", E))
    assert max(int(x.max()) for x in c.counts) == max(E, 1)
    if E == 0:
        assert c.tr.var == 1.0 and c.tr.cut == 0  # (plain CACLA keeps no variance)
    else:
        assert c.tr.var != 1.0


def test_three_distinct_counts_and_a_cut_row():
    c = Case(65, (16, 16, 3), (17, 25, 1), 33, prio=True, E=4, seed=4)
    c.steps(1)
    assert len(set(c.tr.count[c.tr.count > 0].tolist())) >= 3 and c.tr.cut >= 1, (c.tr.count, c.tr.cut)
    assert c.tr.a.t == c.tr.epochs == 4
    c.check("distinct counts")


def test_no_cut_row_under_a_large_variance():
    c = Case(65, (16, 16, 3), (17, 25, 1), 33, prio=True, E=4, var_start=4096.0, seed=4)
    one_and_three(c, "no cut")
    assert c.tr.cut == 0 and c.tr.epochs == 1 and c.tr.sel >= 1


def test_only_negative_td_leaves_the_actor_as_it_is():
    r = -1000.0 - np.arange(40.0)
    c = Case(65, (16, 16, 3), (17, 25, 1), 17, prio=True, rewards=r, E=4, seed=5)
    c.steps(1)
    c.check("negative 1")
    c.steps(2)
    c.check("negative 3")
    assert c.tr.c.t == 3 and c.tr.a.t == 0 and c.tr.sel == 0 and c.tr.epochs == 0
    assert (c.tr.td < 0).all() and c.tr.var != 1.0  # (the variance follows every row, whatever its sign)
    assert moved(c.tr.c.theta, c.c0) > 0 and moved(c.tr.a.theta, c.a0) == 0
    for which in ("m", "v"):
        for W, b in c.st.net_get_weights(which):
            assert not W.view(np.uint32).any() and not b.view(np.uint32).any()


def test_only_positive_td_selects_every_row():
    r = 1000.0 + np.arange(40.0)
    c = Case(65, (16, 16, 3), (17, 25, 1), 17, prio=False, rewards=r, E=4, seed=6)
    one_and_three(c, "positive", selection=False)
    assert (c.tr.td > 0).all() and c.tr.sel == 17 and c.tr.epochs == 4 and c.tr.cut == 3 * 17


def test_a_td_of_exactly_zero_is_not_selected():
    """A critic of zero weights gives V = +0.0 everywhere, so td is the reward: rows with a reward of
    +0.0 or -0.0 have td == 0 and take no part, though the variance follows them."""
    zero = [(np.zeros((65, 17), F32), np.zeros(17, F32)), (np.zeros((17, 1), F32), np.zeros(1, F32))]
    r = np.resize(np.array([0.0, 1.5, -0.0, -2.0, 0.25]), 40)
    c = Case(65, (16, 3), (17, 1), 20, rewards=r, E=4, critic_weights=zero, seed=7)
    u = (np.arange(20)[None, :] + 0.5) / 40
    c.steps(1, u)
    assert c.tr.c.t == 1 and (c.tr.td == 0).sum() == 8 and not c.tr.count[c.tr.td == 0].any()
    assert c.tr.sel == 8 and (c.tr.count[c.tr.td > 0] > 0).all() and moved(c.tr.a.theta, c.a0) > 0
    assert c.tr.c.theta[1][1][0] != 0  # (the critic's head bias moved)
    c.check("zero td")


def test_uniform_memory_writes_no_priorities_and_prioritized_does():
    c = Case(63, (16, 2), (16, 1), 16, prio=False, E=1, seed=4)
    one_and_three(c, "uniform")
    c = Case(63, (16, 2), (16, 1), 16, prio=True, E=1, seed=4)
    before = c.rm.total()
    one_and_three(c, "prioritized")
    assert c.rm.total() != before


def test_done_rows_at_tile_edges_and_a_batch_of_only_done_rows():
    n = 40
    done = np.zeros(n, bool)
    done[[0, 15, 16, 17, 31, 32]] = True
    c = Case(65, (16, 16, 3), (17, 25, 1), 33, done=done, E=4, seed=5)
    u = (np.arange(33)[None, :] + 0.5) / n * np.ones((3, 1))  # slot k in row k: the done rows sit at the tile edges
    c.steps(1, u[:1])
    c.check("edges 1")
    c.steps(2, u[1:])
    c.check("edges 3")
    assert c.tr.c.t == 3 and c.tr.a.t > 0
    c = Case(65, (16, 16, 3), (17, 25, 1), 17, done=np.ones(n, bool), prio=True, E=4, seed=6)
    one_and_three(c, "all done")


@pytest.mark.parametrize("prio", [False, True])
def test_memory_below_min_size_changes_nothing(prio):
    c = Case(64, (15, 2), (25, 1), 16, prio=prio, min_size=41, E=4, seed=11)
    c.steps(1)
    assert (c.tr.c.t, c.tr.a.t, c.tr.skipped, c.tr.var) == (0, 0, 1, 1.0)
    c.check("below min_size")
    c = Case(64, (15, 2), (25, 1), 16, prio=prio, n_mem=12, E=4, seed=11)  # fewer than a batch
    c.steps(2)
    assert (c.tr.c.t, c.tr.skipped) == (0, 2)
    c.check("below the batch")
    c = Case(64, (15, 2), (25, 1), 16, prio=prio, n_mem=0, E=4, seed=11)  # empty
    c.steps(1)
    assert (c.tr.c.t, c.tr.skipped) == (0, 1)
    c.check("empty")


def test_inf_reward_sets_the_warn_bit_and_changes_nothing():
    r = np.linspace(-1, 1, 40)
    r[5] = np.inf
    c = Case(64, (15, 2), (25, 1), 16, prio=True, rewards=r, E=4, seed=12)
    c.st.reset(11)  # (the warn bits are sticky since the last reset)
    assert c.st.warnings(0) & _abi.WARN_TRAIN_NONFINITE == 0
    # a fresh prioritized memory's leaves are all 1.0: u maps to floor(39 u); one row of the batch draws slot 5
    u = (np.arange(16)[None, :] + 20.5) / 39
    u[0, 15] = 5.5 / 39
    c.steps(1, u)
    assert c.last_idx[15] == 5 and c.tr.nonfinite and (c.tr.c.t, c.tr.a.t, c.tr.skipped, c.tr.var) == (0, 0, 1, 1.0)
    assert c.st.warnings(0) & _abi.WARN_TRAIN_NONFINITE
    c.check("inf")
    u[0, 15] = 6.5 / 39
    c.steps(1, u)
    assert c.tr.c.t == 1
    c.check("after inf")


def test_nonfinite_stored_action_skips_the_epoch_and_the_later_ones():
    c = Case(64, (15, 2), (25, 1), 16, prio=False, rewards=np.full(40, 100.0), E=4, seed=13)
    a = np.zeros((1, 4))
    a[0, 1] = np.inf
    row = c.rm.gather([7])[0]
    args = (np.asarray(row[0])[None], a, np.array([100.0]), np.asarray(row[3])[None], np.array([0], np.uint8))
    c.st.reset(11)
    c.st.exp_add(*args)  # slot 40
    c.rm.add(*args)
    u = (np.arange(16)[None, :] + 0.5) / 41
    u[0, 9] = 40.5 / 41
    c.steps(1, u)
    assert c.last_idx[9] == 40 and c.tr.c.t == 1 and c.tr.a.t == 0 and c.tr.eskipped == c.tr.epochs == 4
    assert c.st.warnings(0) & _abi.WARN_TRAIN_NONFINITE
    c.check("inf action")
    u[0, 9] = 9.5 / 41
    c.steps(1, u)
    assert c.tr.a.t == 4 and c.tr.eskipped == 4
    c.check("after inf action")


def test_target_copy_with_target_steps_two_over_five_steps_sync_and_reset():
    c = Case(65, (16, 2), (15, 25, 1), 17, target_steps=2, prio=True, E=1, seed=10)
    c.steps(1)
    c.check("t1")
    assert same_bits(c.tr.target[0][0], c.c0[0][0]) and c.tr.since == 1
    c.steps(2)
    assert c.tr.since == 1 and not same_bits(c.tr.target[0][0], c.c0[0][0])
    assert not same_bits(c.tr.target[0][0], c.tr.c.theta[0][0])  # (step 2's weights, not step 3's)
    c.check("t3")
    c.steps(2)  # the copy after step 4
    assert c.tr.since == 1 and c.tr.c.t == 5
    c.check("t5")
    c.st.actrain_sync_target()
    c.tr.sync_target()
    c.check("synced")
    c.st.actrain_reset()
    c.tr.reset()
    assert c.tr.var == 1.0 and (c.tr.c.t, c.tr.a.t) == (0, 0)
    c.check("reset")
    c.steps(1)
    c.check("after reset")


def test_set_weights_between_steps():
    c = Case(65, (16, 2), (15, 1), 17, prio=True, E=1, seed=13)
    c.steps(2)
    rng = np.random.default_rng(77)
    wa, wc = M.make_weights(rng, 65, (16, 2), hi=2), M.make_weights(rng, 65, (15, 1), hi=2)
    c.st.net_set_weights(wa)
    c.st.critic_set_weights(wc)
    c.tr.a.theta = [(W.copy(), b.copy()) for W, b in wa]
    c.tr.c.theta = [(W.copy(), b.copy()) for W, b in wc]
    c.check("pushed")  # (the target, m, v and the counters are as they were)
    c.steps(2)
    c.check("after push")


@pytest.mark.parametrize("rows", [1, 16, 17])
def test_critic_forward_equals_the_model(rows):
    import torch
    st = handle(65)
    rng = np.random.default_rng(rows)
    st.net_config((65, (4, 2), "relu", "sigmoid"))
    for hidden, units in (("relu", (17, 25, 1)), ("linear", (1,))):
        w = M.make_weights(rng, 65, units, hi=2)
        st.critic_config((65, units, hidden, "linear"))
        st.critic_set_weights(w)
        for dt in (np.float64, np.float32):
            x = M.mixed(rng, (rows, 65), hi=3).astype(dt)
            out = torch.full((rows + 1,), -7.25, dtype=torch.float64, device="cuda")
            st.critic_forward(dev(x), out[:rows])
            out = out.cpu().numpy()
            assert out[-1] == -7.25
            assert same_bits(out[:-1], M.forward(x, w, hidden, "linear")[:, 0])
        got = st.critic_get_weights("online")  # (needs only a critic)
        assert all(same_bits(W, Ww) and same_bits(b, bw) for (W, b), (Ww, bw) in zip(got, w))


def test_own_draws_follow_the_memorys_stream():
    import torch
    c = Case(64, (15, 2), (25, 1), 16, prio=False, E=1, seed=15)
    w = torch.zeros(16, dtype=torch.float64, device="cuda")
    i0 = torch.zeros(16, dtype=torch.int64, device="cuda")
    c.st.exp_sample(w, i0)  # call 0 of the stream
    c2 = Case(64, (15, 2), (25, 1), 16, prio=False, E=1, seed=15)
    c2.st.actrain_step(1)
    idx = torch.zeros(16, dtype=torch.int64, device="cuda")
    c2.st.actrain_td(None, idx, None)
    assert idx.cpu().numpy().tolist() == i0.cpu().numpy().tolist()
    assert c2.st.actrain_info()["steps"] == 1


def test_live_handle_refusals():
    import ctypes as C
    st = handle(64)
    st.net_config(None)
    st.exp_config(CAP)
    crit = (64, (15, 1), "relu", "linear")
    with pytest.raises(RuntimeError, match="critic_config: no acting network"):
        st.critic_config(crit)
    with pytest.raises(RuntimeError, match="actrain_config: no acting network"):
        st.actrain_config(batch=16)
    st.net_config((64, (15, 2), "relu", "sigmoid"))
    with pytest.raises(RuntimeError, match="no critic is configured"):
        st.actrain_config(batch=16)
    with pytest.raises(RuntimeError, match="no critic is configured"):
        st.critic_get_weights("online")
    with pytest.raises(RuntimeError, match="n_in = 63 differs from the acting network's 64"):
        st.critic_config((63, (15, 1), "relu", "linear"))
    with pytest.raises(RuntimeError, match="V\\(s\\) is one linear unit"):
        st.critic_config((64, (15, 2), "relu", "linear"))
    with pytest.raises(RuntimeError, match="V\\(s\\) is one linear unit"):
        st.critic_config((64, (15, 1), "relu", "sigmoid"))
    with pytest.raises(ValueError, match="critic_config: x_dtype must be float64 or float32, got float16"):
        st.critic_config(crit, x_dtype="float16")
    st.critic_config(crit, x_dtype=np.float64)  # (numpy and torch dtypes are taken, as net_config takes them)
    assert st.crit == (64, (15, 1))
    st.critic_config(crit)
    with pytest.raises(RuntimeError, match="the network's head is sigmoid, Q-learning needs a linear head"):
        st.train_config(batch=16)  # (the Q trainer's own message, as before)
    st.exp_config(None)
    with pytest.raises(RuntimeError, match="no replay memory"):
        st.actrain_config(batch=16)
    st.exp_config(CAP)
    st.net_config((64, (15, 2), "relu", "linear"))  # (drops the critic)
    assert st.L.aigar_critic_forward(st.h, None, 0, 1, None) < 0 and b"no critic is configured" in st.L.aigar_last_error()
    st.critic_config(crit)
    with pytest.raises(RuntimeError, match="the network's head is linear, the CACLA actor needs a sigmoid head"):
        st.actrain_config(batch=16)
    st.net_config((64, (15, 5), "relu", "sigmoid"))
    st.critic_config(crit)
    with pytest.raises(RuntimeError, match="5 outputs"):
        st.actrain_config(batch=16)
    st.net_config((64, (15, 2), "relu", "sigmoid"))
    st.critic_config(crit)
    st.actrain_config(batch=16)
    with pytest.raises(RuntimeError, match="n_steps = 0"):
        st.actrain_step(0)
    with pytest.raises(RuntimeError, match="CACLA keeps no actor target"):
        st.net_get_weights("target")
    v = C.c_int64()
    assert st.L.aigar_net_pad_check(st.h, 1, C.byref(v)) < 0 and b"CACLA keeps no actor target" in st.L.aigar_last_error()
    assert st.L.aigar_net_pad_check(st.h, 8, C.byref(v)) < 0 and b"outside 0..7" in st.L.aigar_last_error()
    st.critic_config(crit)  # reconfiguring the critic drops the train configuration
    assert st.L.aigar_actrain_step(st.h, 1, None) < 0 and b"no CACLA training is configured" in st.L.aigar_last_error()
    assert st.L.aigar_net_pad_check(st.h, 5, C.byref(v)) < 0 and b"no CACLA training" in st.L.aigar_last_error()
    st.actrain_config(batch=16)
    st.exp_config(CAP)  # ... and so does the memory
    assert st.L.aigar_actrain_step(st.h, 1, None) < 0 and b"no CACLA training is configured" in st.L.aigar_last_error()
    st.actrain_config(batch=16)
    st.net_config((64, (15, 2), "relu", "sigmoid"))  # ... and the network, with the critic
    assert st.L.aigar_actrain_step(st.h, 1, None) < 0 and b"no CACLA training is configured" in st.L.aigar_last_error()
    st.critic_config(None)
    # a conv part
    from aigar_amd import net as N
    px = _lib.Stepper(make_config(n_arenas=1, bots=2, field_size=100, flags=0))
    try:
        px.pixel_config(8)
        px.exp_config(CAP, dtype="float32")
        px.net_config(N.CnnSpec(8, 1, ((3, 1, 4),), 6 * 6 * 4, (2,), "relu", "sigmoid"), x_dtype="float32")
        with pytest.raises(RuntimeError, match="critic_config: the acting network has a conv part"):
            px.critic_config((6 * 6 * 4, (1,), "relu", "linear"))
        with pytest.raises(RuntimeError, match="actrain_config: a network with a conv part"):
            px.actrain_config(batch=4)
    finally:
        px.close()


def test_tiled_handle_is_refused():
    import ctypes as C
    st = _lib.Stepper(make_config(n_arenas=1, bots=4, field_size=100, flags=0, tile_x=1, tile_y=1, tile_id=0,
                                  tile_flags=_abi.TILE_FORCE))
    try:
        prm = _abi.ActrainParams(16, 0, 0, 0, 1e-4, 1e-4, 0.9, 0.999, 1e-7, 0.85, 1.0, 0.001)
        assert st.L.aigar_actrain_config(st.h, C.byref(prm)) < 0
        assert b"actrain_config: a tiled handle" in st.L.aigar_last_error()
    finally:
        st.close()
