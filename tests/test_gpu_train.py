"""GPU: aigar_train_step (train.inc) against the Python model (tests/train_model.py, checked
by tests/test_train_model.py), bit pattern for bit pattern: online and target weights, Adam's
m and v (read back with aigar_net_get_weights), the TD errors, the drawn indices and the
prioritized memory's trees (through a sample with given draws, whose indices and weights are
functions of the tree sums).  No tolerance anywhere.

Shapes: batches 1 / 15 / 16 / 17 / 32 / 33 (the 4-row MFMA steps of the gradient's chain, the
16-row tiles of the other kernels, more than one workgroup), state widths 1 / 63 / 64 / 65 / 130
(the first layer's 64-wide chunks and the gradient's 16-row k tiles), layer sets from the
head alone to five layers (unit tiles of 1 .. 16 per layer, tiles dealt to four waves).

Magnitudes: states and weights 2^-30 .. 2^2 with subnormals and signed zeros (2^0 for the five
layer case), so that no gradient overflows float32: an overflow would make an inf - inf NaN,
whose payload is not part of the contract."""
import numpy as np
import pytest

import net_model as M
import train_model as T
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
    """A handle with a filled memory, a network and a train configuration, and its model twin."""

    def __init__(self, n_in, units, batch, hidden="relu", dtype="float64", prio=False, n_mem=40, hi=2, seed=0,
                 target_steps=0, min_size=0, done=None, actions=None, rewards=None, weights=None, states=None, lr=1e-2):
        self.st = st = handle(n_in)
        self.rng = rng = np.random.default_rng(1000 * n_in + 10 * batch + seed)
        self.n_in, self.units, self.batch, self.dtype, self.prio = n_in, tuple(units), batch, dtype, prio
        n_out = units[-1]
        np_dt = np.float64 if dtype == "float64" else np.float32
        st.exp_config(CAP, prioritized=prio, dtype=dtype, seed=3)
        st.decide_config(np.zeros((n_out, 4)), q_dtype="float64")
        st.net_config((n_in, self.units, hidden, "linear"), x_dtype=dtype)
        self.w0 = weights if weights is not None else M.make_weights(rng, n_in, self.units, hi=hi)
        st.net_set_weights(self.w0)
        self.rm = ReplayModel(CAP, prio)
        if n_mem:
            s = M.mixed(rng, (n_mem, n_in), hi=3) if states is None else states
            s2 = M.mixed(rng, (n_mem, n_in), hi=3)
            if dtype == "float64":  # float64 rows that are not float32 values: one rounding each
                s, s2 = (np.where(x == 0, x, x.astype(np.float64) * (1 + 2.0 ** -30)) for x in (s, s2))
            a = np.zeros((n_mem, 4))
            a[:, 0] = rng.integers(0, n_out, n_mem) if actions is None else actions
            r = M.mixed(rng, (n_mem,), lo=-10, hi=5).astype(np.float64) if rewards is None else rewards
            d = (rng.random(n_mem) < 0.25) if done is None else done
            d = np.asarray(d, bool)
            s2 = s2.astype(np_dt)
            s2[d] = np.nan  # (the decision's transitions: a dead player's new state is the NaN row)
            args = (s.astype(np_dt), a, np.asarray(r, np.float64), s2, d.astype(np.uint8))
            st.exp_add(*args)
            self.rm.add(*args)
        self.kw = dict(lr=lr, beta1=0.9, beta2=0.999, epsilon=1e-7, discount=0.85, target_steps=target_steps,
                       min_size=min_size)
        st.train_config(batch=batch, **self.kw)
        self.tr = T.Trainer(self.w0, batch, hidden=hidden, **self.kw)

    def model_step(self, u):
        idx, w = self.rm.sample(list(u))
        if not self.tr.can_draw(self.rm.size) or idx[0] < 0:
            self.tr.skipped += 1
            return idx, None
        rows = self.rm.gather(idx)
        s, a, r, s2, d = (np.array([row[k] for row in rows]) for k in range(5))
        prio = self.tr.step(s, a[:, 0], r, s2, d, np.asarray(w))
        if prio is not None:
            self.rm.update(idx, prio)
        return idx, prio

    def steps(self, n, u=None):
        """n steps on both sides from the same draws."""
        u = self.rng.random((n, self.batch)) if u is None else u
        self.st.train_step(n, dev(u))
        for k in range(n):
            self.last_idx, _ = self.model_step(u[k])

    def check(self, what):
        import torch
        st, tr = self.st, self.tr
        info = st.train_info()
        assert (info["steps"], info["skipped"], info["since_target"]) == (tr.t, tr.skipped, tr.since), (what, info)
        for which, want in (("online", tr.theta), ("target", tr.target), ("m", tr.m), ("v", tr.v)):
            got = st.net_get_weights(which)
            for l, ((W, b), (Ww, bw)) in enumerate(zip(got, want)):
                assert np.isfinite(Ww).all() and np.isfinite(bw).all(), (what, which, l)
                assert same_bits(W, Ww), (what, which, l, int((W.view(np.uint32) != Ww.view(np.uint32)).sum()), W.size)
                assert same_bits(b, bw), (what, which, l, b, bw)
            assert st.net_pad_check(which) == 0, (what, which)
        if tr.td is not None:
            td = torch.full((self.batch + 1,), -7.25, dtype=torch.float64, device="cuda")
            idx = torch.full((self.batch + 1,), -7, dtype=torch.int64, device="cuda")
            st.train_td(td[:self.batch], idx[:self.batch])
            td, idx = td.cpu().numpy(), idx.cpu().numpy()
            assert td[-1] == -7.25 and idx[-1] == -7, "the entry behind the last one was written"
            assert idx[:-1].tolist() == list(self.last_idx), what
            fin = np.isfinite(tr.td)
            assert same_bits(td[:-1][fin], tr.td[fin]) and np.array_equal(np.isnan(td[:-1]), np.isnan(tr.td)), what
        if self.prio and self.rm.size >= 2:  # the trees: a sample's indices and weights are functions of their sums
            u = np.linspace(0.0, 0.999, 23)
            w = torch.zeros(23, dtype=torch.float64, device="cuda")
            i = torch.zeros(23, dtype=torch.int64, device="cuda")
            st.exp_sample(w, i, u=dev(u))
            wi, ww = self.rm.sample(list(u))
            assert i.cpu().numpy().tolist() == list(wi), what
            assert same_bits(w.cpu().numpy(), np.asarray(ww, np.float64)), what


def one_and_three(c, what):
    c.steps(1)
    assert c.tr.t == 1, "the model skipped a step the case means to apply"
    c.check((what, 1))
    c.steps(2)
    assert c.tr.t == 3
    c.check((what, 3))
    moved = sum(int((W != W0).sum()) for (W, _), (W0, _) in zip(c.tr.theta, c.w0))
    assert moved > 0, "no weight moved: the case checks nothing"


@pytest.mark.parametrize("batch", [1, 15, 16, 17, 32, 33])
def test_batches(batch):
    one_and_three(Case(65, (17, 25), batch, prio=True, seed=1), batch)


@pytest.mark.parametrize("n_in", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_state_widths_and_dtypes(n_in, dtype):
    one_and_three(Case(n_in, (15, 25), 17, dtype=dtype, prio=(n_in % 2 == 1), seed=2), (n_in, dtype))


LAYERS = [(25,), (15, 25), (16, 16), (17, 100, 25), (256, 3), (33, 256, 17, 64, 5)]


@pytest.mark.parametrize("units", LAYERS, ids=["-".join(map(str, u)) for u in LAYERS])
@pytest.mark.parametrize("hidden", ["relu", "linear"])
def test_layer_sets(units, hidden):
    one_and_three(Case(64, units, 18, hidden=hidden, prio=True, hi=0 if len(units) == 5 else 2, seed=3), (units, hidden))


def test_uniform_memory_writes_no_priorities_and_prioritized_does():
    c = Case(63, (16, 16), 16, prio=False, seed=4)
    one_and_three(c, "uniform")
    c = Case(63, (16, 16), 16, prio=True, seed=4)
    before = c.rm.total()
    one_and_three(c, "prioritized")
    assert c.rm.total() != before


def test_done_rows_at_tile_edges_and_a_batch_of_only_done_rows():
    n = 40
    done = np.zeros(n, bool)
    done[[0, 15, 16, 17, 31, 32]] = True
    c = Case(65, (17, 25), 33, done=done, seed=5)
    u = (np.arange(33)[None, :] + 0.5) / n * np.ones((3, 1))  # slot k in row k: the done rows sit at the tile edges
    c.steps(1, u[:1])
    c.check("edges 1")
    c.steps(2, u[1:])
    c.check("edges 3")
    assert c.tr.t == 3
    c = Case(65, (17, 25), 17, done=np.ones(n, bool), prio=True, seed=6)
    one_and_three(c, "all done")


def test_repeated_index_feeds_the_gradient_twice_and_keeps_the_last_priority():
    c = Case(64, (15, 25), 16, prio=True, seed=7)
    u = c.rng.random((1, 16))
    u[0, 3] = u[0, 11] = u[0, 12] = u[0, 5]
    c.steps(1, u)
    assert len(set(c.last_idx)) < 16 and c.tr.t == 1
    c.check("repeated")
    # the uniform memory maps u straight to the slot: rows 2 and 9 are slot 7
    c = Case(64, (15, 25), 16, prio=False, seed=7)
    u = c.rng.random((1, 16))
    u[0, 2] = u[0, 9] = 7.5 / 40
    c.steps(1, u)
    assert c.last_idx[2] == c.last_idx[9] == 7
    c.check("repeated uniform")
    once = Case(64, (15, 25), 16, prio=False, seed=7)
    u2 = u.copy()
    u2[0, 9] = 8.5 / 40
    once.steps(1, u2)
    assert not same_bits(once.tr.theta[0][0], c.tr.theta[0][0])  # (the second occurrence is in the gradient)


def test_action_index_at_the_tile_edges():
    n = 40
    acts = np.resize(np.array([0, 15, 16, 24]), n)
    c = Case(63, (17, 25), 17, actions=acts, prio=True, seed=8)
    one_and_three(c, "actions")
    assert set(int(c.rm.rows[i][1][0]) for i in c.last_idx) == {0, 15, 16, 24}


def test_relu_gate_is_closed_at_signed_zero_preactivations():
    """Unit 0 of the hidden layer gets y = -0.0f (one product that underflows to -0.0f, the
    others -0.0f, bias -0.0f), unit 1 y = +0.0f (zero column): neither passes an error back, so their incoming
    kernels' gradients are zero while their outgoing ones are not asked."""
    n_in, n = 63, 40
    rng = np.random.default_rng(9)
    w = M.make_weights(rng, n_in, (17, 25))
    W0, b0 = w[0]
    W0[:, 0] = F32(-0.0)  # (against positive states: every later product is -0.0f too)
    W0[0, 0] = F32(-2.0 ** -100)
    b0[0] = F32(-0.0)
    W0[:, 1] = 0.0
    b0[1] = F32(0.0)
    s = np.abs(M.mixed(rng, (n, n_in), hi=3))
    s[:, 0] = F32(2.0 ** -100)
    hs, _ = T.forward_saved(s, w)
    assert (hs[1][:, :2] == 0).all()
    y = M.layer_acc(s, W0) + b0[None, :]
    assert np.signbit(y[:, 0]).all() and not np.signbit(y[:, 1]).any() and (y[:, :2] == 0).all()
    c = Case(n_in, (17, 25), 16, weights=w, states=s, dtype="float32", seed=9)
    c.steps(1)
    assert c.tr.t == 1
    assert (c.tr.grads[0][0][:, :2] == 0).all() and (c.tr.grads[0][0][:, 2:] != 0).any()
    assert (c.tr.grads[1][0][2:] != 0).any()  # (an open gate here would have passed these back)
    c.check("gate")


def test_target_copy_falls_on_step_two_of_three():
    c = Case(65, (15, 25), 17, target_steps=2, prio=True, seed=10)
    c.steps(1)
    c.check("t1")
    assert same_bits(c.tr.target[0][0], c.w0[0][0]) and c.tr.since == 1
    c.steps(2)
    assert c.tr.since == 1 and not same_bits(c.tr.target[0][0], c.w0[0][0])
    assert not same_bits(c.tr.target[0][0], c.tr.theta[0][0])  # (step 2's weights, not step 3's)
    c.check("t3")
    c.steps(3)  # n steps in one call: copies after steps 4 and 6
    assert c.tr.since == 0
    c.check("t6")
    c.st.train_sync_target()
    c.tr.sync_target()
    c.check("synced")


@pytest.mark.parametrize("prio", [False, True])
def test_memory_below_min_size_changes_nothing(prio):
    c = Case(64, (15, 25), 16, prio=prio, min_size=41, seed=11)
    c.steps(1)
    assert (c.tr.t, c.tr.skipped) == (0, 1)
    c.check("below min_size")
    c = Case(64, (15, 25), 16, prio=prio, n_mem=12, seed=11)  # fewer than a batch
    c.steps(2)
    assert (c.tr.t, c.tr.skipped) == (0, 2)
    c.check("below the batch")
    c = Case(64, (15, 25), 16, prio=prio, n_mem=0, seed=11)  # empty
    c.steps(1)
    assert (c.tr.t, c.tr.skipped) == (0, 1)
    c.check("empty")


def test_nan_reward_sets_the_warn_bit_and_changes_nothing():
    r = np.linspace(-1, 1, 40)
    r[5] = np.nan
    c = Case(64, (15, 25), 16, prio=True, rewards=r, seed=12)
    c.st.reset(11)  # (the warn bits are sticky since the last reset)
    assert c.st.warnings(0) & _abi.WARN_TRAIN_NONFINITE == 0
    # a fresh prioritized memory's leaves are all 1.0: u maps to floor(39 u); one row of the batch draws slot 5
    u = (np.arange(16)[None, :] + 20.5) / 39
    u[0, 15] = 5.5 / 39
    c.steps(1, u)
    assert c.last_idx[15] == 5 and c.tr.nonfinite and (c.tr.t, c.tr.skipped) == (0, 1)
    assert c.st.warnings(0) & _abi.WARN_TRAIN_NONFINITE
    c.check("nan")
    u[0, 15] = 6.5 / 39
    c.steps(1, u)
    assert c.tr.t == 1
    c.check("after nan")


def test_set_weights_between_steps_and_train_reset():
    c = Case(65, (15, 25), 17, prio=True, target_steps=5, seed=13)
    c.steps(2)
    w = M.make_weights(np.random.default_rng(77), 65, (15, 25), hi=2)
    c.st.net_set_weights(w)
    c.tr.set_weights(w)
    c.check("pushed")  # (target, m, v and t are as they were)
    c.steps(2)
    assert c.tr.t == 4
    c.check("after push")
    c.st.train_reset()
    c.tr.reset()
    c.check("reset")
    c.steps(1)
    c.check("after reset")


def test_read_back_has_a_canary_and_device_tensors_agree():
    import torch
    c = Case(63, (17, 25), 16, seed=14)
    c.steps(1)
    host = c.st.net_get_weights("online")
    devw = c.st.net_get_weights("online", device=True)
    for (W, b), (Wd, bd) in zip(host, devw):
        assert same_bits(W, Wd.cpu().numpy()) and same_bits(b, bd.cpu().numpy())
    L = c.st.L
    import ctypes as C
    W = torch.full((63 * 17 + 5,), -7.25, dtype=torch.float32, device="cuda")
    b = torch.full((17 + 5,), -7.25, dtype=torch.float32, device="cuda")
    assert L.aigar_net_get_weights(c.st.h, 0, 0, C.c_void_p(W.data_ptr()), C.c_void_p(b.data_ptr()), 1) == 0
    c.st.sync()
    assert (W[63 * 17:] == -7.25).all() and (b[17:] == -7.25).all()
    assert same_bits(W[:63 * 17].cpu().numpy().reshape(63, 17), host[0][0])


def test_own_draws_follow_the_memorys_stream():
    """u = None: the draws of aigar_exp_sample's stream -- a twin handle state that samples with the
    memory's own stream sees the same indices."""
    import torch
    c = Case(64, (15, 25), 16, prio=False, seed=15)
    w = torch.zeros(16, dtype=torch.float64, device="cuda")
    i0 = torch.zeros(16, dtype=torch.int64, device="cuda")
    c.st.exp_sample(w, i0)  # call 0 of the stream
    c2 = Case(64, (15, 25), 16, prio=False, seed=15)
    c2.st.train_step(1)
    idx = torch.zeros(16, dtype=torch.int64, device="cuda")
    c2.st.train_td(None, idx)
    assert idx.cpu().numpy().tolist() == i0.cpu().numpy().tolist()
    assert c2.st.train_info()["steps"] == 1


def test_live_handle_refusals():
    st = handle(64)
    st.train_config(None)
    st.net_config(None)
    st.exp_config(CAP)
    st.decide_config(np.zeros((25, 4)), q_dtype="float64")
    with pytest.raises(RuntimeError, match="no acting network"):
        st.train_config(batch=16)
    st.net_config((64, (15, 25), "relu", "sigmoid"))
    with pytest.raises(RuntimeError, match="linear head"):
        st.train_config(batch=16)
    st.net_config((64, (15, 25), "relu", "linear"))
    st.exp_config(None)
    with pytest.raises(RuntimeError, match="no replay memory"):
        st.train_config(batch=16)
    st.exp_config(CAP)
    st.decide_config(None)
    with pytest.raises(RuntimeError, match="no action selection"):
        st.train_config(batch=16)
    st.decide_config(np.zeros((24, 4)), q_dtype="float64")
    with pytest.raises(RuntimeError, match="25 outputs, the action selection 24"):
        st.train_config(batch=16)
    st.decide_config(np.zeros((25, 4)), q_dtype="float64")
    st.train_config(batch=16)
    with pytest.raises(RuntimeError, match="n_steps = 0"):
        st.train_step(0)
    st.net_config((64, (15, 25), "relu", "linear"))  # reconfiguring the network drops the train configuration
    assert st.L.aigar_train_step(st.h, 1, None) < 0 and b"no training is configured" in st.L.aigar_last_error()
    st.train_config(batch=16)
    st.exp_config(CAP)  # ... and so does the memory
    assert st.L.aigar_train_step(st.h, 1, None) < 0 and b"no training is configured" in st.L.aigar_last_error()
    # a conv part
    from aigar_amd import net as N
    px = _lib.Stepper(make_config(n_arenas=1, bots=2, field_size=100, flags=0))
    try:
        px.pixel_config(8)
        px.exp_config(CAP, dtype="float32")
        px.decide_config(np.zeros((4, 4)), q_dtype="float64")
        px.net_config(N.CnnSpec(8, 1, ((3, 1, 4),), 6 * 6 * 4, (4,), "relu", "linear"), x_dtype="float32")
        with pytest.raises(RuntimeError, match="conv part"):
            px.train_config(batch=4)
    finally:
        px.close()


def test_tiled_handle_is_refused():
    st = _lib.Stepper(make_config(n_arenas=1, bots=4, field_size=100, flags=0, tile_x=1, tile_y=1, tile_id=0,
                                  tile_flags=_abi.TILE_FORCE))
    try:
        prm = _abi.TrainParams(16, 0, 0, 0, 1e-4, 0.9, 0.999, 1e-7, 0.85)
        import ctypes as C
        assert st.L.aigar_train_config(st.h, C.byref(prm)) < 0
        assert b"tiled handle" in st.L.aigar_last_error()
    finally:
        st.close()
