"""GPU: aigar_train_step under aigar_train_config_cnn (convtrain.inc) against the Python model
(tests/cnn_train_model.py, checked by tests/test_cnn_train_model.py), bit pattern for bit
pattern after every one of 3 steps: conv and dense online and target weights, Adam's m and v, the
TD errors, the drawn indices and the prioritized memory's trees.  No tolerance anywhere.

The geometries (tests/cnn_train_cases.py) are the smallest at which the kernels can go wrong:
(a) one layer, F < 16, K = 9; (b) positions that no window reaches, F = 17 across a tile, stride =
kernel, three image channels; (c) three layers down to 1 x 1, overlapping windows, two input
error launches; (d) the reference's default at batch 5, M = 405 and 45 (the gradient chain ends
inside a 4-step), two and four filter tiles."""
import ctypes as C

import numpy as np
import pytest

import cnn_train_cases as W
import cnn_train_model as CT
import conv_model as CM
import net_model as M
from oracle_lib import make_config
from replay_model import ReplayModel

pytestmark = pytest.mark.gpu
from aigar_amd import _abi, _lib  # noqa: E402
from aigar_amd import net as N  # noqa: E402

F32 = np.float32
CAP = 64
PIX = {1: (False, False), 3: (True, False), 2: (False, True)}  # channels -> (rgb, last)
_G = {}


@pytest.fixture(scope="module", autouse=True)
def close_handles():
    yield
    for g in _G.values():
        g.close()
    _G.clear()


def handle(side, channels, twin=0):
    key = (side, channels, twin)
    if key not in _G:
        import torch
        st = _lib.Stepper(make_config(n_arenas=1, bots=2, field_size=100, flags=0))
        st.set_stream(torch.cuda.current_stream().cuda_stream)  # (ordered with the tensors torch makes and reads)
        st.reset(11)
        st.pixel_config(side, *PIX[channels])
        assert st.pixel_state_shape[1:] == (side, side, channels)
        _G[key] = st
    return _G[key]


def dev(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    v = np.uint64 if a.dtype.itemsize == 8 else np.uint32
    return np.array_equal(a.view(v), b.view(v))


def spec(geo, out="linear"):
    side, ch, cg, units = W.GEOMETRIES[geo]
    return N.CnnSpec(side, ch, cg, CM.n_flat(side, cg), units, "relu", out)


class Case:
    """A handle with a filled memory, a CNN and a train configuration, and its model twin."""

    def __init__(self, geo, batch=None, dtype="float64", prio=False, seed=0, target_steps=0, min_size=0, twin=0, **kw):
        side, ch, cg, units = W.GEOMETRIES[geo]
        self.geo, self.batch, self.prio = geo, batch or W.BATCHES[geo], prio
        self.st = st = handle(side, ch, twin)
        self.rng = np.random.default_rng(100 * self.batch + seed)
        st.exp_config(CAP, prioritized=prio, dtype=dtype, seed=3)
        st.net_config(spec(geo), x_dtype=dtype)
        self.convs, self.dense, rows = W.world(geo, seed, dtype, **kw)
        st.net_set_weights(CM.pairs(self.convs, self.dense))
        self.rm = ReplayModel(CAP, prio)
        if len(rows[0]):
            st.exp_add(*rows)
            self.rm.add(rows[0].reshape(len(rows[0]), -1), *rows[1:3], rows[3].reshape(len(rows[0]), -1), rows[4])
        self.kw = dict(W.KW, target_steps=target_steps, min_size=min_size)
        st.train_config_cnn(batch=self.batch, **self.kw)
        self.tr = CT.CnnTrainer(self.convs, self.dense, self.batch, **self.kw)
        self.shape = (side, side, ch)
        self.last_idx = None

    def model_step(self, u):
        idx, w = self.rm.sample(list(u))
        if not self.tr.can_draw(self.rm.size) or idx[0] < 0:
            self.tr.skipped += 1
            return idx, None
        rows = self.rm.gather(idx)
        s, a, r, s2, d = (np.array([row[k] for row in rows]) for k in range(5))
        B = len(rows)
        prio = self.tr.step(s.reshape((B,) + self.shape), a[:, 0], r, s2.reshape((B,) + self.shape), d, np.asarray(w))
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
        for which, name in (("online", "theta"), ("target", "target"), ("m", "m"), ("v", "v")):
            got, want = st.net_get_weights(which), tr.pairs(name)
            assert len(got) == len(want)
            for l, ((Wg, bg), (Ww, bw)) in enumerate(zip(got, want)):
                assert np.isfinite(Ww).all() and np.isfinite(bw).all(), (what, which, l)
                assert same_bits(Wg, Ww), (what, which, l, int((Wg.view(np.uint32) != Ww.view(np.uint32)).sum()), Wg.size)
                assert same_bits(bg, bw), (what, which, l, bg, bw)
            assert st.net_pad_check(which) == 0, (what, which)
        if tr.td is not None and self.last_idx is not None:
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


def three_steps(c, what):
    """Compared after every one of 3 steps."""
    w0 = c.tr.pairs()
    for k in (1, 2, 3):
        c.steps(1)
        assert c.tr.t == k, "the model skipped a step the case means to apply"
        c.check((what, k))
    moved = [int((Wn != Wo).sum()) for (Wn, _), (Wo, _) in zip(c.tr.pairs(), w0)]
    assert all(moved), ("a layer whose kernel did not move: the case checks nothing of it", moved)


@pytest.mark.parametrize("batch", [1, 5, 16, 17, 33])
def test_batches_put_tile_edges_of_m_in_every_kernel(batch):
    three_steps(Case("a", batch, prio=True, seed=1), batch)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_both_memory_dtypes_and_positions_no_window_reaches(dtype):
    c = Case("b", dtype=dtype, prio=(dtype == "float32"), seed=2)
    three_steps(c, dtype)
    # layer 1's row and column 4 are reached by no layer-2 window: their delta is +0.0f
    d1 = c.tr.deltas[0]
    assert d1.shape[1:3] == (5, 5) and (d1.view(np.uint32)[:, 4, :, :] == 0).all() and (d1.view(np.uint32)[:, :, 4, :] == 0).all()
    assert (d1[:, :4, :4, :] != 0).any()


@pytest.mark.parametrize("prio", [False, True])
def test_three_layers_on_uniform_and_prioritized_memories(prio):
    c = Case("c", prio=prio, seed=3)
    before = c.rm.total() if prio else None
    three_steps(c, prio)
    if prio:
        assert c.rm.total() != before


def test_the_default_geometry_at_batch_five():
    three_steps(Case("d", prio=True, seed=4), "default")


def test_target_copy_falls_on_step_two_of_three():
    c = Case("b", target_steps=2, prio=True, seed=5)
    w0 = c.tr.pairs()
    c.steps(1)
    c.check("t1")
    assert all(same_bits(Wt, Wo) for (Wt, _), (Wo, _) in zip(c.tr.pairs("target"), w0)) and c.tr.since == 1
    c.steps(1)
    c.check("t2")
    assert c.tr.since == 0
    for (Wt, _), (Wo, _), (Wn, _) in zip(c.tr.pairs("target"), w0, c.tr.pairs()):
        assert not same_bits(Wt, Wo) and same_bits(Wt, Wn)  # (conv filters included)
    c.steps(1)
    c.check("t3")
    assert c.tr.since == 1
    assert not same_bits(c.tr.pairs("target")[0][0], c.tr.pairs()[0][0])  # (step 2's filters, not step 3's)
    c.st.train_sync_target()
    c.tr.sync_target()
    c.check("synced")


def test_done_rows_at_tile_edges_and_a_batch_of_only_done_rows():
    n = W.N_MEM
    done = np.zeros(n, bool)
    done[[0, 15, 16, 17, 31, 32]] = True
    c = Case("a", 33, done=done, seed=6)
    u = (np.arange(33)[None, :] + 0.5) / n * np.ones((3, 1))  # slot k in row k: the done rows sit at the tile edges
    for k in range(3):
        c.steps(1, u[k:k + 1])
        c.check(("edges", k))
    assert c.tr.t == 3
    three_steps(Case("a", 17, done=np.ones(n, bool), prio=True, seed=7), "all done")


def test_repeated_index_feeds_the_gradient_twice():
    c = Case("a", 16, prio=False, seed=8)
    u = c.rng.random((1, 16))
    u[0, 2] = u[0, 9] = 7.5 / W.N_MEM  # the uniform memory maps u straight to the slot
    c.steps(1, u)
    assert c.last_idx[2] == c.last_idx[9] == 7 and c.tr.t == 1
    c.check("repeated")
    once = Case("a", 16, prio=False, seed=8)
    u2 = u.copy()
    u2[0, 9] = 8.5 / W.N_MEM
    once.steps(1, u2)
    assert not same_bits(once.tr.pairs()[0][0], c.tr.pairs()[0][0])  # (the second occurrence is in the filter gradient)


@pytest.mark.parametrize("prio", [False, True])
def test_memory_below_min_size_changes_nothing_and_counts_the_skip(prio):
    c = Case("a", 16, prio=prio, min_size=W.N_MEM + 1, seed=9)
    c.steps(1)
    assert (c.tr.t, c.tr.skipped) == (0, 1)
    c.check("below min_size")
    for (Wn, bn), (Wo, bo) in zip(c.st.net_get_weights(), CM.pairs(c.convs, c.dense)):
        assert same_bits(Wn, Wo) and same_bits(bn, bo)


def test_infinite_reward_sets_the_warn_bit_and_changes_nothing():
    r = np.linspace(-1, 1, W.N_MEM)
    r[5] = np.inf
    c = Case("b", 6, prio=False, rewards=r, seed=10)
    c.st.reset(11)  # (the warn bits are sticky since the last reset)
    assert c.st.warnings(0) & _abi.WARN_TRAIN_NONFINITE == 0
    u = (np.arange(6)[None, :] + 20.5) / W.N_MEM
    u[0, 5] = 5.5 / W.N_MEM
    c.steps(1, u)
    assert c.last_idx[5] == 5 and c.tr.nonfinite and (c.tr.t, c.tr.skipped) == (0, 1)
    assert c.st.warnings(0) & _abi.WARN_TRAIN_NONFINITE
    c.check("inf")
    for (Wn, bn), (Wo, bo) in zip(c.st.net_get_weights()[:2], CM.pairs(c.convs, c.dense)[:2]):
        assert same_bits(Wn, Wo) and same_bits(bn, bo)  # (the conv weights stay)
    u[0, 5] = 6.5 / W.N_MEM
    c.steps(1, u)
    assert c.tr.t == 1
    c.check("after inf")


def test_set_weights_between_steps_and_train_reset():
    c = Case("c", prio=True, target_steps=5, seed=11)
    c.steps(2)
    convs, dense, _ = W.world("c", seed=77)
    c.st.net_set_weights(CM.pairs(convs, dense))
    c.tr.set_weights(convs, dense)
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
    c = Case("b", seed=12)
    c.steps(1)
    host = c.st.net_get_weights("online")
    devw = c.st.net_get_weights("online", device=True)
    assert [w.shape for w, _ in host[:2]] == [(4, 4, 3, 5), (2, 2, 5, 17)]
    for (Wh, bh), (Wd, bd) in zip(host, devw):
        assert same_bits(Wh, Wd.cpu().numpy()) and same_bits(bh, bd.cpu().numpy())
    L = c.st.L
    for which in range(4):
        for layer, (nw, nb) in enumerate(((4 * 4 * 3 * 5, 5), (2 * 2 * 5 * 17, 17))):
            Wt = torch.full((nw + 5,), -7.25, dtype=torch.float32, device="cuda")
            bt = torch.full((nb + 5,), -7.25, dtype=torch.float32, device="cuda")
            assert L.aigar_net_get_conv_weights(c.st.h, which, layer, C.c_void_p(Wt.data_ptr()), C.c_void_p(bt.data_ptr()), 1) == 0
            c.st.sync()
            assert (Wt[nw:] == -7.25).all() and (bt[nb:] == -7.25).all()
            Wh, bh = np.full(nw + 5, -7.25, F32), np.full(nb + 5, -7.25, F32)
            assert L.aigar_net_get_conv_weights(c.st.h, which, layer, Wh.ctypes.data_as(C.c_void_p),
                                                bh.ctypes.data_as(C.c_void_p), 0) == 0
            assert (Wh[nw:] == -7.25).all() and (bh[nb:] == -7.25).all()
            assert same_bits(Wh[:nw], Wt[:nw].cpu().numpy()) and same_bits(bh[:nb], bt[:nb].cpu().numpy())
            if which == 0:
                assert same_bits(Wh[:nw].reshape(host[layer][0].shape), host[layer][0])
    Wt = torch.zeros(400, dtype=torch.float32, device="cuda")
    p = C.c_void_p(Wt.data_ptr())
    assert L.aigar_net_get_conv_weights(c.st.h, 4, 0, p, p, 1) < 0 and b"outside 0..3" in L.aigar_last_error()
    assert L.aigar_net_get_conv_weights(c.st.h, 0, 2, p, p, 1) < 0 and b"layer 2 is outside 0..1" in L.aigar_last_error()
    assert L.aigar_net_get_conv_weights(c.st.h, 0, 0, None, p, 1) < 0 and b"null argument" in L.aigar_last_error()


def test_own_draws_on_two_handles_with_the_same_seed_give_equal_results():
    c1 = Case("a", 16, prio=True, seed=13)
    c2 = Case("a", 16, prio=True, seed=13, twin=1)
    for c in (c1, c2):
        c.st.train_step(3)
        assert c.st.train_info()["steps"] == 3
    for which in ("online", "target", "m", "v"):
        for (W1, b1), (W2, b2) in zip(c1.st.net_get_weights(which), c2.st.net_get_weights(which)):
            assert same_bits(W1, W2) and same_bits(b1, b2)
    assert not same_bits(c1.st.net_get_weights()[0][0], c1.convs[0][1])


def test_live_handle_refusals():
    st = handle(8, 1)
    L = st.L
    st.exp_config(None)
    st.net_config(None)
    st.exp_config(CAP, dtype="float32")
    with pytest.raises(RuntimeError, match="no acting network"):
        st.train_config_cnn(batch=4)
    st.net_config(N.NetSpec(64, (5, 4), "relu", "linear"), x_dtype="float32")
    with pytest.raises(RuntimeError, match="no conv part.*aigar_train_config"):
        st.train_config_cnn(batch=4)
    st.net_config(spec("a", out="sigmoid"), x_dtype="float32")
    with pytest.raises(RuntimeError, match="linear head"):
        st.train_config_cnn(batch=4)
    st.net_config(spec("a"), x_dtype="float32")
    st.exp_config(None)
    with pytest.raises(RuntimeError, match="no replay memory"):
        st.train_config_cnn(batch=4)
    st.exp_config(CAP, dtype="float32")
    st.net_config(N.CnnSpec(7, 1, ((3, 1, 4),), 5 * 5 * 4, (4,), "relu", "linear"), x_dtype="float32")
    with pytest.raises(RuntimeError, match="7 x 7 x 1 = 49 values, the memory's states 64"):
        st.train_config_cnn(batch=4)
    st.net_config(spec("a"), x_dtype="float32")
    assert L.aigar_train_step(st.h, 1, None) < 0 and b"no training is configured" in L.aigar_last_error()
    assert L.aigar_net_get_conv_weights(st.h, 1, 0, None, None, 0) < 0 and b"no CNN training is configured" in L.aigar_last_error()
    st.train_config_cnn(batch=4)
    with pytest.raises(RuntimeError, match="n_steps = 0"):
        st.train_step(0)
    st.net_config(spec("a"), x_dtype="float32")  # reconfiguring the network drops the train configuration
    assert L.aigar_train_step(st.h, 1, None) < 0 and b"no training is configured" in L.aigar_last_error()
    st.train_config_cnn(batch=4)
    st.exp_config(CAP, dtype="float32")  # ... and so does the memory
    assert L.aigar_train_step(st.h, 1, None) < 0 and b"no training is configured" in L.aigar_last_error()
    st.train_config_cnn(batch=4)
    st.train_config_cnn(None)
    assert L.aigar_train_step(st.h, 1, None) < 0 and b"no training is configured" in L.aigar_last_error()


def test_train_config_on_a_conv_network_is_still_refused():
    st = handle(8, 1)
    st.exp_config(CAP, dtype="float32")
    st.decide_config(np.zeros((4, 4)), q_dtype="float64")
    st.net_config(spec("a"), x_dtype="float32")
    with pytest.raises(RuntimeError, match="train_config: a network with a conv part is not trained on the device"):
        st.train_config(batch=4)
    st.decide_config(None)


def test_tiled_handle_is_refused():
    st = _lib.Stepper(make_config(n_arenas=1, bots=4, field_size=100, flags=0, tile_x=1, tile_y=1, tile_id=0,
                                  tile_flags=_abi.TILE_FORCE))
    try:
        prm = _abi.TrainParams(16, 0, 0, 0, 1e-4, 0.9, 0.999, 1e-7, 0.85)
        assert st.L.aigar_train_config_cnn(st.h, C.byref(prm)) < 0
        assert b"tiled handle" in st.L.aigar_last_error()
    finally:
        st.close()
