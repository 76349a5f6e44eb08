"""GPU: AgarVecEnv(pixels=..., discrete=True, network=<CnnSpec>, memory=..., train=...) -- the
pixel learner's `collect(n)` then `train(k)` against the Python model (tests/cnn_train_model.py)
fed the same transitions and draws through a twin env's `sample(u=...)`; the next `collect` acts
with the trained weights; `train(3)` against three `train(1)`; `get_weights()` with the conv pairs
first and its round trip through aigar_amd.net.cnn_weights_to_torch / cnn_weights_from_torch; the
refusal that stays.  Everything is compared by bit pattern.

The worlds are 2 arenas x 5 players on a field of 100 (three learners an arena among Greedy bots),
the pixel state 12 x 12 x 1, the network [(4, 2, 5), (2, 2, 17)] -> 68 -> (6, 25), the memory 64
prioritized transitions, the batch 4."""
import numpy as np
import pytest

import cnn_train_model as CT
import conv_model as CM
import learner_model as lm
import learner_worlds as lw
import net_model as M

pytestmark = pytest.mark.gpu
from aigar_amd import net as N  # noqa: E402

A, B, FIELD, MV = 2, 5, 100, 3
BATCH = 4
SPEC = N.CnnSpec(12, 1, ((4, 2, 5), (2, 2, 17)), 68, (6, 25), "relu", "linear")
TRAIN = dict(lr=1e-3, min_size=8, target_steps=3, discount=0.9)


def same(x, y):
    x, y = np.asarray(x), np.asarray(y)
    if x.dtype.kind != "f":
        return x.shape == y.shape and np.array_equal(x, y)
    nx, ny = np.isnan(x), np.isnan(y)
    v = np.uint64 if x.dtype.itemsize == 8 else np.uint32
    return x.shape == y.shape and np.array_equal(nx, ny) and np.array_equal(np.where(nx, 0, x).view(v),
                                                                            np.where(ny, 0, y).view(v))


def parameters():
    p = lm.params(0, 2, False, False, False, **lw.REWARD)
    return lw.env_parameters(p, NUM_ACTIONS=25, SQUARE_ACTIONS=True, EXPLORATION_STRATEGY="e-Greedy", EPSILON=0.3,
                             TEMPERATURE=0.7, NOISE_TYPE="Gaussian", GAUSSIAN_NOISE=0.2, ALGORITHM="CACLA")


def make_env(train, **kw):
    import torch
    from aigar_amd.env import AgarVecEnv
    kw.setdefault("discrete", True)
    kw.setdefault("network", SPEC)
    e = AgarVecEnv(B, parameters(), n_arenas=A, field_size=FIELD, max_viruses=MV, roles=lw.roles_of(B), seed=lw.SEED,
                   desync=False, reset_limit=0, pixels=(12, False, False), pixel_dtype=torch.float32,
                   memory=dict(capacity=64, prioritized=True, batch=BATCH), train=train, **kw)
    e.obs.zero_()  # (the Greedy bots' rows are never written)
    e.reset(lw.SEED)
    lw.mature(e.stepper, A, lw.SEED)
    e.observe()
    return e


def weights_for(seed):
    """Pixel values are (gray - 255) / 100, in [-2.55, 0]: kernels below 2^-3 are far from overflow."""
    rng = np.random.default_rng(seed)
    return CM.make_convs(rng, SPEC.channels, SPEC.convs, hi=-3), M.make_weights(rng, SPEC.n_flat, SPEC.units, hi=-3)


def twin_train(b, tr, u):
    """One training step on the model from the twin's memory: sample, the model, the priorities back."""
    if not tr.can_draw(b.memory_size()):
        tr.skipped += 1
        return
    bt = b.sample(BATCH, u)
    s, a, r, s2, d, w = (t.cpu().numpy() for t in (bt.s, bt.a, bt.r, bt.s2, bt.done, bt.w))
    shape = (BATCH, SPEC.side, SPEC.side, SPEC.channels)
    assert tr.step(s.reshape(shape), a[:, 0], r, s2.reshape(shape), d, w) is not None
    b.update_priorities(bt.idx, tr.td)
    b.set_weights(tr.pairs())


def test_collect_then_train_is_the_model_and_the_next_collect_acts_with_the_trained_weights():
    a, b = make_env(TRAIN), make_env(None)
    assert a.training["batch"] == BATCH and a.network == SPEC
    cv, dense = weights_for(3)
    for e in (a, b):
        e.set_weights(CM.pairs(cv, dense))
    a.sync_target()  # (the target was copied at configuration, from the zero weights)
    tr = CT.CnnTrainer(cv, dense, BATCH, beta1=0.9, beta2=0.999, epsilon=1e-7, **TRAIN)
    rng = np.random.default_rng(5)
    for k, n in [(1, 2), (3, 3), (2, 1), (4, 4)]:  # (decisions, training steps): the first steps meet a memory below min_size
        a.collect(k)
        b.collect(k)
        u = rng.random((n, BATCH))
        a.train(n, u)
        for i in range(n):
            twin_train(b, tr, u[i])
    info = a.train_info()
    assert (info["steps"], info["skipped"], info["since_target"]) == (tr.t, tr.skipped, tr.since)
    assert tr.skipped >= 1 and tr.t >= 6
    got, tgt = a.get_weights(), a.get_weights(target=True)
    assert [w.shape for w, _ in got] == [(4, 4, 1, 5), (2, 2, 5, 17), (68, 6), (6, 25)]  # conv pairs first
    for have, want in ((got, tr.pairs()), (tgt, tr.pairs("target")), (b.get_weights(), tr.pairs())):
        for (Wg, bg), (Ww, bw) in zip(have, want):
            assert same(Wg, Ww) and same(bg, bw)
    for (Wn, _), (Wo, _), (Wt, _) in zip(tr.pairs(), CM.pairs(cv, dense), tr.pairs("target")):
        assert not same(Wn, Wo) and not same(Wt, Wo)
    td, idx = a.train_td()
    assert same(td.cpu().numpy(), tr.td)
    assert a.stepper.net_pad_check("online") == 0 and a.stepper.net_pad_check("target") == 0
    # the round trip of the read-back through torch's layouts
    sd = N.cnn_weights_to_torch(got, SPEC)
    assert list(sd) == ["conv0.weight", "conv0.bias", "conv1.weight", "conv1.bias", "fc0.weight", "fc0.bias", "fc1.weight",
                        "fc1.bias"]
    assert tuple(sd["conv1.weight"].shape) == (17, 5, 2, 2) and tuple(sd["fc0.weight"].shape) == (6, 68)
    for (Wg, bg), (Wr, br) in zip(got, N.cnn_weights_from_torch(sd, SPEC)):
        assert same(Wg, Wr) and same(bg, br)
    # acting with the trained weights: the next decision's rows are the model's with the model's theta
    nn = np.array([r == "NN" for r in lw.roles_of(B)] * A)
    obs0 = a.obs.cpu().numpy()
    deciding = ~np.isnan(obs0[:, 0, 0, 0]) & nn
    assert deciding.any()
    a.collect(1)
    b.collect(1)
    want = CM.forward(obs0[deciding], tr.theta[0], tr.theta[1], "relu", "linear")
    out = a.net_output.cpu().numpy()
    assert np.array_equal(M.bits(out[deciding]), M.bits(want))
    assert not np.array_equal(M.bits(want), M.bits(CM.forward(obs0[deciding], cv, dense, "relu", "linear")))
    assert same(out, b.net_output.cpu().numpy()) and same(a.obs.cpu().numpy(), b.obs.cpu().numpy())
    a.close()
    b.close()


def test_train_three_equals_three_times_train_one():
    a, b = make_env(TRAIN), make_env(TRAIN)
    cv, dense = weights_for(4)
    for e in (a, b):
        e.set_weights(CM.pairs(cv, dense))
        e.sync_target()
        e.collect(4)
    u = np.random.default_rng(6).random((3, BATCH))
    a.train(3, u)
    for i in range(3):
        b.train(1, u[i:i + 1])
    assert a.train_info() == b.train_info() and a.train_info()["steps"] == 3
    for t in (False, True):
        for (Wa, ba), (Wb, bb) in zip(a.get_weights(t), b.get_weights(t)):
            assert same(Wa, Wb) and same(ba, bb)
    assert not same(a.get_weights()[0][0], cv[0][1])
    a.train(3)  # the memory's own draws: the two handles share the stream's seed and position
    for i in range(3):
        b.train(1)
    for (Wa, ba), (Wb, bb) in zip(a.get_weights(), b.get_weights()):
        assert same(Wa, Wb) and same(ba, bb)
    a.close()
    b.close()


def test_continuous_with_a_pixel_state_is_still_refused():
    with pytest.raises(ValueError, match="train=: CNN / pixel states are not trained on the device"):
        make_env(True, discrete=None, continuous=True, network=SPEC._replace(units=(6, 2), out="sigmoid"))
