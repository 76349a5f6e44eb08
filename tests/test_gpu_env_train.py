"""GPU: AgarVecEnv(train=...) -- `collect(k)` then `train(n)`, interleaved, against a twin env
driven step by step through the calls that existed before: `sample(u=...)`, the Python model
(tests/train_model.py), `update_priorities`, `set_weights`.  Weights, target weights, memory
and worlds are compared by bit pattern at the end.  The worlds are 2 arenas x 5 players on a
field of 100 (three learners an arena among Greedy bots), the memory 64 prioritized
transitions, the batch 4."""
import numpy as np
import pytest

import learner_model as lm
import learner_worlds as lw
import net_model as M
import parity
import train_model as T

pytestmark = pytest.mark.gpu
from aigar_amd import _abi, _lib  # noqa: E402

HIDDEN = (20, 17)
BATCH = 4
TRAIN = dict(lr=1e-3, min_size=8, target_steps=3, discount=0.9)


def same(x, y):
    x, y = np.asarray(x), np.asarray(y)
    if x.dtype.kind != "f":
        return x.shape == y.shape and np.array_equal(x, y)
    nx, ny = np.isnan(x), np.isnan(y)
    v = np.uint64 if x.dtype.itemsize == 8 else np.uint32
    return x.shape == y.shape and np.array_equal(nx, ny) and np.array_equal(np.where(nx, 0, x).view(v),
                                                                            np.where(ny, 0, y).view(v))


def parameters(**kw):
    p = lm.params(0, 3, True, False, False, **lw.REWARD)
    return lw.env_parameters(p, NUM_ACTIONS=9, SQUARE_ACTIONS=True, EXPLORATION_STRATEGY="e-Greedy", EPSILON=0.3,
                             TEMPERATURE=0.7, Q_LAYERS=HIDDEN, **kw)


def make_env(train, prioritized=True, prm=None):
    from aigar_amd.env import AgarVecEnv
    e = AgarVecEnv(5, prm or parameters(), n_arenas=2, field_size=100, max_viruses=3, roles=lw.roles_of(5), seed=lw.SEED,
                   desync=False, reset_limit=0, discrete=True, network=True,
                   memory=dict(capacity=64, prioritized=prioritized, batch=BATCH), train=train)
    e.obs.zero_()  # (the Greedy bots' rows are never written)
    e.reset(lw.SEED)
    lw.mature(e.stepper, 2, lw.SEED)
    e.observe()
    return e


def weights_for(env, seed):
    s = env.network
    return M.make_weights(np.random.default_rng(seed), s.n_in, s.units, hi=-3)


def ring(env):
    import torch
    cap = env.memory["capacity"]
    idx = torch.arange(cap, device="cuda")
    s = torch.full((cap,) + tuple(env.obs.shape[1:]), -3.0, dtype=env.obs.dtype, device="cuda")
    s2, a = s.clone(), torch.full((cap, 4), -3.0, dtype=torch.float64, device="cuda")
    r, d = torch.full((cap,), -3.0, dtype=torch.float64, device="cuda"), torch.zeros(cap, dtype=torch.bool, device="cuda")
    env.stepper.exp_gather(idx, s=s, a=a, r=r, s2=s2, done=d)
    return [t.cpu().numpy() for t in (s, a, r, s2, d)]


def compare_end(a, b):
    import torch
    assert a.stepper.exp_info() == b.stepper.exp_info()
    for x, y in zip(ring(a), ring(b)):
        assert same(x, y)
    u = torch.linspace(0.0, 0.999, 17, dtype=torch.float64, device="cuda")
    sa, sb = a.sample(17, u), b.sample(17, u)  # (the trees: indices and weights are functions of their sums)
    assert same(sa.idx.cpu().numpy(), sb.idx.cpu().numpy()) and same(sa.w.cpu().numpy(), sb.w.cpu().numpy())
    for k in range(a.A):
        assert parity.diff_states(a.stepper.get_state(k), b.stepper.get_state(k), ftol=0.0) == []
    assert same(a.obs.cpu().numpy(), b.obs.cpu().numpy())


def twin_train(b, tr, u):
    """One training step the parent's way: sample, the model, the priorities and the weights back."""
    size = b.memory_size()
    if not tr.can_draw(size):
        tr.skipped += 1
        return
    bt = b.sample(BATCH, u)
    s, a, r, s2, d, w = (t.cpu().numpy() for t in (bt.s, bt.a, bt.r, bt.s2, bt.done, bt.w))
    prio = tr.step(s, a[:, 0], r, s2, d, w)
    assert prio is not None
    b.update_priorities(bt.idx, tr.td)
    b.set_weights(tr.theta)


@pytest.mark.parametrize("prioritized", [True, False])
def test_collect_and_train_interleaved_equal_the_parents_loop(prioritized):
    import torch
    a, b = make_env(TRAIN, prioritized), make_env(None, prioritized)
    assert a.training["batch"] == BATCH and a.network.units[:-1] == HIDDEN
    w = weights_for(a, 3)
    a.set_weights(w)
    a.stepper.train_sync_target()  # (the target was copied at configuration, from the zero weights)
    b.set_weights(w)
    tr = T.Trainer(w, BATCH, hidden="relu", beta1=0.9, beta2=0.999, epsilon=1e-7, **TRAIN)
    rng = np.random.default_rng(5)
    plan = [(1, 2), (3, 3), (2, 1), (4, 4)]  # (decisions, training steps): the first steps meet a memory below min_size
    for k, n in plan:
        a.collect(k)
        b.collect(k)
        u = rng.random((n, BATCH))
        a.train(n, u)
        for i in range(n):
            twin_train(b, tr, u[i])
    info = a.train_info()
    assert (info["steps"], info["skipped"], info["since_target"]) == (tr.t, tr.skipped, tr.since)
    assert tr.skipped >= 1 and tr.t >= 6
    for got, want in ((a.get_weights(), tr.theta), (a.get_weights(target=True), tr.target), (b.get_weights(), tr.theta)):
        for (W, bb), (Ww, bw) in zip(got, want):
            assert same(W, Ww) and same(bb, bw)
    assert not same(tr.theta[0][0], w[0][0]) and not same(tr.target[0][0], w[0][0])
    td, idx = a.train_td()
    assert same(td.cpu().numpy(), tr.td)
    # acting with the trained weights: one more run of decisions on both
    a.collect(3)
    b.collect(3)
    compare_end(a, b)
    assert same(a.net_output.cpu().numpy(), b.net_output.cpu().numpy())
    a.close()
    b.close()


def test_train_n_equals_n_times_train_one():
    a, b = make_env(TRAIN), make_env(TRAIN)
    w = weights_for(a, 4)
    for e in (a, b):
        e.set_weights(w)
        e.stepper.train_sync_target()
        e.collect(4)
    u = np.random.default_rng(6).random((5, BATCH))
    a.train(5, u)
    for i in range(5):
        b.train(1, u[i:i + 1])
    assert a.train_info() == b.train_info() and a.train_info()["steps"] == 5
    for t in (False, True):
        for (W, bb), (Ww, bw) in zip(a.get_weights(t), b.get_weights(t)):
            assert same(W, Ww) and same(bb, bw)
    # the memory's own draws: the two handles share the stream's seed and position
    a.train(3)
    for i in range(3):
        b.train(1)
    for (W, bb), (Ww, bw) in zip(a.get_weights(), b.get_weights()):
        assert same(W, Ww) and same(bb, bw)
    compare_end(a, b)
    a.close()
    b.close()


def test_an_env_without_train_decides_as_one_with_an_idle_trainer():
    """The decision graph carries nothing of the trainer: the same outputs from the same seed."""
    a, b = make_env(None), make_env(TRAIN)
    assert a.training is None
    with pytest.raises(RuntimeError, match="without train="):
        a.train()
    w = weights_for(a, 5)
    a.set_weights(w)
    b.set_weights(w)
    for _ in range(3):
        oa, ob = a.collect(2), b.collect(2)
        for x, y in zip(oa, ob):
            assert same(x.cpu().numpy(), y.cpu().numpy())
    compare_end(a, b)
    assert b.train_info() == {"steps": 0, "skipped": 0, "since_target": 0}
    a.close()
    b.close()


@pytest.mark.parametrize("kw,word", [(dict(OPTIMIZER="SGD"), "OPTIMIZER"), (dict(AMSGRAD=True), "AMSGRAD"),
                                     (dict(GRADIENT_CLIP=1.0), "GRADIENT_CLIP"), (dict(GRADIENT_CLIP_NORM=2.0), "GRADIENT_CLIP_NORM"),
                                     (dict(Q_WEIGHT_DECAY=0.001), "Q_WEIGHT_DECAY"), (dict(DROPOUT=0.1), "DROPOUT"),
                                     (dict(ENABLE_QV=True), "ENABLE_QV"), (dict(END_DISCOUNT=0.85), "END_DISCOUNT"),
                                     (dict(TD=2), "TD")])
def test_env_refuses_by_name_what_the_device_does_not_train(kw, word):
    with pytest.raises(ValueError, match=word):
        make_env(True, prm=parameters(**kw))


def test_env_train_needs_its_parts_and_reads_the_reference_defaults():
    from aigar_amd.env import AgarVecEnv
    with pytest.raises(ValueError, match="needs discrete=, network= and memory="):
        AgarVecEnv(5, parameters(), n_arenas=1, field_size=100, discrete=True, network=True, train=True)
    with pytest.raises(ValueError, match="unknown keys"):
        make_env(dict(momentum=0.9))
    e = make_env(True, prm=parameters(ALPHA=0.002, DISCOUNT=0.8, TARGET_NETWORK_STEPS=7, NUM_EXPS_BEFORE_TRAIN=9))
    assert e.training == dict(batch=BATCH, min_size=9, target_steps=7, lr=0.002, beta1=0.9, beta2=0.999, epsilon=1e-7,
                              discount=0.8)
    e.close()
