"""GPU: AgarVecEnv(continuous=True, network=True, memory=..., train=...) -- `collect(k)` then
`train(n)`, interleaved, against a twin env driven step by step through the calls that existed
before: `sample(u=...)`, the Python model (tests/cacla_model.py), `update_priorities`,
`set_weights`.  The noisy actions, the stored transitions, the next states, both networks'
weights and the worlds are compared by bit pattern.  The worlds are 2 arenas x 5 players on a
field of 100 (three learners an arena among Greedy bots), the memory 64 prioritized
transitions, the batch 4."""
import numpy as np
import pytest

import cacla_model as CM
import learner_model as lm
import learner_worlds as lw
import net_model as M
import parity

pytestmark = pytest.mark.gpu
from aigar_amd import _abi, _lib  # noqa: E402

HIDDEN = (20, 17)
CRITIC = (19, 9)
BATCH = 4
TRAIN = dict(critic_lr=1e-3, actor_lr=2e-3, min_size=8, target_steps=3, discount=0.9, var_epochs=3, var_start=0.01,
             var_beta=0.05)


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
    d = dict(NOISE_TYPE="Gaussian", GAUSSIAN_NOISE=0.2, ALGORITHM="CACLA", CACLA_ACTOR_LAYERS=HIDDEN,
             CACLA_CRITIC_LAYERS=CRITIC)
    d.update(kw)
    return lw.env_parameters(p, **d)


def make_env(train, prioritized=True, prm=None, **kw):
    from aigar_amd.env import AgarVecEnv
    e = AgarVecEnv(5, prm or parameters(), n_arenas=2, field_size=100, max_viruses=3, roles=lw.roles_of(5), seed=lw.SEED,
                   desync=False, reset_limit=0, continuous=True, network=True,
                   memory=dict(capacity=64, prioritized=prioritized, batch=BATCH), train=train, **kw)
    e.obs.zero_()  # (the Greedy bots' rows are never written)
    e.reset(lw.SEED)
    lw.mature(e.stepper, 2, lw.SEED)
    e.observe()
    return e


def weights_for(env, seed):
    rng = np.random.default_rng(seed)
    s, c = env.network, env.critic
    return M.make_weights(rng, s.n_in, s.units, hi=-3), M.make_weights(rng, c.n_in, c.units, hi=-3)


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
    """One training step the parent's way: sample, the model, the priorities and the actor's weights back."""
    if not tr.can_draw(b.memory_size()):
        tr.skip()
        return
    bt = b.sample(BATCH, u)
    s, a, r, s2, d, w = (t.cpu().numpy() for t in (bt.s, bt.a, bt.r, bt.s2, bt.done, bt.w))
    assert tr.step(s, a, r, s2, d, w) is not None
    b.update_priorities(bt.idx, tr.td)
    b.set_weights(tr.a.theta)


def model_for(env, wa, wc):
    return CM.Trainer(wa, wc, BATCH, hidden_actor=env.network.hidden, hidden_critic=env.critic.hidden, beta1=0.9, beta2=0.999,
                      epsilon=1e-7, **TRAIN)


@pytest.mark.parametrize("prioritized", [True, False])
def test_collect_and_train_interleaved_equal_the_parents_loop(prioritized):
    a, b = make_env(TRAIN, prioritized), make_env(None, prioritized)
    assert a.training["batch"] == BATCH and a.network.units[:-1] == HIDDEN and a.critic.units == CRITIC + (1,)
    assert a.cacla and a.network.out == "sigmoid"
    wa, wc = weights_for(a, 3)
    a.set_weights(wa)
    a.set_critic_weights(wc)
    a.stepper.actrain_sync_target()  # (the target was copied at configuration, from the zero weights)
    b.set_weights(wa)
    tr = model_for(a, wa, wc)
    rng = np.random.default_rng(5)
    plan = [(1, 2), (3, 3), (2, 1), (4, 4)]  # (decisions, training steps): the first steps meet a memory below min_size
    for k, n in plan:
        ra, rb = a.collect(k), b.collect(k)
        for x, y in zip(ra, rb):
            assert same(x.cpu().numpy(), y.cpu().numpy())
        assert same(a.noisy_action.cpu().numpy(), b.noisy_action.cpu().numpy())
        u = rng.random((n, BATCH))
        a.train(n, u)
        for i in range(n):
            twin_train(b, tr, u[i])
    info = a.train_info()
    assert tuple(info[k] for k in ("steps", "skipped", "since_target", "actor_epochs", "selected", "epochs", "cut",
                                   "epochs_skipped")) == tr.info()
    assert tr.skipped >= 1 and tr.c.t >= 6 and tr.a.t >= 1
    for got, want in ((a.get_weights(), tr.a.theta), (b.get_weights(), tr.a.theta), (a.get_critic_weights(), tr.c.theta),
                      (a.get_critic_weights(target=True), tr.target)):
        for (W, bb), (Ww, bw) in zip(got, want):
            assert same(W, Ww) and same(bb, bw)
    assert not same(tr.a.theta[0][0], wa[0][0]) and not same(tr.c.theta[0][0], wc[0][0]) and not same(tr.target[0][0], wc[0][0])
    td, idx = a.train_td()
    assert same(td.cpu().numpy(), tr.td)
    assert same(np.float64(a.cacla_var()), np.float64(tr.var)) and tr.var != TRAIN["var_start"]
    v = a.critic_value(a.obs[a.nn][:3])
    assert same(v.cpu().numpy(), M.forward(a.obs[a.nn][:3].cpu().numpy(), tr.c.theta, a.critic.hidden, "linear")[:, 0])
    # acting with the trained actor: one more run of decisions on both
    ra, rb = a.collect(3), b.collect(3)
    for x, y in zip(ra, rb):
        assert same(x.cpu().numpy(), y.cpu().numpy())
    assert same(a.noisy_action.cpu().numpy(), b.noisy_action.cpu().numpy())
    compare_end(a, b)
    assert same(a.net_output.cpu().numpy(), b.net_output.cpu().numpy())
    a.close()
    b.close()


def test_train_three_equals_three_times_train_one():
    a, b = make_env(TRAIN), make_env(TRAIN)
    wa, wc = weights_for(a, 4)
    for e in (a, b):
        e.set_weights(wa)
        e.set_critic_weights(wc)
        e.stepper.actrain_sync_target()
        e.collect(4)
    u = np.random.default_rng(6).random((3, BATCH))
    a.train(3, u)
    for i in range(3):
        b.train(1, u[i:i + 1])
    assert a.train_info() == b.train_info() and a.train_info()["steps"] == 3
    for ga, gb in ((a.get_weights(), b.get_weights()), (a.get_critic_weights(), b.get_critic_weights()),
                   (a.get_critic_weights(True), b.get_critic_weights(True))):
        for (W, bb), (Ww, bw) in zip(ga, gb):
            assert same(W, Ww) and same(bb, bw)
    # the memory's own draws: the two handles share the stream's seed and position
    a.train(3)
    for i in range(3):
        b.train(1)
    for (W, bb), (Ww, bw) in zip(a.get_weights(), b.get_weights()):
        assert same(W, Ww) and same(bb, bw)
    assert a.cacla_var() == b.cacla_var()
    compare_end(a, b)
    a.close()
    b.close()


@pytest.mark.parametrize("kw,word", [(dict(ALGORITHM="DPG"), "ALGORITHM"), (dict(OCACLA_ENABLED=True), "OCACLA_ENABLED"),
                                     (dict(CACLA_UPDATE_ON_NEGATIVE_TD=True), "CACLA_UPDATE_ON_NEGATIVE_TD"),
                                     (dict(CACLA_CRITIC_WEIGHT_DECAY=0.001), "CACLA_CRITIC_WEIGHT_DECAY"),
                                     (dict(CACLA_OFF_POLICY_CORR=1), "CACLA_OFF_POLICY_CORR"), (dict(ACTOR_IS=True), "ACTOR_IS"),
                                     (dict(AC_ACTOR_TDE=0.5), "AC_ACTOR_TDE"),
                                     (dict(AC_DELAY_ACTOR_TRAINING=0.2), "AC_DELAY_ACTOR_TRAINING"), (dict(AMSGRAD=True), "AMSGRAD"),
                                     (dict(OPTIMIZER_POLICY="SGD"), "OPTIMIZER_POLICY"), (dict(END_DISCOUNT=0.85), "END_DISCOUNT"),
                                     (dict(DROPOUT=0.1), "DROPOUT"), (dict(GRADIENT_CLIP=1.0), "GRADIENT_CLIP"),
                                     (dict(GRADIENT_CLIP_NORM=2.0), "GRADIENT_CLIP_NORM")])
def test_env_refuses_by_name_what_the_device_does_not_train(kw, word):
    with pytest.raises(ValueError, match=word):
        make_env(True, prm=parameters(**kw))


def test_env_train_needs_its_parts_and_reads_the_reference_defaults():
    from aigar_amd.env import AgarVecEnv
    with pytest.raises(ValueError, match="needs discrete=, network= and memory="):  # (the Q trainer's, unchanged)
        AgarVecEnv(5, parameters(), n_arenas=1, field_size=100, network=None, train=True)
    with pytest.raises(ValueError, match="with continuous= needs network= and memory="):
        AgarVecEnv(5, parameters(), n_arenas=1, field_size=100, continuous=True, network=True, train=True)
    with pytest.raises(ValueError, match="critic= needs continuous= and train="):
        AgarVecEnv(5, parameters(), n_arenas=1, field_size=100, continuous=True, network=True, critic=(None, (4, 1), "relu", "linear"))
    with pytest.raises(ValueError, match="unknown keys"):
        make_env(dict(momentum=0.9))
    e = make_env(True, prm=parameters(CACLA_CRITIC_ALPHA=0.002, CACLA_ACTOR_ALPHA=0.003, DISCOUNT=0.8, TARGET_NETWORK_STEPS=7,
                                      NUM_EXPS_BEFORE_TRAIN=9, CACLA_VAR_START=2, CACLA_VAR_BETA=0.01))
    assert e.training == dict(batch=BATCH, min_size=9, target_steps=7, var_epochs=8, critic_lr=0.002, actor_lr=0.003,
                              beta1=0.9, beta2=0.999, epsilon=1e-7, discount=0.8, var_start=2.0, var_beta=0.01)
    assert e.critic.units == CRITIC + (1,) and e.cacla_var() == 2.0
    assert e.train_info() == dict(steps=0, skipped=0, since_target=0, actor_epochs=0, selected=0, epochs=0, cut=0,
                                  epochs_skipped=0)
    with pytest.raises(RuntimeError, match="CACLA keeps no actor target"):
        e.get_weights(target=True)
    e.close()
    e = make_env(dict(var_epochs=0), prm=parameters(CACLA_VAR_ENABLED=False), critic=(None, (7, 1), "linear", "linear"))
    assert e.training["var_epochs"] == 0 and e.critic == (e.network.n_in, (7, 1), "linear", "linear")
    e.close()
