"""GPU: AgarVecEnv(continuous=True, network=True, memory=..., train="dpg") -- `collect(k)` then
`train(n)`, interleaved, against a twin env driven step by step through the calls that existed
before: `sample(u=...)`, the Python model (tests/dpg_model.py), `update_priorities`,
`set_weights`.  The noisy actions, the stored transitions, the next states, both networks'
weights, both targets and the worlds are compared by bit pattern.  The worlds are 2 arenas x 5
players on a field of 100 (three learners an arena among Greedy bots), the memory 64
prioritized transitions, the batch 4."""
import numpy as np
import pytest

import dpg_model as DM
import learner_model as lm
import learner_worlds as lw
import net_model as M
from test_gpu_env_actrain import compare_end, same

pytestmark = pytest.mark.gpu
from aigar_amd import _abi, _lib  # noqa: E402,F401

HIDDEN = (20, 17)
CRITIC = (19, 9)
BATCH = 4
TRAIN = dict(critic_lr=1e-3, actor_lr=2e-3, min_size=8, target_steps=3, discount=0.9, tau=0.125, q_increase=0.5)


def parameters(**kw):
    p = lm.params(0, 3, True, False, False, **lw.REWARD)
    d = dict(NOISE_TYPE="Gaussian", GAUSSIAN_NOISE=0.2, ALGORITHM="DPG", DPG_ACTOR_LAYERS=HIDDEN, DPG_CRITIC_LAYERS=CRITIC)
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


def dpg(**kw):
    return dict(TRAIN, algorithm="dpg", **kw)


def weights_for(env, seed):
    rng = np.random.default_rng(seed)
    s, c = env.network, env.critic
    return M.make_weights(rng, s.n_in, s.units, hi=-3), M.make_weights(rng, c.n_in, c.units, hi=-3)


def twin_train(b, tr, u):
    """One training step the parent's way: sample, the model, the priorities and the actor's weights back."""
    if not tr.can_draw(b.memory_size()):
        tr.skipped += 1
        return
    bt = b.sample(BATCH, u)
    s, a, r, s2, d, w = (t.cpu().numpy() for t in (bt.s, bt.a, bt.r, bt.s2, bt.done, bt.w))
    assert tr.step(s, a, r, s2, d, w) is not None
    b.update_priorities(bt.idx, tr.td)
    b.set_weights(tr.a.theta)


def model_for(env, wa, wc, **kw):
    return DM.Trainer(wa, wc, BATCH, hidden_actor=env.network.hidden, hidden_critic=env.critic.hidden, beta1=0.9, beta2=0.999,
                      epsilon=1e-7, **dict(TRAIN, **kw))


@pytest.mark.parametrize("prioritized,tau", [(True, 0.125), (False, 0.125), (True, 0.0)])
def test_collect_and_train_interleaved_equal_the_parents_loop(prioritized, tau):
    a, b = make_env(dpg(tau=tau), prioritized), make_env(None, prioritized)
    assert a.training["batch"] == BATCH and a.network.units[:-1] == HIDDEN and a.critic.units == CRITIC + (1,)
    assert a.dpg and not a.cacla and a.network.out == "sigmoid" and a.critic.n_in == a.network.n_in + a.network.units[-1]
    wa, wc = weights_for(a, 3)
    a.set_weights(wa)
    a.set_critic_weights(wc)
    a.stepper.dpg_sync_target()  # (the targets were copied at configuration, from the zero weights)
    b.set_weights(wa)
    tr = model_for(a, wa, wc, tau=tau)
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
    assert tuple(info[k] for k in ("steps", "skipped", "since_target", "actor_steps", "actor_skipped")) == tr.info()[:5]
    assert tr.skipped >= 1 and tr.c.t >= 6 and tr.a.t == tr.c.t
    for got, want in ((a.get_weights(), tr.a.theta), (b.get_weights(), tr.a.theta), (a.get_weights(target=True), tr.target_a),
                      (a.get_critic_weights(), tr.c.theta), (a.get_critic_weights(target=True), tr.target_c)):
        for (W, bb), (Ww, bw) in zip(got, want):
            assert same(W, Ww) and same(bb, bw)
    assert not same(tr.a.theta[0][0], wa[0][0]) and not same(tr.c.theta[0][0], wc[0][0])
    assert not same(tr.target_a[0][0], wa[0][0]) and not same(tr.target_c[0][0], wc[0][0])
    td, idx = a.train_td()
    assert same(td.cpu().numpy(), tr.td)
    s3 = a.obs[a.nn][:3]
    act = np.random.default_rng(8).random((3, a.network.units[-1]))
    q = a.q_value(s3, act)
    assert same(q.cpu().numpy(), M.forward(DM.sa_rows(s3.cpu().numpy(), act), tr.c.theta, a.critic.hidden, "linear")[:, 0])
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
    a, b = make_env(dpg()), make_env(dpg())
    wa, wc = weights_for(a, 4)
    for e in (a, b):
        e.set_weights(wa)
        e.set_critic_weights(wc)
        e.stepper.dpg_sync_target()
        e.collect(6)
    u = np.random.default_rng(6).random((3, BATCH))
    a.train(3, u)
    for i in range(3):
        b.train(1, u[i:i + 1])
    assert a.train_info() == b.train_info() and a.train_info()["steps"] == 3 and a.train_info()["actor_steps"] == 3
    sets = lambda e: (e.get_weights(), e.get_weights(True), e.get_critic_weights(), e.get_critic_weights(True))
    for ga, gb in zip(sets(a), sets(b)):
        for (W, bb), (Ww, bw) in zip(ga, gb):
            assert same(W, Ww) and same(bb, bw)
    # the memory's own draws: the two handles share the stream's seed and position
    a.train(3)
    for i in range(3):
        b.train(1)
    for ga, gb in zip(sets(a), sets(b)):
        for (W, bb), (Ww, bw) in zip(ga, gb):
            assert same(W, Ww) and same(bb, bw)
    compare_end(a, b)
    a.close()
    b.close()


@pytest.mark.parametrize("kw,word", [(dict(ALGORITHM="CACLA"), "ALGORITHM"), (dict(DPG_FEED_ACTION_IN_LAYER=2), "DPG_FEED_ACTION_IN_LAYER"),
                                     (dict(DPG_USE_TARGET_MODELS=False), "DPG_USE_TARGET_MODELS"),
                                     (dict(DPG_USE_DPG_ACTOR_TRAINING=False), "DPG_USE_DPG_ACTOR_TRAINING"),
                                     (dict(DPG_USE_CACLA=True), "DPG_USE_CACLA"),
                                     (dict(DPG_CACLA_ALTERNATION=0.5), "DPG_CACLA_ALTERNATION"),
                                     (dict(DPG_CACLA_INV_ALTERNATION=0.5), "DPG_CACLA_INV_ALTERNATION"),
                                     (dict(DPG_CRITIC_WEIGHT_DECAY=0.001), "DPG_CRITIC_WEIGHT_DECAY"),
                                     (dict(DPG_ACTOR_OPTIMIZER="SGD"), "DPG_ACTOR_OPTIMIZER"),
                                     (dict(DPG_ACTOR_NESTEROV=0.9), "DPG_ACTOR_NESTEROV"), (dict(ACTOR_IS=True), "ACTOR_IS"),
                                     (dict(OCACLA_ENABLED=True), "OCACLA_ENABLED"), (dict(AMSGRAD=True), "AMSGRAD"),
                                     (dict(DPG_CRITIC_FUNC="elu"), "DPG_CRITIC_FUNC")])
def test_env_refuses_by_name_what_the_device_does_not_train(kw, word):
    with pytest.raises(ValueError, match=word):
        make_env("dpg", prm=parameters(**kw))


def test_env_train_needs_its_parts_and_reads_the_reference_defaults():
    from aigar_amd.env import AgarVecEnv
    with pytest.raises(ValueError, match="ALGORITHM"):  # train=True stays the CACLA trainer
        make_env(True)
    with pytest.raises(ValueError, match="train='dpg' needs continuous=, network= and memory="):
        AgarVecEnv(5, parameters(), n_arenas=1, field_size=100, continuous=True, network=True, train="dpg")
    with pytest.raises(ValueError, match="train='dpg' needs continuous=, network= and memory="):
        AgarVecEnv(5, parameters(), n_arenas=1, field_size=100, network=None, train=dict(algorithm="dpg"))
    with pytest.raises(ValueError, match="True, a dict or 'dpg'"):
        make_env("spg")
    with pytest.raises(ValueError, match="algorithm = 'spg'"):
        make_env(dict(algorithm="spg"))
    with pytest.raises(ValueError, match="unknown keys"):
        make_env(dpg(var_epochs=3))
    e = make_env("dpg", prm=parameters(DPG_CRITIC_ALPHA=0.002, DPG_ACTOR_ALPHA=0.003, DISCOUNT=0.8, TARGET_NETWORK_STEPS=7,
                                       NUM_EXPS_BEFORE_TRAIN=9, DPG_TAU=0.01, DPG_Q_VAL_INCREASE=3))
    assert e.training == dict(batch=BATCH, min_size=9, target_steps=7, critic_lr=0.002, actor_lr=0.003, beta1=0.9,
                              beta2=0.999, epsilon=1e-7, discount=0.8, tau=0.01, q_increase=3.0)
    n_act = e.network.units[-1]
    assert e.critic == (e.network.n_in + n_act, CRITIC + (1,), "relu", "linear")
    assert e.train_info() == dict(steps=0, skipped=0, since_target=0, actor_steps=0, actor_skipped=0)
    assert len(e.get_weights(target=True)) == len(HIDDEN) + 1
    with pytest.raises(RuntimeError, match="CACLA trainer"):
        e.cacla_var()
    with pytest.raises(ValueError, match="q_value: states"):
        e.q_value(e.obs[:2], np.zeros((2, n_act + 1)))
    e.close()
    e = make_env(dpg(), prm=parameters(SOFT_TARGET_UPDATES=False), critic=(None, (7, 1), "linear", "linear"))
    assert e.training["tau"] == TRAIN["tau"] and e.critic == (e.network.n_in + n_act, (7, 1), "linear", "linear")
    e.close()
    e = make_env("dpg", prm=parameters(SOFT_TARGET_UPDATES=False))
    assert e.training["tau"] == 0.0 and e.training["target_steps"] == 1500
    e.close()
