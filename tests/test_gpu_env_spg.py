"""GPU: AgarSpgEnv(continuous=True, network=True, memory=..., train="dpg", search=...) --
`collect(k)` then `train(n)`, interleaved, against a twin env driven step by step through the
calls that existed before: `sample(u=...)`, `sample_extra`, the Python model (tests/spg_model.py),
`update_priorities`, `update_actions`, `set_weights`.  The noisy actions, the stored transitions,
the memory's fifth field, both networks' weights, both targets and the worlds are compared by bit
pattern.  The worlds are tests/test_gpu_env_dpg.py's: 2 arenas x 5 players on a field of 100,
the memory 64 transitions, the batch 4."""
import numpy as np
import pytest

import dpg_model as DM
import learner_model as lm
import learner_worlds as lw
import net_model as M
import spg_model as SM
from test_gpu_env_actrain import compare_end, same

pytestmark = pytest.mark.gpu

HIDDEN = (20, 17)
CRITIC = (19, 9)
BATCH = 4
TRAIN = dict(critic_lr=1e-3, actor_lr=2e-3, min_size=8, target_steps=3, discount=0.9, tau=0.125)
SEARCH = dict(samples=2, moving=True, replace=True, prio_evals=True, noise=0.25, noise_decay=0.5)
K = SEARCH["samples"]


def parameters(**kw):
    p = lm.params(0, 3, True, False, False, **lw.REWARD)
    d = dict(NOISE_TYPE="Gaussian", GAUSSIAN_NOISE=0.2, ALGORITHM="SPG", CACLA_ACTOR_LAYERS=HIDDEN, DPG_CRITIC_LAYERS=CRITIC)
    d.update(kw)
    return lw.env_parameters(p, **d)


W25, W112 = (2, 5, 100), (1, 12, 90)  # (arenas, players an arena, field): learner_worlds' 2 x 5 and 1 x 12 styles


def make_env(train, search=None, prioritized=True, prm=None, world=W25, **kw):
    from aigar_amd.env import AgarSpgEnv
    A, B, field = world
    e = AgarSpgEnv(B, prm or parameters(), n_arenas=A, field_size=field, max_viruses=3, roles=lw.roles_of(B), seed=lw.SEED,
                   desync=False, reset_limit=0, continuous=True, network=True,
                   memory=dict(capacity=64, prioritized=prioritized, batch=BATCH), train=train, search=search, **kw)
    e.obs.zero_()  # (the Greedy bots' rows are never written)
    e.reset(lw.SEED)
    lw.mature(e.stepper, A, lw.SEED)
    e.observe()
    return e


def dpg(**kw):
    return dict(TRAIN, algorithm="dpg", **kw)


def weights_for(env, seed):
    rng = np.random.default_rng(seed)
    s, c = env.network, env.critic
    wa, wc = M.make_weights(rng, s.n_in, s.units, hi=-3), M.make_weights(rng, c.n_in, c.units, hi=-3)
    # the critic's action rows and head of ordinary size: Q depends on the action by more than its float32 spacing
    wc[0][0][s.n_in:] = rng.uniform(-0.5, 0.5, wc[0][0][s.n_in:].shape).astype(np.float32)
    wc[-1][0][:] = rng.uniform(-0.5, 0.5, wc[-1][0].shape).astype(np.float32)
    wc[1][0][:] = rng.uniform(-0.5, 0.5, wc[1][0].shape).astype(np.float32)
    return wa, wc


def twin_train(b, tr, u, zu):
    """One training step the parent's way: sample, the fifth field, the model, the priorities, the
    best actions and the actor's weights back."""
    if not tr.can_draw(b.memory_size()):
        tr.skip()
        return
    bt = b.sample(BATCH, u)
    extra, valid = b.sample_extra(bt.idx)
    s, a, r, s2, d, w = (t.cpu().numpy() for t in (bt.s, bt.a, bt.r, bt.s2, bt.done, bt.w))
    prio, rows = tr.step(s, a, r, s2, d, w, extra.cpu().numpy(), valid.cpu().numpy(), zu)
    assert prio is not None
    b.update_priorities(bt.idx, tr.q_old if tr.prio_evals else tr.td)
    if rows is not None:
        b.update_actions(bt.idx, rows)
    b.set_weights(tr.a.theta)


def model_for(env, wa, wc, **kw):
    return SM.Trainer(wa, wc, BATCH, hidden_actor=env.network.hidden, hidden_critic=env.critic.hidden, beta1=0.9, beta2=0.999,
                      epsilon=1e-7, **dict(dict(TRAIN, **SEARCH), **kw))


def extras_of(e):
    n = e.memory_size()
    x, v = e.sample_extra(np.arange(n))
    return x.cpu().numpy(), v.cpu().numpy()


@pytest.mark.parametrize("prioritized,tau,evals,fused,world", [(True, 0.125, True, 0, W25), (False, 0.125, True, 1, W25),
                                                              (True, 0.0, False, 1, W25), (True, 0.125, True, 1, W112),
                                                              (False, 0.0, False, 0, W112)])
def test_collect_and_train_interleaved_equal_the_parents_loop(prioritized, tau, evals, fused, world):
    a = make_env(dpg(tau=tau), dict(SEARCH, prio_evals=evals, fused=bool(fused)), prioritized, world=world)
    b = make_env(None, None, prioritized, world=world)
    assert a.training["batch"] == BATCH and a.network.units[:-1] == HIDDEN and a.critic.units == CRITIC + (1,)
    assert a.spg and not a.dpg and not a.cacla and not b.spg and a.training["samples"] == K and a.training["seed"] == lw.SEED
    assert a.continuous["store_raw"] is False and b.continuous["store_raw"] is False
    wa, wc = weights_for(a, 3)
    a.set_weights(wa)
    a.set_critic_weights(wc)
    a.stepper.spg_sync_target()  # (the targets were copied at configuration, from the zero weights)
    b.set_weights(wa)
    tr = model_for(a, wa, wc, tau=tau, prio_evals=int(evals))
    rng = np.random.default_rng(5)
    plan = [(1, 2), (3, 3), (2, 1), (4, 4), (2, 4), (1, 4), (1, 4)]  # (decisions, training steps): the first steps meet a memory below min_size
    own_reads = 0
    for k, n in plan:
        ra, rb = a.collect(k), b.collect(k)
        for x, y in zip(ra, rb):
            assert same(x.cpu().numpy(), y.cpu().numpy())
        assert same(a.noisy_action.cpu().numpy(), b.noisy_action.cpu().numpy())
        u, zu = rng.random((n, BATCH)), rng.random((n, BATCH, K, 2, 16, 2))
        a.train(n, u, zu)
        for i in range(n):
            before = tr.extras_read
            twin_train(b, tr, u[i], zu[i])
            own_reads += tr.extras_read - before  # (the collector leaves every extra empty: a valid one was written by a step)
        (xa, va), (xb, vb) = extras_of(a), extras_of(b)
        assert same(va, vb) and same(xa[va], xb[vb])
    info = a.train_info()
    assert tuple(info[k] for k in ("steps", "skipped", "since_target", "actor_steps", "actor_skipped", "actor_empty",
                                   "selected")) == tr.info()[:7]
    assert tr.skipped >= 1 and tr.c.t >= 8 and tr.a.t >= 1
    # the run is worth comparing: rows selected and left, every kind of source, an extra of a former step read
    assert tr.seen[0] > 0 and tr.seen[1] > 0 and own_reads > 0
    assert {min(v, SM.SRC_SAMPLE) for v in tr.sources} == {SM.SRC_STORED, SM.SRC_EXTRA, SM.SRC_MU, SM.SRC_SAMPLE}
    for got, want in ((a.get_weights(), tr.a.theta), (b.get_weights(), tr.a.theta), (a.get_weights(target=True), tr.target_a),
                      (a.get_critic_weights(), tr.c.theta), (a.get_critic_weights(target=True), tr.target_c),
                      (a.stepper.net_get_weights("m"), tr.a.m), (a.stepper.critic_get_weights("m"), tr.c.m)):
        for (W, bb), (Ww, bw) in zip(got, want):
            assert same(W, Ww) and same(bb, bw)
    assert not same(tr.a.theta[0][0], wa[0][0]) and not same(tr.c.theta[0][0], wc[0][0])
    assert same(a.search_noise.cpu().numpy(), np.array([tr.noise])) and tr.noise == 0.25 * 0.5 ** tr.c.t
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


def test_search_noise_written_by_the_caller_takes_effect_and_train_three_equals_three_times_one():
    a, b = make_env(dpg(), dict(SEARCH, fused=True)), make_env(dpg(), dict(SEARCH, fused=False))  # (fused against the composition)
    wa, wc = weights_for(a, 4)
    for e in (a, b):
        e.set_weights(wa)
        e.set_critic_weights(wc)
        e.stepper.spg_sync_target()
        e.collect(6)
    tr = model_for(a, wa, wc)
    rng = np.random.default_rng(6)
    u, zu = rng.random((3, BATCH)), rng.random((3, BATCH, K, 2, 16, 2))
    for e in (a, b):
        e.search_noise.fill_(0.75)
    a.train(3, u, zu)
    for i in range(3):
        b.train(1, u[i:i + 1], zu[i:i + 1])
    assert a.train_info() == b.train_info() and a.train_info()["steps"] == 3
    assert a.search_noise.item() == b.search_noise.item() == 0.75 * 0.5 ** 3
    sets = lambda e: (e.get_weights(), e.get_weights(True), e.get_critic_weights(), e.get_critic_weights(True))
    for ga, gb in zip(sets(a), sets(b)):
        for (W, bb), (Ww, bw) in zip(ga, gb):
            assert same(W, Ww) and same(bb, bw)
    # the model from the written noise: the twin is a fresh env fed through the old calls
    c = make_env(None)
    c.set_weights(wa)
    c.collect(6)
    tr.noise = 0.75
    for i in range(3):
        twin_train(c, tr, u[i], zu[i])
    # (Adam's first steps move a weight by about lr whatever the gradient's size: its m and the
    # written-back actions tell the two noise levels apart, the weights need not)
    for got, want in ((a.get_weights(), tr.a.theta), (a.stepper.net_get_weights("m"), tr.a.m)):
        for (W, bb), (Ww, bw) in zip(got, want):
            assert same(W, Ww) and same(bb, bw)
    (xa, va), (xc, vc) = extras_of(a), extras_of(c)
    assert same(va, vc) and same(xa[va], xc[vc]) and va.any()
    tr2 = model_for(a, wa, wc)  # ... and with the configured noise the actor ends elsewhere
    d = make_env(None)
    d.set_weights(wa)
    d.collect(6)
    for i in range(3):
        twin_train(d, tr2, u[i], zu[i])
    assert not same(tr2.a.m[0][0], tr.a.m[0][0])
    xd, vd = extras_of(d)
    assert same(vd, vc) and not same(xd[vd], xc[vc])
    # the search's own draws: the two handles share the seed, the key and the ordinal
    a.train(3)
    for i in range(3):
        b.train(1)
    for ga, gb in zip(sets(a), sets(b)):
        for (W, bb), (Ww, bw) in zip(ga, gb):
            assert same(W, Ww) and same(bb, bw)
    compare_end(a, b)
    for e in (a, b, c, d):
        e.close()


@pytest.mark.parametrize("kw,word", [(dict(ALGORITHM="DPG"), "ALGORITHM"), (dict(ALGORITHM="CACLA"), "ALGORITHM"),
                                     (dict(OCACLA_ONLINE_SAMPLES=2), "OCACLA_ONLINE_SAMPLES"), (dict(NOISE_TYPE="Orn-Uhl"), "NOISE_TYPE"),
                                     (dict(OCACLA_EXPL_SAMPLES=9), "OCACLA_EXPL_SAMPLES"),
                                     (dict(ACTOR_IS=True), "ACTOR_IS"), (dict(AC_ACTOR_TRAINING_START=5), "AC_ACTOR_TRAINING_START"),
                                     (dict(DPG_USE_CACLA=True), "DPG_USE_CACLA"), (dict(AMSGRAD=True), "AMSGRAD"),
                                     (dict(DPG_CRITIC_FUNC="elu"), "DPG_CRITIC_FUNC")])
def test_env_refuses_by_name_what_the_device_does_not_train(kw, word):
    with pytest.raises(ValueError, match=word):
        make_env("dpg", True, prm=parameters(**kw))


def test_search_needs_the_dpg_trainer_and_train_accepts_nothing_new():
    from aigar_amd.env import AgarSpgEnv, AgarVecEnv
    for train in (None, True, dict(min_size=3)):
        with pytest.raises(ValueError, match="search= needs train='dpg'"):
            make_env(train, True, prm=parameters(ALGORITHM="CACLA"))
    with pytest.raises(ValueError, match="search= needs train='dpg', continuous=, network= and memory="):
        AgarSpgEnv(5, parameters(), n_arenas=1, field_size=100, continuous=True, network=True, train="dpg", search=True)
    with pytest.raises(ValueError, match="search: unknown keys"):
        make_env("dpg", dict(var_epochs=3))
    with pytest.raises(ValueError, match="train: unknown keys"):
        make_env(dpg(samples=3), True)
    with pytest.raises(ValueError, match="train: q_increase"):
        make_env(dpg(q_increase=0.5), True)
    # the three pinned refusals of train= hold beside search=, with and without it
    dp = parameters(ALGORITHM="DPG", DPG_ACTOR_LAYERS=HIDDEN)
    for search in (None, True):
        with pytest.raises(ValueError, match="True, a dict or 'dpg'"):
            make_env("spg", search)
        with pytest.raises(ValueError, match="algorithm = 'spg'"):
            make_env(dict(algorithm="spg"), search)
    with pytest.raises(ValueError, match="OCACLA_ENABLED"):
        make_env("dpg", None, prm=parameters(ALGORITHM="DPG", DPG_ACTOR_LAYERS=HIDDEN, OCACLA_ENABLED=True))
    with pytest.raises(TypeError):
        AgarVecEnv(5, dp, n_arenas=1, field_size=100, search=True)
    # without search= the class is AgarVecEnv: the DPG trainer, and zu is refused
    e = make_env("dpg", None, prm=dp)
    assert e.dpg and not e.spg and e.train_info() == dict(steps=0, skipped=0, since_target=0, actor_steps=0, actor_skipped=0)
    with pytest.raises(ValueError, match="zu is the SPG search's"):
        e.train(1, None, np.zeros((1, BATCH, K, 2, 16, 2)))
    with pytest.raises(RuntimeError, match="without search="):
        e.search_noise
    e.train(1)
    e.close()
    e = make_env("dpg", True, prm=parameters(OCACLA_EXPL_SAMPLES=2, OCACLA_NOISE=0.5, OCACLA_NOISE_DECAY=0.25,
                                             OCACLA_REPLACE_TRANSITIONS=True, DPG_CRITIC_ALPHA=0.002, DPG_TAU=0.01))
    assert e.training == dict(batch=BATCH, min_size=32, target_steps=1500, critic_lr=0.002, actor_lr=0.0001, beta1=0.9,
                              beta2=0.999, epsilon=1e-7, discount=0.9, tau=0.01, samples=2, moving=True, replace=True,
                              prio_evals=True, fused=True, noise=0.5, noise_decay=0.25, seed=lw.SEED)
    assert e.train_info() == dict(steps=0, skipped=0, since_target=0, actor_steps=0, actor_skipped=0, actor_empty=0, selected=0)
    assert e.search_noise.item() == 0.5 and len(e.get_weights(target=True)) == len(HIDDEN) + 1
    with pytest.raises(RuntimeError, match="CACLA trainer"):
        e.cacla_var()
    e.close()
