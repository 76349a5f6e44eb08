"""GPU: an AgarVecEnv whose stepper keeps its own stream (`torch_stream=False`) against one on
torch's stream.  The facade then orders every call that crosses the two streams itself: torch's
work is finished before the stepper's call, and the stepper's before the call returns.  Both
envs get the same weights and make the same calls with given draws, and everything a call
returns is compared by bit pattern.  The worlds are those of the trainers' tests: 2 arenas x 5
players on a field of 100, 64 prioritized transitions, batch 4.

The decisions themselves (`collect`) are not ordered by the facade; the test orders them (`settle`)
and compares what they leave behind through the ordered calls that follow."""
import numpy as np
import pytest

import learner_worlds as lw
import net_model as M
import test_gpu_env_actrain as AC
import test_gpu_env_dpg as DPG
import test_gpu_env_train as QL
from test_gpu_env_train import same

pytestmark = pytest.mark.gpu

BATCH = 4


def make_env(parameters, own, **kw):
    """make_env of the trainers' tests, with the stream choice; own: the stepper keeps its own stream."""
    import torch
    from aigar_amd.env import AgarVecEnv
    e = AgarVecEnv(5, parameters, n_arenas=2, field_size=100, max_viruses=3, roles=lw.roles_of(5), seed=lw.SEED,
                   desync=False, reset_limit=0, network=True, memory=dict(capacity=64, prioritized=True, batch=BATCH),
                   torch_stream=not own, **kw)
    e.obs.zero_()  # (the Greedy bots' rows are never written)
    torch.cuda.synchronize()
    e.reset(lw.SEED)
    lw.mature(e.stepper, 2, lw.SEED)
    e.observe()
    settle(e)
    return e


def settle(e):
    """Both streams idle: around the calls the facade does not order (set-up, decisions)."""
    e.torch.cuda.synchronize(e.dev)
    e.stepper.sync()


def pair(parameters, **kw):
    return make_env(parameters, False, **kw), make_env(parameters, True, **kw)


def both(envs, call):
    """call(env) on the two envs -> the two results."""
    return [call(e) for e in envs]


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def check(what, got):
    """got: the two envs' results (a tensor, an array, a number, a dict, or a sequence of them)."""
    x, y = got
    if isinstance(x, dict):
        assert x == y, what
    elif isinstance(x, (tuple, list)):
        assert len(x) == len(y), what
        for k, (p, q) in enumerate(zip(x, y)):
            check("%s[%d]" % (what, k), (p, q))
    else:
        assert same(host(x), host(y)), what


def collect(envs, n):
    for e in envs:
        e.collect(n)
        settle(e)
    check("obs after collect", both(envs, lambda e: e.obs))
    check("memory size", both(envs, lambda e: e.memory_size()))


def test_dpg_env_on_its_own_stream_returns_what_one_on_torchs_stream_returns():
    envs = pair(DPG.parameters(), continuous=True, train=DPG.dpg())
    a = envs[0]
    assert a.stepper is not envs[1].stepper and a.dpg and envs[1].dpg
    wa, wc = DPG.weights_for(a, 3)
    for e in envs:
        e.set_weights(wa)
        e.set_critic_weights(wc)
        e.stepper.dpg_sync_target()
    collect(envs, 3)
    rng = np.random.default_rng(11)
    u = rng.random(BATCH)
    bt = both(envs, lambda e: e.sample(u=u))
    check("sample", bt)
    assert (host(bt[0].idx) >= 0).all()
    td = rng.standard_normal(BATCH)
    both(envs, lambda e: e.update_priorities(bt[0].idx, td))
    u17 = np.linspace(0.0, 0.999, 17)
    check("sample after update_priorities", both(envs, lambda e: e.sample(17, u17)))
    check("sample_extra", both(envs, lambda e: e.sample_extra(bt[0].idx)))
    n_act = a.continuous["n_act"]
    best = rng.random((BATCH, n_act))
    both(envs, lambda e: e.update_actions(bt[0].idx, best))
    ex = both(envs, lambda e: e.sample_extra(bt[0].idx))
    check("sample_extra after update_actions", ex)
    assert host(ex[1][1]).all() and same(host(ex[1][0])[:, :n_act], best)
    rows = rng.random((7, n_act))
    un = rng.random((7, 2, 3, 2))
    check("perturb", both(envs, lambda e: e.perturb(rows, u=un)))
    ut = rng.random((2, BATCH))
    both(envs, lambda e: e.train(2, u=ut))
    check("train_td", both(envs, lambda e: e.train_td()))
    info = both(envs, lambda e: e.train_info())
    check("train_info", info)
    assert info[1]["steps"] == 2 and info[1]["skipped"] == 0
    got = both(envs, lambda e: e.get_weights())
    check("get_weights", got)
    assert not same(got[1][0][0], wa[0][0])
    check("get_weights(target=True)", both(envs, lambda e: e.get_weights(target=True)))
    check("get_critic_weights", both(envs, lambda e: e.get_critic_weights()))
    check("get_critic_weights(target=True)", both(envs, lambda e: e.get_critic_weights(target=True)))
    s3 = host(a.obs[a.nn][:3])
    act = rng.random((3, n_act))
    q = both(envs, lambda e: e.q_value(s3, act))
    check("q_value", q)
    assert np.isfinite(host(q[1])).all()
    _, wc2 = DPG.weights_for(a, 4)
    both(envs, lambda e: e.set_critic_weights(wc2))
    got = both(envs, lambda e: e.get_critic_weights())
    check("get_critic_weights after set_critic_weights", got)
    assert same(got[1][0][0], wc2[0][0])
    check("q_value after set_critic_weights", both(envs, lambda e: e.q_value(s3, act)))
    for e in envs:
        e.close()


def test_q_learning_env_on_its_own_stream():
    envs = pair(QL.parameters(), discrete=True, train=QL.TRAIN)
    w = QL.weights_for(envs[0], 3)
    both(envs, lambda e: e.set_weights(w))
    collect(envs, 3)
    rng = np.random.default_rng(12)
    ut = rng.random((2, BATCH))
    both(envs, lambda e: e.train(2, u=ut))
    check("train_td", both(envs, lambda e: e.train_td()))
    info = both(envs, lambda e: e.train_info())
    check("train_info", info)
    assert info[1]["steps"] == 2 and info[1]["skipped"] == 0
    got = both(envs, lambda e: e.get_weights())
    check("get_weights", got)
    assert not same(got[1][0][0], w[0][0])
    u = rng.random(BATCH)
    check("sample", both(envs, lambda e: e.sample(u=u)))
    for e in envs:
        e.close()


def test_cacla_env_on_its_own_stream():
    envs = pair(AC.parameters(), continuous=True, train=AC.TRAIN)
    a = envs[0]
    assert a.cacla and envs[1].cacla
    wa, wc = AC.weights_for(a, 3)
    for e in envs:
        e.set_weights(wa)
        e.set_critic_weights(wc)
        e.stepper.actrain_sync_target()
    collect(envs, 3)
    rng = np.random.default_rng(13)
    ut = rng.random((2, BATCH))
    both(envs, lambda e: e.train(2, u=ut))
    check("train_td", both(envs, lambda e: e.train_td()))
    check("train_info", both(envs, lambda e: e.train_info()))
    s3 = host(a.obs[a.nn][:3])
    v = both(envs, lambda e: e.critic_value(s3))
    check("critic_value", v)
    assert np.isfinite(host(v[1])).all()
    var = both(envs, lambda e: e.cacla_var())
    check("cacla_var", var)
    assert var[1] != AC.TRAIN["var_start"]
    check("get_critic_weights", both(envs, lambda e: e.get_critic_weights()))
    for e in envs:
        e.close()


def test_score_of_an_env_on_its_own_stream():
    envs = pair(DPG.parameters(), continuous=True, train=None, score=True)
    s = envs[0].network
    wa = M.make_weights(np.random.default_rng(3), s.n_in, s.units, hi=-3)
    both(envs, lambda e: e.set_weights(wa))
    for e in envs:
        e.collect(3)
        e.torch.cuda.synchronize(e.dev)  # (the decision's clones; the stepper's stream is score()'s to order)
    sc = both(envs, lambda e: e.score())
    check("score", sc)
    assert (host(sc[1])[:, 0] > 0).all()
    for e in envs:
        e.close()
