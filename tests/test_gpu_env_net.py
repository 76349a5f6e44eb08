"""GPU: AgarVecEnv(network=...) -- `step_net` (the acting network, then the selection or the
noise, inside the decision's graph) against a twin env that evaluates the same network with
`net_forward` on its own `obs` and steps with `step_q` / `step_ac`; `collect(n)` against n
calls of `step_net` across episode ends; the weight push between two collects.  Everything
is compared by bit pattern: obs, reward, alive, done, the chosen indices and values or the
noisy actions, the network's output rows, the replay memory's rows, the fifth field, the
scores and every arena's state.

The worlds are small batched ones (1 x 37, 3 x 100 and 2 x 260 players: arena boundaries
inside the network's 16-row tiles, a partial last tile), NN players among Greedy and Random
bots (tests/learner_worlds.py's roles), matured so that players die from the first ticks;
frame skip 0 and 2.  That NN players die, are dead at decision time and decide again, and
that arenas are reset at different times is asserted below."""
import numpy as np
import pytest

import learner_model as lm
import learner_worlds as lw
import net_model as M
import parity

pytestmark = pytest.mark.gpu
from aigar_amd import _abi, _lib  # noqa: E402

SHAPES = {"1x37": (1, 37, 180, 8), "3x100": (3, 100, 300, 12), "2x260": (2, 260, 480, 30)}
HIDDEN = (20, 17)
T = 4
REWARD = lw.REWARD


def same(x, y):
    """Bit patterns equal, NaN equal to NaN."""
    x, y = x.cpu().numpy(), y.cpu().numpy()
    if x.dtype.kind != "f":
        return x.shape == y.shape and np.array_equal(x, y)
    nx, ny = np.isnan(x), np.isnan(y)
    v = np.uint64 if x.dtype.itemsize == 8 else np.uint32
    return x.shape == y.shape and np.array_equal(nx, ny) and np.array_equal(np.where(nx, 0, x).view(v),
                                                                            np.where(ny, 0, y).view(v))


def make_env(shape, skip, head, kind, algorithm="CACLA", memory=None, score=False, reset_limit=0):
    from aigar_amd.env import AgarVecEnv
    A, B, field, mv = SHAPES[shape]
    p = lm.params(skip, 3, True, False, False, **REWARD)
    prm = lw.env_parameters(p, NUM_ACTIONS=9, SQUARE_ACTIONS=True, EXPLORATION_STRATEGY=kind, EPSILON=0.3,
                            TEMPERATURE=0.7, NOISE_TYPE=kind, GAUSSIAN_NOISE=0.2, ALGORITHM=algorithm,
                            ORN_UHL_THETA=0.3, ORN_UHL_MU=0.25, ORN_UHL_DT=0.5, Q_LAYERS=HIDDEN,
                            CACLA_ACTOR_LAYERS=HIDDEN, DPG_ACTOR_LAYERS=HIDDEN)
    kw = dict(n_arenas=A, field_size=field, max_viruses=mv, roles=lw.roles_of(B), seed=lw.SEED, desync=False,
              reset_limit=reset_limit, score=score, memory=memory, network=True)
    kw["discrete" if head == "q" else "continuous"] = True
    e = AgarVecEnv(B, prm, **kw)
    e.obs.zero_()  # (the Greedy and Random bots' rows are never written)
    e.reset(lw.SEED)
    lw.mature(e.stepper, A, lw.SEED)  # (load_state: the bots start over)
    e.observe()
    return e


def weights_for(env, seed):
    rng = np.random.default_rng(seed)
    s = env.network
    return M.make_weights(rng, s.n_in, s.units, hi=-3)  # (masses of hundreds times 161 inputs: far from overflow)


def draws(gen, env, head):
    import torch
    if head == "q":
        return torch.rand((env.NP, 3), dtype=torch.float64, device="cuda", generator=gen)
    return torch.randint(0, 2 ** 53, (env.NP, 2, T, 2), device="cuda", generator=gen).to(torch.float64) * 2.0 ** -53


def twin_step(b, head, u):
    """The parent's loop on the twin: the network by itself on the twin's states, then the decision."""
    import torch
    out = b._twin_out
    b.stepper.net_forward(b.obs, out)
    return (b.step_q(out, u) if head == "q" else b.step_ac(out, u)), out.clone()


def ring(env, extra):
    import torch
    cap = env.memory["capacity"]
    idx = torch.arange(cap, device="cuda")
    s = torch.full((cap,) + tuple(env.obs.shape[1:]), -3.0, dtype=env.obs.dtype, device="cuda")
    s2, a = s.clone(), torch.full((cap, 4), -3.0, dtype=torch.float64, device="cuda")
    r, d = torch.full((cap,), -3.0, dtype=torch.float64, device="cuda"), torch.zeros(cap, dtype=torch.bool, device="cuda")
    env.stepper.exp_gather(idx, s=s, a=a, r=r, s2=s2, done=d)
    out = [s, a, r, s2, d]
    if extra:
        out += list(env.sample_extra(idx))
    return out


def compare_end(a, b, extra=False):
    A = a.A
    if a.memory is not None:
        ia, ib = a.stepper.exp_info(), b.stepper.exp_info()
        assert ia == ib and ia["added"] > 0
        for x, y in zip(ring(a, extra), ring(b, extra)):
            assert same(x, y)
    for k in range(A):
        assert parity.diff_states(a.stepper.get_state(k), b.stepper.get_state(k), ftol=0.0) == []


CASES = [("1x37", 0, "q", "e-Greedy", True), ("3x100", 2, "q", "Boltzmann", False), ("2x260", 0, "q", "Boltzmann", True),
         ("3x100", 0, "q", "e-Greedy", False),
         ("1x37", 2, "actor", "Gaussian", True), ("3x100", 0, "actor", "Orn-Uhl", False),
         ("2x260", 2, "actor", "Orn-Uhl", True)]


@pytest.mark.parametrize("shape,skip,head,kind,given", CASES, ids=["%s-s%d-%s-%s-u%d" % c for c in CASES])
def test_step_net_is_net_forward_then_the_heads_step(shape, skip, head, kind, given):
    import torch
    decisions = (8 if skip == 0 else 6) * (2 if shape == "1x37" else 1)  # (19 learners: twice the decisions)
    algorithm = "CACLA" if shape != "2x260" else "SPG"
    mem = dict(capacity=4096)
    a = make_env(shape, skip, head, kind, algorithm, mem)
    b = make_env(shape, skip, head, kind, algorithm, mem)
    NP, B = a.NP, a.B
    n_out = a.network.units[-1]
    assert a.network.units[:-1] == HIDDEN and a.network.n_in == a.stepper.obs_len == 161
    assert a.network.out == ("linear" if head == "q" else "sigmoid")
    w = weights_for(a, 3)
    a.set_weights(w)
    b.set_weights([(torch.as_tensor(W, device="cuda"), torch.as_tensor(bb, device="cuda")) for W, bb in w])
    b._twin_out = torch.zeros((NP, n_out), dtype=torch.float64, device="cuda")
    assert same(a.obs, b.obs)
    nn = np.array([r == "NN" for r in lw.roles_of(B)] * a.A)
    deciding = ~np.isnan(a.obs.cpu().numpy()[:, 0]) & nn
    held = np.zeros((NP, n_out))  # the handle's output rows: zero until a player first decides
    gen = torch.Generator(device="cuda").manual_seed(lw.SEED)
    n_died = n_silent = n_back = 0
    model_checked = False
    for t in range(decisions):
        u = draws(gen, a, head) if given else None
        if t == 0:  # the network's rows are the Python model's (the rest of the loop compares devices)
            obs0 = a.obs.cpu().numpy()
            want = M.forward(obs0[deciding], w, "relu", a.network.out)
            model_checked = True
        ra = a.step_net(u)
        rb, out = twin_step(b, head, u)
        for x, y in zip(ra, rb):
            assert same(x, y), t
        out = out.cpu().numpy()
        held = np.where(deciding[:, None], out, held)
        got = a.net_output.cpu().numpy()
        assert np.array_equal(M.bits(got), M.bits(held)), t  # dead and non-NN players keep their rows
        assert not np.isnan(got).any() and (got[~nn] == 0).all()
        if t == 0:
            assert np.array_equal(M.bits(got[deciding]), M.bits(want))
        if head == "q":
            assert same(a.action_idx, b.action_idx) and same(a.action_value, b.action_value), t
            assert ((a.action_idx.cpu().numpy() >= 0) == deciding).all()
        else:
            assert same(a.noisy_action, b.noisy_action), t
            assert (~np.isnan(a.noisy_action.cpu().numpy()[:, 0]) == deciding).all()
        alive_now = ra[2].cpu().numpy()
        n_died += int((deciding & ~alive_now).sum())
        n_silent += int((nn & ~deciding).sum())
        n_back += int((nn & ~deciding & alive_now).sum())
        deciding = alive_now
    print("died %d, dead at decision time %d, deciding again %d" % (n_died, n_silent, n_back))
    assert model_checked and n_died >= 1, n_died
    if shape != "1x37":  # (50 and 260 learners)
        assert n_silent >= 1 and n_back >= 1, (n_silent, n_back)
    compare_end(a, b, extra=head == "actor")
    if head == "actor" and algorithm == "CACLA":
        assert bool(a.sample_extra(torch.arange(8, device="cuda"))[1].any())
    a.close()
    b.close()


COLLECT = [("3x100", 0, "q", "e-Greedy", True), ("2x260", 2, "actor", "Orn-Uhl", False),
           ("1x37", 2, "q", "Boltzmann", False)]


@pytest.mark.parametrize("shape,skip,head,kind,score", COLLECT, ids=["%s-s%d-%s-%s-score%d" % c for c in COLLECT])
def test_collect_is_n_step_nets_and_a_weight_push_takes_effect(shape, skip, head, kind, score):
    import torch
    n1, n2 = 9, 7
    per = skip + 1
    limit = 5 * per
    mem = dict(capacity=8192, prioritized=True, alpha=0.7, beta=0.5, batch=64)
    a = make_env(shape, skip, head, kind, "CACLA", mem, score, limit)
    b = make_env(shape, skip, head, kind, "CACLA", mem, score, limit)
    for e in (a, b):  # the arenas' episodes end at different decisions
        e.age[:] = np.arange(e.A) * 2 * per
    w1, w2 = weights_for(a, 4), weights_for(a, 5)
    done_b = torch.zeros(a.NP, dtype=torch.bool, device="cuda")
    ends = []
    for e in (a, b):
        e.set_weights(w1)
    ra = a.collect(n1)
    for t in range(n1):
        rb = b.step_net()
        done_b |= rb[3]
        if bool(rb[3].any()):
            ends.append((t, tuple(sorted(set((np.nonzero(rb[3].cpu().numpy())[0] // a.B).tolist())))))
    for x, y in zip(ra[:3], rb[:3]):
        assert same(x, y)
    assert same(ra[3], done_b) and same(a.obs, b.obs) and same(a.net_output, b.net_output)
    if a.A > 1:
        assert len(set(ends)) >= 2 and len({e[1] for e in ends}) >= 2, ends  # two arenas ended, at different times
    else:
        assert len(ends) >= 1
    assert (a.age == b.age).all() and a._resets == b._resets
    # the push: the next decision runs on the new weights
    obs_before = a.obs.clone()
    deciding = (~torch.isnan(obs_before[:, 0]) & a.nn).cpu().numpy()
    for e in (a, b):
        e.set_weights(w2)
    a.collect(1)
    b.step_net()
    want = torch.zeros((a.NP, a.network.units[-1]), dtype=torch.float64, device="cuda")
    a.stepper.net_forward(obs_before, want)
    got = a.net_output.cpu().numpy()
    assert np.array_equal(M.bits(got[deciding]), M.bits(want.cpu().numpy()[deciding])) and deciding.any()
    a.set_weights(w1)
    a.stepper.net_forward(obs_before, want)
    assert not np.array_equal(M.bits(got[deciding]), M.bits(want.cpu().numpy()[deciding]))
    a.set_weights(w2)
    ra = a.collect(n2)
    done_b.zero_()
    for t in range(n2):
        rb = b.step_net()
        done_b |= rb[3]
    for x, y in zip(ra[:3], rb[:3]):
        assert same(x, y)
    assert same(ra[3], done_b) and same(a.obs, b.obs) and same(a.net_output, b.net_output)
    if head == "q":
        assert same(a.action_idx, b.action_idx) and same(a.action_value, b.action_value)
    else:
        assert same(a.noisy_action, b.noisy_action)
    if score:
        assert same(a.score(), b.score()) and same(a.last_score, b.last_score) and same(a.last_return, b.last_return)
        assert not bool(torch.isnan(a.last_score).all())
    compare_end(a, b, extra=head == "actor")
    u = torch.rand(64, dtype=torch.float64, device="cuda")
    for x, y in zip(a.sample(u=u), b.sample(u=u)):
        assert same(x, y)
    # one more decision each: the Orn-Uhl states and the held rows were left alike
    for x, y in zip(a.step_net(), b.step_net()):
        assert same(x, y)
    if head == "actor":
        assert same(a.noisy_action, b.noisy_action)
    a.close()
    b.close()


def test_network_needs_its_head_and_its_states():
    import torch
    from aigar_amd.env import AgarVecEnv
    p = lw.env_parameters(lm.params(0, 3, True, False, False, **REWARD), NUM_ACTIONS=9, Q_LAYERS=HIDDEN,
                          CACLA_ACTOR_LAYERS=HIDDEN)
    with pytest.raises(ValueError, match="discrete= or continuous="):
        AgarVecEnv(4, p, field_size=100, network=True)
    off = AgarVecEnv(4, p, field_size=100, discrete=True)
    assert off.network is None and off.stepper.net is None
    with pytest.raises(RuntimeError, match="network"):
        off.step_net()
    off.close()
    with pytest.raises(ValueError, match="elu"):
        AgarVecEnv(4, lw.env_parameters(lm.params(0, 3, True, False, False, **REWARD), ACTIVATION_FUNC_HIDDEN="elu"),
                   field_size=100, discrete=True, network=True)
    env = AgarVecEnv(4, p, field_size=100, discrete=True, network=True)
    with pytest.raises(RuntimeError, match="reset"):
        env.step_net()  # `obs` holds nothing yet
    env.reset()
    g = env.stepper
    n_out = env.network.units[-1]
    # a head without its config, with the wrong dtype, of another width
    args = (env.explore, env._r, env.obs)
    with pytest.raises(RuntimeError, match="noise"):
        g.env_step_net("actor", env.noise_std if hasattr(env, "noise_std") else env.explore[:1].clone(), env._r, env.obs)
    g.decide_config(env._table, "e-Greedy", torch.float32)
    with pytest.raises(RuntimeError, match="q_dtype"):
        g.env_step_net("q", *args, idx=env._idx, val=env._val)
    g.decide_config(None)
    with pytest.raises(RuntimeError, match="action selection"):
        g.env_step_net("q", *args, idx=env._idx, val=env._val)
    g.decide_config(env._table[:5], "e-Greedy", torch.float64)
    with pytest.raises(RuntimeError, match="outputs"):
        g.env_step_net("q", *args, idx=env._idx, val=env._val)
    g.noise_config(3, "Gaussian", torch.float32)
    with pytest.raises(RuntimeError, match="mu_dtype"):
        g.env_step_net("actor", env.explore[:1].clone(), env._r, env.obs)
    g.noise_config(3 if n_out != 3 else 2, "Gaussian", torch.float64)
    with pytest.raises(RuntimeError, match="n_act"):
        g.env_step_net("actor", env.explore[:1].clone(), env._r, env.obs)
    g.decide_config(env._table, "e-Greedy", torch.float64)
    with pytest.raises(RuntimeError, match="n_decisions"):
        g.env_step_net("q", *args, idx=env._idx, val=env._val, n_decisions=0)
    obs32 = env.obs.to(torch.float32)
    with pytest.raises(RuntimeError, match="x_dtype"):
        g.env_step_net("q", env.explore, env._r, obs32, idx=env._idx, val=env._val)
    env.close()
