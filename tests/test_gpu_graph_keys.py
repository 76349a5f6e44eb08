"""GPU: the re-capture paths of the captured graphs ("Graph slots").  One
handle replays graphs; a twin created under AIGAR_NO_GRAPH=1 (read at aigar_create) issues
every launch directly and takes the same calls.  Whatever the graphed handle re-captures,
keeps or drops, both must compute the same: after every decision the rewards and the
observation rows are compared by bit pattern and the worlds at float tolerance 0.

1. the decision graph's key: key A for 3 decisions, key B for 3, A again for 3, one
   sequence per key component that changes;
2. a feature torn down and configured again between two decisions (its buffers are freed
   and, the sizes being the same, likely come back at the same addresses);
3. aigar_step across the change of the eat phase's round count.

The world is the smallest of tests/learner_worlds.py: 1 arena of 12 bots, matured, 4 ticks
per decision."""
import numpy as np
import pytest

import learner_worlds as lw
import parity
import shapes

pytestmark = pytest.mark.gpu
from aigar_amd import _abi, _lib  # noqa: E402

A, B, FIELD, MV = lw.SHAPES[0][:4]
P = lw.model_params(lw.MATRIX[1])  # frame skip 3, 4 values per action, split and eject
ALL_NN = ["NN"] * B


def make_pair(monkeypatch, roles=ALL_NN, **kw):
    """(the graphed env, its twin of direct launches), at the same matured world."""
    from aigar_amd.env import AgarVecEnv
    envs = []
    for no_graph in (False, True):
        if no_graph:
            monkeypatch.setenv("AIGAR_NO_GRAPH", "1")
        else:
            monkeypatch.delenv("AIGAR_NO_GRAPH", raising=False)
        e = AgarVecEnv(B, lw.env_parameters(P, NUM_ACTIONS=16, SQUARE_ACTIONS=True, EPSILON=0.3, GAUSSIAN_NOISE=0.2),
                       n_arenas=A, field_size=FIELD, max_viruses=MV, roles=roles, seed=lw.SEED, desync=False,
                       reset_limit=0, **kw)
        e.obs.zero_()  # (the Greedy and Random bots' rows are never written)
        e.reset(lw.SEED)
        lw.mature(e.stepper, A, lw.SEED)  # (load_state: the bots start over)
        e.observe()
        envs.append(e)
    monkeypatch.delenv("AIGAR_NO_GRAPH")
    return envs


def same(x, y):
    return shapes.obs_bits_equal(x.cpu().numpy(), y.cpu().numpy())


def check(a, b, ra, rb, t):
    """After a decision: rewards and observation rows bit for bit, the worlds at tolerance 0."""
    assert same(ra[1], rb[1]), "decision %d: rewards differ" % t
    oa, ob = ra[0].cpu().numpy().reshape(a.NP, -1), rb[0].cpu().numpy().reshape(b.NP, -1)
    assert shapes.obs_bits_equal(oa, ob), "decision %d: %s" % (t, shapes.bits_diff(oa, ob))
    for k in range(A):
        assert parity.diff_states(a.stepper.get_state(k), b.stepper.get_state(k), ftol=0.0) == [], t


def set_roles(env, roles):
    """aigar_set_roles on a live env, with the env's own view of who is NN."""
    torch = env.torch
    r = np.array([_abi.ROLES[x] for x in roles] * A, np.uint8)
    env.stepper.set_roles(r)
    env.roles = r
    env.nn = torch.as_tensor(r == _abi.ROLE_NN, device=env.dev)
    env._nn_u8 = env.nn.to(torch.uint8)
    env._mixed = bool((r != _abi.ROLE_NN).any())


def env_config(env, salt):
    env.stepper.env_config(greedy_split=True, random_skip=max(1, env.skip), random_split=env.enable_split,
                           random_eject=True, salt=salt)


def swap(name, make):
    """A key component that is a tensor of the env: B is another tensor, A the first one again."""
    def to_b(env):
        env._first = getattr(env, name)
        setattr(env, name, make(env))

    def to_a(env):
        setattr(env, name, env._first)
    return to_b, to_a


def put(name, b, a):
    return (lambda env: setattr(env, name, b)), (lambda env: setattr(env, name, a))


def reward_scale(v):
    return lambda env: setattr(env.reward_params, "reward_scale", v)


# component -> (the roles the env starts with, key A -> key B, key B -> key A)
COMPONENTS = {
    "obs": (ALL_NN,) + swap("obs", lambda env: env.torch.zeros_like(env.obs)),
    "reward": (ALL_NN,) + swap("_r", lambda env: env.torch.zeros_like(env._r)),
    "skip": (ALL_NN,) + put("skip", 0, P.frame_skip),
    "enable_split": (ALL_NN,) + put("enable_split", False, True),
    "reward_param": (ALL_NN, reward_scale(0.7), reward_scale(lw.REWARD["reward_scale"])),
    "dtype": (ALL_NN,) + swap("obs", lambda env: env.torch.zeros(tuple(env.obs.shape), dtype=env.torch.float32,
                                                                   device=env.dev)),
    "roles": (ALL_NN, lambda env: set_roles(env, lw.roles_of(B)), lambda env: set_roles(env, ALL_NN)),
    "salt": (lw.roles_of(B), lambda env: env_config(env, lw.SEED + 1), lambda env: env_config(env, lw.SEED)),
}


@pytest.mark.parametrize("component", list(COMPONENTS))
def test_alternating_keys_on_one_handle(component, monkeypatch):
    import torch
    roles, to_b, to_a = COMPONENTS[component]
    a, b = make_pair(monkeypatch, roles=roles)
    assert P.frame_skip == 3 and a.skip == 3 and a.enable_split and same(a.obs, b.obs)
    gen = torch.Generator(device="cuda").manual_seed(lw.SEED)
    t = 0
    for change in (None, to_b, to_a):
        if change is not None:
            change(a)
            change(b)
        for _ in range(3):
            act = torch.rand((a.NP, 4), dtype=torch.float64, device="cuda", generator=gen)
            ra, rb = a.step(act), b.step(act)
            check(a, b, ra, rb, t)
            t += 1
    assert torch.isfinite(ra[1]).any() and a.stepper.get_state(0)["tick"] > 0
    a.close()
    b.close()


def reconfigure_q(env):
    """decide_config off, then on with another action table (25 -> 9 actions, twice with split)."""
    from aigar_amd import actions
    table = actions.discrete_actions(9, True, True, True)
    assert table.shape[0] != env.discrete["n_out"]
    env.stepper.decide_config(None)
    env.stepper.decide_config(table, env.discrete["strategy"], env._q_dtype, env.discrete["seed"])
    env._table, env._q = table, {}  # (the Q buffers are [NP, n_out])
    env.discrete["n_out"] = int(table.shape[0])


def reconfigure_ac(env):
    """noise_config off, then on: Gaussian -> Orn-Uhl (the same three [NP, 4] buffers)."""
    cc = env.continuous
    env.stepper.noise_config(None)
    env.stepper.noise_config(cc["n_act"], "Orn-Uhl", env.torch.float64, theta=0.3, ou_mu=0.25, dt=0.5, seed=cc["seed"],
                             store_raw=cc["store_raw"])


@pytest.mark.parametrize("head", ["q", "ac"])
def test_reconfigure_between_decisions(head, monkeypatch):
    import torch
    kw = dict(discrete=True) if head == "q" else dict(continuous=dict(noise="Gaussian"))
    a, b = make_pair(monkeypatch, **kw)
    gen = torch.Generator(device="cuda").manual_seed(lw.SEED)
    for t in range(4):
        if t == 2:
            for env in (a, b):
                (reconfigure_q if head == "q" else reconfigure_ac)(env)
        if head == "q":
            q = torch.randn((a.NP, a.discrete["n_out"]), dtype=torch.float32, device="cuda", generator=gen)
            u = torch.rand((a.NP, 3), dtype=torch.float64, device="cuda", generator=gen)
            ra, rb = a.step_q(q, u), b.step_q(q, u)
            assert torch.equal(a.action_idx, b.action_idx) and same(a.action_value, b.action_value), t
            assert int(a.action_idx.max()) < a.discrete["n_out"]
        else:
            mu = torch.rand((a.NP, a.continuous["n_act"]), dtype=torch.float64, device="cuda", generator=gen)
            ra, rb = a.step_ac(mu), b.step_ac(mu)  # (the device's own draws)
            assert same(a.noisy_action, b.noisy_action), t
        check(a, b, ra, rb, t)
    a.close()
    b.close()


def ring(env):
    """exp_info and every slot of the replay memory."""
    import torch
    cap = env.stepper.exp_info()["capacity"]
    idx = torch.arange(cap, device="cuda")
    s = torch.full((cap,) + tuple(env.obs.shape[1:]), -3.0, dtype=env.obs.dtype, device="cuda")
    s2, a = s.clone(), torch.full((cap, 4), -3.0, dtype=torch.float64, device="cuda")
    r, d = torch.full((cap,), -3.0, dtype=torch.float64, device="cuda"), torch.zeros(cap, dtype=torch.bool, device="cuda")
    env.stepper.exp_gather(idx, s=s, a=a, r=r, s2=s2, done=d)
    return env.stepper.exp_info(), [s, a, r, s2, d.to(torch.float64)]


def test_replay_memory_reconfigured_between_decisions(monkeypatch):
    import torch
    a, b = make_pair(monkeypatch, memory=dict(capacity=64))
    gen = torch.Generator(device="cuda").manual_seed(lw.SEED)
    for t in range(5):
        if t == 2:  # free, then another capacity: the control block and the players' buffers keep their sizes
            for env in (a, b):
                assert env.stepper.exp_info()["added"] > 0
                env.stepper.exp_config(None)
                env.stepper.exp_config(48, dtype=env.obs.dtype, seed=lw.SEED)
                env.observe()  # (the players' old states: the next decision has transitions to append)
        act = torch.rand((a.NP, 4), dtype=torch.float64, device="cuda", generator=gen)
        ra, rb = a.step(act), b.step(act)
        check(a, b, ra, rb, t)
        ia, rows_a = ring(a)
        ib, rows_b = ring(b)
        assert ia == ib and ia["capacity"] == (64 if t < 2 else 48), t
        for x, y in zip(rows_a, rows_b):
            assert same(x, y), t
    assert ia["added"] > 0
    a.close()
    b.close()


def test_step_across_the_round_change(monkeypatch):
    """aigar_step's graph has the eat phase's round count in its key: 1 until the handle's
    first Greedy policy, 2 after it."""
    cfg = lw.config(lw.SHAPES[0])
    pair = []
    for no_graph in (False, True):
        if no_graph:
            monkeypatch.setenv("AIGAR_NO_GRAPH", "1")
        else:
            monkeypatch.delenv("AIGAR_NO_GRAPH", raising=False)
        s = _lib.Stepper(cfg)
        s.reset(lw.SEED)
        lw.mature(s, A, lw.SEED)
        pair.append(s)
    monkeypatch.delenv("AIGAR_NO_GRAPH")
    g, d = pair
    for greedy in (False, True):
        for s in pair:
            if greedy:
                s.policy_greedy(True)
            s.step(2)
        assert parity.diff_states(g.get_state(), d.get_state(), ftol=0.0) == [], greedy
    assert g.get_state()["tick"] == 4
    g.close()
    d.close()
