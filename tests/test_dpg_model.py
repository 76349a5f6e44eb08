"""The DPG step's Python model (tests/dpg_model.py), checked without a device: dQ/da and the
actor's gradients against float64 torch.autograd on the combined model Q([s, mu(s)]) -- exactly
where float32 is exact, within the derived float32 bounds on mixed magnitudes -- the soft update
against numpy's own expression, and the trainer's counters, target updates and skips.  CPU only.

Bounds: u = 2^-24 for a value rounded once; gamma_n sum |.||.| with gamma_n = n u / (1 - n u) for a
chain of n fused steps (Higham, Accuracy and Stability of Numerical Algorithms, §3.1; n + 1 where
the operands carry their own u)."""
import numpy as np
import pytest

import dpg_model as DM
import net_model as M
import train_model as T

F32 = np.float32
U = 2.0 ** -24  # float32's unit roundoff


def _int_net(rng, n_in, units, lo=-2, hi=3):
    sizes = (n_in,) + tuple(units)
    return [(rng.integers(lo, hi, (sizes[l], sizes[l + 1])).astype(F32), rng.integers(-1, 2, sizes[l + 1]).astype(F32))
            for l in range(len(units))]


def _leaves(weights):
    import torch
    return [(torch.tensor(W.astype(np.float64), requires_grad=True), torch.tensor(b.astype(np.float64), requires_grad=True))
            for W, b in weights]


def _mlp(ps, x, hidden):
    import torch
    h = x
    for l, (W, b) in enumerate(ps):
        h = h @ W + b
        if l + 1 < len(ps) and hidden == "relu":
            h = torch.relu(h)
    return h


@pytest.mark.parametrize("hidden", ["relu", "linear"])
@pytest.mark.parametrize("critic_units", [(1,), (6, 1), (6, 4, 1)])
def test_dq_da_and_actor_gradients_equal_autograd_where_float32_is_exact(hidden, critic_units):
    """Small integers, B a power of two, a linear actor head standing in for the sigmoid (mu = y,
    so the head's factor is 1): the combined model's loss is mean_r (Q([s_r, mu(s_r)]) - tgt_r)^2
    with the critic's weights frozen.  The model's ea must equal dLoss/dmu and the actor's
    gradients autograd's, exactly."""
    import torch
    rng = np.random.default_rng(3 + len(critic_units))
    n_s, n_act, B = 5, 3, 8
    actor = _int_net(rng, n_s, (4, n_act))
    critic = _int_net(rng, n_s + n_act, critic_units)
    s = rng.integers(-3, 4, (B, n_s)).astype(np.float64)
    tgt = rng.integers(-40, 40, B).astype(np.float64)
    hsa, mu = T.forward_saved(s, actor, hidden)
    hsq, qmu = T.forward_saved(DM.sa_rows(s, mu), critic, hidden)
    dq = DM.q_delta(qmu[:, 0], tgt - 2.0, 2.0)  # (qt + q_increase = tgt)
    d0 = DM.first_layer_error(hsq, critic, dq, hidden)
    ea = DM.action_error(d0, critic[0][0], n_s, n_act)
    grads = T.backward(hsa, actor, ea, hidden)
    pa, pc = _leaves(actor), _leaves(critic)
    mu_t = _mlp(pa, torch.tensor(s), hidden)
    mu_t.retain_grad()
    q_t = _mlp(pc, torch.cat([torch.tensor(s), mu_t], dim=1), hidden)
    assert np.array_equal(mu_t.detach().numpy(), mu) and np.array_equal(q_t.detach().numpy(), qmu)
    ((q_t[:, 0] - torch.tensor(tgt)) ** 2).mean().backward()
    assert np.array_equal(ea.astype(np.float64), mu_t.grad.numpy())
    assert (ea != 0).sum() >= 4
    nonzero = 0
    for (gW, gb), (tW, tb) in zip(grads, pa):
        assert np.array_equal(gW.astype(np.float64), tW.grad.numpy()) and np.array_equal(gb.astype(np.float64), tb.grad.numpy())
        nonzero += int((gW != 0).sum())
    assert nonzero > 8


def test_action_error_takes_the_action_rows_of_the_first_layer():
    """W_0's rows n_s .. n_s + n_act - 1, not its first n_act rows, in one chain over ascending units."""
    d0 = np.array([[1, 2, 4]], F32)
    W0 = np.arange(15, dtype=F32).reshape(5, 3)  # n_s = 3, n_act = 2: rows 3 and 4
    assert DM.action_error(d0, W0, 3, 2).tolist() == [[9 + 20 + 44, 12 + 26 + 56]]
    # the order is observable: 2^24 + 1 - 2^24 is 0 in this order (the 1 is absorbed), 1 in the reverse
    d0 = np.array([[2.0 ** 24, 1.0, -2.0 ** 24]], F32)
    assert DM.action_error(d0, np.ones((2, 3), F32), 1, 1).tolist() == [[0.0]]
    assert DM.action_error(d0[:, ::-1].copy(), np.ones((2, 3), F32), 1, 1).tolist() == [[1.0]]


def test_the_sigmoid_heads_factor_is_one_rounding_of_the_float64_product():
    """delta_L = float32((double)ea (mu (1 - mu))): float64 arithmetic rounded ONCE, so it is within
    u of the exact product (the float64 operations' own error, a few 2^-53, is covered by the
    2^-20 slack), and it is this association, not (ea mu) (1 - mu)."""
    rng = np.random.default_rng(5)
    ea = M.mixed(rng, (64, 4), lo=-20, hi=10, p_sub=0, p_zero=0)
    mu = rng.random((64, 4))
    d = DM.actor_delta(ea, mu)
    want = ea.astype(np.float64) * mu * (1.0 - mu)
    assert (np.abs(d.astype(np.float64) - want) <= U * np.abs(want) * (1 + 2.0 ** -20)).all()
    assert np.array_equal(d, (ea.astype(np.float64) * (mu * (1.0 - mu))).astype(F32))
    assert DM.actor_delta(np.array([[np.inf]], F32), np.array([[0.5]]))[0, 0] == np.inf
    assert np.isnan(DM.actor_delta(np.array([[np.inf]], F32), np.array([[1.0]]))[0, 0])


@pytest.mark.parametrize("hidden", ["relu", "linear"])
def test_dq_da_equals_autograd_within_the_float32_bounds(hidden):
    """Mixed magnitudes, a critic (H, 1).  delta_0[r][j] is ONE fused step from +0.0f, the exact
    product dq_r W_1[j] rounded once: within u of autograd's dLoss/dy_0 on the model's own dq.  ea
    is a chain of H fused steps on those values: within gamma_H sum_j |delta_0||W_0| of the float64
    product of the model's delta_0; against autograd, whose delta_0 differs by u, within
    gamma_(H+1) of the same sum.  The actor's delta then is one rounding of ea mu (1 - mu)."""
    import torch
    rng = np.random.default_rng(11)
    n_s, n_act, H, B = 9, 3, 12, 10
    mk = lambda shape: M.mixed(rng, shape, lo=-4, hi=1, p_sub=0, p_zero=0)
    critic = [(mk((n_s + n_act, H)), mk((H,))), (mk((H, 1)), mk((1,)))]
    s = mk((B, n_s)).astype(np.float64)
    mu = rng.random((B, n_act))
    qt = mk((B,)).astype(np.float64)
    x = DM.sa_rows(s, mu)
    hsq, qmu = T.forward_saved(x, critic, hidden)
    dq = DM.q_delta(qmu[:, 0], qt, 2.0)
    d0 = DM.first_layer_error(hsq, critic, dq, hidden)
    ea = DM.action_error(d0, critic[0][0], n_s, n_act)
    # autograd from the model's own float32 first-layer outputs and output delta
    W0a = critic[0][0][n_s:].astype(np.float64)  # [n_act][H]
    a_t = torch.tensor(x[:, n_s:].astype(np.float64), requires_grad=True)
    y0 = torch.tensor(x[:, :n_s].astype(np.float64)) @ torch.tensor(critic[0][0][:n_s].astype(np.float64)) \
        + a_t @ torch.tensor(W0a) + torch.tensor(critic[0][1].astype(np.float64))
    y0.retain_grad()
    h = torch.relu(y0) if hidden == "relu" else y0
    q = h @ torch.tensor(critic[1][0].astype(np.float64)) + torch.tensor(critic[1][1].astype(np.float64))
    (q[:, 0] * torch.tensor(dq[:, 0].astype(np.float64))).sum().backward()  # dLoss/dq = the model's dq
    gate = hsq[1] > 0 if hidden == "relu" else np.ones_like(hsq[1], bool)
    assert np.array_equal((y0.detach().numpy() > 0) | (hidden != "relu"), gate | (hidden != "relu"))
    want0 = y0.grad.numpy()
    assert (np.abs(d0.astype(np.float64) - want0) <= U * np.abs(want0) * (1 + 2.0 ** -20)).all()
    assert (d0 != 0).sum() > B
    exact = d0.astype(np.float64) @ W0a.T
    mag = np.abs(d0.astype(np.float64)) @ np.abs(W0a).T
    gam = lambda n: n * U / (1 - n * U)
    assert (np.abs(ea.astype(np.float64) - exact) <= gam(H) * mag * (1 + 2.0 ** -20)).all()
    assert (np.abs(ea.astype(np.float64) - a_t.grad.numpy()) <= gam(H + 1) * mag * (1 + 2.0 ** -20)).all()
    assert (ea != 0).all()


@pytest.mark.parametrize("tau", [0.001, 0.25, 1.0, 1e-9])
def test_soft_update_equals_numpys_expression_bit_for_bit(tau):
    rng = np.random.default_rng(2)
    model = M.make_weights(rng, 7, (5, 2), hi=3)
    target = M.make_weights(rng, 7, (5, 2), hi=3)
    got = DM.soft_update(target, model, tau)
    for (gW, gb), (tW, tb), (mW, mb) in zip(got, target, model):
        with np.errstate(all="ignore"):
            wW, wb = tW * (1 - tau) + mW * tau, tb * (1 - tau) + mb * tau  # softlyUpdateTargetModel
        assert wW.dtype == F32 and gW.dtype == F32
        assert np.array_equal(gW.view(np.uint32), wW.view(np.uint32)) and np.array_equal(gb.view(np.uint32), wb.view(np.uint32))
    # a padded entry, +0.0f on both sides, stays +0.0f
    z = DM.soft_update([(np.zeros((1, 1), F32), np.zeros(1, F32))], [(np.zeros((1, 1), F32), np.zeros(1, F32))], tau)
    assert not z[0][0].view(np.uint32).any() and not z[0][1].view(np.uint32).any()
    # ... and it is not the float64 expression rounded once
    if tau == 0.25:
        t64 = (target[0][0].astype(np.float64) * (1 - tau) + model[0][0].astype(np.float64) * tau).astype(F32)
        assert not np.array_equal(t64.view(np.uint32), got[0][0].view(np.uint32))


def _trainer(rng, **kw):
    n_s, n_act = 6, 2
    actor = M.make_weights(rng, n_s, (5, n_act), hi=1)
    critic = M.make_weights(rng, n_s + n_act, (4, 1), hi=1)
    return DM.Trainer(actor, critic, 8, critic_lr=1e-2, actor_lr=1e-2, **kw), actor, critic


def _batch(rng, B=8, n_s=6, n_act=2, reward=None, done=None):
    s = M.mixed(rng, (B, n_s), hi=2).astype(np.float64)
    s2 = M.mixed(rng, (B, n_s), hi=2).astype(np.float64)
    d = np.zeros(B, bool) if done is None else np.asarray(done, bool)
    s2[d] = np.nan
    a = np.zeros((B, 4))
    a[:, :n_act] = rng.random((B, n_act))
    r = M.mixed(rng, (B,), lo=-4, hi=3).astype(np.float64) if reward is None else reward
    return s, a, r, s2, d, np.ones(B)


def same(a, b):
    return all(np.array_equal(W.view(np.uint32), V.view(np.uint32)) and np.array_equal(x.view(np.uint32), y.view(np.uint32))
               for (W, x), (V, y) in zip(a, b))


def test_trainer_counters_soft_update_and_skips():
    rng = np.random.default_rng(9)
    tr, actor, critic = _trainer(rng, tau=0.25, target_steps=2, min_size=10)
    assert tr.step(*_batch(rng), size=9) is None and tr.info() == (0, 1, 0, 0, 0, 0, 0, 0)
    assert same(tr.a.theta, actor) and same(tr.target_c, critic)
    assert tr.step(*_batch(rng), size=10) is not None and tr.info() == (1, 1, 1, 1, 0, 0, 0, 0)
    # the soft update used the networks as this step left them, after the actor half
    assert same(tr.target_a, DM.soft_update(actor, tr.a.theta, 0.25)) and same(tr.target_c, DM.soft_update(critic, tr.c.theta, 0.25))
    assert not same(tr.a.theta, actor) and not same(tr.c.theta, critic)
    assert tr.step(*_batch(rng), size=10) is not None and tr.since == 2  # (tau > 0: no hard copy at target_steps)
    assert not same(tr.target_a, tr.a.theta)
    before = (tr.a.theta, tr.c.theta, tr.target_a, tr.target_c, tr.a.t, tr.c.t)
    bad = np.ones(8)
    bad[3] = np.inf
    assert tr.step(*_batch(rng, reward=bad), size=10) is None and tr.nonfinite and tr.info()[:5] == (2, 2, 2, 2, 0)
    assert all(x is y for x, y in zip(before[:4], (tr.a.theta, tr.c.theta, tr.target_a, tr.target_c)))
    # a done row's reward alone is its target: its NaN q2 does not reach td
    assert tr.step(*_batch(rng, done=[1, 0, 0, 1, 0, 0, 0, 1]), size=10) is not None and np.isfinite(tr.td).all()
    assert tr.info()[:5] == (3, 2, 3, 3, 0)


@pytest.mark.parametrize("target_steps", [0, 1, 3])
def test_trainer_hard_copy(target_steps):
    rng = np.random.default_rng(10)
    tr, actor, critic = _trainer(rng, tau=0.0, target_steps=target_steps)
    for k in range(1, 5):
        assert tr.step(*_batch(rng)) is not None
        due = target_steps > 0 and k % target_steps == 0
        assert same(tr.target_a, tr.a.theta) == due and same(tr.target_c, tr.c.theta) == due
        if target_steps == 0:
            assert same(tr.target_a, actor) and same(tr.target_c, critic) and tr.since == k
    assert tr.since == {0: 4, 1: 0, 3: 1}[target_steps]
    tr.sync_target()
    assert same(tr.target_a, tr.a.theta) and tr.since == 0
    tr.reset()
    assert (tr.c.t, tr.a.t) == (0, 0) and not any(W.any() for W, _ in tr.a.m + tr.c.v)


def test_a_nonfinite_actor_delta_skips_the_actor_half_only():
    rng = np.random.default_rng(12)
    for q_inc in (1e300, 2.0 ** 50):  # a combined delta that is no float32; an ea that overflows
        tr, actor, critic = _trainer(rng, tau=0.5, q_increase=q_inc)
        if q_inc != 1e300:
            # action 0 enters every first-layer unit with 2^58 and the head takes the units with
            # +-2^30 in turn: the pairs cancel exactly in Q, so td is small, and delta_0 W_0 overflows
            tr.c.theta[0][0][6, :] = F32(2.0 ** 58)
            tr.c.theta[1][0][:, 0] = F32(2.0 ** 30) * np.array([1, -1, 1, -1], F32)
            critic = [(W.copy(), b.copy()) for W, b in tr.c.theta]
            tr.sync_target()
        assert tr.step(*_batch(rng)) is not None and np.isfinite(tr.td).all() and np.abs(tr.td).max() < 100
        assert q_inc == 1e300 or (tr.ea is not None and not np.isfinite(tr.ea).all())
        assert tr.info() == (1, 0, 1, 0, 1, 0, 0, 0) and tr.nonfinite
        assert same(tr.a.theta, actor) and not any(W.any() for W, _ in tr.a.m)
        assert same(tr.target_a, actor)  # (the soft update of an actor that did not move)
        assert not same(tr.c.theta, critic)


def test_the_actor_half_sees_the_updated_critic_and_the_old_targets():
    """One step by hand from the pieces, in the order of the contract."""
    rng = np.random.default_rng(13)
    tr, actor, critic = _trainer(rng, tau=0.25, q_increase=0.5)
    s, a, r, s2, d, w = _batch(rng, done=[0, 1, 0, 0, 0, 0, 1, 0])
    assert tr.step(s, a, r, s2, d, w) is not None
    c1 = tr.c.theta  # the critic as the critic half left it
    hsa, y = T.forward_saved(s, actor, "relu")
    mu = DM.sigmoid_rows(y.astype(F32))
    hsq, qmu = T.forward_saved(DM.sa_rows(s, mu), c1, "relu")
    qt = M.forward(DM.sa_rows(s, M.forward(s, actor, "relu", "sigmoid")), critic, "relu", "linear")[:, 0]
    d0 = DM.first_layer_error(hsq, c1, DM.q_delta(qmu[:, 0], qt, 0.5), "relu")
    delta = DM.actor_delta(DM.action_error(d0, c1[0][0], 6, 2), mu)
    assert np.array_equal(delta.view(np.uint32), tr.delta_a.view(np.uint32)) and (delta != 0).any()
    ref = DM.Net(actor, 1e-2)
    ref.apply(T.backward(hsa, actor, delta, "relu"), 0.9, 0.999, 1e-7)
    assert same(ref.theta, tr.a.theta) and same(ref.m, tr.a.m) and tr.a.t == 1
    # with the critic before its update, or the online networks as targets, the delta differs
    hs_old, q_old = T.forward_saved(DM.sa_rows(s, mu), critic, "relu")
    d_old = DM.actor_delta(DM.action_error(DM.first_layer_error(hs_old, critic, DM.q_delta(q_old[:, 0], qt, 0.5), "relu"),
                                           critic[0][0], 6, 2), mu)
    assert not np.array_equal(d_old.view(np.uint32), delta.view(np.uint32))
