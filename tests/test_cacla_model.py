"""The CACLA step's Python model (tests/cacla_model.py), checked without a device: the critic's
and the actor's gradients against torch.autograd, gating against compaction, the selection
against a direct transcription of the rule, the variance against its closed recurrence.  CPU only."""
import math

import numpy as np
import pytest

import cacla_model as CM
import net_model as M
import train_model as T

F32 = np.float32
U = 2.0 ** -24  # float32's unit roundoff


def _torch_net(weights, s, hidden, head):
    import torch
    ps = [(torch.tensor(W.astype(np.float64), requires_grad=True), torch.tensor(b.astype(np.float64), requires_grad=True))
          for W, b in weights]
    h = torch.tensor(np.asarray(s, np.float64))
    for l, (W, b) in enumerate(ps):
        h = h @ W + b
        if l + 1 < len(ps) and hidden == "relu":
            h = torch.relu(h)
    y = h
    if head == "sigmoid":
        h = torch.sigmoid(h)
    return ps, y, h


@pytest.mark.parametrize("hidden", ["relu", "linear"])
def test_critic_gradients_equal_autograd_where_float32_is_exact(hidden):
    """Small integers and a power-of-two B, as test_train_model's exact case: the model must equal
    float64 autograd of mean_r w_r (v_r - t_r)^2 exactly."""
    import torch
    rng = np.random.default_rng(3)
    n_in, units, B = 5, (6, 3, 1), 8
    sizes = (n_in,) + units
    w = [(rng.integers(-3, 4, (sizes[l], sizes[l + 1])).astype(F32), rng.integers(-2, 3, sizes[l + 1]).astype(F32))
         for l in range(3)]
    s = rng.integers(-4, 5, (B, n_in)).astype(np.float64)
    wt = np.ldexp(1.0, rng.integers(-1, 2, B))
    hs, v = T.forward_saved(s, w, hidden)
    target = rng.integers(-50, 50, B).astype(np.float64)
    td = target - v[:, 0]
    grads = T.backward(hs, w, CM.critic_delta(td, wt), hidden)
    ps, _, out = _torch_net(w, s, hidden, "linear")
    assert np.array_equal(out.detach().numpy(), v)
    (torch.tensor(wt) * ((out[:, 0] - torch.tensor(target)) ** 2)).mean().backward()
    nonzero = 0
    for (gW, gb), (tW, tb) in zip(grads, ps):
        assert np.array_equal(gW.astype(np.float64), tW.grad.numpy()) and np.array_equal(gb.astype(np.float64), tb.grad.numpy())
        nonzero += int((gW != 0).sum())
    assert nonzero > 20


@pytest.mark.parametrize("hidden", ["relu", "linear"])
def test_actor_delta_and_head_gradient_equal_autograd_within_the_float32_bounds(hidden):
    """The actor's loss is Keras' mse on the sigmoid head over the rows taking part:
    mean_r mean_j (mu_rj - a_rj)^2.  The model's delta_L is float64 arithmetic on the model's mu
    rounded ONCE to float32: |delta - autograd's dL/dy| <= u |.| plus the float64 operations' own
    error (a few 2^-53, covered by the 2^-20 slack).  The head's kernel gradient is one chain of B
    fused steps on those deltas: gamma_B sum |h||delta| as in test_train_model, plus the deltas'
    own u; the rows left out contribute exact zeros."""
    import torch
    rng = np.random.default_rng(7)
    n_in, units, B = 9, (8, 7, 3), 12
    sizes = (n_in,) + units
    w = [(M.mixed(rng, (sizes[l], sizes[l + 1]), lo=-4, hi=1, p_sub=0, p_zero=0),
          M.mixed(rng, (sizes[l + 1],), lo=-4, hi=1, p_sub=0, p_zero=0)) for l in range(3)]
    s = M.mixed(rng, (B, n_in), lo=-4, hi=1, p_sub=0, p_zero=0).astype(np.float64)
    a = rng.random((B, 3))
    part = rng.random(B) < 0.6
    assert 0 < part.sum() < B
    hs, y = T.forward_saved(s, w, hidden)
    mu = CM.sigmoid_rows(y.astype(F32))
    delta = CM.actor_delta(mu, a, part)
    assert not delta[~part].any() and not np.signbit(delta[~part]).any()
    # autograd on the model's own float32 pre-activations as float64 leaves
    y64 = torch.tensor(y[part], requires_grad=True)
    ((torch.sigmoid(y64) - torch.tensor(a[part])) ** 2).mean().backward()
    want = y64.grad.numpy()
    got = delta[part].astype(np.float64)
    assert (np.abs(got - want) <= U * np.abs(want) * (1 + 2.0 ** -20)).all()
    assert (got != 0).sum() > 10
    # the head's kernel gradient with the exact deltas against the model's chain
    full = np.zeros((B, 3))
    full[part] = want
    exact = hs[2].astype(np.float64).T @ full
    gW, gb = T.backward(hs, w, delta, hidden)[2]
    gam = (B + 1) * U / (1 - (B + 1) * U)
    bound = gam * (np.abs(hs[2].astype(np.float64)).T @ np.abs(full))
    assert (np.abs(gW.astype(np.float64) - exact) <= bound * (1 + 2.0 ** -20)).all()
    assert (gW != 0).sum() > 10
    # (the layers below the head are train_model.backward's chains, checked in test_train_model)


@pytest.mark.parametrize("hidden", ["relu", "linear"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_gating_rows_with_a_zero_delta_equals_compaction_by_value(hidden, seed):
    """The device keeps the rows an epoch leaves out, with a +0.0f output delta; the reference
    compacts them away.  A left-out row's step is fmaf(h, +0.0f, acc), which is acc by value (only
    the sign of a zero acc can change), and its back-propagated errors are zeros as well, so the
    gradients are equal by value."""
    rng = np.random.default_rng(seed)
    n_in, units, B = 11, (9, 6, 2), 13
    w = M.make_weights(rng, n_in, units, hi=2)
    s = M.mixed(rng, (B, n_in), hi=3).astype(np.float64)
    a = rng.random((B, 2))
    part = rng.random(B) < 0.5
    part[[0, B - 1]] = [seed == 0, seed != 0]  # (a left-out row first, or last)
    assert 0 < part.sum() < B
    hs, y = T.forward_saved(s, w, hidden)
    mu = CM.sigmoid_rows(y.astype(F32))
    gated = T.backward(hs, w, CM.actor_delta(mu, a, part), hidden)
    hs_c = [h[part] for h in hs]
    compact = T.backward(hs_c, w, CM.actor_delta(mu[part], a[part], np.ones(int(part.sum()), bool)), hidden)
    moved = 0
    for (gW, gb), (cW, cb) in zip(gated, compact):
        assert np.array_equal(gW, cW) and np.array_equal(gb, cb)  # (==: by value)
        moved += int((gW != 0).sum())
    assert moved > 0


def _select_direct(td, var, beta, E):
    """The rule of include/aigar.h, transcribed with math's functions."""
    count, cut = [], 0
    for x in td:
        x = float(x)
        if E == 0:
            count.append(1 if x > 0 else 0)
            continue
        var = (1.0 - beta) * var + beta * (x * x)
        if x > 0:
            q = x / math.sqrt(var) if var > 0 else math.inf
            c = math.ceil(q) if math.isfinite(q) else math.inf
            if 1 <= c <= E:
                count.append(int(c))
            else:
                count.append(E)
                cut += 1
        else:
            count.append(0)
    return count, var, cut


TDS = {"all positive": [0.5, 1.5, 2.5, 0.25, 3.0], "none positive": [-0.5, -1.5, -2.5, -1e-300],
       "a zero": [0.75, 0.0, -0.0, 1.25, -1.0], "far above E": [0.5, 1e9, 0.25, 3e300],
       "tiny": [1e-200, 5e-324, 1.0]}


@pytest.mark.parametrize("name", sorted(TDS))
@pytest.mark.parametrize("E", [0, 1, 4, 8])
def test_selection_equals_the_rule(name, E):
    td = np.array(TDS[name])
    count, var, cut = CM.select(td, 1.0, 0.001, E)
    wc, wv, wcut = _select_direct(td, 1.0, 0.001, E)
    assert count.tolist() == wc and cut == wcut
    assert M.bits(var) == M.bits(wv)
    assert ((count > 0) == (td > 0)).all()
    if E:
        assert count.max() <= E
    if name == "far above E" and E:
        assert count[1] == E and count[3] == E and cut >= 2
    if name == "none positive":
        assert not count.any() and (E == 0 or var != 1.0)  # (the variance follows every row)


def test_selection_where_c_is_exactly_an_integer():
    """beta = 0 keeps var = 4 exactly: sqrt is 2, td = 6 gives c = ceil(3.0) = 3, not 4; td = 8 gives
    exactly E = 4 and is not cut; the next float above 8 is cut."""
    td = np.array([6.0, 2.0, 8.0, np.nextafter(8.0, 9.0), np.nextafter(6.0, 7.0), -6.0])
    count, var, cut = CM.select(td, 4.0, 0.0, 4)
    assert count.tolist() == [3, 1, 4, 4, 4, 0] and cut == 1 and var == 4.0
    count, _, cut = CM.select(td, 4.0, 0.0, 3)
    assert count.tolist() == [3, 1, 3, 3, 3, 0] and cut == 3


def test_var_after_a_step_equals_the_closed_recurrence():
    """var_B = (1 - b)^B var_0 + b sum_r (1 - b)^(B - 1 - r) td_r^2, to float64 rounding, over two
    steps of a trainer; and exactly the sequential recurrence."""
    rng = np.random.default_rng(5)
    n_in, B = 6, 9
    actor, critic = M.make_weights(rng, n_in, (5, 2), hi=1), M.make_weights(rng, n_in, (4, 1), hi=1)
    tr = CM.Trainer(actor, critic, B, var_epochs=4, var_start=0.5, var_beta=0.01, critic_lr=1e-2, actor_lr=1e-2)
    var = 0.5
    for _ in range(2):
        s = M.mixed(rng, (B, n_in), hi=2).astype(np.float64)
        s2 = M.mixed(rng, (B, n_in), hi=2).astype(np.float64)
        a = np.zeros((B, 4))
        a[:, :2] = rng.random((B, 2))
        r = M.mixed(rng, (B,), lo=-4, hi=3).astype(np.float64)
        d = rng.random(B) < 0.3
        before = tr.var
        assert tr.step(s, a, r, s2, d, np.ones(B)) is not None
        td = tr.td
        closed = (1 - 0.01) ** B * before + 0.01 * sum((1 - 0.01) ** (B - 1 - k) * td[k] ** 2 for k in range(B))
        assert abs(tr.var - closed) <= 64 * np.spacing(closed)
        for x in td:
            var = (1.0 - 0.01) * var + 0.01 * (float(x) * float(x))
        assert M.bits(tr.var) == M.bits(var)
    assert tr.c.t == 2 and tr.a.t >= 1 and (tr.td > 0).any() and (tr.td <= 0).any()


def test_trainer_counters_target_copy_and_skips():
    rng = np.random.default_rng(9)
    n_in, B = 6, 8
    actor, critic = M.make_weights(rng, n_in, (5, 2), hi=1), M.make_weights(rng, n_in, (4, 1), hi=1)
    tr = CM.Trainer(actor, critic, B, var_epochs=2, target_steps=2, min_size=10, critic_lr=1e-2, actor_lr=1e-2)

    def batch(reward=None):
        s = M.mixed(rng, (B, n_in), hi=2).astype(np.float64)
        a = np.zeros((B, 4))
        a[:, :2] = rng.random((B, 2))
        r = M.mixed(rng, (B,), lo=-4, hi=3).astype(np.float64) if reward is None else reward
        return s, a, r, s.copy(), np.zeros(B, bool), np.ones(B)

    assert tr.step(*batch(), size=9) is None and tr.info() == (0, 1, 0, 0, 0, 0, 0, 0) and tr.var == 1.0
    w0 = tr.c.theta[0][0].copy()
    assert tr.step(*batch(), size=10) is not None and tr.since == 1
    assert np.array_equal(tr.target[0][0], w0)
    assert tr.step(*batch(), size=10) is not None and tr.since == 0
    assert np.array_equal(tr.target[0][0], tr.c.theta[0][0]) and not np.array_equal(w0, tr.target[0][0])
    t_a, var = tr.a.t, tr.var
    bad = np.ones(B)
    bad[3] = np.inf
    assert tr.step(*batch(bad), size=10) is None and tr.nonfinite and tr.skipped == 2
    assert (tr.c.t, tr.a.t, tr.var) == (2, t_a, var)
    # an actor epoch advances t_a once; the epochs of a step are its largest count
    assert tr.step(*batch(np.full(B, 50.0)), size=10) is not None
    assert tr.sel == B and tr.epochs == 2 and tr.a.t == t_a + 2 and tr.eskipped == 0
