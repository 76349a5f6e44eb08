"""The training step's Python model (tests/train_model.py), checked without a device: its
vectorised fma against libm's fmaf bit for bit, its gradients against torch.autograd in
float64, its Adam against torch.optim.Adam, the padding facts the kernels rely on, the target
copy and the skip rule.  CPU only."""
import math

import numpy as np
import pytest

import net_model as M
import train_model as T

F32 = np.float32
U = 2.0 ** -24  # float32's unit roundoff


def _weights(rng, n_in, units, lo, hi, p_sub=0.02):
    sizes = [n_in] + list(units)
    return [(M.mixed(rng, (sizes[l], sizes[l + 1]), lo=lo, hi=hi, p_sub=p_sub),
             M.mixed(rng, (sizes[l + 1],), lo=lo, hi=hi, p_sub=p_sub))
            for l in range(len(units))]


def _batch(rng, B, n_in, n_out, hi=3, lo=-30, p_sub=0.02):
    s = M.mixed(rng, (B, n_in), lo=lo, hi=hi, p_sub=p_sub).astype(np.float64)
    s2 = M.mixed(rng, (B, n_in), hi=hi).astype(np.float64)
    a = rng.integers(0, n_out, B)
    r = M.mixed(rng, (B,), lo=-10, hi=5).astype(np.float64)
    d = rng.random(B) < 0.3
    w = rng.random(B) + 0.25
    return s, a, r, s2, d, w


@pytest.mark.parametrize("n_in,units,hidden,B", [(1, (1,), "relu", 1), (5, (3, 4), "relu", 5), (7, (4, 3, 2), "linear", 6),
                                                 (9, (6, 5), "relu", 9)])
def test_step_with_libm_fmaf_equals_the_vectorised_step(n_in, units, hidden, B):
    rng = np.random.default_rng(n_in)
    w = M.make_weights(rng, n_in, units, hi=2)
    a = T.Trainer(w, B, hidden=hidden, lr=1e-2, target_steps=2)
    b = T.Trainer(w, B, hidden=hidden, lr=1e-2, target_steps=2, fma=M._fma_libm)
    for _ in range(3):
        batch = _batch(rng, B, n_in, units[-1])
        pa, pb = a.step(*batch), b.step(*batch)
        assert pa is not None and np.array_equal(M.bits(pa), M.bits(pb))
    for x, y in ((a.theta, b.theta), (a.target, b.target), (a.m, b.m), (a.v, b.v)):
        for (W, bb), (W2, b2) in zip(x, y):
            assert np.array_equal(W.view(np.uint32), W2.view(np.uint32))
            assert np.array_equal(bb.view(np.uint32), b2.view(np.uint32))
    assert a.t == 3 and a.since == 1


def _torch_loss_grads(weights, s, a, target, w, hidden):
    """mean_r w_r mean_j (q - target)^2 in float64 with autograd; target = q except in column a."""
    import torch
    ps = [(torch.tensor(W.astype(np.float64), requires_grad=True), torch.tensor(b.astype(np.float64), requires_grad=True))
          for W, b in weights]
    h = torch.tensor(np.asarray(s, np.float64))
    for l, (W, b) in enumerate(ps):
        h = h @ W + b
        if l + 1 < len(ps) and hidden == "relu":
            h = torch.relu(h)
    tgt = h.detach().clone()
    tgt[np.arange(len(a)), a] = torch.tensor(target)
    loss = (torch.tensor(w) * ((h - tgt) ** 2).mean(dim=1)).mean()
    loss.backward()
    return [(W.grad.numpy(), b.grad.numpy()) for W, b in ps], h.detach().numpy()


@pytest.mark.parametrize("hidden", ["relu", "linear"])
def test_gradients_equal_autograd_where_float32_is_exact(hidden):
    """Small integers and a power-of-two n_out * B: every product, sum and the output delta
    are exact in float32, so each chain's bound gamma_K sum |a||b| multiplies a rounding error
    of zero and the model must equal float64 autograd exactly -- a transposed operand, a wrong
    gate or a wrong scale shows as a wrong integer."""
    rng = np.random.default_rng(3)
    n_in, units, B = 5, (6, 3, 4), 8  # n_out * B = 32
    sizes = (n_in,) + units
    w = [(rng.integers(-3, 4, (sizes[l], sizes[l + 1])).astype(F32), rng.integers(-2, 3, sizes[l + 1]).astype(F32))
         for l in range(3)]
    s = rng.integers(-4, 5, (B, n_in)).astype(np.float64)
    a = rng.integers(0, 4, B)
    wt = np.ldexp(1.0, rng.integers(-1, 2, B))
    hs, q = T.forward_saved(s, w, hidden)
    target = rng.integers(-50, 50, B).astype(np.float64)
    td = target - q[np.arange(B), a]
    grads = T.backward(hs, w, T.output_delta(td, wt, a, 4), hidden)
    want, q64 = _torch_loss_grads(w, s, a, target, wt, hidden)
    assert np.array_equal(q64, q)
    nonzero = 0
    for (gW, gb), (tW, tb) in zip(grads, want):
        assert np.array_equal(gW.astype(np.float64), tW) and np.array_equal(gb.astype(np.float64), tb)
        nonzero += int((gW != 0).sum())
    assert nonzero > 20


@pytest.mark.parametrize("hidden", ["relu", "linear"])
def test_every_chain_is_autograds_dot_product_within_its_forward_bound(hidden):
    """Chain by chain on mixed magnitudes: with the model's own float32 operands of a layer
    (h_{l-1}, delta_l, W_l) as float64 leaves, autograd of sum(delta_l * (h_{l-1} W_l)) gives
    the exact-operand dW_l = h^T delta and e = delta W^T.  A chain of K fused steps rounds K
    times: |fl - exact| <= gamma_K sum_k |a_k||b_k|, gamma_K = K u / (1 - K u) (Higham §3.1);
    the bias sum of B terms rounds B - 1 times.  The float64 reference's own error is
    gamma_K(2^-53) of the same sum, 2^-29 of the bound.  Magnitudes stay far from under- and
    overflow (no subnormal operands), which the relative bound does not cover."""
    import torch
    rng = np.random.default_rng(5)
    n_in, units, B = 37, (19, 23, 6), 21
    w = _weights(rng, n_in, units, -6, 2, p_sub=0)
    s, a, r, s2, d, wt = _batch(rng, B, n_in, 6, hi=2, lo=-6, p_sub=0)
    hs, q = T.forward_saved(s, w, hidden)
    td = r - q[np.arange(B), a]
    delta = T.output_delta(td, wt, a, 6)
    grads = T.backward(hs, w, delta, hidden)
    dl = delta
    for l in (2, 1, 0):
        W64 = torch.tensor(w[l][0].astype(np.float64), requires_grad=True)
        h64 = torch.tensor(hs[l].astype(np.float64), requires_grad=True)
        d64 = torch.tensor(dl.astype(np.float64))
        (d64 * (h64 @ W64)).sum().backward()
        gW, gb = grads[l]
        gam = B * U / (1 - B * U)
        bound = gam * (np.abs(hs[l].astype(np.float64)).T @ np.abs(dl.astype(np.float64)))
        err = np.abs(gW.astype(np.float64) - W64.grad.numpy())
        assert (err <= bound * (1 + 2.0 ** -20)).all(), l
        assert (err > 0).any() or l == 2
        gamb = (B - 1) * U / (1 - (B - 1) * U)
        assert (np.abs(gb.astype(np.float64) - dl.astype(np.float64).sum(0)) <= gamb * np.abs(dl.astype(np.float64)).sum(0)
                * (1 + 2.0 ** -20)).all()
        if l:
            J = dl.shape[1]
            e = T.chain_cols(dl, w[l][0].T)
            gam = J * U / (1 - J * U)
            bound = gam * (np.abs(dl.astype(np.float64)) @ np.abs(w[l][0].astype(np.float64)).T)
            assert (np.abs(e.astype(np.float64) - h64.grad.numpy()) <= bound * (1 + 2.0 ** -20)).all(), l
            dl = np.where(hs[l] > 0, e, F32(0.0)) if hidden == "relu" else e
    assert (dl != 0).any()


def _ulp32(p):
    return np.spacing(np.abs(np.asarray(p, F32))).astype(np.float64)


def test_adam_first_step_is_torch_adam_within_one_ulp():
    """torch.optim.Adam(eps=1e-7) on float64 tensors, one step from zero state.  torch adds
    eps to sqrt(v_hat), Keras 2.2.4 to sqrt(v): after one step the two updates are
    lr g / (|g| + eps) and lr g / (|g| + eps / sqrt(1 - beta2)), which differ by less than
    lr eps / (sqrt(1 - beta2) |g|) <= 1e-4 * 3.2e-6 * 2^6 < 2.1e-8 for |g| >= 2^-6 -- under a
    fifth of the float32 ulp of a parameter in [1, 2), 1.19e-7.  The model rounds m, v
    (relative 2^-24 each: 2^-23 of an update of at most 1e-4) and p once (half an ulp), float32(torch's
    value) another half: one ulp in all."""
    import torch
    rng = np.random.default_rng(7)
    n = 4000
    p = (1.0 + rng.random(n)).astype(F32)
    g = (np.ldexp(1.0 + rng.random(n), rng.integers(-6, 6, n)) * rng.choice([-1.0, 1.0], n)).astype(F32)
    tp = torch.tensor(p.astype(np.float64), requires_grad=True)
    opt = torch.optim.Adam([tp], lr=1e-4, betas=(0.9, 0.999), eps=1e-7)
    tp.grad = torch.tensor(g.astype(np.float64))
    opt.step()
    z = np.zeros(n, F32)
    got, m, v = T.adam(p, g, z, z, T.adam_lr_t(1e-4, 0.9, 0.999, 1), 0.9, 0.999, 1e-7)
    want = tp.detach().numpy().astype(F32)
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= _ulp32(p)).all()
    assert (got != p).all() and m.dtype == v.dtype == F32


def test_adam_with_the_models_gradients_and_the_equalised_epsilon():
    """The model's own gradients, of every magnitude: torch's Adam with eps / sqrt(1 - beta2) is
    Keras' formula after one step, so the one-ulp margin holds with no condition on |g|."""
    import torch
    rng = np.random.default_rng(8)
    n_in, units, B = 12, (9, 5), 7
    w = _weights(rng, n_in, units, -3, 1)
    tr = T.Trainer(w, B, lr=1e-4)
    assert tr.step(*_batch(rng, B, n_in, 5)) is not None
    for l, ((W, b), (gW, gb)) in enumerate(zip(w, tr.grads)):
        for p, g, got in ((W, gW, tr.theta[l][0]), (b, gb, tr.theta[l][1])):
            tp = torch.tensor(p.astype(np.float64), requires_grad=True)
            opt = torch.optim.Adam([tp], lr=1e-4, betas=(0.9, 0.999), eps=1e-7 / math.sqrt(1 - 0.999))
            tp.grad = torch.tensor(g.astype(np.float64))
            opt.step()
            want = tp.detach().numpy().astype(F32)
            margin = np.maximum(_ulp32(p), _ulp32(want))
            assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= margin).all(), l


def test_adam_rounds_every_operation_on_its_own():
    # one parameter by hand, in Python floats: the model's order of operations is the contract's
    p, g, m, v = F32(0.3), F32(-1.7e-3), F32(2.5e-4), F32(9e-7)
    lr_t = T.adam_lr_t(1e-4, 0.9, 0.999, 5)
    assert lr_t == 1e-4 * math.sqrt(1.0 - math.pow(0.999, 5)) / (1.0 - math.pow(0.9, 5))
    mn = F32(0.9 * float(m) + (1.0 - 0.9) * float(g))
    vn = F32(0.999 * float(v) + (1.0 - 0.999) * (float(g) * float(g)))
    pn = F32(float(p) - lr_t * float(mn) / (math.sqrt(float(vn)) + 1e-7))
    got = T.adam(np.array([p]), np.array([g]), np.array([m]), np.array([v]), lr_t, 0.9, 0.999, 1e-7)
    assert (got[0][0], got[1][0], got[2][0]) == (pn, mn, vn)


def test_row_padding_with_minus_zero_products_is_an_identity_and_plus_zero_is_not():
    """The gradient's chain runs over the batch rows padded up to the MFMA step: a padded row
    enters as h = -0.0f against delta = +0.0f.  acc + (-0.0f) == acc for every acc; a chain
    reaches -0.0f only by underflow, and there a +0.0f product would turn it into +0.0f."""
    rng = np.random.default_rng(9)
    for acc in [F32(-0.0), F32(0.0), F32(1.5), F32(-2.0 ** -140)] + list(M.mixed(rng, (50,))):
        got = M.fmaf(F32(-0.0), F32(0.0), acc)
        assert got.view(np.uint32) == np.asarray(acc, F32).view(np.uint32)
    under = M.fmaf(F32(-2.0 ** -100), F32(2.0 ** -100), F32(0.0))
    assert under == 0 and np.signbit(under)
    assert not np.signbit(M.fmaf(F32(0.0), F32(0.0), under))  # +0.0f products are no identity
    assert np.signbit(M.fmaf(F32(-0.0), F32(0.0), under))
    # the whole chain: B = 5 rows padded to 8
    h = np.array([[-2.0 ** -100], [-0.0], [0.0], [-0.0], [-0.0]], F32)  # every product is -0.0f
    d = np.array([[2.0 ** -100], [1.0], [-3.0], [0.0], [2.0]], F32)
    plain = T.chain_cols(h.T, d)
    pad_h, pad_d = np.vstack([h, np.full((3, 1), -0.0, F32)]), np.vstack([d, np.zeros((3, 1), F32)])
    assert np.signbit(plain[0, 0]) and np.signbit(T.chain_cols(pad_h.T, pad_d)[0, 0])
    assert not np.signbit(T.chain_cols(np.vstack([h, np.zeros((3, 1), F32)]).T, pad_d)[0, 0])


def test_target_copy_at_multiples_of_target_steps_and_never_at_zero():
    rng = np.random.default_rng(10)
    w = M.make_weights(rng, 4, (3, 2), hi=1)
    tr = T.Trainer(w, 3, lr=1e-2, target_steps=2)
    never = T.Trainer(w, 3, lr=1e-2, target_steps=0)
    snaps = []
    for k in range(4):
        batch = _batch(rng, 3, 4, 2)
        tr.step(*batch)
        never.step(*batch)
        snaps.append(tr.theta[0][0].copy())
        want = w[0][0] if k == 0 else snaps[1] if k < 3 else snaps[3]
        assert np.array_equal(tr.target[0][0], want), k
        assert tr.since == (k + 1) % 2
    assert np.array_equal(never.target[0][0], w[0][0]) and never.since == 4
    assert not np.array_equal(never.theta[0][0], w[0][0])


def test_skip_rule_and_nonfinite_td():
    rng = np.random.default_rng(11)
    w = M.make_weights(rng, 4, (3, 2), hi=1)
    tr = T.Trainer(w, 3, min_size=10)
    batch = _batch(rng, 3, 4, 2)
    assert tr.step(*batch, size=9) is None and tr.step(*batch, size=2) is None
    assert (tr.t, tr.skipped, tr.nonfinite) == (0, 2, False)
    assert T.Trainer(w, 12, min_size=10).can_draw(11) is False  # below the batch
    assert tr.step(*batch, size=10) is not None and tr.t == 1
    before = [W.copy() for W, _ in tr.theta]
    s, a, r, s2, d, wt = batch
    r = r.copy()
    r[1] = np.nan
    assert tr.step(s, a, r, s2, d, wt, size=10) is None
    assert (tr.t, tr.skipped, tr.nonfinite) == (1, 3, True)
    assert all(np.array_equal(W, B) for (W, _), B in zip(tr.theta, before))
    # a done row's s2 is not evaluated: a NaN there is no NaN in the step
    d2 = np.array([True, False, False])
    s2n = s2.copy()
    s2n[0] = np.nan
    tr2 = T.Trainer(w, 3)
    assert tr2.step(s, a, batch[2], s2n, d2, wt) is not None and np.isfinite(tr2.td).all()
    assert tr2.td[0] == batch[2][0] - T.forward_saved(s, w)[1][0, a[0]]
