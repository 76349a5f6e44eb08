"""The CNN training step's Python model (tests/cnn_train_model.py), checked without a device:
its vectorised fma against libm's fmaf bit for bit, its gradients against torch.autograd on a
float64 conv2d + linear network within each chain's own gamma bound, the padded-step definition
of the input error against the form that skips the invalid taps, and that the worlds of
tests/test_gpu_cnn_train.py are worth comparing.  CPU only."""
import numpy as np
import pytest

import cnn_train_cases as W
import cnn_train_model as CT
import conv_model as CM
import net_model as M
import train_model as T
from test_conv_model import U  # float32's unit roundoff, as the forward bounds have it

F32 = np.float32


def gamma(K):
    """gamma_K = K u / (1 - K u), the bound tests/test_conv_model.py and tests/test_train_model.py construct."""
    return K * U / (1 - K * U)


def _batch(rng, B, shape, n_out):
    s = M.mixed(rng, (B,) + shape, hi=3).astype(np.float64)
    s2 = M.mixed(rng, (B,) + shape, hi=3).astype(np.float64)
    a = rng.integers(0, n_out, B)
    r = M.mixed(rng, (B,), lo=-10, hi=5).astype(np.float64)
    d = rng.random(B) < 0.3
    s2[d] = np.nan
    return s, a, r, s2, d, rng.random(B) + 0.25


def test_step_with_libm_fmaf_equals_the_vectorised_step():
    rng = np.random.default_rng(1)
    cg, units, side, C, B = ((2, 1, 3), (2, 2, 2)), (3, 2), 5, 2, 3  # 5 -> 4 -> 2; column 3... all reached; tiny
    convs = CM.make_convs(rng, C, cg, lo=-30, hi=2)
    dense = M.make_weights(rng, CM.n_flat(side, cg), units, hi=2)
    a = CT.CnnTrainer(convs, dense, B, lr=1e-2, target_steps=2)
    b = CT.CnnTrainer(convs, dense, B, lr=1e-2, target_steps=2, fma=M._fma_libm)
    for _ in range(2):
        batch = _batch(rng, B, (side, side, C), units[-1])
        pa, pb = a.step(*batch), b.step(*batch)
        assert pa is not None and np.array_equal(M.bits(pa), M.bits(pb))
    for what in ("theta", "target", "m", "v"):
        for (Wa, ba), (Wb, bb) in zip(a.pairs(what), b.pairs(what)):
            assert np.array_equal(Wa.view(np.uint32), Wb.view(np.uint32))
            assert np.array_equal(ba.view(np.uint32), bb.view(np.uint32))
    assert a.t == 2 and a.since == 0
    assert all((Wn != Wo).any() for (Wn, _), (_, Wo, _) in zip(a.pairs()[:2], convs))


GEOS = [(7, 2, ((3, 2, 5), (2, 1, 4)), (6, 3)), (9, 1, ((2, 2, 3), (2, 2, 17)), (5, 2)),  # (9 -> 4 -> 2: stride = kernel)
        (10, 2, ((3, 1, 4), (4, 2, 6), (3, 1, 8)), (7, 3)), (11, 3, ((4, 2, 5), (2, 2, 6)), (4,))]  # (11 -> 4 -> 2)


@pytest.mark.parametrize("side,C,cg,units", GEOS)
def test_every_chain_is_autograds_within_its_own_bound(side, C, cg, units):
    """Chain by chain on mixed magnitudes far from under- and overflow: with the model's own
    float32 operands of a layer as float64 leaves, autograd of sum(delta_l * conv2d(h_{l-1}, W_l))
    gives the exact-operand dW_l and e_{l-1}, and of sum(delta_1 * (feat @ W0)) the feature
    error.  A chain of K fused steps rounds K times: |fl - exact| <= gamma_K sum |a||b|, with
    K = M for dW, k k F for the input error (the padded steps' products are zeros) and the unit
    count for the feature error; the bias sum of M terms rounds M - 1 times."""
    import torch
    import torch.nn.functional as tf
    rng = np.random.default_rng(side)
    B = 3
    convs = CM.make_convs(rng, C, cg, -6, 2)
    convs = [(g, np.abs(Wc) if i else Wc, b) for i, (g, Wc, b) in enumerate(convs)]  # (relu leaves enough alive)
    n_flat = CM.n_flat(side, cg)
    dense = [(M.mixed(rng, (i, o), -6, 2, 0, 0), M.mixed(rng, (o,), -6, 2, 0, 0)) for i, o in zip((n_flat,) + units, units)]
    x = M.mixed(rng, (B, side, side, C), -6, 2, 0, 0)
    hs, feat, _ = CT.features_saved(x, convs)
    dhs, q = T.forward_saved(feat, dense)
    a = rng.integers(0, units[-1], B)
    td = M.mixed(rng, (B,), -6, 2, 0, 0).astype(np.float64)
    d = T.output_delta(td, rng.random(B) + 0.25, a, units[-1])
    for l in range(len(dense) - 1, 0, -1):
        d = np.where(dhs[l] > 0, T.chain_cols(d, dense[l][0].T), F32(0.0))
    # the feature error: chains of the first dense layer's unit count
    f64 = torch.tensor(feat.astype(np.float64), requires_grad=True)
    (torch.tensor(d.astype(np.float64)) * (f64 @ torch.tensor(dense[0][0].astype(np.float64)))).sum().backward()
    e = T.chain_cols(d, dense[0][0].T)
    J = d.shape[1]
    bound = gamma(J) * (np.abs(d.astype(np.float64)) @ np.abs(dense[0][0].astype(np.float64)).T)
    assert (np.abs(e.astype(np.float64) - f64.grad.numpy()) <= bound * (1 + 2.0 ** -20)).all()
    dl = CT.feature_error(d, dense[0][0], feat).reshape(hs[-1].shape)
    assert np.array_equal(dl.reshape(B, -1) != 0, (e != 0) & (feat > 0))
    grads, deltas = CT.conv_backward(hs, convs, dl)
    nhwc = lambda t: t.permute(0, 2, 3, 1).numpy()
    for l in range(len(convs) - 1, -1, -1):
        (k, s, F), Wc, _ = convs[l]
        dl = deltas[l]
        assert (dl != 0).any(), l
        h64 = torch.tensor(hs[l].astype(np.float64)).permute(0, 3, 1, 2).requires_grad_(True)
        W64 = torch.tensor(Wc.astype(np.float64)).permute(3, 2, 0, 1).requires_grad_(True)
        d64 = torch.tensor(dl.astype(np.float64)).permute(0, 3, 1, 2)
        (d64 * tf.conv2d(h64, W64, None, stride=s)).sum().backward()
        # sum |a||b| of every chain: the same products of the absolute values
        ha = torch.tensor(np.abs(hs[l]).astype(np.float64)).permute(0, 3, 1, 2).requires_grad_(True)
        Wa = torch.tensor(np.abs(Wc).astype(np.float64)).permute(3, 2, 0, 1).requires_grad_(True)
        (d64.abs() * tf.conv2d(ha, Wa, None, stride=s)).sum().backward()
        gW, gb = grads[l]
        Mm = dl.shape[0] * dl.shape[1] * dl.shape[2]
        err = np.abs(gW.astype(np.float64) - W64.grad.permute(2, 3, 1, 0).numpy())
        assert (err <= gamma(Mm) * Wa.grad.permute(2, 3, 1, 0).numpy() * (1 + 2.0 ** -20)).all(), l
        assert (gW != 0).any()
        d2 = dl.astype(np.float64).reshape(Mm, F)
        assert (np.abs(gb.astype(np.float64) - d2.sum(0)) <= gamma(Mm - 1) * np.abs(d2).sum(0) * (1 + 2.0 ** -20)).all()
        if l:
            e = CT.conv_input_error(dl, Wc, s, hs[l].shape[1])
            err = np.abs(e.astype(np.float64) - nhwc(h64.grad))
            assert (err <= gamma(k * k * F) * nhwc(ha.grad) * (1 + 2.0 ** -20)).all(), l
            assert np.array_equal(deltas[l - 1], np.where(hs[l] > 0, e, F32(0.0)))


def test_gradients_equal_autograd_of_the_whole_network_where_float32_is_exact():
    """Small integers and a power-of-two n_out * B: every product and sum is exact in float32, so
    the model equals float64 autograd of the whole CNN's weighted mse exactly -- a transposed
    kernel, a wrong gate, a swapped (ky, kx) or a wrong flatten order shows as a wrong integer."""
    import torch
    import torch.nn.functional as tf
    rng = np.random.default_rng(3)
    side, C, cg, units, B = 7, 2, ((3, 2, 3), (2, 1, 2)), (4, 4), 8  # 7 -> 3 -> 2; n_out * B = 32
    convs, cin = [], C
    for k, s, F in cg:
        convs.append(((k, s, F), rng.integers(-2, 3, (k, k, cin, F)).astype(F32), rng.integers(-1, 2, F).astype(F32)))
        cin = F
    sizes = (CM.n_flat(side, cg),) + units
    dense = [(rng.integers(-2, 3, (sizes[l], sizes[l + 1])).astype(F32), rng.integers(-1, 2, sizes[l + 1]).astype(F32))
             for l in range(2)]
    x = rng.integers(-2, 3, (B, side, side, C)).astype(np.float64)
    a = rng.integers(0, 4, B)
    wt = np.ldexp(1.0, rng.integers(-1, 2, B))
    hs, feat, _ = CT.features_saved(x, convs)
    dhs, q = T.forward_saved(feat, dense)
    target = rng.integers(-50, 50, B).astype(np.float64)
    td = target - q[np.arange(B), a]
    delta = T.output_delta(td, wt, a, 4)
    dgr = T.backward(dhs, dense, delta)
    d1 = np.where(dhs[1] > 0, T.chain_cols(delta, dense[1][0].T), F32(0.0))
    cgr, _ = CT.conv_backward(hs, convs, CT.feature_error(d1, dense[0][0], feat).reshape(hs[-1].shape))
    # torch, float64
    cw = [(torch.tensor(Wc.astype(np.float64)).permute(3, 2, 0, 1).requires_grad_(True),
           torch.tensor(b.astype(np.float64), requires_grad=True)) for _, Wc, b in convs]
    dw = [(torch.tensor(Wd.astype(np.float64), requires_grad=True), torch.tensor(b.astype(np.float64), requires_grad=True))
          for Wd, b in dense]
    h = torch.tensor(x).permute(0, 3, 1, 2)
    for ((k, s, F), _, _), (Wt, bt) in zip(convs, cw):
        h = torch.relu(tf.conv2d(h, Wt, bt, stride=s))
    h = h.permute(0, 2, 3, 1).reshape(B, -1)  # (y, x, f)
    h = torch.relu(h @ dw[0][0] + dw[0][1]) @ dw[1][0] + dw[1][1]
    assert np.array_equal(h.detach().numpy(), q)
    tgt = h.detach().clone()
    tgt[np.arange(B), a] = torch.tensor(target)
    (torch.tensor(wt) * ((h - tgt) ** 2).mean(dim=1)).mean().backward()
    nonzero = 0
    for (gW, gb), (Wt, bt) in zip(cgr, cw):
        assert np.array_equal(gW.astype(np.float64), Wt.grad.permute(2, 3, 1, 0).numpy())
        assert np.array_equal(gb.astype(np.float64), bt.grad.numpy())
        nonzero += int((gW != 0).sum())
    for (gW, gb), (Wt, bt) in zip(dgr, dw):
        assert np.array_equal(gW.astype(np.float64), Wt.grad.numpy()) and np.array_equal(gb.astype(np.float64), bt.grad.numpy())
    assert nonzero > 20


@pytest.mark.parametrize("geo", ["b", "c", "d"])
def test_padded_steps_equal_skipped_taps_as_numbers(geo):
    """The contract executes the steps at taps whose window position does not exist (x = -0.0f);
    skipping them gives the same numbers (== , not by bits: a chain that sits at -0.0f by
    underflow goes to +0.0f under a padded step) on the test geometries."""
    side, C, cg, _ = W.GEOMETRIES[geo]
    rng = np.random.default_rng(5)
    B, H = 2, CM.out_side(side, cg[0][0], cg[0][1])
    cin = cg[0][2]
    for k, s, F in cg[1:]:
        O = CM.out_side(H, k, s)
        d = M.mixed(rng, (B, O, O, F), hi=2)
        Wc = M.mixed(rng, (k, k, cin, F), hi=2)
        e, e2 = CT.conv_input_error(d, Wc, s, H), CT.conv_input_error_skip(d, Wc, s, H)
        assert e.shape == (B, H, H, cin) and (e == e2).all() and (e != 0).any()
        reach = s * (O - 1) + k  # positions at and beyond it are reached by no window
        assert (e.view(np.uint32)[:, reach:] == 0).all() and (e.view(np.uint32)[:, :, reach:] == 0).all()
        H, cin = O, F
    if geo == "b":
        assert reach == 4 and e.shape[1] == 5  # (the row and column that get +0.0f)


@pytest.mark.parametrize("geo", sorted(W.GEOMETRIES))
def test_the_gpu_tests_worlds_are_worth_comparing(geo):
    """For every geometry of tests/test_gpu_cnn_train.py, on its own weights and transitions: some
    relu gate of every conv layer is closed and some is open, where the error that meets it is
    not zero, and every filter gradient has more than a handful of distinct nonzero values."""
    convs, dense, (s, a, r, s2, d) = W.world(geo, seed=0)
    B = W.BATCHES[geo]
    tr = CT.CnnTrainer(convs, dense, B, **W.KW)
    assert tr.step(s[:B], a[:B, 0], r[:B], s2[:B], d[:B].astype(bool), np.ones(B)) is not None
    hs, feat, nan_row = CT.features_saved(s[:B], convs)
    assert not nan_row.any()
    for l, dl in enumerate(tr.deltas):
        act = hs[l + 1]
        assert (act > 0).any() and (act == 0).any(), l
        assert (dl != 0).any() and ((dl == 0) & (act == 0)).any(), l
        gW, gb = tr.grads[0][l]
        assert len(np.unique(gW[gW != 0])) > 8, (l, len(np.unique(gW[gW != 0])))
        assert (gb != 0).any(), l
