"""The acting network's specification (tests/net_model.py) against libm's fmaf and the
textbook error bound of a dot product, and the Python side that needs no device:
aigar_amd.net.mlp_spec on the reference's parameters and weights_from_torch.  CPU only."""
import math

import numpy as np
import pytest

import net_model as M
from aigar_amd import net as N

F32 = np.float32


def _operands(n, seed):
    """Triples that stress an fma: mixed magnitudes, exact cancellation, halfway cases of the
    float32 rounding, subnormal operands and results."""
    rng = np.random.default_rng(seed)
    a, b, c = M.mixed(rng, n, -60, 40), M.mixed(rng, n, -60, 40), M.mixed(rng, n, -100, 80)
    q = n // 5
    # cancellation: c = -(a * b) rounded, so the sum is the product's rounding error
    c[:q] = -(a[:q].astype(np.float64) * b[:q].astype(np.float64)).astype(F32)
    # halfway: a * b = 1 + 2^-24 + small or exactly 1 + 2^-24 (ties), c nudges it
    a[q:2 * q] = F32(1.0) + F32(2.0 ** -12)
    b[q:2 * q] = F32(1.0) + F32(2.0 ** -12) * rng.integers(-3, 4, q).astype(F32)
    c[q:2 * q] = np.ldexp(rng.integers(-4, 5, q).astype(np.float64), rng.integers(-75, -40, q)).astype(F32)
    # subnormal results
    a[2 * q:3 * q] = M.mixed(rng, q, -80, -60)
    b[2 * q:3 * q] = M.mixed(rng, q, -80, -60)
    c[2 * q:3 * q] = np.ldexp(rng.integers(-9, 10, q).astype(np.float64), -149).astype(F32)
    return a, b, c


def test_emulated_fma_is_libm_fmaf():
    a, b, c = _operands(120000, 1)
    got = M.fma32(a, b, c)
    ref = np.array([M.fmaf(x, y, z) for x, y, z in zip(a, b, c)], F32)
    bad = np.nonzero(got.view(np.uint32) != ref.view(np.uint32))[0]
    assert len(bad) == 0, (len(bad), a[bad[:3]], b[bad[:3]], c[bad[:3]], got[bad[:3]], ref[bad[:3]])
    # the cases that tell an fma from a rounded float64 multiply-add are among them
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)
    assert (naive.view(np.uint32) != ref.view(np.uint32)).sum() > 0


def test_model_fma_is_exact_float32_fma():
    # 1 + 2^-12 squared is 1 + 2^-11 + 2^-24: the tie is broken by c, which a float64
    # multiply-add rounded twice cannot see
    a = F32(1.0) + F32(2.0 ** -12)
    for c, want in ((F32(2.0 ** -60), 1.0 + 2.0 ** -11 + 2.0 ** -23), (F32(-2.0 ** -60), 1.0 + 2.0 ** -11)):
        assert float(M.fmaf(a, a, c)) == want
        assert float(M.fma32(a, a, c)) == want
    assert math.copysign(1.0, float(M.fmaf(F32(-2.0 ** -100), F32(2.0 ** -100), F32(0.0)))) == -1.0


def test_forward_vectorised_equals_forward_libm():
    rng = np.random.default_rng(2)
    for n_in, units, hidden, out in ((1, (1,), "relu", "linear"), (5, (3,), "relu", "sigmoid"),
                                      (33, (7, 2), "relu", "linear"), (12, (3, 5, 4), "linear", "sigmoid")):
        w = M.make_weights(rng, n_in, units)
        x = M.mixed(rng, (9, n_in)).astype(np.float64) * (1 + 2.0 ** -40)  # (not float32 values)
        x[4, 0] = np.nan
        got, ref = M.forward(x, w, hidden, out), M.forward_libm(x, w, hidden, out)
        assert np.isnan(got[4]).all() and np.isnan(ref[4]).all()
        keep = np.arange(9) != 4
        assert (M.bits(got[keep]) == M.bits(ref[keep])).all()


def test_model_is_a_dot_product_within_the_forward_bound():
    # |fl(sum) - sum| <= gamma_K * sum |x_k| |w_k| for K fused steps (each fma rounds once:
    # K roundings), plus the bias add's one rounding 2^-24 |y|; u = 2^-24.  (Higham, Accuracy
    # and Stability of Numerical Algorithms, §3.1.)  Magnitudes stay far from under- and overflow.
    rng = np.random.default_rng(3)
    K, n = 365, 40
    x = M.mixed(rng, (17, K), -8, 8, 0, 0)
    W, b = M.mixed(rng, (K, n), -8, 8, 0, 0), M.mixed(rng, (n,), -8, 8, 0, 0)
    y = M.forward(x, [(W, b)], "relu", "linear")
    x64, W64 = x.astype(np.float64), W.astype(np.float64)
    exact = x64 @ W64 + b.astype(np.float64)
    u = 2.0 ** -24
    gamma = K * u / (1 - K * u)
    bound = gamma * (np.abs(x64) @ np.abs(W64)) + u * np.abs(y)
    # (the float64 matmul's own error, gamma_K(2^-53) relative to the same sum, is 2^-29 of the bound)
    assert (np.abs(y - exact) <= bound * (1 + 2.0 ** -20)).all()
    assert (np.abs(y - exact) > 0).any()


def test_acc_is_plus_zero_after_exact_cancellation_and_minus_zero_only_by_underflow():
    rng = np.random.default_rng(4)
    K = 64
    # 11-bit mantissas: every product is exact in float32, so x_2i w + (-x_2i) w cancels exactly
    short = lambda shape: np.ldexp(rng.integers(1, 2048, shape) * rng.choice([-1.0, 1.0], shape),
                                   rng.integers(-20, 20, shape)).astype(F32)
    x = short((8, K))
    x[:, 1::2] = -x[:, 0::2]
    W = np.repeat(short((K // 2, 6)), 2, axis=0)  # w_2i == w_2i+1
    for fma in (M.fma32, M._fma_libm):
        acc = M.layer_acc(x, W, fma)
        assert (acc.view(np.uint32) == 0).all()  # +0.0f, never -0.0f
    # all-negative-zero products too: +0 + (-0) is +0 in round to nearest
    acc = M.layer_acc(np.full((1, 4), -0.0, F32), np.ones((4, 1), F32))
    assert acc.view(np.uint32)[0, 0] == 0
    # the one way to -0.0f is underflow; the device's k padding (x = -0.0f against w = +0.0f, a
    # product of -0.0f) keeps it, where a +0 product would turn it into +0.0f
    acc = M.layer_acc(np.array([[-2.0 ** -100]], F32), np.array([[2.0 ** -100]], F32))
    assert acc.view(np.uint32)[0, 0] == 0x80000000
    assert M.fmaf(F32(-0.0), F32(0.0), acc[0, 0]).view(np.uint32) == 0x80000000
    assert M.fmaf(F32(0.0), F32(0.0), acc[0, 0]).view(np.uint32) == 0
    for v in (F32(0.0), F32(1.5), F32(-3e-40)):
        assert M.fmaf(F32(-0.0), F32(0.0), v).view(np.uint32) == v.view(np.uint32)


def test_sigmoid_endpoints():
    s = M.sigmoid64
    assert s(0.0) == 0.5 and s(-0.0) == 0.5
    assert s(750.0) == 1.0 and s(3e38) == 1.0 and s(800.0) == 1.0
    tiny = math.e ** -750.0
    assert tiny == 0.0 or tiny < 5e-324 * 2  # (pow underflows: the clamp keeps pow's argument in its checked range)
    assert s(-750.0) == tiny / (1.0 + tiny) and s(-3e38) == s(-750.0) and s(-800.0) == s(-750.0)
    assert s(-745.0) > 0.0 and s(-745.0) == math.e ** -745.0 / (1.0 + math.e ** -745.0)
    assert s(1e-30) == 0.5 and 0.5 < s(1e-3) < s(1.0) < 1.0 and s(-1.0) + s(1.0) == pytest.approx(1.0, abs=2e-16)
    assert s(-1.0) == math.e ** -1.0 / (1.0 + math.e ** -1.0)


class _P:
    pass


def _params(**kw):
    p = _P()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_mlp_spec_on_the_reference_defaults():
    assert N.mlp_spec(None, "q", n_in=365, n_out=25) == N.NetSpec(365, (100, 100, 25), "relu", "linear")
    assert N.mlp_spec(None, "actor", n_in=365, n_out=3) == N.NetSpec(365, (100, 100, 3), "relu", "sigmoid")
    p = _params(Q_LAYERS=(3, 0, 5), ACTIVATION_FUNC_HIDDEN="linear", ALGORITHM="DPG", DPG_ACTOR_LAYERS=(7,),
                CACLA_ACTOR_LAYERS=(9, 9), DROPOUT=0.5)
    assert N.mlp_spec(p, "q", n_in=12, n_out=4) == N.NetSpec(12, (3, 5, 4), "linear", "linear")  # (the 0 is skipped)
    assert N.mlp_spec(p, "actor", n_in=12, n_out=2).units == (7, 2)
    assert N.mlp_spec(_params(ALGORITHM="CACLA", CACLA_ACTOR_LAYERS=(9, 9)), "actor").units == (9, 9)
    assert N.mlp_spec({"Q_LAYERS": ()}, "q", n_in=5, n_out=3).units == (3,)


@pytest.mark.parametrize("kw, word", [
    (dict(ACTIVATION_FUNC_HIDDEN="elu"), "elu"), (dict(ACTIVATION_FUNC_HIDDEN="tanh"), "tanh"),
    (dict(ACTIVATION_FUNC_OUTPUT="tanh"), "tanh"), (dict(BATCHNORM=True), "BATCHNORM"),
    (dict(USE_ACTION_AS_INPUT=True), "USE_ACTION_AS_INPUT"), (dict(NEURON_TYPE="LSTM"), "NEURON_TYPE"),
    (dict(CNN_REPR=True), "CNN"), (dict(Q_LAYERS=(10, 10, 10, 10, 10)), "hidden layers"),
    (dict(Q_LAYERS=(257,)), "257"),
])
def test_mlp_spec_refuses_what_the_device_cannot_evaluate(kw, word):
    with pytest.raises(ValueError, match=word):
        N.mlp_spec(_params(**kw), "q", n_in=12, n_out=4)


def test_mlp_spec_refuses_the_actor_settings_too():
    with pytest.raises(ValueError, match="elu"):
        N.mlp_spec(_params(ACTIVATION_FUNC_HIDDEN_POLICY="elu"), "actor")
    with pytest.raises(ValueError, match="head"):
        N.mlp_spec(None, "critic")
    with pytest.raises(ValueError, match="16385"):
        N.mlp_spec(None, "q", n_in=16385, n_out=4)


def test_weights_from_torch_transposes_linear_layers():
    import torch
    m = torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.ReLU(), torch.nn.Linear(2, 4))
    with torch.no_grad():
        m[0].weight.copy_(torch.tensor([[1., 2., 3.], [4., 5., 6.]]))  # [out][in], asymmetric
        m[0].bias.copy_(torch.tensor([7., 8.]))
    for src in (m, m.state_dict()):
        w = N.weights_from_torch(src)
        assert [a.shape for a, _ in w] == [(3, 2), (2, 4)] and all(a.dtype == F32 and a.flags.c_contiguous for a, _ in w)
        assert w[0][0].tolist() == [[1., 4.], [2., 5.], [3., 6.]] and w[0][1].tolist() == [7., 8.]
        assert (w[1][0] == m[2].weight.detach().numpy().T).all()
    # Keras-layout lists pass through, flat or paired
    W0, b0 = np.arange(6, dtype=np.float64).reshape(3, 2), np.array([1., 2.])
    for src in ([W0, b0], [(W0, b0)]):
        w = N.weights_from_torch(src)
        assert w[0][0].dtype == F32 and (w[0][0] == W0).all() and (w[0][1] == b0).all()
    with pytest.raises(ValueError):
        N.weights_from_torch([W0.T, b0])
