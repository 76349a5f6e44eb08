"""The CNN acting network's specification (tests/conv_model.py) against libm's fmaf, against
torch's conv2d in float64 within the textbook error bound of a dot product, and the Python
side that needs no device: aigar_amd.net.cnn_spec on the reference's parameters and
cnn_weights_from_torch.  CPU only.

The bound, as tests/test_net_model.py has it for the dense layers: a chain of K fused steps
rounds K times, so |fl(sum) - sum| <= gamma_K * sum |x| |w| with gamma_K = K u / (1 - K u),
u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, §3.1), plus the bias add's
one rounding u |y|; relu is 1-Lipschitz, so the bound holds behind it.  Every layer is fed
the model's own float32 input, so the bound is per layer.  (torch's float64 result has an
error of its own, gamma_K(2^-53) of the same sum: 2^-29 of the bound, covered by the factor
1 + 2^-20.)"""
import copy

import numpy as np
import pytest

import conv_model as CM
import net_model as M
from aigar_amd import net as N

F32 = np.float32
U = 2.0 ** -24
# (side, C, convs, flattened length): the geometries tests/test_gpu_conv.py runs on the device
GEOMETRIES = [(42, 1, ((8, 4, 32), (4, 2, 64)), 576), (42, 6, ((8, 4, 32), (4, 2, 64)), 576),
              (42, 1, ((8, 4, 32), (4, 2, 64), (3, 1, 64)), 64), (84, 1, ((8, 4, 32), (4, 2, 64)), 5184),
              (5, 3, ((3, 2, 5),), 20), (7, 2, ((2, 1, 17), (3, 3, 3)), 12), (8, 1, ((8, 4, 16),), 16),
              (3, 4, ((1, 1, 64),), 576)]
IDS = ["%d-%d-%s" % (g[0], g[1], "_".join("%d.%d.%d" % c for c in g[2])) for g in GEOMETRIES]


def within(y, exact, absdot, K):
    gamma = K * U / (1 - K * U)
    return bool((np.abs(y - exact) <= (gamma * absdot + U * np.abs(y)) * (1 + 2.0 ** -20)).all())


def torch_conv(h, W, b, s):
    """The layer in float64 by torch: h [rows][H][H][Cin] (NHWC), W Keras' [k][k][Cin][F] ->
    relu(conv + b) and sum |x| |w|, both [rows][O][O][F]."""
    import torch
    import torch.nn.functional as tf
    x = torch.as_tensor(np.asarray(h, np.float64)).permute(0, 3, 1, 2)
    w = torch.as_tensor(np.asarray(W, np.float64)).permute(3, 2, 0, 1)
    y = tf.conv2d(x, w, torch.as_tensor(np.asarray(b, np.float64)), stride=s)
    a = tf.conv2d(x.abs(), w.abs(), None, stride=s)
    return torch.relu(y).permute(0, 2, 3, 1).numpy(), a.permute(0, 2, 3, 1).numpy()


def test_model_with_emulated_fma_is_the_model_with_libm_fmaf():
    rng = np.random.default_rng(1)
    convs = CM.make_convs(rng, 2, ((2, 1, 17), (3, 3, 3)))
    dense = M.make_weights(rng, 12, (5, 3))
    x = M.mixed(rng, (3, 7, 7, 2)).astype(np.float64) * (1 + 2.0 ** -40)  # (not float32 values)
    x[1, 0, 0, 0] = np.nan
    for out in ("linear", "sigmoid"):
        got, ref = CM.forward(x, convs, dense, "relu", out), CM.forward_fmaf(x, convs, dense, "relu", out)
        assert got.shape == (3, 3) and np.isnan(got[1]).all() and np.isnan(ref[1]).all()
        assert (M.bits(got[[0, 2]]) == M.bits(ref[[0, 2]])).all()
    f1, _ = CM.features(x, convs)
    f2, _ = CM.features(x, convs, M._fma_libm)
    assert f1.shape == (3, 12) and (f1.view(np.uint32) == f2.view(np.uint32)).all() and (f1[[0, 2]] != 0).any()


@pytest.mark.parametrize("side,C,convs,flat", GEOMETRIES, ids=IDS)
def test_model_is_torchs_conv2d_within_the_forward_bound(side, C, convs, flat):
    rng = np.random.default_rng(side * 10 + C)
    layers = CM.make_convs(rng, C, convs, -8, 8)
    layers = [(g, np.abs(W) if i else W, b) for i, (g, W, b) in enumerate(layers)]  # (relu leaves enough alive)
    rows = 2
    h = M.mixed(rng, (rows, side, side, C), -8, 8, 0, 0)
    assert CM.n_flat(side, convs) == flat
    cin = C
    for (k, s, F), W, b in layers:
        y = CM.conv_layer(h, ((k, s, F), W, b))
        exact, absdot = torch_conv(h, W, b, s)
        o = (h.shape[1] - k) // s + 1  # the floor
        assert y.shape == exact.shape == (rows, o, o, F)
        assert within(y.astype(np.float64), exact, absdot, k * k * cin), (k, s, F)
        assert (y > 0).any()
        h, cin = y, F
    # the flatten order: (y, x, f), Keras' Flatten on channels_last
    feat, nan_row = CM.features(np.zeros((1, side, side, C)), layers)
    assert feat.shape == (1, flat) and not nan_row.any()
    assert np.array_equal(h.reshape(rows, -1)[:, :h.shape[3]], h[:, 0, 0, :])
    assert np.array_equal(h.reshape(rows, -1)[:, -h.shape[3]:], h[:, -1, -1, :])


def test_model_kernel_layout_is_not_symmetric():
    """An asymmetric kernel on an asymmetric image in exact small integers: (ky, kx) swapped,
    or the image transposed, gives another integer."""
    x = (np.arange(5)[:, None, None] * 7 + np.arange(5)[None, :, None] * 3 + np.arange(2)[None, None, :] - 9)
    x = x.astype(np.float64)[None]
    W = (np.arange(3)[:, None, None, None] * 5 + np.arange(3)[None, :, None, None] * 2
         + np.arange(2)[None, None, :, None] * 11 + np.arange(4)[None, None, None, :] - 6).astype(F32)
    b = np.arange(4, dtype=F32)
    y = CM.conv_layer(x, ((3, 2, 4), W, b))
    exact, _ = torch_conv(x, W, b, 2)
    assert np.array_equal(y, exact)
    assert not np.array_equal(y, torch_conv(x, W.transpose(1, 0, 2, 3), b, 2)[0])
    assert not np.array_equal(y, torch_conv(x.transpose(0, 2, 1, 3), W, b, 2)[0].transpose(0, 2, 1, 3))


def test_cnn_weights_from_torch_against_the_module_in_float64():
    import torch
    torch.manual_seed(3)
    m = torch.nn.Sequential(torch.nn.Conv2d(2, 5, 3, stride=2), torch.nn.ReLU(), torch.nn.Conv2d(5, 4, 2),
                            torch.nn.ReLU(), torch.nn.Flatten(), torch.nn.Linear(36, 3))
    spec = N.CnnSpec(9, 2, ((3, 2, 5), (2, 1, 4)), 36, (3,), "relu", "linear")
    rng = np.random.default_rng(4)
    x = M.mixed(rng, (4, 9, 9, 2), -4, 4, 0, 0)
    for src in (m, m.state_dict()):
        w = N.cnn_weights_from_torch(src, spec)
        assert [a.shape for a, _ in w] == [(3, 3, 2, 5), (2, 2, 5, 4), (36, 3)]
        assert all(a.dtype == F32 and a.flags.c_contiguous and b.dtype == F32 for a, b in w)
        assert (w[0][0][1, 2, 0, 3] == m[0].weight[3, 0, 1, 2].item()) and (w[0][1] == m[0].bias.detach().numpy()).all()
        # (c, y, x) -> (y, x, c): input (y 1, x 2, c 3) of the first Linear
        assert w[2][0][(1 * 3 + 2) * 4 + 3, 1] == m[5].weight[1, 3 * 9 + 1 * 3 + 2].item()
    md = copy.deepcopy(m).double()  # the module in float64, on the same float32 weight values
    h, cin = x, 2
    for i, ((k, s, F), (W, b)) in enumerate(zip(spec.convs, w[:2])):
        y = CM.conv_layer(h, ((k, s, F), W, b))
        xt = torch.as_tensor(h.astype(np.float64)).permute(0, 3, 1, 2)
        with torch.no_grad():
            conv = md[2 * i]
            exact = torch.relu(conv(xt)).permute(0, 2, 3, 1).numpy()
            absdot = torch.nn.functional.conv2d(xt.abs(), conv.weight.abs(), None, stride=s).permute(0, 2, 3, 1).numpy()
        assert within(y.astype(np.float64), exact, absdot, k * k * cin)
        h, cin = y, F
    feat = h.reshape(4, -1)
    y = M.forward(feat, [w[2]], "relu", "linear")
    with torch.no_grad():
        flat = torch.as_tensor(h.astype(np.float64)).permute(0, 3, 1, 2).flatten(1)  # torch's (c, y, x) order
        exact = md[5](flat).numpy()
        absdot = (flat.abs() @ md[5].weight.abs().T).numpy()
    assert within(y, exact, absdot, 36)
    # the whole model on the converted weights runs, and differs from the unpermuted Linear
    convs = [(g, W, b) for g, (W, b) in zip(spec.convs, w[:2])]
    full = CM.forward(x, convs, [w[2]])
    assert np.array_equal(M.bits(full), M.bits(y))
    plain = np.ascontiguousarray(m[5].weight.detach().numpy().T)
    assert not np.array_equal(CM.forward(x, convs, [(plain, w[2][1])]), full)
    # Keras-layout lists pass through, flat or paired; a wrong shape is refused
    for src in ([a for p in w for a in p], [tuple(p) for p in w]):
        v = N.cnn_weights_from_torch(src, spec)
        assert all((a == c).all() and (b == d).all() for (a, b), (c, d) in zip(v, w))
    with pytest.raises(ValueError, match="shapes"):
        N.cnn_weights_from_torch([(w[0][0].transpose(1, 0, 3, 2), w[0][1])] + w[1:], spec)
    with pytest.raises(ValueError, match="shapes"):
        N.cnn_weights_from_torch(w[:2], spec)


class _P:
    pass


def _params(**kw):
    p = _P()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_cnn_spec_on_the_reference_defaults():
    want = N.CnnSpec(42, 1, ((8, 4, 32), (4, 2, 64)), 576, (100, 100, 25), "relu", "linear")
    assert N.cnn_spec(None, "q", 25) == want
    assert N.cnn_spec(_params(CNN_REPR=True, CNN_P_REPR=True), "q", 25) == want
    assert N.cnn_spec(None, "actor", 3) == want._replace(units=(100, 100, 3), out="sigmoid")
    p = _params(CNN_REPR=True, CNN_P_REPR=True, CNN_P_RGB=True, CNN_LAST_GRID=True, CNN_USE_L3=True, Q_LAYERS=(16,))
    assert N.cnn_spec(p, "q", 9) == N.CnnSpec(42, 6, ((8, 4, 32), (4, 2, 64), (3, 1, 64)), 64, (16, 9), "relu", "linear")
    # the image side is the first used layer's CNN_INPUT_DIM_* (rgbGenerator.py:16-21)
    p = _params(CNN_USE_L1=False, CNN_USE_L3=True, CNN_INPUT_DIM_2=20, CNN_L2=(4, 2, 8))
    assert N.cnn_spec(p, "q", 4)[:4] == (20, 1, ((4, 2, 8), (3, 1, 64)), 7 * 7 * 64)
    assert N.cnn_spec({"CNN_L1": (4, 2, 8), "CNN_L2": (2, 1, 16), "CNN_INPUT_DIM_1": 12, "Q_LAYERS": (16,)}, "q", 25) \
        == N.CnnSpec(12, 1, ((4, 2, 8), (2, 1, 16)), 256, (16, 25), "relu", "linear")


@pytest.mark.parametrize("kw, word", [
    (dict(CNN_REPR=True, CNN_P_REPR=False), "CNN_P_REPR"), (dict(CNN_REPR=True), "CNN_P_REPR"),
    (dict(CNN_P_INCEPTION=True), "CNN_P_INCEPTION"),
    (dict(CNN_USE_L1=False, CNN_USE_L2=False), "CNN_USE_L"),
    (dict(CNN_USE_L1=False), "flattened length 107584"),  # 84 x 84 with only CNN_L2: 41 * 41 * 64
    (dict(CNN_L1=(9, 4, 32)), "CNN_L1"), (dict(CNN_L2=(4, 9, 64)), "CNN_L2"), (dict(CNN_L2=(4, 2, 65)), "CNN_L2"),
    (dict(CNN_L1=(8, 4)), "CNN_L1"), (dict(CNN_USE_L3=True, CNN_L3=(4, 1, 64)), "CNN_L3"),
    (dict(CNN_INPUT_DIM_1=129), "CNN_INPUT_DIM_1"),
    (dict(ACTIVATION_FUNC_HIDDEN="elu"), "elu"), (dict(ACTIVATION_FUNC_OUTPUT="tanh"), "tanh"),
    (dict(BATCHNORM=True), "BATCHNORM"), (dict(USE_ACTION_AS_INPUT=True), "USE_ACTION_AS_INPUT"),
    (dict(NEURON_TYPE="LSTM"), "NEURON_TYPE"), (dict(Q_LAYERS=(10, 10, 10, 10, 10)), "hidden layers"),
    (dict(Q_LAYERS=(257,)), "257"),
])
def test_cnn_spec_refuses_by_name(kw, word):
    with pytest.raises(ValueError, match=word) as e:
        N.cnn_spec(_params(**kw), "q", 4)
    assert "cnn_spec" in str(e.value)
    with pytest.raises(ValueError, match="head"):
        N.cnn_spec(None, "critic", 4)


def test_mlp_spec_still_refuses_the_cnn():
    with pytest.raises(ValueError, match="CNN"):
        N.mlp_spec(_params(CNN_REPR=True, CNN_P_REPR=True), "q", n_in=12, n_out=4)
