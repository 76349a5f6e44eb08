"""The CNN learners' acting network in plain Python: the specification of aigar_net_forward
with a conv part (include/aigar.h aigar_net_config_cnn), an extension of
tests/net_model.py, checked against libm's fmaf and torch's conv2d (tests/test_conv_model.py)
and compared bit for bit with the device (tests/test_gpu_conv.py).

An image is x [side][side][C], each value rounded once to float32.  A conv layer is
((k, s, F), W [k][k][Cin][F], b [F]) in float32, Keras' layout, valid padding: the output
side is (in - k) // s + 1.  One output (oy, ox, f): acc = +0.0f,
acc = fmaf(x[oy s + ky][ox s + kx][c], W[ky][kx][c][f], acc) as ONE chain in ascending order
of the flattened index (ky k + kx) Cin + c, then acc + b[f] as one float32 add, then relu
(y > 0 ? y : +0.0f).  The last conv layer's output, flattened in (y, x, f) order (Keras'
Flatten on channels_last), is the dense model's float32 input row (net_model.forward).  A
sample whose first image value is a NaN is not evaluated: its output row is NaN."""
import numpy as np

import net_model as M
from net_model import F32, fma32, forward_libm  # noqa: F401  (the definition this one extends)


def out_side(side, k, s):
    return (side - k) // s + 1


def conv_acc(x, W, s, fma=fma32):
    """The layer sums before the bias: x [rows][H][H][Cin] float32, W [k][k][Cin][F] ->
    acc [rows][O][O][F], every output's chain in ascending (ky, kx, c)."""
    x, W = np.asarray(x, F32), np.asarray(W, F32)
    k, cin, F = W.shape[0], W.shape[2], W.shape[3]
    assert W.shape[1] == k and x.shape[3] == cin and x.shape[1] == x.shape[2]
    o = out_side(x.shape[1], k, s)
    acc = np.zeros((x.shape[0], o, o, F), F32)  # +0.0f
    span = s * (o - 1) + 1
    for ky in range(k):
        for kx in range(k):
            for c in range(cin):
                patch = x[:, ky:ky + span:s, kx:kx + span:s, c]
                acc = fma(patch[..., None], W[ky, kx, c][None, None, None, :], acc)
    return acc


def conv_layer(h, layer, fma=fma32):
    (k, s, F), W, b = layer
    assert np.shape(W)[0] == k and np.shape(W)[3] == F
    with np.errstate(all="ignore"):
        y = conv_acc(h, W, s, fma) + np.asarray(b, F32)[None, None, None, :]  # one float32 add
    return np.where(y > 0, y, F32(0.0))


def features(x, convs, fma=fma32):
    """x [rows][side][side][C] float64 / float32 -> the flattened float32 feature rows
    [rows][n_flat] in (y, x, f) order, and which samples are NaN samples."""
    x = np.asarray(x)
    nan_row = np.isnan(x[:, 0, 0, 0])
    with np.errstate(all="ignore"):
        h = np.where(nan_row[:, None, None, None], 0, x).astype(F32)  # one rounding, nearest even
    for layer in convs:
        h = conv_layer(h, layer, fma)
    return h.reshape(h.shape[0], -1), nan_row


def forward(x, convs, dense, hidden="relu", out="linear", fma=fma32):
    """x [rows][side][side][C] -> [rows][n_out] float64: the conv layers, then the dense model."""
    feat, nan_row = features(x, convs, fma)
    res = M.forward(feat, dense, hidden, out, fma)
    res[nan_row] = np.nan
    return res


def forward_fmaf(x, convs, dense, hidden="relu", out="linear"):
    """`forward` with every fma made by libm's fmaf (slow: small cases)."""
    return forward(x, convs, dense, hidden, out, fma=M._fma_libm)


def make_convs(rng, channels, convs, lo=-30, hi=15):
    """Random conv layers [((k, s, F), W, b), ...] of net_model.mixed values."""
    out, cin = [], channels
    for k, s, F in convs:
        out.append(((k, s, F), M.mixed(rng, (k, k, cin, F), lo, hi), M.mixed(rng, (F,), lo, hi)))
        cin = F
    return out


def n_flat(side, convs):
    for k, s, _ in convs:
        side = out_side(side, k, s)
    return side * side * convs[-1][2]


def pairs(convs, dense):
    """The weight list as Stepper.net_set_weights takes it: conv pairs first."""
    return [(W, b) for _, W, b in convs] + list(dense)
