"""The learners' acting network in plain Python: the specification of aigar_net_forward
(include/aigar.h), checked against libm's fmaf (tests/test_net_model.py)
and compared bit for bit with the device (tests/test_gpu_net.py).

A network is a list of (W [in][out], b [out]) float32 layers (Keras' layout).  One row:
the input rounded once to float32; per unit acc = +0.0f, acc = fmaf(x_k, W[k][j], acc) for
k = 0, 1, ..., in - 1 as ONE chain, then y_j = acc + b_j as one float32 add; hidden layers
relu (y > 0 ? y : +0.0f) or linear; the head linear (widened to float64) or the sigmoid in
float64.  A row whose first value is a NaN is not evaluated: its output row is NaN.

Python 3.10 has no math.fma, and a float64 multiply-add rounded to float32 rounds twice.
The yardstick is libm's fmaf through ctypes (`fmaf`, `forward_libm`); `fma32` is a
vectorised emulation for the larger cases: the product of two float32 is exact in
float64, TwoSum gives the sum's error, the sum is rounded to odd, and one cast to float32
then rounds once (53 >= 2 * 24 + 2 bits: innocuous double rounding)."""
import ctypes
import ctypes.util
import math

import numpy as np

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fmaf.restype = ctypes.c_float
_libm.fmaf.argtypes = [ctypes.c_float, ctypes.c_float, ctypes.c_float]

F32 = np.float32


def fmaf(a, b, c):
    """libm's fmaf on three float32 values -> numpy float32."""
    return F32(_libm.fmaf(float(a), float(b), float(c)))


def fma32(a, b, c):
    """Exact float32 fma of float32 arrays (broadcast), vectorised."""
    a, b, c = np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32)
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)  # exact: 48 bits, far inside the range
        c64 = np.broadcast_to(c.astype(np.float64), p.shape)
        s = p + c64
        bb = s - p
        err = (p - (s - bb)) + (c64 - bb)  # TwoSum: s + err == p + c exactly
        fin = np.isfinite(s)
        bits = s.view(np.int64).copy()
        # round to odd: an inexact sum whose last bit is even moves one step towards the error
        fix = fin & (err != 0) & ((bits & 1) == 0)
        up = (err > 0) == (s > 0)  # the exact sum is larger in magnitude
        bits = np.where(fix, bits + np.where(up, 1, -1), bits)
        return bits.view(np.float64).astype(F32)


def sigmoid64(y):
    """The head's sigmoid, the project's own definition: float64 throughout."""
    v = float(y)
    t = -abs(v)
    if not t >= -750.0:
        t = -750.0
    z = math.e ** t  # libm's pow
    return 1.0 / (1.0 + z) if v >= 0 else z / (1.0 + z)


def layer_acc(x, W, fma=fma32):
    """The layer sums before the bias: x [rows][in] float32, W [in][out] -> acc [rows][out]."""
    x, W = np.asarray(x, F32), np.asarray(W, F32)
    acc = np.zeros((x.shape[0], W.shape[1]), F32)  # +0.0f
    for k in range(W.shape[0]):
        acc = fma(x[:, k:k + 1], W[k][None, :], acc)
    return acc


def forward(x, weights, hidden="relu", out="linear", fma=fma32):
    """x [rows][in] float64 / float32 -> [rows][n_out] float64."""
    x = np.asarray(x)
    nan_row = np.isnan(x[:, 0])
    with np.errstate(all="ignore"):
        h = np.where(nan_row[:, None], 0, x).astype(F32)  # one rounding, nearest even
    for l, (W, b) in enumerate(weights):
        with np.errstate(all="ignore"):
            y = layer_acc(h, W, fma) + np.asarray(b, F32)[None, :]  # one float32 add
        if l + 1 < len(weights):
            h = np.where(y > 0, y, F32(0.0)) if hidden == "relu" else y
        else:
            h = y
    res = h.astype(np.float64)
    if out == "sigmoid":
        res = np.array([[sigmoid64(v) for v in row] for row in h], np.float64).reshape(h.shape)
    res[nan_row] = np.nan
    return res


def _fma_libm(a, b, c):
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    return np.array([fmaf(p, q, r) for p, q, r in zip(a.ravel(), b.ravel(), c.ravel())], F32).reshape(a.shape)


def forward_libm(x, weights, hidden="relu", out="linear"):
    """`forward` with every fma made by libm's fmaf (slow: small cases)."""
    return forward(x, weights, hidden, out, fma=_fma_libm)


def mixed(rng, shape, lo=-30, hi=15, p_sub=0.02, p_zero=0.03):
    """float32 values of mixed magnitudes 2^lo .. 2^hi, both signs, some subnormals and
    signed zeros."""
    n = int(np.prod(shape))
    v = np.ldexp(1.0 + rng.random(n), rng.integers(lo, hi, n)) * rng.choice([-1.0, 1.0], n)
    v = v.astype(F32)
    sub = rng.random(n) < p_sub
    v[sub] = (rng.integers(1, 1 << 23, int(sub.sum())).astype(np.uint32)
              | (rng.integers(0, 2, int(sub.sum())).astype(np.uint32) << 31)).view(F32)
    z = rng.random(n) < p_zero
    v[z] = np.where(rng.random(int(z.sum())) < 0.5, F32(0.0), F32(-0.0))
    return v.reshape(shape)


def make_weights(rng, n_in, units, hi=15):
    sizes = [n_in] + list(units)
    return [(mixed(rng, (sizes[l], sizes[l + 1]), hi=hi), mixed(rng, (sizes[l + 1],), hi=hi))
            for l in range(len(units))]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)
