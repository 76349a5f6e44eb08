"""GPU: aigar_net_forward with a conv part (k_conv, conv.inc, then k_net) against the Python
model (tests/conv_model.py, checked against libm's fmaf and torch's conv2d by
tests/test_conv_model.py), bit pattern for bit pattern: the geometries that hit every edge of
the implicit GEMM (K = k k Cin no multiple of the 4-wide MFMA step or of the 32-wide chunk, a
single step, F below, at and across a 16-wide filter tile, stride = kernel, kernel = image,
(42 - 8) / 4 flooring, one to three layers, the largest activations), 1, 15, 16, 17 and 33
samples (rows of M that end inside, at and behind a 16-row tile), both input dtypes, NaN samples
at tile edges with a canary row behind the output, more samples than the activation buffers
hold, and the weight push from device tensors and from host arrays.  No tolerance anywhere.

Magnitudes.  net_model.mixed(lo, hi) gives |v| < 2^hi.  With images below 2^8 and every kernel
and bias below 2^12, a layer of K inputs below 2^a gives outputs below (K + 1) 2^(a + 12), so
the longest network here (K = 384, 512, 576 in the conv layers, then 5184 or less and 7 in the
dense ones: factors below 2^9, 2^10, 2^10, 2^13, 2^3) stays below 2^(8 + 5 * 12 + 45) = 2^113 <
2^128: no layer overflows (an overflow would make an inf - inf NaN, whose payload is not part of
the contract).  Subnormals and signed zeros are among the values."""
import numpy as np
import pytest

import conv_model as CM
import net_model as M
from oracle_lib import make_config

pytestmark = pytest.mark.gpu
from aigar_amd import _abi, _lib, net as N  # noqa: E402

F32 = np.float32
ROWS = (1, 15, 16, 17, 33)
X_HI, W_HI = 8, 12
DENSE = (7, 3)
# (side, C, convs, flattened length, most rows)
GEOMETRIES = [(42, 1, ((8, 4, 32), (4, 2, 64)), 576, 33), (42, 6, ((8, 4, 32), (4, 2, 64)), 576, 33),
              (42, 1, ((8, 4, 32), (4, 2, 64), (3, 1, 64)), 64, 33), (84, 1, ((8, 4, 32), (4, 2, 64)), 5184, 17),
              (5, 3, ((3, 2, 5),), 20, 33), (7, 2, ((2, 1, 17), (3, 3, 3)), 12, 33), (8, 1, ((8, 4, 16),), 16, 33),
              (3, 4, ((1, 1, 64),), 576, 33)]
IDS = ["%d-%d-%s" % (g[0], g[1], "_".join("%d.%d.%d" % c for c in g[2])) for g in GEOMETRIES]
_G = {}


@pytest.fixture(scope="module", autouse=True)
def close_handle():
    yield
    for g in _G.values():
        g.close()
    _G.clear()


def handle():
    """aigar_net_forward ignores liveness and roles: one small fresh world serves every case."""
    if "g" not in _G:
        g = _lib.Stepper(make_config(n_arenas=2, bots=5, field_size=100, flags=0))
        g.reset(11)
        _G["g"] = g
    return _G["g"]


def spec_of(side, C, convs, flat, hidden="relu", out="linear"):
    return N.CnnSpec(side, C, convs, flat, DENSE, hidden, out)


def network(rng, side, C, convs, flat):
    cv = CM.make_convs(rng, C, convs, hi=W_HI)
    return cv, M.make_weights(rng, flat, DENSE, hi=W_HI)


def run(g, x, n_out):
    """x (numpy, float64 or float32) through the configured network; with a canary row behind."""
    import torch
    rows = x.shape[0]
    out = torch.full((rows + 1, n_out), -7.25, dtype=torch.float64, device="cuda")
    xt = torch.as_tensor(x, device="cuda")
    torch.cuda.synchronize()  # (the handle runs on its own stream)
    g.net_forward(xt, out[:rows])
    g.sync()
    got = out.cpu().numpy()
    assert (got[rows] == -7.25).all(), "the row behind the last one was written"
    return got[:rows]


def check(got, want, what):
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    assert np.array_equal(nan_g, nan_w), what
    bad = np.nonzero((M.bits(np.where(nan_g, 0, got)) != M.bits(np.where(nan_w, 0, want))))
    assert len(bad[0]) == 0, (what, len(bad[0]), bad[0][:4], bad[1][:4], got[bad][:4], want[bad][:4])


def images(rng, rows, side, C):
    x = M.mixed(rng, (rows, side, side, C), hi=X_HI)
    x64 = x.astype(np.float64) * (1 + 2.0 ** -30)  # float64 values that are not float32 values: one rounding each
    x64[x == 0] = x[x == 0]
    return x, x64


@pytest.mark.parametrize("side,C,convs,flat,most", GEOMETRIES, ids=IDS)
def test_forward_is_the_models_fmaf_chain(side, C, convs, flat, most):
    import torch
    g = handle()
    i = GEOMETRIES.index((side, C, convs, flat, most))
    rng = np.random.default_rng(1000 + i)
    cv, dense = network(rng, side, C, convs, flat)
    assert CM.n_flat(side, convs) == flat
    g.net_config(spec_of(side, C, convs, flat))
    w = CM.pairs(cv, dense)
    if i % 2:  # the push from device tensors, or from host arrays
        w = [(torch.as_tensor(W, device="cuda"), torch.as_tensor(b, device="cuda")) for W, b in w]
        torch.cuda.synchronize()
    g.net_set_weights(w)
    x, x64 = images(rng, most, side, C)
    nan_at = [r for r in (2, 16) if r < most]
    for r in nan_at:  # NaN samples among the others (a dead player's pixel state: all NaN)
        x[r, 0, 0, 0] = x64[r, 0, 0, 0] = np.nan
    x[nan_at[0]] = np.nan
    want32, want64 = CM.forward(x, cv, dense), CM.forward(x64, cv, dense)
    live = np.delete(np.arange(most), nan_at)
    assert np.isfinite(want32[live]).all() and np.isfinite(want64[live]).all()
    assert np.isnan(want32[nan_at]).all() and len(np.unique(want32[live])) > want32[live].size // 4
    for rows in ROWS:
        if rows > most:
            continue
        check(run(g, x[:rows], DENSE[-1]), want32[:rows], ("float32", rows))
        check(run(g, x64[:rows], DENSE[-1]), want64[:rows], ("float64", rows))


def test_small_case_against_libm_and_a_sigmoid_head():
    g = handle()
    rng = np.random.default_rng(3)
    side, C, convs, flat = 7, 2, ((2, 1, 17), (3, 3, 3)), 12
    _, dense = network(rng, side, C, convs, flat)
    cv = CM.make_convs(rng, C, convs, -6, 0)
    g.net_config(spec_of(side, C, convs, flat, "linear", "sigmoid"))
    x = M.mixed(rng, (3, side, side, C), -6, 2).astype(np.float64)
    # (the sigmoid away from 0 and 1: images below 2^2, kernels below 1 and the dense ones below 2^-8
    # leave the head's input below 9 * 154 * 13 * 8 * 2^(2 - 16) < 2^4)
    dense_s = [(W * F32(2.0 ** -20), b * F32(2.0 ** -20)) for W, b in dense]
    g.net_set_weights(CM.pairs(cv, dense_s))
    want = CM.forward_fmaf(x, cv, dense_s, "linear", "sigmoid")
    check(run(g, x, 3), want, "libm")
    assert ((want > 0) & (want < 1)).all()


@pytest.mark.parametrize("side,C,convs,flat,dead", [
    (7, 2, ((2, 1, 17), (3, 3, 3)), 12, (0, 3, 4, 7, 8, 15, 16, 32)),  # 4 positions a sample: tiles of 4 samples
    (42, 1, ((8, 4, 32), (4, 2, 64)), 576, (0, 1, 2, 15, 16, 30, 32)),  # 81 and 9: samples across tile edges
], ids=["7-2", "42-1"])
def test_nan_samples_at_tile_edges_and_their_neighbours(side, C, convs, flat, dead):
    g = handle()
    rng = np.random.default_rng(6)
    cv, dense = network(rng, side, C, convs, flat)
    g.net_config(spec_of(side, C, convs, flat))
    g.net_set_weights(CM.pairs(cv, dense))
    x, x64 = images(rng, 33, side, C)
    dead = list(dead)
    for a in (x, x64):
        a[dead, 0, 0, 0] = np.nan
        a[dead[1]] = np.nan  # (a dead player's state: all NaN)
        a[5, 0, 0, C - 1 if C > 1 else 0] = a[5, 0, 0, 0]  # (a live neighbour is untouched)
    want = CM.forward(x64, cv, dense)
    got = run(g, x64, DENSE[-1])
    assert np.isnan(got[dead]).all() and not np.isnan(np.delete(got, dead, 0)).any()
    check(got, want, "nan samples")
    check(run(g, x, DENSE[-1]), CM.forward(x, cv, dense), "nan samples float32")
    # the same buffers afterwards, without the NaNs: nothing of them stays
    x2, _ = images(rng, 33, side, C)
    check(run(g, x2, DENSE[-1]), CM.forward(x2, cv, dense), "after the NaNs")


def test_more_samples_than_the_activation_buffers_hold():
    g = handle()
    rng = np.random.default_rng(8)
    side, C, convs, flat = 5, 3, ((3, 2, 5),), 20
    cv, dense = network(rng, side, C, convs, flat)
    g.net_config(spec_of(side, C, convs, flat))
    g.net_set_weights(CM.pairs(cv, dense))
    x, _ = images(rng, 131, side, C)  # (the buffers hold max(A * B, 64) samples: slabs of 64, 64 and 3)
    x[[63, 64, 130], 0, 0, 0] = np.nan
    check(run(g, x, DENSE[-1]), CM.forward(x, cv, dense), "131 samples")


def test_set_weights_replaces_everything_and_plain_config_turns_the_conv_part_off():
    import torch
    g = handle()
    rng = np.random.default_rng(7)
    side, C, convs, flat = 7, 2, ((2, 1, 17), (3, 3, 3)), 12
    g.net_config(spec_of(side, C, convs, flat, "relu", "sigmoid"))
    x, _ = images(rng, 17, side, C)
    assert (run(g, x, 3) == 0.5).all()  # zero weights until the first push: sigmoid(0) everywhere
    big = network(rng, side, C, convs, flat)
    small = network(rng, side, C, convs, flat)
    small = ([(gm, W * F32(2.0 ** -12), b * F32(2.0 ** -12)) for gm, W, b in small[0]],
             [(W * F32(2.0 ** -24), b * F32(2.0 ** -24)) for W, b in small[1]])  # (the head's input stays below 2^2)
    dev = [(torch.as_tensor(W, device="cuda"), torch.as_tensor(b, device="cuda")) for W, b in CM.pairs(*big)]
    torch.cuda.synchronize()
    g.net_set_weights(dev)
    check(run(g, x, 3), CM.forward(x, big[0], big[1], "relu", "sigmoid"), "device tensors")
    g.net_set_weights(CM.pairs(*small))  # host arrays; nothing of the larger set may stay
    want = CM.forward(x, small[0], small[1], "relu", "sigmoid")
    check(run(g, x, 3), want, "host arrays")
    assert len(np.unique(want)) > 8
    # a narrower conv part on the same handle, then none: the dense network alone again
    g.net_config(spec_of(5, 3, ((3, 2, 5),), 20))
    cv, dense = network(rng, 5, 3, ((3, 2, 5),), 20)
    g.net_set_weights(CM.pairs(cv, dense))
    x5, _ = images(rng, 9, 5, 3)
    check(run(g, x5, 3), CM.forward(x5, cv, dense), "narrower")
    g.net_config((20, DENSE, "relu", "linear"))
    assert g.conv is None
    g.net_set_weights(dense)
    rows = x5.reshape(9, -1)[:, :20].astype(np.float64)
    check(run(g, rows, 3), M.forward(rows, dense), "dense alone")
    with pytest.raises(RuntimeError, match="no conv part"):
        g._chk(g.L.aigar_net_set_conv_weights(g.h, 0, dev[0][0].data_ptr(), dev[0][1].data_ptr(), 1))


def test_refusals_on_a_live_handle():
    import torch
    g = handle()
    good = spec_of(7, 2, ((2, 1, 17), (3, 3, 3)), 12)
    with pytest.raises(RuntimeError, match="n_in = 13"):
        g.net_config(good._replace(n_flat=13))
    with pytest.raises(RuntimeError, match="filters = 65"):
        g.net_config(good._replace(convs=((2, 1, 65), (3, 3, 3))))
    with pytest.raises(RuntimeError, match="flattened length"):
        g.net_config(N.CnnSpec(84, 1, ((4, 2, 64),), 41 * 41 * 64, DENSE, "relu", "linear"))
    with pytest.raises(RuntimeError, match="elu"):
        g.net_config(good._replace(hidden="elu"))
    g.net_config(good)
    assert g.conv == (7, 2, ((2, 1, 17), (3, 3, 3))) and g.net[0] == 12
    cv, dense = network(np.random.default_rng(1), 7, 2, good.convs, 12)
    w = CM.pairs(cv, dense)
    with pytest.raises(ValueError):
        g.net_set_weights(w[2:])  # the dense pairs alone
    with pytest.raises(ValueError):
        g.net_set_weights([(w[0][0].transpose(3, 2, 0, 1).copy(), w[0][1])] + w[1:])  # torch's layout, not Keras'
    with pytest.raises(ValueError):
        g.net_set_weights([w[0], (w[1][0][:, :, :16].copy(), w[1][1])] + w[2:])  # Cin of the first layer's 17 filters
    with pytest.raises(RuntimeError, match="layer 2"):
        g._chk(g.L.aigar_net_set_conv_weights(g.h, 2, w[0][0].ctypes.data, w[0][1].ctypes.data, 0))
    o = torch.zeros((4, 3), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        g.net_forward(torch.zeros((4, 12), dtype=torch.float64, device="cuda"), o)  # a flat row, not an image
    with pytest.raises(ValueError):
        g.net_forward(torch.zeros((4, 7, 7, 1), dtype=torch.float64, device="cuda"), o)
    tiled = _lib.Stepper(make_config(bots=4, tile_flags=_abi.TILE_FORCE))
    with pytest.raises(RuntimeError, match="tiled"):
        tiled.net_config(good)
    tiled.close()
