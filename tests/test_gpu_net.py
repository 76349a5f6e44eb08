"""GPU: aigar_net_forward (k_net, net.inc) against the Python model (tests/net_model.py,
checked against libm's fmaf by tests/test_net_model.py), bit pattern for bit pattern: the
sizes that hit every edge of the tiled MFMA kernel (16-row tiles, 16-unit tiles dealt to four
waves, 64-wide k chunks of the first layer, 4-wide k steps of the others), both input
dtypes, NaN rows at tile edges with a canary behind the last output row, the A = I check
with asymmetric operands in both orientations, the activations on chosen pre-activations,
and the weight push from device tensors and host arrays.  No tolerance anywhere.

Magnitudes: inputs 2^-30 .. 2^15 with subnormals and signed zeros; weights the same where
three layers cannot overflow float32 (2^15 * (2^15 * 854) * (2^15 * 100) * (2^15 * 100) <
2^98), and 2^-30 .. 2^5 for the five-layer case at the caps (an overflow would make an
inf - inf NaN, whose payload is not part of the contract)."""
import numpy as np
import pytest

import net_model as M
from oracle_lib import make_config

pytestmark = pytest.mark.gpu
from aigar_amd import _abi, _lib, net as N  # noqa: E402

F32 = np.float32
ROWS = (1, 15, 16, 17, 63, 64, 65, 300)
# (in, hidden, out, weights' largest exponent)
SIZES = [(365, (100, 100), 25, 15), (854, (100, 100), 25, 15), (1, (), 1, 15), (5, (), 3, 15), (33, (7,), 2, 15),
         (16, (16,), 16, 15), (17, (17,), 17, 15), (64, (256, 256, 256, 256), 256, 5)]
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


def run(g, x, n_out, canary=True):
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


@pytest.mark.parametrize("n_in,hidden,n_out,hi", SIZES, ids=["%d-%s-%d" % s[:3] for s in SIZES])
def test_forward_is_the_models_fmaf_chain(n_in, hidden, n_out, hi):
    g = handle()
    rng = np.random.default_rng(n_in * 1000 + n_out)
    units = tuple(hidden) + (n_out,)
    w = M.make_weights(rng, n_in, units, hi=hi)
    g.net_config((n_in, units, "relu", "linear"))
    g.net_set_weights(w)
    x = M.mixed(rng, (max(ROWS), n_in))
    x64 = x.astype(np.float64) * (1 + 2.0 ** -30)  # float64 rows that are not float32 values: one rounding each
    x64[x == 0] = x[x == 0]
    want32, want64 = M.forward(x, w), M.forward(x64, w)
    assert np.isfinite(want32).all() and np.isfinite(want64).all()
    assert len(np.unique(want32)) > want32.size // 4
    for rows in ROWS:
        check(run(g, x[:rows], n_out), want32[:rows], ("float32", rows))
        check(run(g, x64[:rows], n_out), want64[:rows], ("float64", rows))


def test_zero_layers_are_skipped_through_mlp_spec():
    g = handle()
    rng = np.random.default_rng(5)
    spec = N.mlp_spec({"Q_LAYERS": (3, 0, 5)}, "q", n_in=12, n_out=4)
    assert spec.units == (3, 5, 4)
    w = M.make_weights(rng, 12, spec.units)
    g.net_config(spec)
    g.net_set_weights(w)
    x = M.mixed(rng, (65, 12)).astype(np.float64)
    check(run(g, x, 4), M.forward(x, w), "12-(3,0,5)-4")
    check(run(g, x[:9], 4), M.forward_libm(x[:9], w), "libm")


@pytest.mark.parametrize("n", [16, 21])
def test_identity_first_layer_with_asymmetric_operands(n):
    """A = I: W0 the identity, an asymmetric second layer, an asymmetric input (exact small
    integers, so every sum is exact and a transposed or row-swapped tile shows as a wrong
    integer), and the other orientation: the asymmetric matrix first, the identity second."""
    g = handle()
    eye = np.eye(n, dtype=F32)
    asym = (np.arange(n)[:, None] * 3 + np.arange(n)[None, :] * 7 + 1).astype(F32)  # asym[i][j] != asym[j][i]
    x = (np.arange(37)[:, None] * 5 + np.arange(n)[None, :] * 2 - 11).astype(np.float64)
    zero = np.zeros(n, F32)
    for w in ([(eye, zero), (asym, zero)], [(asym, zero), (eye, zero)]):
        g.net_config((n, (n, n), "linear", "linear"))
        g.net_set_weights(w)
        want = x @ asym.astype(np.float64)
        assert not np.array_equal(want, x @ asym.T.astype(np.float64))
        got = run(g, x, n)
        assert np.array_equal(got, want)
        check(got, M.forward(x, w, "linear"), "model")


def test_nan_rows_at_tile_edges_and_their_neighbours():
    g = handle()
    rng = np.random.default_rng(6)
    n_in, units = 70, (20, 6)
    w = M.make_weights(rng, n_in, units)
    g.net_config((n_in, units, "relu", "linear"))
    g.net_set_weights(w)
    x = M.mixed(rng, (81, n_in)).astype(np.float64)
    dead = [0, 15, 16, 31, 32, 47, 63, 64, 80]
    x[dead, 0] = np.nan
    x[dead[1], :] = np.nan  # (a dead player's state: all NaN)
    want = M.forward(x, w)
    got = run(g, x, 6)
    assert np.isnan(got[dead]).all() and not np.isnan(np.delete(got, dead, 0)).any()
    check(got, want, "nan rows")
    xf = x.astype(F32)
    check(run(g, xf, 6), M.forward(xf, w), "nan rows float32")


@pytest.mark.parametrize("hidden", ["relu", "linear"])
def test_activations_on_chosen_preactivations(hidden):
    """W0 = I and b0 = 0 make the hidden pre-activations the inputs themselves, W1 = I makes
    the head's the hidden values: exact 0, -0, tiny negatives, +-100, +-750 and beyond."""
    g = handle()
    v = np.array([0.0, -0.0, -1e-45, -1e-38, 1e-45, 1e-30, -1e-30, 1.0, -1.0, 100.0, -100.0, 745.0, -745.0, 750.0,
                  -750.0, 800.0, -800.0, 3e38, -3e38, 0.5, -0.5, 88.0, -88.0, 20.0], F32)
    n = len(v)
    eye, zero = np.eye(n, dtype=F32), np.zeros(n, F32)
    x = np.stack([v, -v, np.roll(v, 5)]).astype(np.float64)
    for out in ("sigmoid", "linear"):
        w = [(eye, zero), (eye, zero)]
        g.net_config((n, (n, n), hidden, out))
        g.net_set_weights(w)
        want = M.forward(x, w, hidden, out)
        check(run(g, x, n), want, (hidden, out))
        if out == "sigmoid":
            assert ((want >= 0) & (want <= 1)).all() and want[0, 0] == 0.5
        # a single layer: the head alone on the raw values (negative ones reach the sigmoid)
        g.net_config((n, (n,), hidden, out))
        g.net_set_weights([(eye, zero)])
        want = M.forward(x, [(eye, zero)], hidden, out)
        check(run(g, x, n), want, (hidden, out, "single"))
        if out == "sigmoid":
            assert want[0, 16] == M.sigmoid64(-800.0) == M.sigmoid64(-750.0) and want[0, 15] == 1.0


def test_set_weights_from_device_and_host_and_no_stale_padding():
    import torch
    g = handle()
    rng = np.random.default_rng(7)
    n_in, units = 21, (19, 5)
    g.net_config((n_in, units, "relu", "sigmoid"))
    x = M.mixed(rng, (33, n_in), -8, 4).astype(np.float64)
    out = torch.empty((33, 5), dtype=torch.float64, device="cuda")
    # zero weights until the first push: sigmoid(0) everywhere
    assert (run(g, x, 5) == 0.5).all()
    big = M.make_weights(rng, n_in, units, hi=6)
    small = [(W * F32(2.0 ** -12), b * F32(2.0 ** -12)) for W, b in M.make_weights(rng, n_in, units, hi=6)]
    dev = [(torch.as_tensor(W, device="cuda"), torch.as_tensor(b, device="cuda")) for W, b in big]
    torch.cuda.synchronize()  # (the handle runs on its own stream)
    g.net_set_weights(dev)
    check(run(g, x, 5), M.forward(x, big, "relu", "sigmoid"), "device tensors")
    g.net_set_weights(small)  # host arrays; nothing of the larger set may stay
    check(run(g, x, 5), M.forward(x, small, "relu", "sigmoid"), "host arrays")
    # the same padded buffers serve a narrower network configured afterwards
    g.net_config((5, (3,), "relu", "linear"))
    w = M.make_weights(rng, 5, (3,))
    g.net_set_weights(w)
    check(run(g, x[:, :5].copy(), 3), M.forward(x[:, :5], w), "narrower")
    # stand-alone calls run on the caller's stream: a side stream adopted by the handle
    side = torch.cuda.Stream()
    g.sync()
    g.set_stream(side.cuda_stream)
    try:
        with torch.cuda.stream(side):
            xt = torch.as_tensor(x[:, :5].copy(), device="cuda")
            o = torch.full((33, 3), -1.0, dtype=torch.float64, device="cuda")
            g.net_set_weights([(torch.as_tensor(W, device="cuda"), torch.as_tensor(b, device="cuda")) for W, b in w])
            g.net_forward(xt, o)
        side.synchronize()
        check(o.cpu().numpy(), M.forward(x[:, :5], w), "side stream")
    finally:
        g.set_stream(torch.cuda.current_stream().cuda_stream)


def test_refusals_on_a_live_handle():
    import torch
    g = handle()
    g.net_config(None)
    x = torch.zeros((4, 5), dtype=torch.float64, device="cuda")
    o = torch.zeros((4, 3), dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="no acting network"):
        g.net_forward(x, o)
    with pytest.raises(RuntimeError, match="no acting network"):
        g.net_set_weights([])
    g.net_config((5, (3,), "relu", "linear"))
    with pytest.raises(ValueError):
        g.net_forward(x[:, :4].contiguous(), o)
    with pytest.raises(ValueError):
        g.net_set_weights([(np.zeros((3, 5), F32), np.zeros(3, F32))])  # [out][in]: not Keras' layout
    with pytest.raises(RuntimeError, match="elu"):
        g.net_config((5, (3, 2), "elu", "linear"))
    with pytest.raises(RuntimeError, match="257"):
        g.net_config((5, (257, 2), "relu", "linear"))
    with pytest.raises(RuntimeError, match="n_layers = 6"):
        g.net_config((5, (2,) * 6, "relu", "linear"))
    assert g.L.aigar_net_forward(g.h, x.data_ptr(), 0, 0, o.data_ptr()) < 0  # rows >= 1
    tiled = _lib.Stepper(make_config(bots=4, tile_flags=_abi.TILE_FORCE))
    with pytest.raises(RuntimeError, match="tiled"):
        tiled.net_config((5, (3,), "relu", "linear"))
    tiled.close()
