"""The worlds of the CNN trainer's tests: the geometries of tests/test_gpu_cnn_train.py and the
transitions, weights and draws they are run on, shared with tests/test_cnn_train_model.py, which
checks without a device that these worlds are worth comparing (open and closed relu gates in
every conv layer, filter gradients of many distinct values)."""
import numpy as np

import conv_model as CM
import net_model as M

F32 = np.float32
# name -> (side, channels, convs (k, stride, F), dense units)
GEOMETRIES = {
    "a": (8, 1, ((3, 1, 4),), (5, 4)),  # one layer; F < 16; K = 9
    "b": (12, 3, ((4, 2, 5), (2, 2, 17)), (6, 4)),  # row and column 4 of layer 1's 5 x 5 reached by no window; F = 17
    "c": (10, 2, ((3, 1, 4), (4, 2, 6), (3, 1, 8)), (7, 3)),  # three layers down to 1 x 1; overlapping windows
    "d": (42, 1, ((8, 4, 32), (4, 2, 64)), (100, 100, 25)),  # the default: M = 405 and 45 at batch 5
}
BATCHES = {"a": 17, "b": 6, "c": 7, "d": 5}  # the batch of a geometry's general cases
N_MEM = 40


def world(geo, seed=0, dtype="float64", n_mem=N_MEM, done=None, rewards=None):
    """-> (convs, dense, (s, a, r, s2, done)) for a geometry: weights of mixed magnitudes 2^-30 .. 2^2,
    images 2^-30 .. 2^3 (float64 rows that are not float32 values), rewards 2^-10 .. 2^5."""
    side, C, cg, units = GEOMETRIES[geo]
    rng = np.random.default_rng(7000 + 100 * sorted(GEOMETRIES).index(geo) + seed)
    convs = CM.make_convs(rng, C, cg, lo=-30, hi=2)
    dense = M.make_weights(rng, CM.n_flat(side, cg), units, hi=2)
    np_dt = np.float64 if dtype == "float64" else np.float32
    s = M.mixed(rng, (n_mem, side, side, C), hi=3)
    s2 = M.mixed(rng, (n_mem, side, side, C), hi=3)
    if dtype == "float64":
        s, s2 = (np.where(x == 0, x, x.astype(np.float64) * (1 + 2.0 ** -30)) for x in (s, s2))
    a = np.zeros((n_mem, 4))
    a[:, 0] = rng.integers(0, units[-1], n_mem)
    r = M.mixed(rng, (n_mem,), lo=-10, hi=5).astype(np.float64) if rewards is None else np.asarray(rewards, np.float64)
    d = (rng.random(n_mem) < 0.25) if done is None else np.asarray(done, bool)
    s, s2 = s.astype(np_dt), s2.astype(np_dt)
    s2[d] = np.nan  # (a dead player's new state is the NaN image)
    return convs, dense, (s, a, r, s2, d.astype(np.uint8))


KW = dict(lr=1e-2, beta1=0.9, beta2=0.999, epsilon=1e-7, discount=0.85)
