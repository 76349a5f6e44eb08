"""The actor-critic learners' exploration noise in plain Python: the specification of
aigar_noise / aigar_env_step_ac (include/aigar.h; actorCritic.py:922-966), pinned to the
reference by tests/golden/noise_cases.npz and to numpy.random.RandomState.normal
(tests/test_noise_model.py), and compared bit for bit with the device
(tests/test_gpu_noise.py, tests/test_gpu_env_ac.py).

Values are Python floats, so every operation is one IEEE float64 operation, as in the
reference; math.log is libm's log, which numpy's legacy Gaussian calls; math.sqrt is
correctly rounded everywhere."""
import math

import numpy as np

GAUSSIAN, ORN_UHL = 0, 1
ST_NOISE = 11  # the Philox stream word of the own draws (aigar_sem.h)
MAX_T, OWN_T = 16, 16
NAN = float("nan")
GRID = 1.0 / 9007199254740992.0  # numpy's 53-bit uniforms: (x >> 11) * 2^-53


def normal_pair(u):
    """numpy's legacy_gauss on the attempts u = [(ua, ub), ...]: (z0, z1, attempts used), or
    (0.0, 0.0, None) when every attempt is rejected.  numpy returns f * x2 first and keeps
    f * x1 for its next call."""
    for t, (ua, ub) in enumerate(u):
        x1 = 2.0 * ua - 1.0
        x2 = 2.0 * ub - 1.0
        r2 = x1 * x1 + x2 * x2
        if r2 < 1.0 and r2 != 0.0:
            f = math.sqrt(-2.0 * math.log(r2) / r2)
            return f * x2, f * x1, t + 1
    return 0.0, 0.0, None


def clip01(a):
    """numpy.clip(a, 0, 1) of a finite a: only a < 0 becomes 0.0, so a -0.0 stays -0.0."""
    a = 0.0 if a < 0.0 else a
    return 1.0 if a > 1.0 else a


def noise_row(mu, std, u, kind=GAUSSIAN, prev=None, theta=0.0, ou_mu=0.0, dt=0.0):
    """One row: mu [n] (n = 2..4), u [2][T][2] the attempts of pair 0 and pair 1 ->
    (noisy [n], new Orn-Uhl state [n] or None, exhausted pairs, non-finite input).  Values 0
    and 1 take pair 0, values 2 and 3 pair 1; an odd n drops the leftover normal."""
    n = len(mu)
    bad = False
    std = float(std)
    if not (std >= 0.0 and std < math.inf):
        std, bad = 0.0, True
    z, exhausted = [], 0
    for pair in range((n + 1) // 2):
        z0, z1, used = normal_pair([(float(a), float(b)) for a, b in u[pair]])
        exhausted += used is None
        z += [z0, z1]
    out, state = [], None if kind == GAUSSIAN else []
    for i in range(n):
        m = float(mu[i])
        if math.isnan(m) or math.isinf(m):
            m, bad = 0.0, True
        if kind == GAUSSIAN:
            a = m + std * z[i]
        else:  # actorCritic.py:930-935
            p = float(prev[i])
            nz = p + theta * (ou_mu - p) * dt + std * math.sqrt(dt) * z[i]
            if math.isnan(nz) or math.isinf(nz):  # outside the contract: the state restarts at 0, flagged
                nz, bad = 0.0, True
            state.append(nz)
            a = m + nz
        out.append(clip01(a))
    return out, state, exhausted, bad


def own_draws(row, pair, tick, seed, key):
    """The OWN_T attempts of (row, pair): attempts 2 b and 2 b + 1 are words {0, 1} and {2, 3}
    of Philox4x64-10 keyed by the arena's key at the counter (row, ST_NOISE | pair << 8 |
    b << 16, tick, seed); numpy's Philox returns the block of counter + 1."""
    out = []
    for b in range(OWN_T // 2):
        c1 = ST_NOISE | pair << 8 | b << 16
        c = (int(row) | c1 << 64 | int(tick) << 128 | (int(seed) & (2 ** 64 - 1)) << 192) - 1
        ctr = [(c % 2 ** 256) >> (64 * k) & (2 ** 64 - 1) for k in range(4)]
        raw = np.random.Philox(key=np.array(key, np.uint64), counter=np.array(ctr, np.uint64)).random_raw(4)
        w = [float(int(x) >> 11) * GRID for x in raw]
        out += [(w[0], w[1]), (w[2], w[3])]
    return out


def noise(mu, std, deciding=None, u=None, kind=GAUSSIAN, prev=None, theta=0.0, ou_mu=0.0, dt=0.0, seed=0, ticks=None,
          keys=None, B=None):
    """All rows: mu [rows][n] (any float dtype: widened exactly), deciding [rows] (None: all),
    u [rows][2][T][2] or None (own draws: ticks / keys per arena, B rows per arena, row r in
    arena (r // B) % len(keys)), prev [rows][n] for Orn-Uhl.  Returns noisy float64 [rows, n]
    (NaN rows where nobody decides), the new state [rows, n] (None for Gaussian; unchanged
    where nobody decides), exhausted [rows] pair counts and nonfinite [rows]."""
    mu = np.asarray(mu)
    rows, n = mu.shape
    noisy = np.full((rows, n), np.nan)
    state = None if kind == GAUSSIAN else np.array(prev, np.float64).reshape(rows, n).copy()
    exhausted = np.zeros(rows, np.int64)
    bad = np.zeros(rows, bool)
    for r in range(rows):
        if deciding is not None and not deciding[r]:
            continue
        if u is not None:
            ur = u[r]
        else:
            a = (r // B) % len(keys)
            ur = [own_draws(r, pair, ticks[a], seed, keys[a]) for pair in range(2)]
        o, s, e, b = noise_row(np.asarray(mu[r], np.float64).tolist(), std, ur, kind,
                               None if state is None else state[r].tolist(), theta, ou_mu, dt)
        noisy[r] = o
        if state is not None:
            state[r] = s
        exhausted[r], bad[r] = e, b
    return noisy, state, exhausted, bad


def bits_equal(a, b):
    """Equality by bit pattern (zero signs and NaN positions count; NaN payloads do not)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return False
    return bool(np.array_equal(np.where(na, 0.0, a).view(np.uint64), np.where(nb, 0.0, b).view(np.uint64)))
