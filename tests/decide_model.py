"""The Q-learning bots' action selection in plain Python: the specification of
aigar_decide (include/aigar.h; qLearning.py:8-13, 208-243), pinned to the reference by
tests/golden/decide_*.npz (tests/test_decide_model.py) and compared bit for bit with the
device (tests/test_gpu_decide.py).

Rows are lists of Python floats, so every operation is one IEEE float64 operation, as in
the reference; `math.e ** y` is libm's pow; numpy.sum and numpy.cumsum are the reference's
own calls (the pairwise sum, the left-to-right running sum)."""
import math

import numpy as np

E_GREEDY, BOLTZMANN = 0, 1
ST_DECIDE = 10  # the Philox stream word of the own draws (aigar_sem.h)
NAN = float("nan")


def greedy(q):
    """numpy.argmax: the first index of the maximum."""
    m, mi = q[0], 0
    for i in range(1, len(q)):
        if q[i] > m:
            m, mi = q[i], i
    return mi, q[mi]


def boltzmann_dist(q, temperature):
    """boltzmannDist (qLearning.py:8-13)."""
    m = max(q)
    d = [math.e ** ((v - m) / temperature) for v in q]
    s = float(np.sum(d))
    return [v / s for v in d]


def boltzmann_cdf(p):
    """numpy.random.choice's cdf of p (mtrand: p.cumsum(), then /= its last entry)."""
    cdf = np.cumsum(np.array(p, np.float64))
    cdf /= cdf[-1]
    return cdf


def boltzmann(q, temperature, u2):
    p = boltzmann_dist(q, temperature)
    cdf = boltzmann_cdf(p)
    k = min(int(np.searchsorted(cdf, u2, side="right")), len(q) - 1)
    idx = p.index(p[k])  # numpy.argmax(q_Values == action_value): the first equal one
    return idx, p[idx]


def decide_row(q, strategy, epsilon, temperature, u):
    """One live NN player's decision: (index, reported value, non-finite row)."""
    q = [float(v) for v in q]
    n = len(q)
    if any(math.isnan(v) or math.isinf(v) for v in q):
        return 0, q[0], True
    if strategy == E_GREEDY:
        if u[0] < epsilon:
            x = u[1] * n
            return (min(int(x), n - 1) if x >= 0 else 0), NAN, False
    elif temperature != 0:
        return boltzmann(q, temperature, u[2]) + (False,)
    return greedy(q) + (False,)


def own_draws(gp, tick, seed, key):
    """u0, u1, u2 of global player gp: Philox4x64-10 keyed by the arena's key at the
    counter (gp, ST_DECIDE, tick, seed); numpy's Philox returns the block of counter + 1."""
    c = (int(gp) | ST_DECIDE << 64 | int(tick) << 128 | (int(seed) & (2 ** 64 - 1)) << 192) - 1
    ctr = [(c % 2 ** 256) >> (64 * k) & (2 ** 64 - 1) for k in range(4)]
    raw = np.random.Philox(key=np.array(key, np.uint64), counter=np.array(ctr, np.uint64)).random_raw(4)
    return [float(int(w) >> 11) * (1.0 / 9007199254740992.0) for w in raw[:3]]


def decide(q, table, strategy, epsilon, temperature, deciding, u=None, seed=0, ticks=None, keys=None, B=None):
    """All players: q [NP][n_out] (any float dtype: widened exactly), table [n_out][4],
    deciding [NP] (alive and NN), u [NP][3] or None (own draws: ticks / keys per arena, B
    players per arena).  Returns idx int32 [NP], val float64 [NP], act float64 [NP, 4]
    (NaN rows where nobody decides: the device leaves those untouched) and nonfinite [NP]."""
    NP = len(q)
    idx = np.full(NP, -1, np.int32)
    val = np.full(NP, np.nan)
    act = np.full((NP, 4), np.nan)
    bad = np.zeros(NP, bool)
    for gp in range(NP):
        if not deciding[gp]:
            continue
        if u is not None:
            ug = [float(v) for v in u[gp]]
        else:
            a = gp // B
            ug = own_draws(gp, ticks[a], seed, keys[a])
        i, v, b = decide_row(np.asarray(q[gp], np.float64).tolist(), strategy, epsilon, temperature, ug)
        idx[gp], val[gp], bad[gp] = i, v, b
        act[gp] = table[i]
    return idx, val, act, bad
