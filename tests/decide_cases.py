"""The inputs of tests/test_gpu_decide.py, built without a GPU so that
tests/test_decide_pow_host.py can check pow_glibc on exactly the exponents those tests
send through the kernel.

Shapes (the smallest at which k_decide can go wrong): n_out around the lane count (63, 64,
65), around numpy.sum's regimes (below 8, 8, 9, 128, 129, two splits at 300, the bound
1024); players as arenas x bots with partial blocks of four and arena boundaries inside
a block (2 x 65, 3 x 100)."""
import numpy as np

N_OUT = (1, 2, 7, 8, 9, 63, 64, 65, 128, 129, 300, 1024)
PLAYERS = ((1, 1), (1, 3), (2, 65), (3, 100))
DTYPES = ("float64", "float32")
EPSILONS = (0.0, 1.0, 0.5)
TEMPERATURES = (7.0, 0.05, 1e-3, 0.0)
KINDS = 6


def q_rows(n_out, n_players, dtype, seed=0):
    """[n_players, n_out] rows of dtype; player i's row is of kind i % 6:
    0 spread values; 1 a few distinct values with period 13 (equal probabilities and equal
    maxima: the first index wins); 2 the maximum last; 3 a ladder whose steps, divided by
    each tested temperature, land in pow's subnormal range (about -720) and below its
    flush to zero (-800); 4 two equal maxima among spread values; 5 all equal."""
    rng = np.random.default_rng(1000003 * n_out + 101 * n_players + seed)
    q = np.zeros((n_players, n_out))
    for i in range(n_players):
        kind = i % KINDS
        if kind == 0:
            r = rng.standard_normal(n_out) * 3.0
        elif kind == 1:
            r = (np.arange(n_out) % 13) * 0.25 - 1.0
            r = np.roll(r, i % 5)
        elif kind == 2:
            r = rng.standard_normal(n_out)
            r[-1] = r.max() + 1.5
        elif kind == 3:
            steps = np.array([0.0, -0.72, -0.8, -36.0, -40.0, -5040.0, -5600.0, -0.735, -37.0, -5100.0])
            r = steps[np.arange(n_out) % len(steps)]
        elif kind == 4:
            r = rng.standard_normal(n_out) * 2.0
            if n_out > 1:
                r[n_out - 1] = r[n_out // 2] = r.max() + 0.25
        else:
            r = np.full(n_out, 0.375)
        q[i] = r
    return np.ascontiguousarray(q.astype(dtype))


def exponents(q, temperature):
    """The y of every pow(e, y) a Boltzmann decision of these rows makes (float64)."""
    q = q.astype(np.float64)
    return ((q - q.max(axis=1, keepdims=True)) / temperature).reshape(-1)


def roles_and_dead(A, B):
    """Roles per player ("NN" / "Greedy" / "Random") and the players made dead: with four
    or more players every block of four holds a dead one, and non-NN players are mixed in."""
    NP = A * B
    roles = ["Greedy" if i % 5 == 2 else "Random" if i % 7 == 4 else "NN" for i in range(NP)]
    dead = [i % 4 == 1 and NP > 1 for i in range(NP)]
    return roles, dead


def all_shapes():
    for n_out in N_OUT:
        for A, B in PLAYERS:
            for dtype in DTYPES:
                yield n_out, A, B, dtype
