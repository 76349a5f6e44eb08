"""GPU: aigar_decide (k_decide, decide.inc) against the Python model
(tests/decide_model.py, pinned to the reference by tests/test_decide_model.py): the chosen
indices, the reported values and the chosen action rows by bit pattern, over the shapes of
tests/decide_cases.py, both Q dtypes, e-Greedy at epsilon 0 / 1 / 0.5 and Boltzmann at
temperature 7 / 0.05 / 1e-3 / 0, caller draws (0, 1 - 2^-53, a cdf entry among them) and
the device's own.  Dead and non-NN players sit in every block: -1, NaN, row untouched."""
import ctypes as C

import numpy as np
import pytest

import decide_cases as dc
import decide_model as dm
from oracle_lib import make_config

pytestmark = pytest.mark.gpu
_lib = pytest.importorskip("aigar_amd._lib")
from aigar_amd import _abi  # noqa: E402

SENTINEL = -7.0
_WORLDS = {}


@pytest.fixture(scope="module", autouse=True)
def close_worlds():
    yield
    for g, _ in _WORLDS.values():
        g.close()
    _WORLDS.clear()


def world(A, B):
    """One handle per population shape, shared by the cases: mixed roles, every fourth
    player dead (a dead player as the tick leaves it: no cells, on the dead list)."""
    if (A, B) in _WORLDS:
        return _WORLDS[(A, B)]
    g = _lib.Stepper(make_config(n_arenas=A, bots=B, field_size=max(100, 12 * B), flags=0))
    g.reset(11)
    roles, dead = dc.roles_and_dead(A, B)
    g.set_roles(roles)
    for a in range(A):
        st = g.get_state(a)
        gone = [p for p in range(B) if dead[a * B + p]]
        if not gone:
            continue
        keep = ~np.isin(st["cells_i"][:, 0], gone)
        st["cells_f"], st["cells_i"] = st["cells_f"][keep], st["cells_i"][keep]
        for p in gone:
            st["players_i"][p, 0], st["players_i"][p, 1], st["players_i"][p, 4] = 0, 40, 0
        st["dead"] = np.concatenate([st["dead"], np.array(gone, np.int64)])
        g.load_state(st, a)
    alive = np.concatenate([g.get_state(a)["players_i"][:, 0] for a in range(A)]).astype(bool)
    assert np.array_equal(alive, ~np.array(dead))
    deciding = alive & np.array([r == "NN" for r in roles])
    _WORLDS[(A, B)] = (g, deciding)
    return g, deciding


def table_for(n_out):
    rng = np.random.default_rng(n_out)
    t = rng.random((n_out, 4))
    t[:, 2:] = rng.integers(0, 2, (n_out, 2))
    return t


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(np.where(na, 0, a).view(np.uint64), np.where(nb, 0, b).view(np.uint64))


def draws(q, deciding, temperature, seed):
    """[NP][3] caller draws: random, with u2 = 0, 1 - 2^-53 and (Boltzmann) an entry of the
    player's own cdf, taken from the model, on every eighth player each; also returns the
    players whose draw is a cdf entry."""
    NP = len(q)
    u = np.random.default_rng(seed).random((NP, 3))
    u[0::8, 2] = 0.0
    u[4::8, 2] = 1.0 - 2.0 ** -53
    hits = set()
    if temperature:
        for i in range(2, NP, 8):
            if deciding[i]:
                row = q[i].astype(np.float64).tolist()
                if any(np.isnan(row)) or any(np.isinf(row)):
                    continue
                cdf = dm.boltzmann_cdf(dm.boltzmann_dist(row, temperature))
                below = np.nonzero(cdf < 1.0)[0]  # (a draw stays below 1, and the cdf's last entry is 1.0)
                if len(below):
                    u[i, 2] = cdf[below[min(len(below) - 1, len(cdf) // 3)]]
                    hits.add(i)
    return u, hits


def run_device(torch, g, q, explore, u):
    NP = g.NP
    dev = lambda x: torch.as_tensor(x, device="cuda")  # noqa: E731
    idx = torch.full((NP,), 77, dtype=torch.int32, device="cuda")
    val = torch.full((NP,), SENTINEL, dtype=torch.float64, device="cuda")
    act = torch.full((NP, 4), SENTINEL, dtype=torch.float64, device="cuda")
    g.decide(dev(q), dev(np.array(explore, np.float64)), idx, val, u=None if u is None else dev(u), act=act)
    g.sync()
    return idx.cpu().numpy(), val.cpu().numpy(), act.cpu().numpy()


def compare(torch, g, q, table, strategy, eps, temp, deciding, u):
    want = dm.decide(q, table, strategy, eps, temp, deciding, u=u)
    got = run_device(torch, g, q, (eps, temp), u)
    assert np.array_equal(got[0], want[0]), (strategy, eps, temp)
    assert same_bits(got[1], want[1]), (strategy, eps, temp)
    rows = np.where(deciding[:, None], want[2], SENTINEL)  # nobody decides: the row is untouched
    assert same_bits(got[2], rows), (strategy, eps, temp)
    assert not want[3].any()
    return want


@pytest.mark.parametrize("dtype", dc.DTYPES)
@pytest.mark.parametrize("A,B", dc.PLAYERS)
@pytest.mark.parametrize("n_out", dc.N_OUT)
def test_decide_matches_the_model(n_out, A, B, dtype):
    torch = pytest.importorskip("torch")
    g, deciding = world(A, B)
    table = table_for(n_out)
    q = dc.q_rows(n_out, A * B, dtype)
    for strategy in (dm.E_GREEDY, dm.BOLTZMANN):
        g.decide_config(table, strategy, dtype, seed=5)
        for k, x in enumerate(dc.EPSILONS if strategy == dm.E_GREEDY else dc.TEMPERATURES):
            eps, temp = (x, 3.0) if strategy == dm.E_GREEDY else (0.9, x)  # (Boltzmann never tosses the coin)
            u, _ = draws(q, deciding, temp if strategy == dm.BOLTZMANN else 0.0, 31 * n_out + k)
            compare(torch, g, q, table, strategy, eps, temp, deciding, u)
    for a in range(A):
        assert g.warnings(a) & _abi.WARN_Q_NONFINITE == 0


def test_the_cases_are_not_vacuous_and_match():
    """On the model's side first: subnormal and exactly zero probabilities, a tie that moves
    the index, a draw that equals a cdf entry, explore and exploit at epsilon 0.5, argmax
    ties; then the device agrees on those very cases."""
    torch = pytest.importorskip("torch")
    A, B, n_out = 2, 65, 65
    g, deciding = world(A, B)
    table = table_for(n_out)
    q = dc.q_rows(n_out, A * B, "float64")
    assert deciding.sum() >= 6 * 4 and (~deciding).sum() >= 30
    for blk in range(0, A * B - 3, 4):
        assert not deciding[blk:blk + 4].all()  # a dead or non-NN player in every full block
    sub = zero = moved = hit = 0
    for temp in (7.0, 0.05, 1e-3):
        u, hits = draws(q, deciding, temp, 3)
        hit += len(hits)
        for i in np.nonzero(deciding)[0]:
            p = dm.boltzmann_dist(q[i].tolist(), temp)
            sub += any(0.0 < v < 2.0 ** -1022 for v in p)
            zero += any(v == 0.0 for v in p)
            cdf = dm.boltzmann_cdf(p)
            k = min(int(np.searchsorted(cdf, u[i, 2], side="right")), n_out - 1)
            moved += p.index(p[k]) != k
            if i in hits:
                assert (cdf == u[i, 2]).any()
        g.decide_config(table, dm.BOLTZMANN, "float64", seed=5)
        compare(torch, g, q, table, dm.BOLTZMANN, 0.0, temp, deciding, u)
    assert sub >= 1 and zero >= 1 and moved >= 1 and hit >= 1, (sub, zero, moved, hit)
    g.decide_config(table, dm.E_GREEDY, "float64", seed=5)
    u, _ = draws(q, deciding, 0.0, 4)
    want = compare(torch, g, q, table, dm.E_GREEDY, 0.5, 0.0, deciding, u)
    explored = np.isnan(want[1]) & deciding
    assert explored.any() and (deciding & ~explored).any()
    first = [i for i in np.nonzero(deciding)[0] if i % dc.KINDS in (1, 4, 5)]  # rows with equal maxima
    assert first and all((q[i] == q[i].max()).sum() > 1 and want[0][i] == int(np.argmax(q[i]))
                         for i in first if not explored[i])


def test_nonfinite_rows_take_index_0_and_set_the_warn_bit():
    torch = pytest.importorskip("torch")
    g = _lib.Stepper(make_config(n_arenas=2, bots=3, field_size=100, flags=0))
    g.reset(3)
    table = table_for(9)
    q = dc.q_rows(9, 6, "float64")
    q[1, 4] = float("nan")
    q[5, 8] = float("-inf")
    for strategy, eps, temp in ((dm.E_GREEDY, 1.0, 0.0), (dm.BOLTZMANN, 0.0, 0.05)):
        g.reset(3)
        assert g.warnings(0) == 0 and g.warnings(1) == 0
        g.decide_config(table, strategy, "float64")
        u = np.random.default_rng(1).random((6, 3))
        want = dm.decide(q, table, strategy, eps, temp, np.ones(6, bool), u=u)
        assert want[3].tolist() == [False, True, False, False, False, True]
        got = run_device(torch, g, q, (eps, temp), u)  # (no error return)
        assert np.array_equal(got[0], want[0]) and got[0][1] == 0 and got[0][5] == 0
        assert same_bits(got[1], want[1]) and same_bits(got[2], want[2])
        assert g.warnings(0) & _abi.WARN_Q_NONFINITE and g.warnings(1) & _abi.WARN_Q_NONFINITE
    g.close()


def test_own_draws_are_the_models_philox():
    """u NULL: Philox at (global player, stream 10, the arena's tick, seed) under the arena's
    key -- over two decisions at different ticks and two arenas; another seed, other draws."""
    torch = pytest.importorskip("torch")
    A, B, n_out = 2, 5, 25
    g = _lib.Stepper(make_config(n_arenas=A, bots=B, field_size=100, flags=0))
    g.reset(21)
    roles = ["NN", "NN", "Greedy", "NN", "NN"]
    g.set_roles(roles * A)
    table = table_for(n_out)
    q = dc.q_rows(n_out, A * B, "float32")
    seen = []
    for decision in range(2):
        st = [g.get_state(a) for a in range(A)]
        ticks, keys = [int(s["tick"]) for s in st], [s["philox_key"] for s in st]
        deciding = np.concatenate([s["players_i"][:, 0] for s in st]).astype(bool) & np.array([r == "NN" for r in roles * A])
        assert deciding.sum() >= 6 and keys[0].tolist() != keys[1].tolist()
        for strategy, eps, temp, seed in ((dm.E_GREEDY, 0.5, 0.0, 9), (dm.E_GREEDY, 1.0, 0.0, 9), (dm.E_GREEDY, 1.0, 0.0, 10),
                                          (dm.BOLTZMANN, 0.0, 7.0, 9)):
            g.decide_config(table, strategy, "float32", seed=seed)
            want = dm.decide(q, table, strategy, eps, temp, deciding, seed=seed, ticks=ticks, keys=keys, B=B)
            got = run_device(torch, g, q, (eps, temp), None)
            assert np.array_equal(got[0], want[0]) and same_bits(got[1], want[1]), (decision, strategy, eps, seed)
            if strategy == dm.E_GREEDY and eps == 1.0:
                seen.append(got[0][deciding].tolist())
        assert seen[-2] != seen[-1]  # another seed, other draws
        g.policy_random(0.0, 0.0, 1)
        g.step(3)
        assert int(g.get_state(0)["tick"]) == ticks[0] + 3
    assert seen[0] != seen[2]  # another tick, other draws
    g.close()


def test_refusals():
    torch = pytest.importorskip("torch")
    g = _lib.Stepper(make_config(n_arenas=1, bots=2, field_size=100, flags=0))
    g.reset(1)
    L = _lib.load()
    one = torch.zeros(8, dtype=torch.float64, device="cuda")
    p = C.c_void_p(one.data_ptr())
    assert L.aigar_decide(g.h, p, p, None, p, p, None) < 0 and b"decide_config" in L.aigar_last_error()
    prm = _abi.RewardParams.from_parameters(None)
    assert L.aigar_env_step_q(g.h, p, p, None, 0, 0, C.byref(prm), p, p, 0, p, p) < 0
    assert b"decide_config" in L.aigar_last_error()
    with pytest.raises(RuntimeError, match="decide_config"):
        g.decide(one, one, one, one)
    for bad in (np.zeros((0, 4)), np.zeros((1025, 4))):
        with pytest.raises(RuntimeError, match="n_out"):
            g.decide_config(bad)
    with pytest.raises(ValueError):
        g.decide_config(np.zeros((4, 3)))
    g.decide_config(np.zeros((1024, 4)), "Boltzmann", "float64")  # the bound itself is fine
    g.decide_config(None)
    assert g.dec is None
    g.close()
    tiled = _lib.Stepper(make_config(bots=4, tile_flags=_abi.TILE_FORCE))
    with pytest.raises(RuntimeError, match="tiled"):
        tiled.decide_config(np.zeros((4, 4)))
    tiled.close()
