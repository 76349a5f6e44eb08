"""GPU vs oracle at ragged batched shapes (tests/shapes.py: the table and what
each row cuts): arena boundaries inside 256-thread blocks and 64-lane waves,
partial k_players tiles, wave-per-player grids that are no multiple of 8 and
the Greedy graph's cell-sharing kernels away from their aligned sizes.

Every shape runs the full channel mask with every extra from the matured start
under three drivers -- separate calls with synthetic commands, the aigar_run
graph with the random policy folded into the tick, and the aigar_run graph with
the Greedy policy fused into the observation -- with a fresh device / oracle
pair each.  Events and worlds are compared at tolerance 0, observation rows by
bit pattern (signed zeros included).  The oracle's logs must show the run was
worth comparing (test_oracle_shapes.py asserts the same without a GPU)."""
import numpy as np
import pytest

from oracle_lib import Oracle
import parity
import shapes as S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
_lib = pytest.importorskip("aigar_amd._lib")


def _stepper(cfg, A):
    g = _lib.Stepper(cfg)
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    return S.start(g, A, S.SHAPE_SEED)


def _pair(shape):
    cfg = S.shape_config(shape)
    g, o = _stepper(cfg, shape[0]), S.start(Oracle(cfg), shape[0], S.SHAPE_SEED)
    assert g.obs_len == o.obs_len
    _same_world(g, o, shape[0], "start")
    return g, o


def _same_world(g, o, A, what):
    for a in range(A):
        dif = parity.diff_states(g.get_state(a), o.get_state(a), ftol=0)
        assert dif == [], "%s, arena %d: %s" % (what, a, dif[:3])


def _same_events(g, o_logs, A, what):
    for a in range(A):
        eg = g.events(a)
        assert np.array_equal(eg, o_logs[a]), "%s, arena %d: event logs differ (device %d rows, oracle %d)" % (
            what, a, len(eg), len(o_logs[a]))


def _same_rows(got, want, what):
    assert S.obs_bits_equal(got, want), "%s: rows differ: %s" % (what, S.bits_diff(got, want))


def _obs_tensor(g):
    return torch.full((g.NP, g.obs_len), -7.0, dtype=torch.float64, device="cuda")


def _rows(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.mark.parametrize("shape", S.SHAPES, ids=S.SHAPE_IDS)
def test_separate_calls(shape):
    A = shape[0]
    g, o = _pair(shape)
    w, rng, seen = S.Worth(A), S.synthetic_rng(), S.Seen(S.FULL_CH, 11)
    for t in range(S.SHAPE_TICKS):
        cmd = S.synthetic(rng, shape)
        g.set_commands(cmd)
        o.set_commands(cmd)
        g.step(1)
        o.step(1)
        what = "tick %d" % t
        logs = [o.events(a) for a in range(A)]
        _same_events(g, logs, A, what)
        _same_world(g, o, A, what)
        w.tick(o, logs)
        assert np.array_equal(g.player_stats(), o.player_stats(), equal_nan=True), what
        if (t + 1) % 5 == 0:
            want = o.observe()
            _same_rows(g.observe(), want, what)
            seen.rows(want)
    w.check_synthetic()
    seen.check()
    g.close()
    o.close()


def test_heavy_cells_beside_arena_boundaries():
    """shapes.heavy_start: a cell near the mass cap for the first player of arenas 1
    and 2 of 3 x 100, whose wave and block begin in the arena before -- what a wave
    or a block reduces per arena (the radius bound of the cell grids, the queues of
    many-cell players) must stay in its arena."""
    shape, A = S.HEAVY_SHAPE, S.HEAVY_SHAPE[0]
    cfg = S.shape_config(shape)
    g = _lib.Stepper(cfg)
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    S.heavy_start(g)
    o = S.heavy_start(Oracle(cfg))
    _same_world(g, o, A, "start")
    rng, meals = S.synthetic_rng(), S.HeavyMeals()
    meals.before(o)
    for t in range(S.HEAVY_TICKS):
        cmd = S.heavy_commands(rng)
        g.set_commands(cmd)
        o.set_commands(cmd)
        g.step(1)
        o.step(1)
        what = "tick %d" % t
        logs = [o.events(a) for a in range(A)]
        _same_events(g, logs, A, what)
        _same_world(g, o, A, what)
        meals.after(o, logs)
        assert np.array_equal(g.player_stats(), o.player_stats(), equal_nan=True), what
        _same_rows(g.observe(), o.observe(), what)
    meals.check()
    g.close()
    o.close()


@pytest.mark.parametrize("shape", S.SHAPES, ids=S.SHAPE_IDS)
def test_graph_random_policy(shape):
    """The commands the folded policy made are read back after every replay and
    given to the oracle.  A twin that is 9 ticks behind catches up in one call
    (two unrolled replays and a single one) and lands on the same world and rows."""
    A = shape[0]
    g, o = _pair(shape)
    twin = _stepper(S.shape_config(shape), A)
    obs, obs_t = _obs_tensor(g), _obs_tensor(g)
    kw = dict(p_split=S.P_SPLIT, p_eject=S.P_EJECT, seed=3)
    splits = ejects = 0
    for t in range(S.RANDOM_TICKS):
        g.run(1, "random", obs, **kw)
        if t < S.RANDOM_TICKS - 9:
            twin.run(1, "random", obs_t, **kw)
        got = _rows(obs)
        cmd = S.commands(g, A)
        splits += int(cmd[:, 2].sum())
        ejects += int(cmd[:, 3].sum())
        o.set_commands(cmd)
        o.step(1)
        what = "step %d" % t
        _same_world(g, o, A, what)
        _same_events(g, [o.events(a) for a in range(A)], A, what)
        _same_rows(got, o.observe(), what)
    assert splits > 0 and ejects > 0, (splits, ejects)
    twin.run(9, "random", obs_t, **kw)
    _same_rows(_rows(obs_t), got, "twin")
    for a in range(A):
        assert parity.diff_states(twin.get_state(a), g.get_state(a), ftol=0) == [], a
    for x in (g, twin, o):
        x.close()


@pytest.mark.parametrize("shape", S.SHAPES, ids=S.SHAPE_IDS)
def test_graph_greedy_policy(shape):
    """The cell-sharing kernels (k_food_prep<true>, k_pp_active<true>) and the
    observation that also picks the next step's Greedy moves, five steps a call."""
    A = shape[0]
    g, o = _pair(shape)
    obs = _obs_tensor(g)
    w = S.Worth(A)
    for c in range(S.GREEDY_CALLS):
        g.run(S.GREEDY_STEPS, "greedy", obs, greedy_split=True)
        got = _rows(obs)
        logs = [[] for _ in range(A)]
        for _ in range(S.GREEDY_STEPS):
            o.policy_greedy(True)
            o.step(1)
            want = o.observe()
            w.tick(o)
            for a in range(A):
                logs[a].append(o.events(a))
        what = "call %d" % c
        _same_world(g, o, A, what)
        _same_rows(got, want, what)
        _same_events(g, [np.concatenate(l) for l in logs], A, what)
    w.check_greedy()
    g.close()
    o.close()
