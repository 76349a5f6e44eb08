"""GPU vs oracle over the observation layouts the rest of the suite never
configures (tests/shapes.py: MASKS): ALL_PLAYER_GRID, rows without the pellet
channel, a second-last-frame grid without its last-frame grid, one of the self /
enemy pairs alone and extras subsets with an earlier feature absent -- at 11 and
16 squares per side (k_observe), 17 and 42 (k_observe_wide) and the simple
representation (k_observe_simple); their float32 instantiations; the masked
observation; and aigar_run with a Greedy population whose observation cannot
pick the moves (no pellet channel, more than 16 squares, the simple
representation).  Rows are compared by bit pattern, signed zeros included."""
import numpy as np
import pytest

from aigar_amd import _abi
from oracle_lib import Oracle
import parity
import shapes as S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
_lib = pytest.importorskip("aigar_amd._lib")


def _mask_pair(cfg, n_dev=1):
    o = S.start(Oracle(cfg), 1, S.MASK_SEED, hi=S.MASK_HI)
    devs = []
    for _ in range(n_dev):
        g = _lib.Stepper(cfg)
        g.set_stream(torch.cuda.current_stream().cuda_stream)
        S.start(g, 1, S.MASK_SEED, hi=S.MASK_HI)
        assert g.obs_len == o.obs_len
        assert parity.diff_states(g.get_state(), o.get_state(), ftol=0) == []
        devs.append(g)
    return devs, o


def _tick(xs, rng):
    cmd = S.mask_commands(rng)
    for x in xs:
        x.set_actions(cmd, 0.5 * cmd)  # distinct numbers in the action extras
        x.set_commands(cmd)
        x.step(1)


def _same_rows(got, want, what):
    assert S.obs_bits_equal(got, want), "%s: rows differ: %s" % (what, S.bits_diff(got, want))


@pytest.mark.parametrize("G", S.MASK_GRIDS)
@pytest.mark.parametrize("channels,extras", S.MASKS, ids=S.MASK_IDS)
def test_mask_matches_oracle(channels, extras, G):
    (g,), o = _mask_pair(S.mask_config(channels, extras, G))
    n_grids = bin(channels).count("1")
    n_extras = sum(n for b, n in ((1, 1), (2, 1), (4, 1), (8, 4), (16, 4)) if extras & b)
    assert g.obs_len == n_grids * G * G + n_extras
    seen, rng = S.Seen(channels, G), np.random.default_rng(S.MASK_SEED)
    for t in range(S.MASK_TICKS):
        _tick((g, o), rng)
        want = o.observe()
        _same_rows(g.observe(), want, "tick %d" % t)
        seen.rows(want)
    seen.check()
    assert parity.diff_states(g.get_state(), o.get_state(), ftol=0) == []
    g.close()
    o.close()


F32_CASES = [(S.MASKS[1], 11), (S.MASKS[6], 11), (S.MASKS[8], 11), (S.MASKS[1], 42), (S.MASKS[6], 42),
             (S.MASKS[8], 42), ((_abi.OBS_SIMPLE, 0), 11)]


@pytest.mark.parametrize("mask,G", F32_CASES, ids=["%s-g%d" % ("ch%03x-ex%02x" % m, G) for m, G in F32_CASES])
def test_float32_rows_are_the_rounded_float64_rows(mask, G):
    """The float kernels compute in double and convert each value once on the
    store: round to nearest even, as numpy's astype does."""
    (g64, g32), o = _mask_pair(S.mask_config(mask[0], mask[1], G), n_dev=2)
    rng = np.random.default_rng(S.MASK_SEED)
    for t in range(S.MASK_TICKS):
        _tick((g64, g32, o), rng)
        want = o.observe()
        _same_rows(g64.observe(), want, "tick %d" % t)
        got = g32.observe(out=np.zeros((g32.NP, g32.obs_len), np.float32))
        assert got.dtype == np.float32
        _same_rows(got, want.astype(np.float32), "tick %d, float32" % t)
    for x in (g64, g32, o):
        x.close()


MASKED_CASES = [(S.MASKS[6], 11), (S.MASKS[8], 11), (S.MASKS[8], 42)]
SENTINEL = -7.25


@pytest.mark.parametrize("mask,G", MASKED_CASES, ids=["%s-g%d" % ("ch%03x-ex%02x" % m, G) for m, G in MASKED_CASES])
def test_masked_observation(mask, G):
    """A fresh random bot mask every tick, from the host on even ticks and as a
    device tensor on odd ones: the masked bots' rows are the oracle's
    observe_one (which advances that bot's history alone), the others stay as
    the buffer had them, and a closing unmasked observation agrees -- so the
    histories advanced for exactly the masked bots."""
    (g,), o = _mask_pair(S.mask_config(mask[0], mask[1], G))
    rng, mrng = np.random.default_rng(S.MASK_SEED), np.random.default_rng(S.MASK_SEED + 1)
    n_rows = n_dead = 0
    for t in range(S.MASK_TICKS):
        _tick((g, o), rng)
        m = (mrng.random(g.NP) < 0.5).astype(np.uint8)
        out = np.full((g.NP, g.obs_len), SENTINEL)
        if t % 2 == 0:
            g.observe(out=out, mask=m)
        else:
            dm = torch.tensor(m, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            g.observe(out=out, mask=dm)
        alive = o.player_stats()[:, 0]
        for p in range(g.NP):
            if m[p]:
                _same_rows(out[p:p + 1], o.observe_one(p)[None], "tick %d bot %d" % (t, p))
                if not alive[p]:
                    assert np.isnan(out[p]).all(), (t, p)
                    n_dead += 1
                n_rows += 1
            else:
                assert (out[p] == SENTINEL).all(), (t, p)
    assert 0 < n_rows < S.MASK_TICKS * g.NP
    _same_rows(g.observe(), o.observe(), "closing unmasked observation")
    g.close()
    o.close()


@pytest.mark.parametrize("shape", S.FALLBACK_SHAPES, ids=["5x67", "1x257"])
@pytest.mark.parametrize("channels,G", S.FALLBACK, ids=S.FALLBACK_IDS)
def test_greedy_run_without_fused_moves(channels, G, shape):
    """aigar_run with the Greedy policy where the observation cannot pick the
    moves: k_policy_greedy runs as its own node of the captured graph.  Against
    the oracle, and against a twin driven by separate policy / step / observe
    calls."""
    A = shape[0]
    cfg = S.shape_config(shape, channels, 0 if channels & _abi.OBS_SIMPLE else S.FULL_EX, G)
    o = S.start(Oracle(cfg), A, S.SHAPE_SEED)
    fused, sep = _lib.Stepper(cfg), _lib.Stepper(cfg)
    for x in (fused, sep):
        x.set_stream(torch.cuda.current_stream().cuda_stream)
        S.start(x, A, S.SHAPE_SEED)
    assert fused.obs_len == o.obs_len
    obs = torch.full((fused.NP, fused.obs_len), -7.0, dtype=torch.float64, device="cuda")
    w = S.Worth(A)
    for c in range(S.GREEDY_CALLS):
        fused.run(S.GREEDY_STEPS, "greedy", obs, greedy_split=True)
        torch.cuda.synchronize()
        got = obs.cpu().numpy()
        logs = [[] for _ in range(A)]
        for _ in range(S.GREEDY_STEPS):
            o.policy_greedy(True)
            o.step(1)
            want = o.observe()
            w.tick(o)
            for a in range(A):
                logs[a].append(o.events(a))
            sep.policy_greedy(True)
            sep.step(1)
            rows = sep.observe()
        what = "call %d" % c
        _same_rows(got, want, what)
        _same_rows(rows, want, what + ", separate calls")
        for a in range(A):
            assert parity.diff_states(fused.get_state(a), o.get_state(a), ftol=0) == [], (what, a)
            assert parity.diff_states(sep.get_state(a), o.get_state(a), ftol=0) == [], (what, a)
            assert np.array_equal(fused.events(a), np.concatenate(logs[a])), (what, a)
    w.check_greedy()
    for x in (fused, sep, o):
        x.close()


@pytest.mark.parametrize("bit", [_abi.OBS_SELF_SLF, _abi.OBS_SELF_LF, _abi.OBS_ENEMY_SLF, _abi.OBS_ENEMY_LF])
def test_all_player_grid_with_a_last_frame_grid_is_refused(bit):
    with pytest.raises(RuntimeError, match="ALL_PLAYER_GRID with last-frame grids is undefined in the reference"):
        _lib.Stepper(S.mask_config(_abi.OBS_ALL | bit, 0))
