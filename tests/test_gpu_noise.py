"""GPU: the device's log (aigar_selftest_log) against the host's, and aigar_noise (k_noise,
noise.inc) against the Python model (tests/noise_model.py, pinned to the reference by
tests/test_noise_model.py): the noisy rows, the Orn-Uhl state, the exhaustion counter and
the warn bits, by bit pattern, over rows 1 / 63 / 64 / 65 / 257 / 300, 2 / 3 / 4 values, both
mu dtypes, both noise types, std 0 / 0.02 / 1, caller draws with T 1 / 4 / 16 (rejections at
every attempt, r2 == 0 and exhausted pairs among them), the reference's recorded calls fed
as draws, and the device's own Philox draws."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import noise_model as nm
from oracle_lib import make_config

pytestmark = pytest.mark.gpu
from aigar_amd import _abi, _lib  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "noise_cases.npz")
OU = ((0.15, 0.0, 0.01), (0.3, 0.25, 0.5))  # theta, mu, dt
_G = {}


@pytest.fixture(scope="module", autouse=True)
def close_handle():
    yield
    for g in _G.values():
        g.close()
    _G.clear()


def handle():
    """aigar_noise ignores liveness and roles: one small fresh world serves every case."""
    if "g" not in _G:
        g = _lib.Stepper(make_config(n_arenas=2, bots=5, field_size=100, flags=0))
        g.reset(11)
        _G["g"] = g
    return _G["g"]


def log_inputs(count, seed=42):
    """The sets of tools/gen/check_log.cpp: the polar method's r2 on the 53-bit grid (small r2
    included), 1 - k 2^-53 and 1 + k 2^-52, both ends of the branch near 1 +- 300 ulps, every
    power of two, 2^-104, subnormals, the branch near 1 densely, random values over 2^+-1000."""
    rng = np.random.default_rng(seed)
    k = np.arange(4097, dtype=np.float64)
    around = lambda x, w: (np.array([x]).view(np.int64)[0] + np.arange(-w, w + 1)).view(np.float64)  # noqa: E731
    sets = [1.0 - k * 2.0 ** -53, 1.0 + k * 2.0 ** -52, around(1.0 - 2.0 ** -4, 300), around(1.0 + float.fromhex("0x1.09p-4"), 300),
            np.ldexp(1.0, np.arange(-1074, 1024)), around(2.0 ** -104, 8), np.arange(1, 4097) * 5e-324,
            rng.integers(1, 2 ** 52, 4096).view(np.float64), around(2.0 ** -1022, 300),
            np.array([float.fromhex("0x1.fffffffffffffp1023")])]
    per = (count - sum(len(s) for s in sets)) // 4 + 1
    ua, ub = (rng.integers(0, 2 ** 53, 2 * per) * nm.GRID for _ in range(2))
    x1, x2 = 2.0 * ua - 1.0, 2.0 * ub - 1.0
    r2 = x1 * x1 + x2 * x2
    sets.append(r2[(r2 < 1.0) & (r2 != 0.0)][:per])
    sh = rng.integers(1, 53, per)  # offsets of +-2^51 .. +-1 grid steps around 1/2
    oa, ob = ((rng.integers(-2 ** 51, 2 ** 51, per) >> (52 - sh)) for _ in range(2))
    y1, y2 = 2.0 * (0.5 + oa * nm.GRID) - 1.0, 2.0 * (0.5 + ob * nm.GRID) - 1.0
    s2 = y1 * y1 + y2 * y2
    sets.append(s2[s2 != 0.0])
    sets.append((0x3fee000000000000 + rng.integers(0, 0x0003090000000000, per)).view(np.float64))
    sets.append(np.ldexp(1.0 + rng.integers(0, 2 ** 52, per) * 2.0 ** -52, rng.integers(-1000, 1001, per)))
    x = np.concatenate([np.asarray(s, np.float64) for s in sets])
    assert (x > 0).all() and np.isfinite(x).all()
    return x


def test_device_log_is_the_hosts_log():
    x = log_inputs(310000)
    assert len(x) >= 300000
    assert (x < 2.0 ** -1022).sum() > 8000 and ((x > 0.9375) & (x < 1.0647)).sum() > 70000 and (x < 1e-20).sum() > 1000
    want = np.array([math.log(v) for v in x.tolist()])
    got = _lib.selftest_log(x)
    bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
    assert len(bad) == 0, [(float(x[i]).hex(), float(got[i]).hex(), float(want[i]).hex()) for i in bad[:5]]
    # outside the positive finite domain: glibc's special values
    sp = _lib.selftest_log(np.array([0.0, -0.0, np.inf, -1.0, np.nan]))
    assert sp[0] == -np.inf and sp[1] == -np.inf and sp[2] == np.inf and np.isnan(sp[3]) and np.isnan(sp[4])


def grid_uniforms(rng, shape):
    return rng.integers(0, 2 ** 53, shape) * nm.GRID


def crafted_draws(rng, rows, T):
    """[rows][2][T][2] uniforms on numpy's grid; on top of the random ones (21 % rejected):
    rows = 1 mod 7 accept exactly at the last attempt of pair 0 (after r2 >= 1 and r2 == 0
    rejections), rows = 3 mod 7 exhaust pair 1, rows = 5 mod 7 exhaust pair 0."""
    u = grid_uniforms(rng, (rows, 2, T, 2))
    far, centre = 1.0 - nm.GRID, 0.5
    for r in range(rows):
        if r % 7 == 1:
            if T > 1:
                u[r, 0, :T - 1] = [[far, far] if t % 2 else [centre, centre] for t in range(T - 1)]
            u[r, 0, T - 1] = [0.25 + nm.GRID * r, 0.625]
        elif r % 7 == 3:
            u[r, 1] = [[centre, centre] if t % 2 else [far, 0.0] for t in range(T)]
        elif r % 7 == 5:
            u[r, 0] = [[0.0, far] for t in range(T)]
    return u


def mu_rows(rng, rows, n, dtype):
    mu = rng.random((rows, n))
    mu[0::5, 0] = 0.0
    mu[1::5, n - 1] = 1.0
    mu[2::5, 1] = -0.0
    return mu.astype(dtype)


def run_device(torch, g, mu, std, u, prev=None, count=True):
    dev = lambda x: torch.as_tensor(np.ascontiguousarray(x), device="cuda")  # noqa: E731
    out = torch.full(mu.shape, -7.0, dtype=torch.float64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda") if count else None
    pv = None if prev is None else dev(np.array(prev, np.float64))
    g.noise(dev(mu), dev(np.array([std], np.float64)), out, u=None if u is None else dev(u), prev=pv, n_exhausted=cnt)
    g.sync()
    return out.cpu().numpy(), None if pv is None else pv.cpu().numpy(), None if cnt is None else int(cnt.item())


@pytest.mark.parametrize("n", (2, 3, 4))
@pytest.mark.parametrize("rows", (1, 63, 64, 65, 257, 300))
def test_noise_matches_the_model(rows, n):
    import torch
    g = handle()
    rng = np.random.default_rng(1000 * rows + n)
    exhausted_seen = 0
    for dtype in ("float32", "float64"):
        mu = mu_rows(rng, rows, n, dtype)
        for kind in (nm.GAUSSIAN, nm.ORN_UHL):
            theta, ou_mu, dt = OU[(rows + n) % 2]
            g.noise_config(n, kind, dtype, theta=theta, ou_mu=ou_mu, dt=dt, seed=1)
            for std in (0.0, 0.02, 1.0):
                for T in (1, 4, 16):
                    u = crafted_draws(rng, rows, T)
                    prev = rng.standard_normal((rows, n)) * 0.1 if kind == nm.ORN_UHL else None
                    want, state, exh, bad = nm.noise(mu, std, None, u, kind, prev, theta, ou_mu, dt)
                    got, got_state, cnt = run_device(torch, g, mu, std, u, prev)
                    assert not bad.any()
                    assert nm.bits_equal(got, want), (dtype, kind, std, T)
                    assert cnt == int(exh.sum()), (dtype, kind, std, T)
                    if kind == nm.ORN_UHL:
                        assert nm.bits_equal(got_state, state), (dtype, std, T)
                    exhausted_seen += int(exh.sum())
    assert exhausted_seen > 0 or rows == 1
    if rows >= 63:  # the crafted rows did what they were crafted for, on the model's side
        u = crafted_draws(rng, rows, 4)
        assert nm.normal_pair(u[1, 0].tolist())[2] == 4 and nm.normal_pair(u[5, 0].tolist())[2] is None
        assert nm.normal_pair(u[3, 1].tolist())[2] is None


def test_the_references_recorded_calls_fed_as_draws():
    import torch
    g = handle()
    c = dict(np.load(GOLD))
    keys = np.stack([c["n"], c["kind"], c["std"], c["theta"], c["ou_mu"], c["dt"]], axis=1)
    groups = {}
    for k, key in enumerate(map(tuple, keys.tolist())):
        groups.setdefault(key, []).append(k)
    assert len(groups) >= 18
    for (n, kind, std, theta, ou_mu, dt), ks in groups.items():
        n, kind = int(n), int(kind)
        g.noise_config(n, kind, "float64", theta=theta, ou_mu=ou_mu, dt=dt)
        prev = c["prev"][ks][:, :n] if kind == nm.ORN_UHL else None
        got, state, cnt = run_device(torch, g, c["mu"][ks][:, :n], std, c["u"][ks], prev)
        assert nm.bits_equal(got, c["out"][ks][:, :n]), (n, kind, std)
        assert cnt == 0
        if kind == nm.ORN_UHL:
            assert nm.bits_equal(state, c["post"][ks][:, :n]), (n, std)


def test_own_draws_are_the_models_philox():
    """u NULL: Philox at (row, 11 | pair << 8 | block << 16, the arena's tick, seed) under the
    arena's key -- at two ticks, on the players' rows and on more rows than players (row r
    in arena (r / B) % A); another seed, other draws."""
    import torch
    A, B = 2, 5
    g = _lib.Stepper(make_config(n_arenas=A, bots=B, field_size=100, flags=0))
    g.reset(21)
    seen = []
    for decision in range(2):
        st = [g.get_state(a) for a in range(A)]
        ticks, keys = [int(s["tick"]) for s in st], [s["philox_key"] for s in st]
        assert keys[0].tolist() != keys[1].tolist()
        for rows, n, kind, seed in ((A * B, 3, nm.GAUSSIAN, 9), (23, 4, nm.GAUSSIAN, 9), (23, 4, nm.GAUSSIAN, 10),
                                    (A * B, 2, nm.ORN_UHL, 9)):
            mu = mu_rows(np.random.default_rng(rows + n), rows, n, "float32")
            prev = np.full((rows, n), 0.125) if kind == nm.ORN_UHL else None
            g.noise_config(n, kind, "float32", theta=0.15, ou_mu=0.0, dt=0.01, seed=seed)
            want, state, exh, _ = nm.noise(mu, 0.5, None, None, kind, prev, 0.15, 0.0, 0.01, seed=seed, ticks=ticks,
                                           keys=keys, B=B)
            got, got_state, cnt = run_device(torch, g, mu, 0.5, None, prev)
            assert nm.bits_equal(got, want) and cnt == int(exh.sum()) == 0, (decision, rows, n, kind, seed)
            if kind == nm.ORN_UHL:
                assert nm.bits_equal(got_state, state)
            if rows == 23:
                seen.append(got.tolist())
        assert seen[-2] != seen[-1]  # another seed, other draws
        g.policy_random(0.0, 0.0, 1)
        g.step(3)
    assert seen[0] != seen[2]  # another tick, other draws
    g.close()


def test_exhaustion_and_nonfinite_inputs_set_their_warn_bits():
    import torch
    A, B = 2, 3
    g = _lib.Stepper(make_config(n_arenas=A, bots=B, field_size=100, flags=0))
    g.reset(3)
    g.noise_config(4, nm.GAUSSIAN, "float64")
    rng = np.random.default_rng(5)
    mu = rng.random((6, 4))
    ok = np.tile(np.array([0.75, 0.5]), (6, 2, 4, 1))
    # arena 1 (rows 3..5): row 4's pair 1 is all r2 == 0
    u = ok.copy()
    u[4, 1] = 0.5
    want, _, exh, bad = nm.noise(mu, 1.0, None, u)
    got, _, cnt = run_device(torch, g, mu, 1.0, u)
    assert nm.bits_equal(got, want) and cnt == 1 and exh.tolist() == [0, 0, 0, 0, 1, 0]
    assert nm.bits_equal(got[4, 2:], mu[4, 2:])  # the exhausted pair is (0.0, 0.0)
    assert g.warnings(0) == 0 and g.warnings(1) == _abi.WARN_NOISE_EXHAUSTED
    # a NaN and an infinity in arena 0's rows: taken as 0, no error, the bit of that arena
    g.reset(3)
    mu2 = mu.copy()
    mu2[1, 2], mu2[2, 0] = np.nan, -np.inf
    want, _, exh, bad = nm.noise(mu2, 0.02, None, ok)
    got, _, cnt = run_device(torch, g, mu2, 0.02, ok)
    assert nm.bits_equal(got, want) and cnt == 0 and bad.tolist() == [False, True, True, False, False, False]
    assert g.warnings(0) == _abi.WARN_NOISE_NONFINITE and g.warnings(1) == 0
    # a negative, a NaN and an infinite std: no noise, every arena's bit
    for std in (-1.0, float("nan"), float("inf")):
        g.reset(3)
        want, _, _, bad = nm.noise(mu, std, None, ok)
        got, _, _ = run_device(torch, g, mu, std, ok)
        assert nm.bits_equal(got, want) and nm.bits_equal(got, mu) and bad.all()
        assert g.warnings(0) == g.warnings(1) == _abi.WARN_NOISE_NONFINITE
    # a finite but huge std overflows the Orn-Uhl state: that value restarts at 0 with no noise, flagged,
    # so the next call starts from finite numbers (ok: z = (0.0, 1.66...), sd * z[1] = inf)
    g.reset(3)
    g.noise_config(2, nm.ORN_UHL, "float64", theta=0.15, ou_mu=0.0, dt=1.0)
    mu3, prev = mu[:, :2].copy(), np.full((6, 2), 0.25)
    want, state, _, bad = nm.noise(mu3, 1.7e308, None, ok, nm.ORN_UHL, prev, 0.15, 0.0, 1.0)
    got, got_state, _ = run_device(torch, g, mu3, 1.7e308, ok, prev)
    assert bad.all() and np.isfinite(state).all() and (state[:, 1] == 0.0).all() and (state[:, 0] != 0.0).all()
    assert nm.bits_equal(got, want) and nm.bits_equal(got_state, state) and nm.bits_equal(got[:, 1], mu3[:, 1])
    assert g.warnings(0) == g.warnings(1) == _abi.WARN_NOISE_NONFINITE
    want2, state2, _, bad2 = nm.noise(mu3, 0.02, None, ok, nm.ORN_UHL, state, 0.15, 0.0, 1.0)
    got2, got_state2, _ = run_device(torch, g, mu3, 0.02, ok, got_state)
    assert not bad2.any() and nm.bits_equal(got2, want2) and nm.bits_equal(got_state2, state2)
    g.close()


def test_refusals():
    import torch
    g = _lib.Stepper(make_config(n_arenas=1, bots=2, field_size=100, flags=0))
    g.reset(1)
    L = _lib.load()
    one = torch.zeros(64, dtype=torch.float64, device="cuda")
    p = C.c_void_p(one.data_ptr())
    prm = _abi.RewardParams.from_parameters(None)
    # no config
    assert L.aigar_noise(g.h, p, 2, p, None, 0, None, p, None) < 0 and b"noise_config" in L.aigar_last_error()
    assert L.aigar_env_step_ac(g.h, p, p, None, 0, 0, 0, C.byref(prm), p, p, 0, None) < 0
    assert b"noise_config" in L.aigar_last_error()
    with pytest.raises(RuntimeError, match="noise_config"):
        g.noise(one[:4].view(2, 2), one[:1], one[:4].view(2, 2))
    for n in (1, 5):
        with pytest.raises(RuntimeError, match="n_act"):
            g.noise_config(n)
    with pytest.raises(RuntimeError, match="type"):
        g.noise_config(2, 2)
    with pytest.raises(RuntimeError, match="Orn-Uhl"):
        g.noise_config(2, "Orn-Uhl", dt=-1.0)
    # an Orn-Uhl config needs the caller's state; T is bounded
    g.noise_config(2, "Orn-Uhl", "float64")
    assert L.aigar_noise(g.h, p, 2, p, None, 0, None, p, None) < 0 and b"prev" in L.aigar_last_error()
    for T in (0, 17):
        assert L.aigar_noise(g.h, p, 2, p, p, T, p, p, None) < 0 and b"T = " in L.aigar_last_error()
        assert L.aigar_env_step_ac(g.h, p, p, p, T, 0, 0, C.byref(prm), p, p, 0, None) < 0
    assert L.aigar_noise(g.h, p, -1, p, None, 0, p, p, None) < 0
    assert L.aigar_noise(g.h, p, 0, p, None, 0, p, p, None) == 0  # no rows: nothing to do
    g.noise_config(None)
    assert g.noi is None
    # the fifth field's calls: no memory, then a memory without the flag
    idx = torch.zeros(2, dtype=torch.int64, device="cuda")
    ip = C.c_void_p(idx.data_ptr())
    assert L.aigar_exp_extra_get(g.h, ip, 2, p, None) < 0 and b"exp_config" in L.aigar_last_error()
    assert L.aigar_exp_extra_set(g.h, ip, p, 2) < 0 and b"exp_config" in L.aigar_last_error()
    g.exp_config(8)
    assert L.aigar_exp_extra_get(g.h, ip, 2, p, None) < 0 and b"AIGAR_EXP_EXTRA" in L.aigar_last_error()
    assert L.aigar_exp_extra_set(g.h, ip, p, 2) < 0 and b"AIGAR_EXP_EXTRA" in L.aigar_last_error()
    with pytest.raises(RuntimeError, match="AIGAR_EXP_EXTRA"):
        g.exp_extra_set(idx, one[:8].view(2, 4))
    g.close()
    tiled = _lib.Stepper(make_config(bots=4, tile_flags=_abi.TILE_FORCE))
    with pytest.raises(RuntimeError, match="tiled"):
        tiled.noise_config(2)
    tiled.close()
