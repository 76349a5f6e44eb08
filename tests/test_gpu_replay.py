"""GPU: the replay memory (aigar_exp_*) at tolerance 0 -- the golden scripts recorded from
the reference's ReplayBuffer / PrioritizedReplayBuffer, then random op scripts against
tests/replay_model.py at shapes chosen to break the kernels: capacities 5 / 64 / 1000
(it_cap 8 / 64 / 1024; 64 exactly full), state widths 1 / 9 / 123 / 854 in both dtypes
(caller rows aligned to 4 and 8 bytes only), adds that cross the ring's end, carry
masked-out rows or hold exactly capacity rows, updates of 1 / 33 / 257 heavily repeated
indices, samples of 1 / 32 / 300 draws with u = 0 and the largest double below 1."""
import math
import os

import numpy as np
import pytest

from aigar_amd import _abi
from oracle_lib import make_config
from replay_model import ReplayModel, golden_u, load_golden

pytestmark = pytest.mark.gpu
_lib = pytest.importorskip("aigar_amd._lib")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
C3 = (_abi.OBS_PELLET | _abi.OBS_SELF | _abi.OBS_WALL | _abi.OBS_ENEMY | _abi.OBS_VIRUS | _abi.OBS_SELF_LF
      | _abi.OBS_ENEMY_LF)
# state width -> (grid_squares, channels, extras) of a handle whose observation row has it
WIDTHS = {1: (1, _abi.OBS_PELLET, 0), 3: (1, _abi.OBS_PELLET, _abi.EX_FOV | _abi.EX_MASS), 9: (3, _abi.OBS_PELLET, 0),
          123: (11, _abi.OBS_PELLET, _abi.EX_FOV | _abi.EX_MASS),
          854: (11, C3, _abi.EX_LAST_FOV | _abi.EX_FOV | _abi.EX_MASS | _abi.EX_LAST_ACT)}
BELOW_ONE = math.nextafter(1.0, 0.0)


def stepper(width, capacity, prioritized, dtype="float64", alpha=0.6, beta=0.4, seed=0, bots=2):
    g, ch, ex = WIDTHS[width]
    st = _lib.Stepper(make_config(bots=bots, grid_squares=g, channels=ch, extras=ex, virus=bool(ch & _abi.OBS_VIRUS)))
    assert st.obs_len == width
    import torch
    st.set_stream(torch.cuda.current_stream().cuda_stream)  # (ordered with the tensors torch makes and reads)
    st.exp_config(capacity, prioritized=prioritized, alpha=alpha, beta=beta, dtype=dtype, seed=seed)
    return st


def dev(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def sample(st, u, width, dtype):
    import torch
    n = len(u)
    tdt = torch.float64 if dtype == "float64" else torch.float32
    out = {"s": torch.full((n, width), 7.0, dtype=tdt, device="cuda"), "a": torch.full((n, 4), 7.0, dtype=torch.float64,
                                                                                      device="cuda"),
           "r": torch.full((n,), 7.0, dtype=torch.float64, device="cuda"),
           "s2": torch.full((n, width), 7.0, dtype=tdt, device="cuda"),
           "done": torch.full((n,), 7, dtype=torch.uint8, device="cuda")}
    w = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    idx = torch.full((n,), 7, dtype=torch.int64, device="cuda")
    st.exp_sample(w, idx, u=None if u is None else dev(np.asarray(u, np.float64)), **out)
    return idx.cpu().numpy(), w.cpu().numpy(), {k: v.cpu().numpy() for k, v in out.items()}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    v = np.uint64 if a.dtype.itemsize == 8 else np.uint32 if a.dtype.itemsize == 4 else np.uint8
    return np.array_equal(a.view(v), b.view(v))


def check_rows(rows, got, what):
    """rows: the model's transitions (None: outside the memory) against the fetched tensors' rows."""
    for k, row in enumerate(rows):
        assert row is not None, what
        s, a, r, s2, done = row
        assert same_bits(got["s"][k], s), (what, k)
        assert same_bits(got["a"][k], a), (what, k)
        assert same_bits(got["r"][k:k + 1], np.array([r])), (what, k)
        assert same_bits(got["s2"][k], s2), (what, k)
        assert int(got["done"][k]) == int(done), (what, k)


def check_all(st, m, width, dtype, what):
    """Every slot of the memory against the model, and the ring's counters."""
    import torch
    info = st.exp_info()
    assert (info["capacity"], info["size"], info["next_idx"], info["added"]) == (m.cap, m.size, m.next, m.added), what
    if m.size == 0:
        return
    tdt = torch.float64 if dtype == "float64" else torch.float32
    n = m.size
    got = {"s": torch.zeros((n, width), dtype=tdt, device="cuda"), "a": torch.zeros((n, 4), dtype=torch.float64,
                                                                                    device="cuda"),
           "r": torch.zeros(n, dtype=torch.float64, device="cuda"), "s2": torch.zeros((n, width), dtype=tdt, device="cuda"),
           "done": torch.zeros(n, dtype=torch.uint8, device="cuda")}
    st.exp_gather(torch.arange(n, device="cuda"), **got)
    check_rows(m.gather(range(n)), {k: v.cpu().numpy() for k, v in got.items()}, what)


# ------------------------------------------------------------------ (a) golden scripts
@pytest.mark.parametrize("name", ["replay_prio", "replay_uniform"])
def test_golden_script_bit_for_bit(name):
    meta, ops = load_golden(os.path.join(GOLDEN, name + ".npz"))
    st = stepper(3, meta["capacity"], meta["prioritized"], alpha=meta["alpha"], beta=meta["beta"])
    m = ReplayModel(meta["capacity"], meta["prioritized"], meta["alpha"], meta["beta"])  # (the rows' store)
    for k, (kind, op) in enumerate(ops):
        if kind == "add":
            args = [np.ascontiguousarray(op[n]) for n in ("add_s", "add_a", "add_r", "add_s2", "add_done")]
            st.exp_add(*args)
            m.add(*args)
        elif kind == "sample":
            idx, w, got = sample(st, golden_u(op, meta["prioritized"], m.size), 3, "float64")
            assert idx.tolist() == op["samp_idx"].tolist(), "op %d" % k
            assert same_bits(w, op["samp_w"]), "op %d: %r != %r" % (k, w, op["samp_w"])
            assert same_bits(got["r"], op["samp_r"])
            check_rows(m.gather(idx), got, "op %d" % k)
        else:
            st.exp_update_priorities(dev(op["upd_idx"]), dev(op["upd_prio"]))
            m.update(op["upd_idx"], op["upd_prio"])
        info = st.exp_info()
        assert (info["size"], info["next_idx"]) == (op["size"], op["next_idx"]), "op %d" % k
    check_all(st, m, 3, "float64", name)
    st.close()


# ------------------------------------------------------------------ (b) random scripts
def make_rows(rng, n, width, dtype):
    s = rng.standard_normal((n, width)).astype(dtype)
    s2 = rng.standard_normal((n, width)).astype(dtype)
    done = (rng.random(n) < 0.25).astype(np.uint8)
    s2[done != 0] = np.nan
    return s, rng.random((n, 4)), rng.standard_normal(n), s2, done


def run_script(capacity, width, dtype, prioritized, seed):
    rng = np.random.default_rng(seed)
    st = stepper(width, capacity, prioritized, dtype=dtype, alpha=0.7, beta=0.5)
    m = ReplayModel(capacity, prioritized, 0.7, 0.5)

    def add(n, masked, on_device):
        rows = make_rows(rng, n, width, dtype)
        mask = (rng.random(n) < 0.6).astype(np.uint8) if masked else None
        if masked:
            mask[0], mask[1:3] = 0, 1  # (a masked-out row for certain, and at least two rows added)
        if on_device:
            st.exp_add(*[dev(x) for x in rows], mask=None if mask is None else dev(mask))
        else:
            st.exp_add(*rows, mask=mask)
        m.add(*rows, mask=mask)

    def draw(n):
        u = rng.random(n)
        u[0] = 0.0
        if n > 1:
            u[n // 2] = BELOW_ONE
        idx, w, got = sample(st, u, width, dtype)
        want_idx, want_w = m.sample(u)
        assert idx.tolist() == want_idx, "sample of %d" % n
        assert same_bits(w, np.array(want_w)), "weights of %d draws" % n
        assert not m.too_small()
        check_rows(m.gather(idx), got, "sample of %d" % n)

    def update(n):
        idx = rng.integers(0, max(1, min(m.size, 7)), n)  # (heavy duplication: at most 7 distinct slots)
        if n > 1:
            idx[n // 3] = m.size - 1
        prio = rng.random(n) * 3 + 1e-4
        st.exp_update_priorities(dev(idx.astype(np.int64)), dev(prio))
        m.update(idx, prio)

    add(capacity // 2 + 1, True, False)   # some rows masked out; the ring not yet full
    check_all(st, m, width, dtype, "first add")
    draw(1)
    update(1)
    add(capacity - 1, False, True)        # crosses the ring's end
    assert m.added > capacity > m.next
    check_all(st, m, width, dtype, "add across the end")
    draw(32)
    update(33)
    draw(32)
    add(capacity, False, True)            # exactly capacity rows: every slot rewritten
    check_all(st, m, width, dtype, "add of capacity rows")
    draw(300)
    update(257)
    add(min(capacity, 40), True, False)
    draw(32)
    check_all(st, m, width, dtype, "end")
    st.close()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("width", [1, 9, 123, 854])
@pytest.mark.parametrize("capacity", [5, 64, 1000])
def test_random_script_matches_model(capacity, width, dtype):
    run_script(capacity, width, dtype, True, seed=capacity * 1000 + width)


@pytest.mark.parametrize("capacity,width,dtype", [(5, 9, "float32"), (64, 123, "float64"), (1000, 1, "float64")])
def test_random_script_uniform(capacity, width, dtype):
    run_script(capacity, width, dtype, False, seed=capacity + width)


def test_capacity_64_exactly_full():
    """it_cap == capacity == size: the whole leaf level in use, the mass spans leaves [0, 62]."""
    rng = np.random.default_rng(64)
    st, m = stepper(9, 64, True), ReplayModel(64, True)
    rows = make_rows(rng, 64, 9, "float64")
    st.exp_add(*rows)
    m.add(*rows)
    assert m.size == m.it_cap == 64 and m.next == 0
    prio = rng.random(64) * 2 + 0.01
    st.exp_update_priorities(dev(np.arange(64)), dev(prio))
    m.update(np.arange(64), prio)
    u = np.r_[0.0, BELOW_ONE, rng.random(30)]
    idx, w, got = sample(st, u, 9, "float64")
    want_idx, want_w = m.sample(u)
    assert idx.tolist() == want_idx and same_bits(w, np.array(want_w))
    assert max(want_idx) <= 62  # (the reference's quirk: the newest-indexed item is never drawn)
    check_rows(m.gather(idx), got, "full")
    st.close()


def _skip_case(make_batch):
    """Updates of 1, 33 and 257 entries, each with entries the update must skip."""
    rng = np.random.default_rng(11)
    st, m = stepper(9, 64, True), ReplayModel(64, True)
    rows = make_rows(rng, 40, 9, "float64")  # size 40 of 64
    st.exp_add(*rows)
    m.add(*rows)
    for n in (1, 33, 257):
        idx, prio, skipped = make_batch(rng, n)
        before = (m.total(), m.max_priority)
        st.exp_update_priorities(dev(idx), dev(prio))
        m.update(idx, prio)
        if n == 1:
            assert skipped.all() and (m.total(), m.max_priority) == before  # the one entry is the skipped one
        u = rng.random(32)
        got_idx, w, _ = sample(st, u, 9, "float64")
        want_idx, want_w = m.sample(u)
        assert got_idx.tolist() == want_idx and same_bits(w, np.array(want_w)), n
    # a skipped entry moved neither a leaf nor max_priority: new rows still enter at the model's leaf
    rows = make_rows(rng, 5, 9, "float64")
    st.exp_add(*rows)
    m.add(*rows)
    u = rng.random(64)
    got_idx, w, _ = sample(st, u, 9, "float64")
    want_idx, want_w = m.sample(u)
    assert got_idx.tolist() == want_idx and same_bits(w, np.array(want_w))
    check_all(st, m, 9, "float64", "skip case")  # (the handle raised no error)
    st.close()


def test_update_skips_priorities_not_above_zero():
    def batch(rng, n):
        idx = rng.integers(0, 6, n).astype(np.int64)
        prio = rng.random(n) * 2 + 0.01
        skipped = np.zeros(n, bool)
        skipped[::4] = True
        prio[skipped] = np.where(np.arange(skipped.sum()) % 2 == 0, 0.0, -50.0)  # (-50: must not reach max_priority)
        return idx, prio, skipped
    _skip_case(batch)


def test_update_skips_indices_outside_the_memory():
    def batch(rng, n):
        idx = rng.integers(0, 6, n).astype(np.int64)
        prio = rng.random(n) * 2 + 0.01
        skipped = np.zeros(n, bool)
        skipped[::4] = True
        idx[skipped] = np.where(np.arange(skipped.sum()) % 2 == 0, 40 + rng.integers(0, 24, skipped.sum()), -1)
        prio[skipped] = 99.0  # (must not reach max_priority)
        return idx, prio, skipped
    _skip_case(batch)


# ------------------------------------------------------------------ (c) too small a memory
@pytest.mark.parametrize("prioritized,rows", [(False, 0), (True, 0), (True, 1)])
def test_too_small_memory_gives_minus_one_and_nan(prioritized, rows):
    rng = np.random.default_rng(3)
    st, m = stepper(9, 5, prioritized), ReplayModel(5, prioritized)
    if rows:
        r = make_rows(rng, rows, 9, "float64")
        st.exp_add(*r)
        m.add(*r)
    for u in ([0.0, 0.5, BELOW_ONE], None):
        idx, w, got = sample(st, u, 9, "float64") if u is not None else sample_own(st, 3, 9)
        assert idx.tolist() == [-1, -1, -1] and np.isnan(w).all()
        assert all((v == 7).all() for v in got.values())  # outputs untouched
    # the handle still works: fill it, draw, update
    r = make_rows(rng, 4, 9, "float64")
    st.exp_add(*r)
    m.add(*r)
    st.exp_update_priorities(dev(np.array([0, 1], np.int64)), dev(np.array([2.0, 0.5])))
    m.update([0, 1], [2.0, 0.5])
    u = rng.random(32)
    idx, w, got = sample(st, u, 9, "float64")
    want_idx, want_w = m.sample(u)
    assert idx.tolist() == want_idx and same_bits(w, np.array(want_w))
    check_rows(m.gather(idx), got, "after the empty draws")
    check_all(st, m, 9, "float64", "after the empty draws")
    st.close()


# ------------------------------------------------------------------ (d) the memory's own draws
def sample_own(st, n, width):
    import torch
    out = {"s": torch.full((n, width), 7.0, dtype=torch.float64, device="cuda"),
           "a": torch.full((n, 4), 7.0, dtype=torch.float64, device="cuda"),
           "r": torch.full((n,), 7.0, dtype=torch.float64, device="cuda"),
           "s2": torch.full((n, width), 7.0, dtype=torch.float64, device="cuda"),
           "done": torch.full((n,), 7, dtype=torch.uint8, device="cuda")}
    w = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    idx = torch.full((n,), 7, dtype=torch.int64, device="cuda")
    st.exp_sample(w, idx, u=None, **out)
    return idx.cpu().numpy(), w.cpu().numpy(), {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("prioritized", [False, True])
def test_own_draws_are_seeded_and_advance(prioritized):
    rng = np.random.default_rng(5)
    rows = make_rows(rng, 50, 9, "float64")
    hs = [stepper(9, 64, prioritized, seed=1234) for _ in range(2)]
    for st in hs:
        st.exp_add(*rows)
    (i0, w0, g0), (i1, w1, g1) = [sample_own(st, 300, 9) for st in hs]
    assert np.array_equal(i0, i1) and same_bits(w0, w1)
    assert ((i0 >= 0) & (i0 < 50)).all()
    assert same_bits(g0["s"], rows[0][i0]) and same_bits(g0["r"], rows[2][i0])  # the rows of those indices
    i2, _, _ = sample_own(hs[0], 300, 9)
    assert ((i2 >= 0) & (i2 < 50)).all() and not np.array_equal(i2, i0)  # the second call draws anew
    other = stepper(9, 64, prioritized, seed=99)
    other.exp_add(*rows)
    assert not np.array_equal(sample_own(other, 300, 9)[0], i0)  # another seed, another stream
    for st in hs + [other]:
        st.close()


# ------------------------------------------------------------------ refusals
def test_config_refusals_and_free():
    st = stepper(9, 5, True)
    with pytest.raises(RuntimeError, match="replay memory"):
        st.pixel_config(12)
    with pytest.raises(RuntimeError, match="capacity"):
        st.exp_config(1)  # below the handle's 2 players
    st.exp_config(None)
    with pytest.raises(RuntimeError, match="no replay memory"):
        st.exp_info()
    st.pixel_config(12)  # (free again)
    st.exp_config(8, dtype="float32")
    assert st.exp[0] == (12, 12, 1) and st.exp_info()["capacity"] == 8
    st.close()
