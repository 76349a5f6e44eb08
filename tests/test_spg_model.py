"""CPU: the SPG model (tests/spg_model.py) against the reference's own train_actor_OCACLA
(tests/golden/spg_cases.npz, tools/golden/gen_spg_golden.py): every recorded pick, the selection,
updated_actions and count; the gated batch against the reference's compacted batch; and that the
worlds of the GPU tests are worth comparing (tests/spg_worlds.py)."""
import os

import numpy as np
import pytest

import dpg_model as DM
import net_model as M
import spg_model as SM
import spg_worlds as W
import train_model as T
from cacla_model import actor_delta, sigmoid_rows

F32 = np.float32


@pytest.fixture(scope="module")
def golden(golden_dir):
    return W.load_golden(os.path.join(golden_dir, "spg_cases.npz"))


def test_golden_covers_what_it_is_there_for(golden):
    g = golden
    assert set(g["n_act"]) == {2, 3, 4} and set(g["K"]) == {0, 1, 5}
    assert len(set(zip(g["n_act"], g["K"], g["moving"], g["replace"]))) == 36
    sel, pick = g["selected"].astype(bool), g["pick"]
    assert sel.any() and (~sel).any() and {0, 1, 2, 3} <= set(pick) and (pick > 3).any()
    assert (g["cnt"] > 1).any(), "no rejected attempt"


def test_model_reproduces_the_references_search(golden):
    g, B = golden, golden["B"]
    for c in range(len(g["K"])):
        n, K = int(g["n_act"][c]), int(g["K"][c])
        i = {2: 0, 3: 1, 4: 2}[n]
        theta = [(g["w0"][i][:3 + n], g["b0"][i]), (g["w1"][i], g["b1"][i])]
        rows = slice(c * B, (c + 1) * B)
        s, a, mu = g["s"][rows], g["a"][rows][:, :n], g["mu"][rows][:, :n]
        q = lambda x, act: M.forward(DM.sa_rows(x, act), theta, "relu", "linear")[:, 0]
        qmu = q(s, mu)
        best, be, src, exhausted = SM.search(lambda r, act: q(s[r], act), mu, a, g["evals"][rows], qmu, g["extra"][rows],
                                             g["valid"][rows], K, bool(g["moving"][c]), bool(g["replace"][c]),
                                             float(g["noise"][c]), g["zu"][rows])
        sel = be > qmu
        assert exhausted == 0
        assert sel.tolist() == g["selected"][rows].astype(bool).tolist(), c
        assert int(sel.sum()) == g["count"][c], c
        want = g["pick"][rows]
        assert src[sel].tolist() == want[sel].tolist(), c
        if K:  # (an unselected row ended on mu's value, or on a stored action that ties with it)
            assert all(k == SM.SRC_MU or be[r] == qmu[r] for r, k in enumerate(src) if not sel[r]), c
        updated = a.copy()
        updated[sel] = best[sel]
        assert np.array_equal(updated, g["updated"][rows][:, :n]), c


def test_compacted_and_gated_batches_give_equal_gradients():
    """The reference trains on the selected rows only; the device keeps every row and gives the
    others a +0.0f delta.  Both give == gradients (the sign of a zero aside)."""
    rng = np.random.default_rng(3)
    for n_in, units, B in ((5, (7, 3), 9), (20, (16, 17, 2), 33)):
        theta = M.make_weights(rng, n_in, units, hi=1)
        s = M.mixed(rng, (B, n_in), hi=2).astype(np.float64)
        best = rng.random((B, units[-1]))
        sel = rng.random(B) < 0.5
        assert 0 < sel.sum() < B
        hs, y = T.forward_saved(s, theta, "relu")
        mu = sigmoid_rows(y.astype(F32))
        gated = T.backward(hs, theta, actor_delta(mu, best, sel), "relu")
        hs_c, y_c = T.forward_saved(s[sel], theta, "relu")
        mu_c = sigmoid_rows(y_c.astype(F32))
        assert np.array_equal(mu_c, mu[sel])
        compact = T.backward(hs_c, theta, actor_delta(mu_c, best[sel], np.ones(int(sel.sum()), bool)), "relu")
        for (gw, gb), (cw, cb) in zip(gated, compact):
            assert np.array_equal(gw, cw) and np.array_equal(gb, cb) and np.abs(gw).max() > 0


@pytest.mark.parametrize("name", list(W.CASES))
def test_the_gpu_tests_worlds_are_worth_comparing(name):
    """Over each run the model selects a row and leaves one unselected; with K > 0 every kind of
    source wins a row (stored action, extra, mu, a sample); with replace a search reads an extra
    that an earlier step of the run wrote."""
    kw, n = W.CASES[name]
    w = W.World(**kw)
    run = W.ModelRun(w)
    u, zu = w.draws(n)
    run.run(u, zu)
    tr = run.tr
    assert tr.c.t == n and tr.skipped == 0 and not tr.nonfinite
    assert run.worth_comparing(sources=w.batch > 1), (tr.seen, sorted(tr.sources), run.own_reads)


def test_a_batch_of_one_row_meets_the_conditions_over_its_run():
    kw, n = W.CASES["batch1"]
    run = W.ModelRun(W.World(**kw))
    run.run(*run.w.draws(n))
    assert run.tr.seen[0] > 0 and run.tr.seen[1] > 0 and len(run.tr.sources) > 2


def test_own_draws_are_order_free_and_keyed():
    key = np.array([11, 12], np.uint64)
    a = SM.own_zu(3, 2, 0, 9, key)
    assert a.shape == (3, 2, 2, 16, 2) and (a >= 0).all() and (a < 1).all()
    assert np.array_equal(a[1], SM.own_zu(2, 2, 0, 9, key)[1])  # (a row's draws do not depend on the batch)
    for other in (SM.own_zu(3, 2, 1, 9, key), SM.own_zu(3, 2, 0, 10, key), SM.own_zu(3, 2, 0, 9, key + np.uint64(1))):
        assert not np.array_equal(a, other)
    assert len(np.unique(a)) == a.size
