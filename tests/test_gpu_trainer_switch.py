"""GPU: one handle through every trainer in turn, Q-learning -> CACLA (CACLA-Var, E = 4) -> DPG ->
Q-learning, and another through the two Q(s, a) trainers, DPG -> SPG (fused 0, then 1) -> DPG.  The
trainers share the handle's one block of buffers and its one step graph, and DPG and SPG also the
critic half, the setup and the tail's body, so after each switch the configured trainer's one step
and three steps equal its Python model bit for bit (the Case helpers of tests/test_gpu_train.py,
tests/test_gpu_actrain.py, tests/test_gpu_dpg.py and tests/test_gpu_spg.py), and the step and info
calls of the others are refused, each with its own message.  65 or 64 inputs, batch 17 (one full
16-row tile and one with a single row), a prioritized memory, layers of at most 25 units."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu
import test_gpu_actrain as TA  # noqa: E402
import test_gpu_dpg as TD  # noqa: E402
import test_gpu_spg as TS  # noqa: E402
import test_gpu_train as TQ  # noqa: E402

N_IN, N_QSA, BATCH = 65, 64, 17
REFUSALS = {"train": b"no training is configured", "actrain": b"no CACLA training is configured",
            "dpg": b"no DPG training is configured", "spg": b"no SPG training is configured"}


def refused(st, live):
    info = (C.c_int64 * 8)()
    for kind, msg in REFUSALS.items():
        if kind == live:
            continue
        more = (None,) if kind == "spg" else ()  # (aigar_spg_step takes the search's uniforms too)
        for r in (getattr(st.L, "aigar_%s_step" % kind)(st.h, 1, None, *more),
                  getattr(st.L, "aigar_%s_info" % kind)(st.h, info)):
            assert r < 0 and msg in st.L.aigar_last_error(), (live, kind, st.L.aigar_last_error())


def shared(mods, width):
    """One handle of this test's own that the Case of every module in mods configures; the
    modules' own handles of that width, where they are open, are put back afterwards."""
    own = [m._G.pop(width, None) for m in mods]
    st = mods[0].handle(width)
    for m in mods[1:]:
        m._G[width] = st
    yield st
    st.close()
    for m, old in zip(mods, own):
        del m._G[width]
        if old is not None:
            m._G[width] = old


@pytest.fixture
def st():
    yield from shared((TQ, TA, TD), N_IN)


@pytest.fixture
def st_qsa():
    yield from shared((TD, TS), N_QSA)


def test_one_handle_through_q_cacla_dpg_and_q_again(st):
    c = TQ.Case(N_IN, (17, 25), BATCH, prio=True, seed=1)
    refused(st, "train")
    TQ.one_and_three(c, "q")
    c = TA.Case(N_IN, (16, 16, 3), (17, 25, 1), BATCH, prio=True, E=4, seed=1)
    assert c.st is st
    refused(st, "actrain")
    TA.one_and_three(c, "cacla after q")
    c = TD.Case(N_IN, (16, 16, 3), (17, 25, 1), BATCH, prio=True, seed=19)
    assert c.st is st
    refused(st, "dpg")
    TD.one_and_three(c, "dpg after cacla")
    c = TQ.Case(N_IN, (17, 25), BATCH, prio=True, seed=1)
    assert c.st is st
    refused(st, "train")
    TQ.one_and_three(c, "q after dpg")


def spg_one_and_three(c, what):
    c.steps(1)
    assert c.tr.c.t == 1 and c.tr.a.t == 1, "the model skipped a step or a half the case means to apply"
    c.check((what, 1))
    c.steps(2)
    assert c.tr.c.t == 3 and c.tr.a.t == 3
    c.check((what, 3))
    assert TS.moved(c.tr.c.theta, c.w.c0) > 0 and TS.moved(c.tr.a.theta, c.w.a0) > 0, "a network did not move"
    assert TS.moved(c.tr.target_c, c.w.c0) > 0 and TS.moved(c.tr.target_a, c.w.a0) > 0, "a target did not move"


def test_one_handle_through_dpg_spg_and_dpg_again(st_qsa):
    st = st_qsa
    dpg = dict(prio=True, extra=True, seed=19)
    spg = dict(n_in=N_QSA, actor=(16, 16, 3), critic=(17, 25, 1), batch=BATCH, prio=True, seed=19)
    c = TD.Case(N_QSA, (16, 16, 3), (17, 25, 1), BATCH, **dpg)
    assert c.st is st
    refused(st, "dpg")
    TD.one_and_three(c, "dpg")
    for fused in (0, 1):
        c = TS.Case(fused=fused, **spg)
        assert c.st is st and c.w.kw["replace"] and c.w.kw["prio_evals"]
        refused(st, "spg")
        spg_one_and_three(c, "spg fused %d after %s" % (fused, "spg" if fused else "dpg"))
    c = TD.Case(N_QSA, (16, 16, 3), (17, 25, 1), BATCH, **dpg)
    assert c.st is st
    refused(st, "dpg")
    TD.one_and_three(c, "dpg after spg")
