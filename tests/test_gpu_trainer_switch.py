"""GPU: one handle through every trainer in turn, Q-learning -> CACLA (CACLA-Var, E = 4) -> DPG ->
Q-learning.  The three trainers share the handle's one block of buffers and its one step graph, so
after each switch the configured trainer's one step and three steps equal its Python model bit for
bit (the Case helpers of tests/test_gpu_train.py, tests/test_gpu_actrain.py and
tests/test_gpu_dpg.py), and the step and info calls of the two others are refused, each with its
own message.  65 inputs, batch 17, a prioritized memory, layers of at most 25 units."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu
import test_gpu_actrain as TA  # noqa: E402
import test_gpu_dpg as TD  # noqa: E402
import test_gpu_train as TQ  # noqa: E402

N_IN, BATCH = 65, 17
REFUSALS = {"train": b"no training is configured", "actrain": b"no CACLA training is configured",
            "dpg": b"no DPG training is configured"}


def refused(st, live):
    info = (C.c_int64 * 8)()
    for kind, msg in REFUSALS.items():
        if kind == live:
            continue
        for r in (getattr(st.L, "aigar_%s_step" % kind)(st.h, 1, None), getattr(st.L, "aigar_%s_info" % kind)(st.h, info)):
            assert r < 0 and msg in st.L.aigar_last_error(), (live, kind, st.L.aigar_last_error())


@pytest.fixture
def st():
    """One handle of this test's own that the Case of every trainer module configures; the
    modules' own handles of that width, where they are open, are put back afterwards."""
    mods = (TQ, TA, TD)
    own = [m._G.pop(N_IN, None) for m in mods]
    st = TQ.handle(N_IN)
    TA._G[N_IN] = TD._G[N_IN] = st
    yield st
    st.close()
    for m, old in zip(mods, own):
        del m._G[N_IN]
        if old is not None:
            m._G[N_IN] = old


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
