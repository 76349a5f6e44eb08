"""The worlds of the SPG tests: the data of a case (weights, a filled memory with its fifth
field, the settings) and the model's side of a run, shared by tests/test_spg_model.py (which
checks on the CPU that every run is worth comparing) and tests/test_gpu_spg.py (which runs the
same worlds on the device).  No device is needed here."""
import numpy as np

import net_model as M
import spg_model as SM
from replay_model import ReplayModel

CAP = 64


class World:
    """Weights, memory rows and settings.  Magnitudes as tests/test_gpu_dpg.py's: states and
    weights 2^-30 .. 2^hi with subnormals and signed zeros, rewards 2^-10 .. 2^5 of both signs,
    stored actions in [0, 1).  Half of the slots start with a valid fifth field."""

    def __init__(self, n_in, actor, critic, batch, ha="relu", hc="relu", dtype="float64", prio=False, n_mem=40, hi=2,
                 seed=0, target_steps=0, min_size=0, done=None, rewards=None, tau=0.25, lr=1e-2, samples=5, moving=True,
                 replace=True, prio_evals=1, noise=0.3, noise_decay=2.0 ** -9, critic_weights=None, zseed=0):
        self.rng = rng = np.random.default_rng(1000 * n_in + 10 * batch + seed)
        self.n_in, self.batch, self.dtype, self.prio, self.n_mem = n_in, batch, dtype, prio, n_mem
        self.actor, self.critic, self.ha, self.hc = tuple(actor), tuple(critic), ha, hc
        self.n_act = n_act = self.actor[-1]
        np_dt = np.float64 if dtype == "float64" else np.float32
        self.a0 = M.make_weights(rng, n_in, self.actor, hi=hi)
        self.c0 = M.make_weights(rng, n_in + n_act, self.critic, hi=hi) if critic_weights is None else critic_weights
        self.rows = None
        if n_mem:
            s = M.mixed(rng, (n_mem, n_in), hi=3)
            s2 = M.mixed(rng, (n_mem, n_in), hi=3)
            if dtype == "float64":  # float64 rows that are not float32 values: one rounding each
                s, s2 = (np.where(x == 0, x, x.astype(np.float64) * (1 + 2.0 ** -30)) for x in (s, s2))
            a = np.zeros((n_mem, 4))
            a[:, :n_act] = rng.random((n_mem, n_act))  # (float64 values that are not float32 values)
            r = M.mixed(rng, (n_mem,), lo=-10, hi=5).astype(np.float64) if rewards is None else rewards
            d = np.asarray((rng.random(n_mem) < 0.25) if done is None else done, bool)
            s2 = s2.astype(np_dt)
            s2[d] = np.nan  # (the decision's transitions: a dead player's new state is the NaN row)
            self.rows = (s.astype(np_dt), a, np.asarray(r, np.float64), s2, d.astype(np.uint8))
        self.extra = np.full((CAP, 4), np.nan)
        self.valid = np.zeros(CAP, np.uint8)
        if replace and n_mem:
            v = np.flatnonzero(rng.random(n_mem) < 0.5)
            self.extra[v] = 0.0
            self.extra[v, :n_act] = rng.random((len(v), n_act))
            self.valid[v] = 1
        self.kw = dict(critic_lr=lr, actor_lr=lr / 2, beta1=0.9, beta2=0.999, epsilon=1e-7, discount=0.85,
                       target_steps=target_steps, min_size=min_size, tau=tau, samples=samples, moving=moving,
                       replace=replace, prio_evals=prio_evals, noise=noise, noise_decay=noise_decay)
        self.zrng = np.random.default_rng(77 + zseed)

    def draws(self, n):
        """The memory's draws u [n][B] and the search's uniforms zu [n][B][K][2][16][2]."""
        K = self.kw["samples"]
        return self.rng.random((n, self.batch)), self.zrng.random((n, self.batch, K, 2, 16, 2))


class ModelRun:
    """The model's side of a run: the memory, its fifth field and the trainer."""

    def __init__(self, w):
        self.w = w
        self.rm = ReplayModel(CAP, w.prio)
        if w.rows is not None:
            self.rm.add(*w.rows)
        self.extra, self.valid = w.extra.copy(), w.valid.copy()
        self.written = np.zeros(CAP, bool)  # slots whose extra a step of this run wrote
        self.own_reads = 0                  # ... and how many of those a later search read
        self.tr = SM.Trainer(w.a0, w.c0, w.batch, hidden_actor=w.ha, hidden_critic=w.hc, **w.kw)
        self.last_idx = None

    def step(self, u, zu):
        tr = self.tr
        idx, wt = self.rm.sample(list(u))
        self.last_idx = idx
        if not tr.can_draw(self.rm.size) or idx[0] < 0:
            tr.skip()
            return
        rows = self.rm.gather(idx)
        s, a, r, s2, d = (np.array([row[k] for row in rows]) for k in range(5))
        i = np.asarray(idx)
        prio, back = tr.step(s, a, r, s2, d, np.asarray(wt), self.extra[i], self.valid[i], zu)
        if prio is None:
            return
        if tr.K > 0 and tr.replace:
            self.own_reads += int((self.written[i] & self.valid[i].astype(bool)).sum())
        self.rm.update(idx, prio)  # (a uniform memory keeps none)
        if back is not None:
            SM.write_back(self.extra, self.valid, idx, back)
            self.written[i] = True

    def run(self, u, zu):
        for k in range(len(u)):
            self.step(u[k], zu[k])

    def worth_comparing(self, sources=True):
        """The run selected a row and left one unselected; with K > 0 every kind of source won
        once; with replace a search read an extra that an earlier step wrote."""
        tr = self.tr
        ok = tr.seen[0] > 0 and tr.seen[1] > 0
        if sources and tr.K > 0:
            kinds = {min(v, SM.SRC_SAMPLE) for v in tr.sources}
            want = {SM.SRC_STORED, SM.SRC_MU, SM.SRC_SAMPLE} | ({SM.SRC_EXTRA} if tr.replace else set())
            ok = ok and want <= kinds
        if sources and tr.K > 0 and tr.replace:
            ok = ok and self.own_reads > 0
        return ok


# The Stepper-level cases of tests/test_gpu_spg.py: name -> (World's arguments, steps).  Shapes: the
# batches 1 / 15 / 16 / 17 / 33; 2..4 actions; state widths 3 (no whole 64-chunk below it), 61 (with
# 4 actions the action columns straddle a chunk boundary), 62 (with 2 actions the input ends on
# one), 64 (the actions open a chunk) and 130; critics with 0, 1 and 2 hidden layers of widths 17,
# 100 and 256; K 0 / 1 / 5 / 8; moving and replace on and off; both dtypes; both memories and
# both priorities.
def _cases():
    c = {}
    for b in (1, 15, 16, 17, 33):
        c["batch%d" % b] = (dict(n_in=61, actor=(16, 16, 3), critic=(17, 25, 1), batch=b, prio=True, seed=1), 8 if b == 1 else 4)
    for n_in, n_act in ((3, 2), (61, 4), (62, 2), (64, 3), (130, 2)):
        for dt in ("float64", "float32"):
            c["w%d_a%d_%s" % (n_in, n_act, dt)] = (dict(n_in=n_in, actor=(15, n_act), critic=(25, 1), batch=17, dtype=dt,
                                                       prio=(n_in % 2 == 1), seed=2), 4)
    for name, critic in (("h0", (1,)), ("h1_17", (17, 1)), ("h1_100", (100, 1)), ("h1_256", (256, 1)),
                         ("h2", (100, 17, 1)), ("h2_256", (17, 256, 1))):
        c["critic_" + name] = (dict(n_in=61, actor=(16, 3), critic=critic, batch=18, prio=True, seed=3,
                                    hc="linear" if name == "h2" else "relu"), 4)
    for K in (0, 1, 5, 8):
        for moving in (False, True):
            for replace in (False, True):
                c["K%d_m%d_r%d" % (K, moving, replace)] = (dict(n_in=62, actor=(15, 2), critic=(25, 1), batch=17, samples=K,
                                                                moving=moving, replace=replace, prio=bool(K % 2), seed=4), 4)
    for prio in (False, True):
        for pe in (0, 1):
            c["prio%d_evals%d" % (prio, pe)] = (dict(n_in=64, actor=(15, 3), critic=(25, 1), batch=16, prio=prio,
                                                     prio_evals=pe, seed=5), 4)
    return c


CASES = _cases()


def load_golden(path):
    """tests/golden/spg_cases.npz (tools/golden/gen_spg_golden.py) -> its arrays, with `zu` [R][5][2][16][2]:
    every row's recorded attempts, padded with (0.5, 0.5), an attempt that is rejected (r2 = 0)."""
    g = dict(np.load(path))
    R, C = len(g["s"]), len(g["K"])
    B = R // C
    zu = np.full((R, 5, 2, 16, 2), 0.5)
    call = at = 0
    for c in range(C):
        for r in range(B):
            for x in range(int(g["K"][c])):
                for pair in range(2):
                    n = int(g["cnt"][call][pair])
                    zu[c * B + r, x, pair, :n] = g["att"][at:at + n]
                    at += n
                call += 1
    assert call == len(g["cnt"]) and at == len(g["att"])
    g["zu"], g["B"] = zu, B
    return g
