"""One SPG (Sampled Policy Gradient) training step in plain Python: the specification of
aigar_spg_step (include/aigar.h), built on net_model, train_model, cacla_model,
dpg_model and noise_model, and compared bit for bit with the device (tests/test_gpu_spg.py).

The reference (actorCritic.py, OCACLA_ENABLED: ActorCritic.learn 730-733,
train_critic_DPG(get_evals=True) 986-1029, train_actor_OCACLA 860-919): the critic Q(s, a) is
trained as DPG's; then every row of the batch searches for an action that the updated critic
rates above the actor's own -- the stored action, the action a former search left in the
memory's fifth field, the actor's action and K Gaussian samples around the best so far
(OCACLA_MOVING_GAUSSIAN) or around the actor's action -- and the actor is regressed towards
the winners of the rows that found one.  With OCACLA_REPLACE_TRANSITIONS the winners go back
into the fifth field of the drawn slots.

Differences from the reference, as the header states them: the actor trains from the first
step; both targets are updated (softly or by the hard copy); the write-back does not depend on
the memory being prioritized; Gaussian search noise only; the search draws are the caller's
uniforms or order-free Philox draws; K <= MAX_SAMPLES."""
import numpy as np

import dpg_model as DM
import noise_model as NM
import train_model as T
from cacla_model import actor_delta, critic_delta, sigmoid_rows, td_errors
from net_model import F32

PRIO_EPS = T.PRIO_EPS
MAX_SAMPLES = 8
ST_SPG = 12  # the Philox stream word of the search's own draws
# where a row's best action came from
SRC_STORED, SRC_EXTRA, SRC_MU, SRC_SAMPLE = 0, 1, 2, 3  # (sample x is SRC_SAMPLE + x)


def own_draws(row, pair, x, ordinal, seed, key):
    """The 16 attempts of (row, sample x, pair) of the step `ordinal`: attempts 2 b and 2 b + 1 are
    words {0, 1} and {2, 3} of Philox4x64-10 keyed by arena 0's key at the counter (row, ST_SPG |
    pair << 8 | b << 16 | x << 24, ordinal, seed); numpy's Philox returns the block of counter + 1."""
    out = []
    for b in range(NM.OWN_T // 2):
        c1 = ST_SPG | pair << 8 | b << 16 | x << 24
        c = (int(row) | c1 << 64 | int(ordinal) << 128 | (int(seed) & (2 ** 64 - 1)) << 192) - 1
        ctr = [(c % 2 ** 256) >> (64 * k) & (2 ** 64 - 1) for k in range(4)]
        raw = np.random.Philox(key=np.array(key, np.uint64), counter=np.array(ctr, np.uint64)).random_raw(4)
        w = [float(int(v) >> 11) * NM.GRID for v in raw]
        out += [(w[0], w[1]), (w[2], w[3])]
    return out


def own_zu(B, K, ordinal, seed, key):
    """[B][K][2][16][2]: what a step with zu = NULL draws."""
    zu = np.zeros((B, max(K, 1), 2, NM.OWN_T, 2))
    for r in range(B):
        for x in range(K):
            for pair in range(2):
                zu[r, x, pair] = own_draws(r, pair, x, ordinal, seed, key)
    return zu[:, :K]


def search(qf, mu, a, q_old, qmu, extra, valid, K, moving, replace, noise, zu):
    """Every row's search; the rows do not depend on one another.  qf(rows [n] int, actions
    [n][n_act] float64) -> Q([s_row, action]) [n] with the critic as just updated.  Returns (best
    [B][n_act], best_eval [B], source [B], exhausted pairs).  Every comparison is a float64 `>`:
    a NaN never wins."""
    mu, a = np.asarray(mu, np.float64), np.asarray(a, np.float64)
    B, n_act = mu.shape
    best, be, src = a[:, :n_act].copy(), np.array(q_old, np.float64), np.full(B, SRC_STORED, np.int64)
    every, exhausted = np.arange(B), 0

    def take(rows, cand, ev, source):
        with np.errstate(invalid="ignore"):
            win = ev > be[rows]
        best[rows[win]], be[rows[win]], src[rows[win]] = cand[win], ev[win], source

    if K > 0:
        v = np.flatnonzero(np.asarray(valid).astype(bool)) if replace else every[:0]
        if len(v):
            cand = np.asarray(extra, np.float64)[v, :n_act]
            take(v, cand, np.asarray(qf(v, cand), np.float64), SRC_EXTRA)
        take(every, mu, np.asarray(qmu, np.float64), SRC_MU)
        for x in range(K):
            base = best if moving else mu
            cand = np.zeros((B, n_act))
            for r in range(B):
                cand[r], _, e, _ = NM.noise_row(base[r].tolist(), noise, zu[r][x])
                exhausted += e
            take(every, cand, np.asarray(qf(every, cand), np.float64), SRC_SAMPLE + x)
    return best, be, src, exhausted


class Trainer(DM.Trainer):
    """The device's SPG training state: DPG's, the search's settings and the noise double."""

    def __init__(self, actor, critic, batch, samples=5, moving=True, replace=True, prio_evals=1, noise=0.1,
                 noise_decay=1.0, **kw):
        kw.setdefault("q_increase", 0.0)
        DM.Trainer.__init__(self, actor, critic, batch, **kw)
        assert 0 <= samples <= MAX_SAMPLES and self.n_act <= 4
        self.K, self.moving, self.replace, self.prio_evals = int(samples), bool(moving), bool(replace), int(prio_evals)
        self.noise, self.noise_decay = float(noise), float(noise_decay)
        self.aempty = self.selected = self.ordinal = 0
        self.exhausted = 0
        self.src = self.sel = self.best = None
        self.sources = set()  # every source a row's best came from, over the run
        self.seen = [0, 0]    # rows left unselected / selected, over the run
        self.extras_read = 0  # valid extras that entered a search

    def reset(self):
        DM.Trainer.reset(self)
        self.ordinal = 0

    def info(self):
        return (self.c.t, self.skipped, self.since, self.a.t, self.askipped, self.aempty, self.selected, 0)

    def skip(self):
        self.skipped += 1
        self.ordinal += 1
        return None, None

    def step(self, s, a, rew, s2, done, w, extra, valid, zu, size=None):
        """One step on a drawn batch -> (priorities [B], extra rows [B][4] to write back or None);
        (None, None) when the step is skipped.  a, extra [B][4]; valid [B]; zu [B][K][2][16][2]."""
        if size is not None and not self.can_draw(size):
            return self.skip()
        s, s2, a = np.asarray(s), np.asarray(s2), np.asarray(a, np.float64)
        n_act, B = self.n_act, len(a)
        # the critic half (dpg_model's, entry for entry)
        mu2 = self.mu(s2, self.target_a)
        q2 = self.q(DM.sa_rows(s2, mu2), self.target_c)
        hs, q = T.forward_saved(DM.sa_rows(s, a[:, :n_act]), self.c.theta, self.hc, self.fma)
        q_old = np.asarray(q[:, 0], np.float64)
        self.q_old = q_old
        self.td = td = td_errors(q_old, q2, rew, done, self.discount)
        if not np.isfinite(td).all():
            self.nonfinite = True
            return self.skip()
        self.c.apply(T.backward(hs, self.c.theta, critic_delta(td, w), self.hc, self.fma), self.b1, self.b2, self.eps)
        prio = (np.abs(q_old) if self.prio_evals else np.abs(td)) + PRIO_EPS
        # the search: the critic as just updated, the actor as it is
        hsa, y = T.forward_saved(s, self.a.theta, self.ha, self.fma)
        mu = sigmoid_rows(y.astype(F32))
        qmu = self.q(DM.sa_rows(s, mu), self.c.theta)
        qf = lambda rows, act: self.q(DM.sa_rows(s[rows], act), self.c.theta)
        best, be, src, ex = search(qf, mu, a, q_old, qmu, extra, valid, self.K, self.moving, self.replace, self.noise, zu)
        with np.errstate(invalid="ignore"):
            sel = be > qmu
        self.exhausted += ex
        if self.K > 0 and self.replace:
            self.extras_read += int(np.asarray(valid).astype(bool).sum())
        self.best, self.sel, self.src = best, sel, src
        self.sources |= set(int(v) for v in src)
        self.seen[0] += int((~sel).sum())
        self.seen[1] += int(sel.sum())
        # the actor half
        self.selected = count = int(sel.sum())
        if count == 0:
            self.aempty += 1
        else:
            self.delta_a = actor_delta(mu, best, sel)
            if np.isfinite(self.delta_a).all():
                self.a.apply(T.backward(hsa, self.a.theta, self.delta_a, self.ha, self.fma), self.b1, self.b2, self.eps)
            else:
                self.nonfinite = True
                self.askipped += 1
        # the write-back
        rows = None
        if self.replace:
            rows = a.copy()
            rows[sel] = 0.0
            rows[sel, :n_act] = best[sel]
        # the tail
        self.since += 1
        self.ordinal += 1
        if self.tau > 0:
            self.target_a = DM.soft_update(self.target_a, self.a.theta, self.tau)
            self.target_c = DM.soft_update(self.target_c, self.c.theta, self.tau)
        elif self.target_steps > 0 and self.c.t % self.target_steps == 0:
            self.sync_target()
        self.noise = self.noise * self.noise_decay
        return prio, rows


def write_back(extra, valid, idx, rows):
    """aigar_exp_extra_set on the model's side arrays: the last entry of a repeated index wins."""
    for j, i in enumerate(idx):
        extra[i] = rows[j]
        valid[i] = 1
