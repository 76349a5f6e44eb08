"""One DPG training step in plain Python: the specification of aigar_dpg_step (include/aigar.h;
DESIGN.md §4n), built on net_model, train_model and cacla_model, checked against torch.autograd
(tests/test_dpg_model.py) and compared bit for bit with the device (tests/test_gpu_dpg.py).

The reference (actorCritic.py, ALGORITHM == "DPG"): train_critic_DPG fits Q(s, a) to
rew + discount Q'(s2, mu'(s2)) with the memory's importance weights; train_actor_DPG fits the
combined model Q(s, mu(s)), the critic's weights frozen, to Q'(s, mu'(s)) + DPG_Q_VAL_INCREASE, so
the actor's gradient is the critic's error carried through its first layer onto the action
columns of its input (dQ/da) times the sigmoid head's mu (1 - mu); both targets follow their
networks softly (tau) or by a hard copy.  The critic's input row is [s, a]
(DPG_FEED_ACTION_IN_LAYER = 1).  Forward passes, `backward` and `adam` are train_model's."""
import numpy as np

import net_model
import train_model as T
from cacla_model import Net, critic_delta, sigmoid_rows, td_errors
from net_model import F32, fma32

PRIO_EPS = T.PRIO_EPS


def sa_rows(s, a):
    """[s, a] float32: state and float64 action, each value rounded once to float32 (a NaN state
    row stays one: net_model.forward leaves it unevaluated)."""
    with np.errstate(all="ignore"):
        return np.concatenate([np.asarray(s).astype(F32), np.asarray(a, np.float64).astype(F32)], axis=1)


def q_delta(qmu, qt, q_increase):
    """The combined model's output delta [B][1] float32: float32((2.0 (qmu_r - (qt_r + q_increase))) / (1 B))."""
    B = len(qmu)
    d = np.zeros((B, 1), F32)
    with np.errstate(all="ignore"):
        for r in range(B):
            tgt = float(qt[r]) + float(q_increase)
            d[r, 0] = F32((2.0 * (float(qmu[r]) - tgt)) / float(1 * B))
    return d


def first_layer_error(hs, weights, delta, hidden="relu", fma=fma32):
    """delta_L [B][1] -> delta_0 [B][units of layer 0]: train_model.backward's error chain through
    the layers L-1 .. 1 with the weights as they are; no gradient is formed."""
    d = np.asarray(delta, F32)
    for l in range(len(weights) - 1, 0, -1):
        with np.errstate(all="ignore"):
            e = T.chain_cols(d, np.asarray(weights[l][0], F32).T, fma)
        d = np.where(hs[l] > 0, e, F32(0.0)) if hidden == "relu" else e
    return d


def action_error(d0, W0, n_s, n_act, fma=fma32):
    """ea [B][n_act] float32: ONE fmaf chain over ascending unit j of d0[r][j] W0[n_s + k][j] from +0.0f."""
    with np.errstate(all="ignore"):
        return T.chain_cols(d0, np.asarray(W0, F32)[n_s:n_s + n_act].T, fma)


def actor_delta(ea, mu):
    """delta_L [B][n_act] float32: float32((double)ea (mu (1.0 - mu)))."""
    B, n = ea.shape
    d = np.zeros((B, n), F32)
    with np.errstate(all="ignore"):
        for r in range(B):
            for k in range(n):
                m = float(mu[r, k])
                d[r, k] = F32(float(ea[r, k]) * (m * (1.0 - m)))
    return d


def soft_update(target, model, tau):
    """theta- = float32(float32(theta- float32(1.0 - tau)) + float32(theta float32(tau))), every
    operation rounding on its own: numpy's `target * (1 - tau) + model * tau` on float32 arrays."""
    keep, t = F32(1.0 - float(tau)), F32(float(tau))
    with np.errstate(all="ignore"):
        return [tuple(((tp * keep).astype(F32) + (mp * t).astype(F32)).astype(F32) for tp, mp in zip(tl, ml))
                for tl, ml in zip(target, model)]


class Trainer:
    """The device's DPG training state."""

    def __init__(self, actor, critic, batch, hidden_actor="relu", hidden_critic="relu", critic_lr=5e-4, actor_lr=1e-4,
                 beta1=0.9, beta2=0.999, epsilon=1e-7, discount=0.9, tau=0.001, q_increase=2.0, target_steps=0,
                 min_size=0, fma=fma32):
        self.a, self.c = Net(actor, actor_lr), Net(critic, critic_lr)
        self.batch, self.ha, self.hc, self.fma = int(batch), hidden_actor, hidden_critic, fma
        self.b1, self.b2, self.eps = float(beta1), float(beta2), float(epsilon)
        self.discount, self.tau, self.q_increase = float(discount), float(tau), float(q_increase)
        self.target_steps, self.min_size = int(target_steps), int(min_size)
        self.n_s, self.n_act = self.a.theta[0][0].shape[0], self.a.theta[-1][0].shape[1]
        assert self.c.theta[0][0].shape[0] == self.n_s + self.n_act and self.c.theta[-1][0].shape[1] == 1
        self.skipped = self.since = self.askipped = 0
        self.nonfinite = False
        self.td = self.ea = self.delta_a = None
        self.sync_target()

    def reset(self):
        self.a.reset()
        self.c.reset()

    def sync_target(self):
        cp = lambda ws: [(W.copy(), b.copy()) for W, b in ws]
        self.target_a, self.target_c = cp(self.a.theta), cp(self.c.theta)
        self.since = 0

    def can_draw(self, size):
        return size >= max(self.batch, self.min_size)

    def info(self):
        return (self.c.t, self.skipped, self.since, self.a.t, self.askipped, 0, 0, 0)

    def mu(self, s, theta):
        return net_model.forward(s, theta, self.ha, "sigmoid", self.fma)

    def q(self, x, theta):
        return net_model.forward(x, theta, self.hc, "linear", self.fma)[:, 0]

    def step(self, s, a, rew, s2, done, w, size=None):
        """One step on a drawn batch -> priorities [B] (None when the step is skipped).  a [B][4]."""
        if size is not None and not self.can_draw(size):
            self.skipped += 1
            return None
        s, s2 = np.asarray(s), np.asarray(s2)
        n_s, n_act = self.n_s, self.n_act
        # the critic half
        mu2 = self.mu(s2, self.target_a)  # (a done row's s2 is the NaN row: mu2 and q2 are NaN rows, unused)
        q2 = self.q(sa_rows(s2, mu2), self.target_c)
        hs, q = T.forward_saved(sa_rows(s, np.asarray(a)[:, :n_act]), self.c.theta, self.hc, self.fma)
        self.td = td = td_errors(q[:, 0], q2, rew, done, self.discount)
        if not np.isfinite(td).all():
            self.nonfinite = True
            self.skipped += 1
            return None
        self.c.apply(T.backward(hs, self.c.theta, critic_delta(td, w), self.hc, self.fma), self.b1, self.b2, self.eps)
        # the actor half: the critic as just updated, the targets as before this step
        hsa, y = T.forward_saved(s, self.a.theta, self.ha, self.fma)
        mu = sigmoid_rows(y.astype(F32))
        mut = self.mu(s, self.target_a)
        hsq, qmu = T.forward_saved(sa_rows(s, mu), self.c.theta, self.hc, self.fma)
        qt = self.q(sa_rows(s, mut), self.target_c)
        dq = q_delta(qmu[:, 0], qt, self.q_increase)
        ok = bool(np.isfinite(dq).all())
        if ok:
            d0 = first_layer_error(hsq, self.c.theta, dq, self.hc, self.fma)
            self.ea = action_error(d0, self.c.theta[0][0], n_s, n_act, self.fma)
            self.delta_a = actor_delta(self.ea, mu)
            ok = bool(np.isfinite(self.delta_a).all())
        if ok:
            self.a.apply(T.backward(hsa, self.a.theta, self.delta_a, self.ha, self.fma), self.b1, self.b2, self.eps)
        else:
            self.nonfinite = True
            self.askipped += 1
        # the tail
        self.since += 1
        if self.tau > 0:
            self.target_a = soft_update(self.target_a, self.a.theta, self.tau)
            self.target_c = soft_update(self.target_c, self.c.theta, self.tau)
        elif self.target_steps > 0 and self.c.t % self.target_steps == 0:
            self.sync_target()
        return np.abs(td) + PRIO_EPS
