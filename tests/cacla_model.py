"""One CACLA training step in plain Python: the specification of aigar_actrain_step
(include/aigar.h), built on net_model and train_model, checked against
torch.autograd (tests/test_cacla_model.py) and compared bit for bit with the device
(tests/test_gpu_actrain.py).

The reference (actorCritic.py, ALGORITHM == "CACLA"): train_critic fits V(s) to rew + discount
V'(s2) with the memory's importance weights; train_actor_batch fits mu(s) to the stored noisy
action on the rows whose TD error is positive, CACLA-Var (CACLA_VAR_ENABLED) as often as
ceil(td / sqrt(var)) says; the critic's target is copied every TARGET_NETWORK_STEPS.  Forward
passes, `backward` and `adam` are train_model's.  The rows an actor epoch leaves out enter with a
+0.0f output delta instead of being compacted away: the gradients are equal by value
(test_cacla_model.py)."""
import numpy as np

import net_model
import train_model as T
from net_model import F32, fma32

PRIO_EPS = T.PRIO_EPS


def td_errors(v, v2, rew, done, discount):
    """float64: t = rew (done) or rew + discount * v2 (one multiply, one add); td = t - v."""
    B = len(v)
    td = np.zeros(B, np.float64)
    with np.errstate(all="ignore"):
        for r in range(B):
            t = float(rew[r])
            if not done[r]:
                t = float(rew[r]) + float(discount) * float(v2[r])
            td[r] = t - float(v[r])
    return td


def critic_delta(td, w):
    """delta_L [B][1] float32: float32(((2 w_r) (-td_r)) / (1 B))."""
    B = len(td)
    d = np.zeros((B, 1), F32)
    with np.errstate(all="ignore"):
        for r in range(B):
            d[r, 0] = F32(((2.0 * float(w[r])) * (-float(td[r]))) / float(1 * B))
    return d


def select(td, var, beta, E):
    """-> (count [B] int, var after the step, rows cut).  E == 0: plain CACLA."""
    B = len(td)
    count = np.zeros(B, np.int64)
    cut = 0
    if E == 0:
        return (np.asarray(td) > 0).astype(np.int64), var, 0
    with np.errstate(all="ignore"):
        for r in range(B):
            x = float(td[r])
            var = (1.0 - beta) * var + beta * (x * x)
            if x > 0:
                q = np.float64(x) / np.sqrt(np.float64(var))
                c = np.ceil(q)
                if 1.0 <= c <= float(E):
                    count[r] = int(c)
                else:  # (an infinity or a NaN too)
                    count[r] = E
                    cut += 1
    return count, var, cut


def actor_delta(mu, a, part):
    """delta_L [B][n_out] float32 of one epoch: part [B] bool, n_e = its sum."""
    B, n_out = mu.shape
    n_e = int(np.sum(part))
    d = np.zeros((B, n_out), F32)
    with np.errstate(all="ignore"):
        for r in range(B):
            if part[r]:
                for j in range(n_out):
                    m = float(mu[r, j])
                    d[r, j] = F32(((2.0 * (m - float(a[r, j]))) / float(n_out * n_e)) * (m * (1.0 - m)))
    return d


def sigmoid_rows(y):
    return np.array([[net_model.sigmoid64(v) for v in row] for row in y], np.float64).reshape(y.shape)


class Net:
    """One network's training state: weights, Adam's m and v, its step counter."""

    def __init__(self, weights, lr):
        self.theta = [(np.array(W, F32), np.array(b, F32)) for W, b in weights]
        self.lr = float(lr)
        self.reset()

    def reset(self):
        self.m = [(np.zeros_like(W), np.zeros_like(b)) for W, b in self.theta]
        self.v = [(np.zeros_like(W), np.zeros_like(b)) for W, b in self.theta]
        self.t = 0

    def apply(self, grads, b1, b2, eps):
        t = self.t + 1
        lr_t = T.adam_lr_t(self.lr, b1, b2, t)
        for l, ((W, b), (gW, gb)) in enumerate(zip(self.theta, grads)):
            Wn, mW, vW = T.adam(W, gW, self.m[l][0], self.v[l][0], lr_t, b1, b2, eps)
            bn, mb, vb = T.adam(b, gb, self.m[l][1], self.v[l][1], lr_t, b1, b2, eps)
            self.theta[l], self.m[l], self.v[l] = (Wn, bn), (mW, mb), (vW, vb)
        self.t = t


class Trainer:
    """The device's CACLA training state."""

    def __init__(self, actor, critic, batch, hidden_actor="relu", hidden_critic="relu", critic_lr=7.5e-5,
                 actor_lr=5e-4, beta1=0.9, beta2=0.999, epsilon=1e-7, discount=0.9, target_steps=0, min_size=0,
                 var_epochs=0, var_start=1.0, var_beta=0.001, fma=fma32):
        self.a, self.c = Net(actor, actor_lr), Net(critic, critic_lr)
        self.target = [(W.copy(), b.copy()) for W, b in self.c.theta]
        self.batch, self.ha, self.hc, self.fma = int(batch), hidden_actor, hidden_critic, fma
        self.b1, self.b2, self.eps = float(beta1), float(beta2), float(epsilon)
        self.discount, self.target_steps, self.min_size = float(discount), int(target_steps), int(min_size)
        self.E, self.var_start, self.beta = int(var_epochs), float(var_start), float(var_beta)
        self.var = self.var_start
        self.skipped = self.since = self.cut = self.eskipped = 0
        self.sel = self.epochs = 0
        self.nonfinite = False
        self.td = self.count = None
        self.grads_c = self.grads_a = None

    def reset(self):
        self.a.reset()
        self.c.reset()
        self.var = self.var_start

    def sync_target(self):
        self.target = [(W.copy(), b.copy()) for W, b in self.c.theta]
        self.since = 0

    def can_draw(self, size):
        return size >= max(self.batch, self.min_size)

    def skip(self):
        self.skipped += 1
        self.sel = self.epochs = 0
        self.count = np.zeros(self.batch, np.int64)

    def info(self):
        return (self.c.t, self.skipped, self.since, self.a.t, self.sel, self.epochs, self.cut, self.eskipped)

    def step(self, s, a, rew, s2, done, w, size=None):
        """One step on a drawn batch -> priorities [B] (None when the step is skipped).  a [B][4]."""
        if size is not None and not self.can_draw(size):
            self.skip()
            return None
        B = len(rew)
        hs, v = T.forward_saved(s, self.c.theta, self.hc, self.fma)
        live = ~np.asarray(done, bool)
        v2 = np.zeros(B, np.float64)
        if live.any():
            v2[live] = net_model.forward(np.asarray(s2)[live], self.target, self.hc, "linear", self.fma)[:, 0]
        self.td = td = td_errors(v[:, 0], v2, rew, done, self.discount)
        if not np.isfinite(td).all():
            self.nonfinite = True
            self.skip()
            return None
        self.grads_c = T.backward(hs, self.c.theta, critic_delta(td, w), self.hc, self.fma)
        self.c.apply(self.grads_c, self.b1, self.b2, self.eps)
        self.count, self.var, cut = select(td, self.var, self.beta, self.E)
        self.cut += cut
        self.sel, self.epochs = int((self.count > 0).sum()), int(self.count.max())
        n_out = self.a.theta[-1][0].shape[1]
        self.grads_a = []
        for e in range(self.epochs):
            part = self.count > e
            hs, y = T.forward_saved(s, self.a.theta, self.ha, self.fma)
            mu = sigmoid_rows(y.astype(F32))
            delta = actor_delta(mu, np.asarray(a)[:, :n_out], part)
            if not np.isfinite(delta).all():  # this epoch and the step's later ones
                self.nonfinite = True
                self.eskipped += self.epochs - e
                break
            g = T.backward(hs, self.a.theta, delta, self.ha, self.fma)
            self.grads_a.append(g)
            self.a.apply(g, self.b1, self.b2, self.eps)
        self.since += 1
        if self.target_steps > 0 and self.c.t % self.target_steps == 0:
            self.sync_target()
        return np.abs(td) + PRIO_EPS
