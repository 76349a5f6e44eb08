"""One Q-learning training step in plain Python: the specification of aigar_train_step
(include/aigar.h), checked against libm's fmaf, torch.autograd and
torch.optim.Adam (tests/test_train_model.py) and compared bit for bit with the device
(tests/test_gpu_train.py).

The arithmetic is the project's own definition of Keras 2.2.4's Adam on loss='mse' with
sample weights (network.py:378-392, qLearning.py:116-193): the forward pass is
net_model.forward; targets and TD errors are float64 in the reference's order; the output
delta is rounded once to float32; the backward pass is float32 with ONE fmaf chain per
gradient entry (ascending batch row) and per back-propagated error (ascending unit); the
biases' gradients are plain float32 sums in ascending row order; Adam keeps m and v in float32 and computes in
float64 on the widened values, every operation rounding on its own."""
import math

import numpy as np

import net_model
from net_model import F32, fma32

PRIO_EPS = 1e-4  # qLearning.py: |td| + 1e-4


def forward_saved(x, weights, hidden="relu", fma=fma32):
    """x [rows][in] -> ([h_0 .. h_{L-1}], q [rows][n_out] float64): the float32 activations that
    feed each layer (h_0 = float32(x)) and the linear head widened to float64."""
    with np.errstate(all="ignore"):
        h = np.asarray(x).astype(F32)
    hs = []
    for l, (W, b) in enumerate(weights):
        hs.append(h)
        with np.errstate(all="ignore"):
            y = net_model.layer_acc(h, W, fma) + np.asarray(b, F32)[None, :]
        if l + 1 < len(weights):
            h = np.where(y > 0, y, F32(0.0)) if hidden == "relu" else y
        else:
            h = y
    return hs, h.astype(np.float64)


def td_errors(q, q2, a, rew, done, discount):
    """float64 targets and TD errors: t = rew (done) or rew + discount * max_j q2 (one multiply, one
    add; a NaN in the row makes the maximum NaN); td = t - q[r][a]."""
    B = q.shape[0]
    td = np.zeros(B, np.float64)
    with np.errstate(all="ignore"):
        for r in range(B):
            t = float(rew[r])
            if not done[r]:
                row = q2[r]
                m = np.nan if np.isnan(row).any() else float(np.max(row))
                t = float(rew[r]) + float(discount) * m
            td[r] = t - float(q[r, int(a[r])])
    return td


def output_delta(td, w, a, n_out):
    """delta_L [B][n_out] float32: g_r = float32(((2 w_r) (-td_r)) / (n_out B)) in column a_r, +0.0f elsewhere."""
    B = td.shape[0]
    d = np.zeros((B, n_out), F32)
    with np.errstate(all="ignore"):
        for r in range(B):
            d[r, int(a[r])] = F32(((2.0 * float(w[r])) * (-float(td[r]))) / float(n_out * B))
    return d


def chain_cols(A, Bm, fma=fma32):
    """out[i][j]: acc = +0.0f, acc = fmaf(A[i][k], Bm[k][j], acc) for ascending k, as one chain."""
    return net_model.layer_acc(A, Bm, fma)


def backward(hs, weights, delta, hidden="relu", fma=fma32):
    """-> [(dW_l [in][out], db_l [out])] float32 with the weights as they are."""
    L = len(weights)
    grads = [None] * L
    d = np.asarray(delta, F32)
    for l in range(L - 1, -1, -1):
        W = np.asarray(weights[l][0], F32)
        with np.errstate(all="ignore"):
            dW = chain_cols(hs[l].T, d, fma)  # chain over the batch rows, ascending
            db = np.zeros(d.shape[1], F32)
            for r in range(d.shape[0]):
                db = (db + d[r]).astype(F32)
            grads[l] = (dW, db)
            if l > 0:
                e = chain_cols(d, W.T, fma)  # chain over this layer's units, ascending
                # relu: y > 0 exactly where the stored activation is > 0
                d = np.where(hs[l] > 0, e, F32(0.0)) if hidden == "relu" else e
    return grads


def adam_lr_t(lr, b1, b2, t):
    return lr * math.sqrt(1.0 - math.pow(b2, t)) / (1.0 - math.pow(b1, t))


def adam(p, g, m, v, lr_t, b1, b2, eps):
    """One parameter array: float32 p, g, m, v -> (p, m, v) float32; float64 arithmetic on widened values."""
    p64, g64, m64, v64 = (np.asarray(x, F32).astype(np.float64) for x in (p, g, m, v))
    with np.errstate(all="ignore"):
        m_new = (b1 * m64 + (1.0 - b1) * g64).astype(F32)
        v_new = (b2 * v64 + (1.0 - b2) * (g64 * g64)).astype(F32)
        p_new = (p64 - lr_t * m_new.astype(np.float64) / (np.sqrt(v_new.astype(np.float64)) + eps)).astype(F32)
    return p_new, m_new, v_new


class Trainer:
    """The device's training state: online and target weights, Adam's m and v, the step counters."""

    def __init__(self, weights, batch, hidden="relu", lr=1e-4, beta1=0.9, beta2=0.999, epsilon=1e-7, discount=0.85,
                 target_steps=0, min_size=0, fma=fma32):
        cp = lambda ws: [(np.array(W, F32), np.array(b, F32)) for W, b in ws]
        self.theta, self.target = cp(weights), cp(weights)
        self.reset()
        self.batch, self.hidden, self.fma = int(batch), hidden, fma
        self.lr, self.b1, self.b2, self.eps = float(lr), float(beta1), float(beta2), float(epsilon)
        self.discount, self.target_steps, self.min_size = float(discount), int(target_steps), int(min_size)
        self.skipped = self.since = 0
        self.nonfinite = False
        self.td = self.grads = None

    def reset(self):
        z = lambda ws: [(np.zeros_like(W), np.zeros_like(b)) for W, b in ws]
        self.m, self.v = z(self.theta), z(self.theta)
        self.t = 0

    def set_weights(self, weights):
        self.theta = [(np.array(W, F32), np.array(b, F32)) for W, b in weights]

    def sync_target(self):
        self.target = [(W.copy(), b.copy()) for W, b in self.theta]
        self.since = 0

    def can_draw(self, size):
        return size >= max(self.batch, self.min_size)

    def step(self, s, a, rew, s2, done, w, size=None):
        """One step on a drawn batch -> priorities [B] (None when the step is skipped).  a [B] indices."""
        if size is not None and not self.can_draw(size):
            self.skipped += 1
            return None
        n_out = self.theta[-1][0].shape[1]
        hs, q = forward_saved(s, self.theta, self.hidden, self.fma)
        live = ~np.asarray(done, bool)
        q2 = np.zeros((len(a), n_out), np.float64)
        if live.any():
            q2[live] = net_model.forward(np.asarray(s2)[live], self.target, self.hidden, "linear", self.fma)
        self.td = td_errors(q, q2, a, rew, done, self.discount)
        if not np.isfinite(self.td).all():
            self.skipped += 1
            self.nonfinite = True
            return None
        delta = output_delta(self.td, w, a, n_out)
        self.grads = backward(hs, self.theta, delta, self.hidden, self.fma)
        t = self.t + 1
        lr_t = adam_lr_t(self.lr, self.b1, self.b2, t)
        for l, ((W, b), (gW, gb)) in enumerate(zip(self.theta, self.grads)):
            Wn, mW, vW = adam(W, gW, self.m[l][0], self.v[l][0], lr_t, self.b1, self.b2, self.eps)
            bn, mb, vb = adam(b, gb, self.m[l][1], self.v[l][1], lr_t, self.b1, self.b2, self.eps)
            self.theta[l], self.m[l], self.v[l] = (Wn, bn), (mW, mb), (vW, vb)
        self.t = t
        self.since += 1
        if self.target_steps > 0 and t % self.target_steps == 0:
            self.sync_target()
        return np.abs(self.td) + PRIO_EPS
