"""One Q-learning training step of the CNN acting network in plain Python: the specification of
aigar_train_step under aigar_train_config_cnn (include/aigar.h), built on
tests/conv_model.py (the forward pass) and tests/train_model.py (targets, TD errors, the dense
backward pass, Adam), checked against libm's fmaf and torch.autograd
(tests/test_cnn_train_model.py) and compared bit for bit with the device
(tests/test_gpu_cnn_train.py).

The arithmetic is the project's own definition, mathematically Keras' train_on_batch on the
whole CNN.  Forward: every conv layer's post-relu output a_l is kept; feat = a_last flattened in
(y, x, f) order is the dense model's float32 input.  Backward, all float32:
  feature error   e[r][i]: ONE fmaf chain from +0.0f over ascending unit j of
                  delta_1[r][j] W_dense0[i][j]; delta_conv_last = e where feat > 0, else +0.0f.
  filter gradient dW_l[ky][kx][c][f]: ONE fmaf chain from +0.0f over ascending
                  m = (r O + oy) O + ox of h_{l-1}[r][oy s + ky][ox s + kx][c] delta_l[r][oy][ox][f];
                  db_l[f] the plain float32 sum of delta_l[m][f] over ascending m.
  input error     (l >= 2) e_{l-1}[r][iy][ix][c]: ONE chain from +0.0f over ALL k k F taps in
                  ascending (ky k + kx) F + f of fmaf(x, W_l[ky][kx][c][f], acc), where
                  x = delta_l[r][(iy - ky) / s][(ix - kx) / s][f] when both differences are >= 0,
                  divisible by s and their quotients < O, else x = -0.0f (the padded steps are
                  executed); delta_{l-1} = e where a_{l-1} > 0, else +0.0f.
Adam is train_model.adam on every conv W and b as on the dense ones, one lr_t and one step
counter; every gradient of a step is taken with the weights as they were before the step; the
hard target copy takes the conv filters as well."""
import numpy as np

import conv_model as CM
import net_model
import train_model as T
from net_model import F32, fma32


def features_saved(x, convs, fma=fma32):
    """x [rows][side][side][C] -> ([h_0, a_1 .. a_n] float32 (h_0 = float32(x), a NaN sample as
    zeros), feat [rows][n_flat], nan_row [rows])."""
    x = np.asarray(x)
    nan_row = np.isnan(x[:, 0, 0, 0])
    with np.errstate(all="ignore"):
        h = np.where(nan_row[:, None, None, None], 0, x).astype(F32)
    hs = [h]
    for layer in convs:
        h = CM.conv_layer(h, layer, fma)
        hs.append(h)
    return hs, h.reshape(h.shape[0], -1), nan_row


def feature_error(d1, W0, feat, fma=fma32):
    """delta_1 [B][units], W0 [n_flat][units], feat [B][n_flat] -> delta_conv_last [B][n_flat]."""
    with np.errstate(all="ignore"):
        e = T.chain_cols(np.asarray(d1, F32), np.asarray(W0, F32).T, fma)
    return np.where(feat > 0, e, F32(0.0))


def conv_grad(h, d, k, s, fma=fma32):
    """h [B][H][H][Cin], d [B][O][O][F] -> (dW [k][k][Cin][F], db [F]): the chains over ascending m."""
    h, d = np.asarray(h, F32), np.asarray(d, F32)
    B, O, F = d.shape[0], d.shape[1], d.shape[3]
    cin = h.shape[3]
    dW = np.zeros((k, k, cin, F), F32)
    db = np.zeros(F, F32)
    with np.errstate(all="ignore"):
        for r in range(B):
            for oy in range(O):
                for ox in range(O):
                    patch = h[r, oy * s:oy * s + k, ox * s:ox * s + k, :]  # [k][k][cin]
                    dW = fma(patch[..., None], d[r, oy, ox][None, None, None, :], dW)
                    db = (db + d[r, oy, ox]).astype(F32)
    return dW, db


def _shifted(d, H, k, s, ky, kx):
    """x [B][H][H][F] of the tap (ky, kx): delta where the window position exists, -0.0f elsewhere."""
    B, O, F = d.shape[0], d.shape[1], d.shape[3]
    x = np.full((B, H, H, F), F32(-0.0), F32)
    for iy in range(H):
        dy = iy - ky
        if dy < 0 or dy % s or dy // s >= O:
            continue
        for ix in range(H):
            dx = ix - kx
            if dx < 0 or dx % s or dx // s >= O:
                continue
            x[:, iy, ix, :] = d[:, dy // s, dx // s, :]
    return x


def conv_input_error(d, W, s, H, fma=fma32):
    """d [B][O][O][F], W [k][k][Cin][F] -> e [B][H][H][Cin]: every entry's chain over all k k F
    taps, the padded steps (x = -0.0f) executed."""
    d, W = np.asarray(d, F32), np.asarray(W, F32)
    k, cin, F = W.shape[0], W.shape[2], W.shape[3]
    B = d.shape[0]
    e = np.zeros((B, H, H, cin), F32)
    with np.errstate(all="ignore"):
        for ky in range(k):
            for kx in range(k):
                x = _shifted(d, H, k, s, ky, kx)
                for f in range(F):
                    e = fma(x[..., f][..., None], W[ky, kx, :, f][None, None, None, :], e)
    return e


def conv_input_error_skip(d, W, s, H, fma=fma32):
    """The same error with the invalid taps skipped instead of executed (equal as numbers)."""
    d, W = np.asarray(d, F32), np.asarray(W, F32)
    k, cin, F = W.shape[0], W.shape[2], W.shape[3]
    B, O = d.shape[0], d.shape[1]
    e = np.zeros((B, H, H, cin), F32)
    with np.errstate(all="ignore"):
        for iy in range(H):
            for ix in range(H):
                acc = np.zeros((B, cin), F32)
                for ky in range(k):
                    dy = iy - ky
                    if dy < 0 or dy % s or dy // s >= O:
                        continue
                    for kx in range(k):
                        dx = ix - kx
                        if dx < 0 or dx % s or dx // s >= O:
                            continue
                        for f in range(F):
                            acc = fma(d[:, dy // s, dx // s, f][:, None], W[ky, kx, :, f][None, :], acc)
                e[:, iy, ix, :] = acc
    return e


def conv_backward(hs, convs, d_last, fma=fma32):
    """hs from features_saved, d_last [B][O][O][F] -> ([(dW_l, db_l)], [delta_l]) with the weights as they are."""
    n = len(convs)
    grads, deltas = [None] * n, [None] * n
    d = np.asarray(d_last, F32)
    for l in range(n - 1, -1, -1):
        (k, s, _), W, _ = convs[l]
        deltas[l] = d
        grads[l] = conv_grad(hs[l], d, k, s, fma)
        if l > 0:
            e = conv_input_error(d, W, s, hs[l].shape[1], fma)
            d = np.where(hs[l] > 0, e, F32(0.0))
    return grads, deltas


class CnnTrainer:
    """train_model.Trainer for theta = (convs, dense): convs [((k, s, F), W, b)], dense [(W, b)]."""

    def __init__(self, convs, dense, batch, hidden="relu", lr=1e-4, beta1=0.9, beta2=0.999, epsilon=1e-7,
                 discount=0.85, target_steps=0, min_size=0, fma=fma32):
        self.theta = self._cp(convs, dense)
        self.target = self._cp(convs, dense)
        self.reset()
        self.batch, self.hidden, self.fma = int(batch), hidden, fma
        self.lr, self.b1, self.b2, self.eps = float(lr), float(beta1), float(beta2), float(epsilon)
        self.discount, self.target_steps, self.min_size = float(discount), int(target_steps), int(min_size)
        self.skipped = self.since = 0
        self.nonfinite = False
        self.td = self.grads = self.deltas = None

    @staticmethod
    def _cp(convs, dense):
        return ([(tuple(g), np.array(W, F32), np.array(b, F32)) for g, W, b in convs],
                [(np.array(W, F32), np.array(b, F32)) for W, b in dense])

    def pairs(self, what="theta"):
        """The (W, b) list in the device's order, conv pairs first: what is theta, target, m or v."""
        convs, dense = getattr(self, what)
        return [(W, b) for _, W, b in convs] + list(dense)

    def reset(self):
        convs, dense = self.theta
        z = lambda: ([(g, np.zeros_like(W), np.zeros_like(b)) for g, W, b in convs],
                     [(np.zeros_like(W), np.zeros_like(b)) for W, b in dense])
        self.m, self.v = z(), z()
        self.t = 0

    def set_weights(self, convs, dense):
        self.theta = self._cp(convs, dense)

    def sync_target(self):
        self.target = self._cp(*self.theta)
        self.since = 0

    def can_draw(self, size):
        return size >= max(self.batch, self.min_size)

    def step(self, s, a, rew, s2, done, w, size=None):
        """One step on a drawn batch -> priorities [B] (None when the step is skipped)."""
        if size is not None and not self.can_draw(size):
            self.skipped += 1
            return None
        convs, dense = self.theta
        n_out = dense[-1][0].shape[1]
        hs, feat, nan_row = features_saved(s, convs, self.fma)
        dhs, q = T.forward_saved(feat, dense, self.hidden, self.fma)
        q[nan_row] = np.nan
        live = ~np.asarray(done, bool)
        q2 = np.zeros((len(a), n_out), np.float64)
        if live.any():
            q2[live] = CM.forward(np.asarray(s2)[live], self.target[0], self.target[1], self.hidden, "linear", self.fma)
        self.td = T.td_errors(q, q2, a, rew, done, self.discount)
        if not np.isfinite(self.td).all():
            self.skipped += 1
            self.nonfinite = True
            return None
        delta = T.output_delta(self.td, w, a, n_out)
        dgrads = T.backward(dhs, dense, delta, self.hidden, self.fma)
        # delta_1, the first dense layer's output delta: train_model.backward's own recursion
        d = np.asarray(delta, F32)
        for l in range(len(dense) - 1, 0, -1):
            with np.errstate(all="ignore"):
                e = T.chain_cols(d, np.asarray(dense[l][0], F32).T, self.fma)
            d = np.where(dhs[l] > 0, e, F32(0.0)) if self.hidden == "relu" else e
        d_last = feature_error(d, dense[0][0], feat, self.fma).reshape(hs[-1].shape)
        cgrads, self.deltas = conv_backward(hs, convs, d_last, self.fma)
        self.grads = (cgrads, dgrads)
        t = self.t + 1
        lr_t = T.adam_lr_t(self.lr, self.b1, self.b2, t)
        ad = lambda p, g, m, v: T.adam(p, g, m, v, lr_t, self.b1, self.b2, self.eps)
        for l, ((g, W, b), (gW, gb)) in enumerate(zip(convs, cgrads)):
            Wn, mW, vW = ad(W, gW, self.m[0][l][1], self.v[0][l][1])
            bn, mb, vb = ad(b, gb, self.m[0][l][2], self.v[0][l][2])
            convs[l], self.m[0][l], self.v[0][l] = (g, Wn, bn), (g, mW, mb), (g, vW, vb)
        for l, ((W, b), (gW, gb)) in enumerate(zip(dense, dgrads)):
            Wn, mW, vW = ad(W, gW, self.m[1][l][0], self.v[1][l][0])
            bn, mb, vb = ad(b, gb, self.m[1][l][1], self.v[1][l][1])
            dense[l], self.m[1][l], self.v[1][l] = (Wn, bn), (mW, mb), (vW, vb)
        self.t = t
        self.since += 1
        if self.target_steps > 0 and t % self.target_steps == 0:
            self.sync_target()
        return np.abs(self.td) + T.PRIO_EPS
