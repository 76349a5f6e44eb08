"""A plain-Python model of the replay memory's specification (include/aigar.h,
aigar_exp_*): the ring, the two trees, the draw, the importance weights and the
priority update.  Written from the specification, not from the reference; the golden
scripts (tests/golden/replay_*.npz, recorded from the reference) are replayed through
it at tolerance 0 by test_replay_model.py, which makes it the oracle of the larger
random scripts of test_gpu_replay.py.  Python floats are IEEE doubles and `**` is the
C library's pow, as in the reference."""
import math

import numpy as np


class ReplayModel:
    def __init__(self, capacity, prioritized=False, alpha=0.6, beta=0.4):
        self.cap = int(capacity)
        self.prio = bool(prioritized)
        self.alpha, self.beta = float(alpha), float(beta)
        self.rows = [None] * self.cap  # (s, a, r, s2, done)
        self.size = self.next = self.added = 0
        self.it_cap = 1
        while self.it_cap < self.cap:
            self.it_cap *= 2
        self.vsum = [0.0] * (2 * self.it_cap)
        self.vmin = [math.inf] * (2 * self.it_cap)
        self.max_priority = 1.0

    # ---- trees: leaf it_cap + i; node k = f(node 2k, node 2k + 1)
    def _set_leaves(self, leaves):
        """leaves {slot: value}: write them, then rebuild the touched ancestors level by level."""
        nodes = set()
        for i, v in leaves.items():
            self.vsum[self.it_cap + i] = v
            self.vmin[self.it_cap + i] = v
            nodes.add((self.it_cap + i) // 2)
        while nodes and min(nodes) >= 1:
            for k in nodes:
                self.vsum[k] = self.vsum[2 * k] + self.vsum[2 * k + 1]
                a, b = self.vmin[2 * k], self.vmin[2 * k + 1]
                self.vmin[k] = b if b < a else a
            nodes = {k // 2 for k in nodes if k // 2 >= 1}

    def total(self):
        return self.vsum[1]

    def minimum(self):
        return self.vmin[1]

    def _prefix(self, end):
        """The sum of the leaves [0, end], nested v[left] + (v[left'] + (...))."""
        terms, node, lo, hi = [], 1, 0, self.it_cap - 1
        while hi != end:
            mid = (lo + hi) // 2
            if end <= mid:
                node, hi = 2 * node, mid
            else:
                terms.append(self.vsum[2 * node])
                node, lo = 2 * node + 1, mid + 1
        acc = self.vsum[node]
        for t in reversed(terms):
            acc = t + acc
        return acc

    # ---- the ring
    def add(self, s, a, r, s2, done, mask=None):
        """Rows with mask != 0 (all if None), in row order, one slot each from next_idx."""
        leaves = {}
        leaf = self.max_priority ** self.alpha
        for i in range(len(r)):
            if mask is not None and not mask[i]:
                continue
            self.rows[self.next] = (np.array(s[i]), np.array(a[i], np.float64), float(r[i]), np.array(s2[i]),
                                    bool(done[i]))
            leaves[self.next] = leaf
            self.next = (self.next + 1) % self.cap
            self.size = min(self.size + 1, self.cap)
            self.added += 1
        if self.prio:
            self._set_leaves(leaves)

    def too_small(self):
        return self.size == 0 or (self.prio and self.size < 2)

    def sample(self, u):
        """draws u -> (indices, weights); (-1, NaN) from a memory too small to draw from."""
        if self.too_small():
            return [-1] * len(u), [math.nan] * len(u)
        idx, w = [], []
        for x in u:
            x = float(x)
            if not self.prio:
                idx.append(int(math.floor(x * self.size)))
                w.append(1.0)
                continue
            mass = x * self._prefix(self.size - 2)  # (the newest-indexed item is left out of the mass)
            k = 1
            while k < self.it_cap:
                if self.vsum[2 * k] > mass:
                    k = 2 * k
                else:
                    mass -= self.vsum[2 * k]
                    k = 2 * k + 1
            i = k - self.it_cap
            idx.append(i)
            total = self.vsum[1]
            top = (self.vmin[1] / total * self.size) ** (-self.beta)
            w.append((self.vsum[self.it_cap + i] / total * self.size) ** (-self.beta) / top)
        return idx, w

    def gather(self, idx):
        return [self.rows[i] if 0 <= i < self.size else None for i in idx]

    def update(self, idx, prio):
        if not self.prio:
            return
        leaves = {}
        for i, p in zip(idx, prio):
            i, p = int(i), float(p)
            if not p > 0 or not 0 <= i < self.size:
                continue
            leaves[i] = p ** self.alpha  # (the last occurrence wins)
            self.max_priority = max(self.max_priority, p)
        self._set_leaves(leaves)


def load_golden(path):
    """The ops of a golden file: a list of (kind, dict of that op's arrays and recorded results)."""
    d = np.load(path)
    ops = []
    for k in range(len(d["op_kind"])):
        kind, a, b = int(d["op_kind"][k]), int(d["op_off"][k]), int(d["op_end"][k])
        names = {0: ("add_s", "add_a", "add_r", "add_s2", "add_done"), 1: ("draws", "samp_idx", "samp_w", "samp_r"),
                 2: ("upd_idx", "upd_prio")}[kind]
        op = {n: d[n][a:b] for n in names}
        for n in ("size", "next_idx", "total", "vmin", "max_priority"):
            op[n] = d[n][k]
        ops.append((("add", "sample", "update")[kind], op))
    meta = {"capacity": int(d["capacity"]), "alpha": float(d["alpha"]), "beta": float(d["beta"]),
            "prioritized": bool(int(d["prioritized"]))}
    return meta, ops


def golden_u(op, prioritized, size):
    """The draws of a recorded sample as u in [0, 1): the prioritized buffer's random.random
    values as they are; the uniform buffer's randint results k as (k + 0.5) / size, which
    floor(u * size) maps back to k."""
    if prioritized:
        return np.array(op["draws"], np.float64)
    u = (np.array(op["draws"], np.float64) + 0.5) / size
    assert np.array_equal(np.floor(u * size), op["draws"])
    return u


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)
