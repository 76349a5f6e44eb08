#!/usr/bin/env python3
"""Golden vectors for the replay memory (aigar_exp_*; tests/replay_model.py).

CPU-ONLY TEST INFRASTRUCTURE, on the model of gen_golden.py: this script imports the
read-only reference (`model/replay_buffer.py` over `model/common/segment_tree.py`) and
runs its ReplayBuffer and PrioritizedReplayBuffer through a scripted sequence of adds,
samples and priority updates, with `random.random` and `random.randint` wrapped to
record their draws.  It writes `tests/golden/replay_prio.npz` and `replay_uniform.npz`,
numbers only: the op script, the rows added, the draws and, after every op, size,
next_idx, the tree roots and max_priority, and for every sample the indices, weights and
the sampled rewards.

File layout (n ops, flat arrays with offsets):
  capacity, alpha, beta, prioritized          scalars
  op_kind [n]            0 add, 1 sample, 2 update_priorities
  op_off, op_end [n]     op k's slice [op_off[k]:op_end[k]] of the flat arrays of its kind:
     add     rows add_s / add_a / add_r / add_s2 / add_done
     sample  draws / samp_idx / samp_w / samp_r             (uniform: draws are the
             randint results; prioritized: the random.random values)
     update  upd_idx / upd_prio
  size, next_idx [n]     after the op
  total, vmin, max_priority [n]   after the op (prioritized; NaN otherwise)

Usage:  python tools/golden/gen_replay_golden.py [--out tests/golden] [--ref SRC]
"""
import argparse
import os
import random
import sys

import numpy as np

REF_SRC = "/root/reference/src"

CAPACITY, ALPHA, BETA, WIDTH = 10, 0.6, 0.4, 3

# (kind, argument): add n rows | sample n draws | update (indices, priorities)
SCRIPT = [
    ("add", 2),
    ("sample", 3),                                        # the smallest memory a prioritized draw works on
    ("add", 2),
    ("sample", 5),                                        # before the wrap
    ("update", ([1, 3, 1, 0], [0.5, 2.5, 0.3, 1e-4])),    # index 1 twice, its last value not its largest;
    ("add", 5),                                           # 2.5 moves max_priority, these adds use it
    ("sample", 6),
    ("add", 4),                                           # 13 adds: the ring wraps (next_idx 3)
    ("sample", 8),                                        # after the wrap
    ("update", ([9, 2, 9, 9, 5], [0.7, 1e-4, 3.0, 1.2, 0.9])),
    ("add", 2),
    ("sample", 8),
    ("update", ([0, 0], [0.25, 0.125])),
    ("sample", 4),
]


def run(ref_src, prioritized):
    sys.dont_write_bytecode = True
    if ref_src not in sys.path:
        sys.path.insert(0, ref_src)
    import model.replay_buffer as rb

    draws = []
    real_random, real_randint = random.random, random.randint

    def rec_random():
        v = real_random()
        draws.append(v)
        return v

    def rec_randint(a, b):
        v = real_randint(a, b)
        draws.append(float(v))
        return v

    random.seed(20240611)
    random.random, random.randint = rec_random, rec_randint
    try:
        buf = rb.PrioritizedReplayBuffer(CAPACITY, ALPHA, BETA) if prioritized else rb.ReplayBuffer(CAPACITY)
        rng = np.random.default_rng(7)
        out = {k: [] for k in ("op_kind", "op_off", "size", "next_idx", "total", "vmin", "max_priority", "add_s",
                               "add_a", "add_r", "add_s2", "add_done", "draws", "samp_idx", "samp_w", "samp_r",
                               "upd_idx", "upd_prio")}
        n_add = n_samp = n_upd = 0
        for kind, arg in SCRIPT:
            if kind == "add":
                out["op_kind"].append(0)
                out["op_off"].append(n_add)
                for _ in range(arg):
                    s, s2 = rng.standard_normal(WIDTH), rng.standard_normal(WIDTH)
                    a, r, done = rng.random(4), float(rng.standard_normal()), bool(n_add % 4 == 3)
                    if done:
                        s2 = np.full(WIDTH, np.nan)
                    buf.add(s, a, r, s2, done)  # (arrays: np.array(..., copy=False) rejects scalars under numpy 2)
                    for k, v in (("add_s", s), ("add_a", a), ("add_r", r), ("add_s2", s2), ("add_done", done)):
                        out[k].append(v)
                    n_add += 1
            elif kind == "sample":
                out["op_kind"].append(1)
                out["op_off"].append(n_samp)
                before = len(draws)
                res = buf.sample(arg)
                assert len(draws) - before == arg
                if prioritized:
                    idx, w = list(res[6]), list(res[5])
                else:
                    idx, w = [int(v) for v in draws[before:]], [1.0] * arg
                out["draws"] += draws[before:]
                out["samp_idx"] += [int(i) for i in idx]
                out["samp_w"] += [float(x) for x in w]
                out["samp_r"] += [float(x) for x in res[2]]
                assert all(buf._storage[i][2] == x for i, x in zip(idx, res[2]))
                n_samp += arg
            else:
                out["op_kind"].append(2)
                out["op_off"].append(n_upd)
                buf.update_priorities(arg[0], arg[1])
                out["upd_idx"] += list(arg[0])
                out["upd_prio"] += list(arg[1])
                n_upd += len(arg[0])
            out["size"].append(len(buf))
            out["next_idx"].append(buf._next_idx)
            out["total"].append(buf._it_sum.sum() if prioritized else np.nan)
            out["vmin"].append(buf._it_min.min() if prioritized else np.nan)
            out["max_priority"].append(buf._max_priority if prioritized else np.nan)
        # the end offsets of each kind: op_off[k + 1] of the last op of a kind
        ends = {0: n_add, 1: n_samp, 2: n_upd}
    finally:
        random.random, random.randint = real_random, real_randint
    kinds = out["op_kind"]
    off_end = []
    for k in range(len(kinds)):  # the next op of the same kind starts where this one ends
        nxt = [out["op_off"][j] for j in range(k + 1, len(kinds)) if kinds[j] == kinds[k]]
        off_end.append(nxt[0] if nxt else ends[kinds[k]])
    ints = ("op_kind", "op_off", "size", "next_idx", "samp_idx", "upd_idx")
    data = {k: np.array(v, np.int64 if k in ints else np.float64) for k, v in out.items() if k != "add_done"}
    data["add_done"] = np.array(out["add_done"], np.uint8)
    data["op_end"] = np.array(off_end, np.int64)
    data.update(capacity=np.int64(CAPACITY), alpha=np.float64(ALPHA), beta=np.float64(BETA),
                prioritized=np.int64(prioritized))
    return data


def main():
    ap = argparse.ArgumentParser()
    here = os.path.dirname(os.path.abspath(__file__))
    ap.add_argument("--out", default=os.path.join(here, "..", "..", "tests", "golden"))
    ap.add_argument("--ref", default=REF_SRC)
    args = ap.parse_args()
    for name, prio in (("replay_prio", True), ("replay_uniform", False)):
        data = run(args.ref, prio)
        path = os.path.join(args.out, name + ".npz")
        np.savez_compressed(path, **data)
        print(path, os.path.getsize(path), "bytes;", len(data["op_kind"]), "ops,", len(data["add_r"]), "adds,",
              len(data["samp_idx"]), "draws")


if __name__ == "__main__":
    main()
