#!/usr/bin/env python3
"""Golden vectors for the Q-learning bots' action selection (aigar_decide*;
tests/decide_model.py, aigar_amd/actions.py).

CPU-ONLY TEST INFRASTRUCTURE, on the model of gen_replay_golden.py: this script imports
the read-only reference (`model/qLearning.py`, `model/network.py`) and writes numbers only
into `tests/golden/decide_tables.npz` and `tests/golden/decide_cases.npz`.

The reference imports keras, tensorflow and pygame at module level; a `sys.meta_path`
finder answers every import below those three names with an empty stub package, so the
two modules import with numpy alone.  A `QLearn.__new__` object with a stub network
(`predict_action` returns the recorded row, `actions` is the table) runs the reference's
own `decideMove`.

Draws.  Boltzmann: numpy.random.choice(p=p) makes exactly one random_sample(); the script
saves the legacy generator's state, draws that sample, restores the state and calls
decideMove, so the recorded u is choice's draw.  A case that wants a particular u (0,
just under 1, a cdf entry) cannot get it from the generator: for those, marked `forced`,
`numpy.random.choice` is replaced for the call by mtrand's own steps (p.cumsum(), the
division by the last entry, searchsorted(side='right')) with that u; everything around it
(boltzmannDist, the argmax fold, the book-keeping) is still the reference's.
e-Greedy: numpy.random.random(1) and numpy.random.randint(n) are wrapped to record the
coin and the index the reference drew.

File layout, decide_cases.npz (n cases, rows flat with offsets):
  q [sum n_out], off [n + 1]       the rows (float64; the reference sees Python floats)
  strategy [n]                     0 e-Greedy, 1 Boltzmann
  epsilon, temperature [n]
  u [n][3]                         coin, index draw (idx + 0.5) / n_out, Boltzmann draw
  forced [n]                       1: the Boltzmann u was handed to choice (see above)
  idx [n], value [n]               decideMove's index and the qValues entry it appended
decide_tables.npz: for every recorded table t: t_num, t_square, t_split, t_eject [m] and
  rows [sum][4] with t_off [m + 1].

Usage:  python tools/golden/gen_decide_golden.py --ref SRC [--out tests/golden]
        (SRC: the reference's src directory, the one that holds model/)
"""
import argparse
import importlib.abc
import importlib.machinery
import os
import sys
import types

import numpy as np

STUBBED = ("keras", "tensorflow", "pygame")


class _Anything:
    """What a stub module's attributes are: callable, subscriptable, attribute-bearing."""

    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        return _Anything()

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Anything()


class _StubModule(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Anything()


class _StubFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, fullname, path, target=None):
        if fullname.split(".")[0] in STUBBED:
            return importlib.machinery.ModuleSpec(fullname, self, is_package=True)
        return None

    def create_module(self, spec):
        m = _StubModule(spec.name)
        m.__path__ = []
        return m

    def exec_module(self, module):
        pass


def import_reference(ref_src):
    sys.dont_write_bytecode = True
    sys.meta_path.insert(0, _StubFinder())
    if ref_src not in sys.path:
        sys.path.insert(0, ref_src)
    import model.network as network
    import model.qLearning as ql
    return ql, network


class _Net:
    def __init__(self, table):
        self.actions = table
        self.row = None

    def getActions(self):
        return self.actions

    def predict_action(self, state):
        return self.row


def make_learner(ql, strategy, table):
    learner = ql.QLearn.__new__(ql.QLearn)
    learner.parameters = types.SimpleNamespace(EXPLORATION_STRATEGY=strategy)
    learner.network = _Net(table)
    learner.qValues = []
    learner.epsilon = 0.0
    learner.temperature = 0.0
    return learner


def _choice_with(u):
    """numpy.random.choice(a, p=p) for one draw with the uniform sample u: mtrand's
    cdf = p.cumsum(); cdf /= cdf[-1]; idx = cdf.searchsorted(u, side='right')."""
    def choice(a, p=None):
        cdf = np.array(p, np.float64).cumsum()
        cdf /= cdf[-1]
        k = int(cdf.searchsorted(u, side="right"))
        return np.asarray(a)[min(k, len(cdf) - 1)]
    return choice


def rows_for(rng, n, kind):
    if kind == "normal":
        return [float(v) for v in rng.standard_normal(n) * 3.0]
    if kind == "ties":  # a few distinct values with period 13: equal probabilities, equal maxima
        return [float((i % 13) * 0.25 - 1.0) for i in range(n)]
    if kind == "maxlast":
        r = [float(v) for v in rng.standard_normal(n)]
        r[-1] = max(r) + 1.5
        return r
    if kind == "wide":  # differences that underflow at small temperatures
        return [float(v) for v in rng.standard_normal(n) * 40.0]
    raise ValueError(kind)


def run_cases(ql):
    rng = np.random.default_rng(20241019)
    np.random.seed(97)
    out = {k: [] for k in ("q", "off", "strategy", "epsilon", "temperature", "u", "forced", "idx", "value")}
    out["off"].append(0)

    def record(row, strategy, eps, temp, u, forced, idx, value):
        out["q"] += row
        out["off"].append(len(out["q"]))
        out["strategy"].append(strategy)
        out["epsilon"].append(eps)
        out["temperature"].append(temp)
        out["u"].append(u)
        out["forced"].append(forced)
        out["idx"].append(int(idx))
        out["value"].append(float(value))

    # ---- Boltzmann
    for n in (1, 7, 8, 9, 25, 75, 128, 129, 300):
        table = [[0.0, 0.0, 0, 0]] * n
        for temp in (7.0, 0.5, 0.05, 0.0):
            for kind in ("normal", "ties", "maxlast", "wide"):
                row = rows_for(rng, n, kind)
                learner = make_learner(ql, "Boltzmann", table)
                learner.network.row = row
                learner.temperature = temp
                # the reference's own draw
                state = np.random.get_state()
                u = float(np.random.random_sample())
                np.random.set_state(state)
                idx, _ = learner.decideMove(None, updateNoise=False)
                record(row, 1, 0.0, temp, [0.0, 0.0, u], 0, idx, learner.qValues[-1])
                if temp == 0.0:
                    continue
                # forced draws: 0, just under 1, and a cdf entry (searchsorted's right side)
                p = ql.boltzmannDist(row, temp)
                cdf = np.array(p, np.float64).cumsum()
                cdf /= cdf[-1]
                for uf in (0.0, 1.0 - 2.0 ** -53, float(cdf[min(n - 1, n // 3)]) if cdf[min(n - 1, n // 3)] < 1.0 else 0.5):
                    learner = make_learner(ql, "Boltzmann", table)
                    learner.network.row = row
                    learner.temperature = temp
                    real = np.random.choice
                    np.random.choice = _choice_with(uf)
                    try:
                        idx, _ = learner.decideMove(None, updateNoise=False)
                    finally:
                        np.random.choice = real
                    record(row, 1, 0.0, temp, [0.0, 0.0, uf], 1, idx, learner.qValues[-1])

    # ---- e-Greedy: the coin and the index the reference drew
    real_random, real_randint = np.random.random, np.random.randint
    seen = {}

    def rec_random(*a):
        v = real_random(*a)
        seen["coin"] = float(np.asarray(v).reshape(-1)[0])
        return v

    def rec_randint(*a):
        v = real_randint(*a)
        seen["idx"] = int(v)
        return v

    np.random.random, np.random.randint = rec_random, rec_randint
    try:
        for n in (1, 7, 25, 75, 300):
            table = [[0.0, 0.0, 0, 0]] * n
            for eps in (0.0, 1.0, 0.5):
                for kind in ("normal", "ties", "maxlast"):
                    for _ in range(3):
                        row = rows_for(rng, n, kind)
                        learner = make_learner(ql, "e-Greedy", table)
                        learner.network.row = row
                        learner.epsilon = eps
                        seen.clear()
                        idx, _ = learner.decideMove(None, updateNoise=False)
                        u1 = (seen["idx"] + 0.5) / n if "idx" in seen else 0.0
                        assert ("idx" in seen) == (seen["coin"] < eps)
                        record(row, 0, eps, 0.0, [seen["coin"], u1, 0.0], 0, idx, learner.qValues[-1])
    finally:
        np.random.random, np.random.randint = real_random, real_randint
    ints = ("off", "strategy", "forced", "idx")
    return {k: np.array(v, np.int64 if k in ints else np.float64) for k, v in out.items()}


def run_tables(network):
    out = {k: [] for k in ("t_num", "t_square", "t_split", "t_eject", "rows", "t_off")}
    out["t_off"].append(0)
    for num in (1, 4, 8, 25, 100):
        for square in (0, 1):
            for split in (0, 1):
                for eject in (0, 1):
                    try:
                        f = network.createDiscreteActionsSquare if square else network.createDiscreteActionsCircle
                        t = f(num, split, eject)
                    except (SystemExit, ZeroDivisionError):
                        continue  # (the reference quits on a non-square count; its is_square(1) divides by zero)
                    out["t_num"].append(num)
                    out["t_square"].append(square)
                    out["t_split"].append(split)
                    out["t_eject"].append(eject)
                    out["rows"] += [[float(v) for v in r] for r in t]
                    out["t_off"].append(len(out["rows"]))
    return {k: np.array(v, np.float64 if k == "rows" else np.int64) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    here = os.path.dirname(os.path.abspath(__file__))
    ap.add_argument("--out", default=os.path.join(here, "..", "..", "tests", "golden"))
    ap.add_argument("--ref", required=True, help="the reference's src directory (holds model/)")
    args = ap.parse_args()
    ql, network = import_reference(args.ref)
    for name, data in (("decide_tables", run_tables(network)), ("decide_cases", run_cases(ql))):
        path = os.path.join(args.out, name + ".npz")
        np.savez_compressed(path, **data)
        print(path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in data.items()})


if __name__ == "__main__":
    main()
