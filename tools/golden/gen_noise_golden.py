#!/usr/bin/env python3
"""Golden vectors for the actor-critic learners' exploration noise (aigar_noise*;
tests/noise_model.py).

CPU-ONLY TEST INFRASTRUCTURE, on the model of gen_decide_golden.py (whose stub finder it
uses): this script imports the read-only reference (`model/actorCritic.py`) and writes
numbers only into `tests/golden/noise_cases.npz`.

An `ActorCritic.__new__` object with a stub actor (`predict` returns a fresh float64
copy of the recorded row) runs the reference's own `decideMove` (which calls `applyNoise`)
or, for the explicit-std form of SPG's offline exploration, `applyNoise(action, std)`.

Draws.  Every recorded call starts from a freshly seeded legacy generator
(numpy.random.seed), so no cached normal crosses calls.  Beside each call the script
records the uniforms it consumed: a twin RandomState(seed) is stepped two random_sample()
at a time (one attempt of the polar method) until its key and position equal the global
generator's after the call.  The attempts are split into pair 0's and pair 1's by the
polar method's own acceptance test on those uniforms.

File layout, noise_cases.npz (N calls):
  n [N]                  values per action, 2..4
  kind [N]               0 Gaussian, 1 Orn-Uhl
  std [N]
  theta, ou_mu, dt [N]   the Orn-Uhl parameters
  mu [N][4]              the actor's output (NaN padded)
  u [N][2][16][2]        the attempts of pair 0 / pair 1 (padded with 0.5, 0.5: rejected)
  cnt [N][2]             attempts each pair consumed (0: the pair was not drawn)
  prev, post [N][4]      the Orn-Uhl state before / after the call (NaN padded; NaN for Gaussian)
  out [N][4]             the noisy action (NaN padded)
  chain [N]              -1, or the number of the Orn-Uhl chain the call belongs to (its calls
                         are consecutive: each starts from the previous call's state)

Usage:  python tools/golden/gen_noise_golden.py --ref SRC [--out tests/golden]
        (SRC: the reference's src directory, the one that holds model/)
"""
import argparse
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_decide_golden as gdg  # noqa: E402  (the stub finder)

T = 16


def import_reference(ref_src):
    sys.dont_write_bytecode = True
    sys.meta_path.insert(0, gdg._StubFinder())
    if ref_src not in sys.path:
        sys.path.insert(0, ref_src)
    import model.actorCritic as ac
    return ac


class _Actor:
    def __init__(self):
        self.row = None

    def predict(self, state):
        return np.array(self.row, np.float64)  # (a fresh array: the Orn-Uhl branch adds into it)


def make_learner(ac, kind, n, std, theta, ou_mu, dt):
    learner = ac.ActorCritic.__new__(ac.ActorCritic)
    learner.parameters = types.SimpleNamespace(NOISE_TYPE="Gaussian" if kind == 0 else "Orn-Uhl", ORN_UHL_THETA=theta,
                                               ORN_UHL_MU=ou_mu, ORN_UHL_DT=dt, OCACLA_ONLINE_SAMPLES=0,
                                               OCACLA_ONLINE_SAMPLING_NOISE=0)
    learner.actor = _Actor()
    learner.std = std
    learner.action_len = n
    learner.ornUhlPrev = np.zeros(n)
    return learner


def consumed(seed):
    """The attempts (ua, ub) the global generator consumed since numpy.random.seed(seed)."""
    want = np.random.get_state()
    twin = np.random.RandomState(seed)
    out = []
    for _ in range(4 * T):
        st = twin.get_state()
        if st[2] == want[2] and np.array_equal(st[1], want[1]):
            return out
        out.append((float(twin.random_sample()), float(twin.random_sample())))
    raise AssertionError("the twin generator never met the reference's stream")


def accepted(a):
    x1 = 2.0 * a[0] - 1.0
    x2 = 2.0 * a[1] - 1.0
    r2 = x1 * x1 + x2 * x2
    return r2 < 1.0 and r2 != 0.0


def run_cases(ac):
    rng = np.random.default_rng(20241020)
    keys = ("n", "kind", "std", "theta", "ou_mu", "dt", "mu", "u", "cnt", "prev", "post", "out", "chain")
    out = {k: [] for k in keys}
    seed_box = [1000]
    rejections = set()

    def pad(v):
        return [float(x) for x in v] + [np.nan] * (4 - len(v))

    def call(learner, kind, n, mu, std, chain, explicit_std):
        seed_box[0] += 1
        seed = seed_box[0]
        prev = learner.ornUhlPrev.copy() if kind == 1 else None
        np.random.seed(seed)
        if explicit_std:
            noisy = learner.applyNoise(np.array(mu, np.float64), std)
        else:
            learner.actor.row = mu
            _, noisy = learner.decideMove(None, updateNoise=False)
        att = consumed(seed)
        # pair 0's attempts end with the first accepted one, pair 1's are the rest
        k0 = next(i for i, a in enumerate(att) if accepted(a)) + 1
        pairs = [att[:k0], att[k0:]]
        assert (len(pairs[1]) > 0) == (n > 2) and all(len(p) <= T for p in pairs)
        assert not pairs[1] or (accepted(pairs[1][-1]) and not any(accepted(a) for a in pairs[1][:-1]))
        for p in pairs:
            if p:
                rejections.add(min(len(p) - 1, 3))
        u = [[list(a) for a in p] + [[0.5, 0.5]] * (T - len(p)) for p in pairs]
        p = learner.parameters
        out["n"].append(n)
        out["kind"].append(kind)
        out["std"].append(std)
        out["theta"].append(float(p.ORN_UHL_THETA))
        out["ou_mu"].append(float(p.ORN_UHL_MU))
        out["dt"].append(float(p.ORN_UHL_DT))
        out["mu"].append(pad(mu))
        out["u"].append(u)
        out["cnt"].append([len(pairs[0]), len(pairs[1])])
        out["prev"].append(pad(prev) if kind == 1 else [np.nan] * 4)
        out["post"].append(pad(learner.ornUhlPrev) if kind == 1 else [np.nan] * 4)
        out["out"].append(pad(noisy))
        out["chain"].append(chain)

    def mus(n):
        inside = [float(v) for v in rng.random(n)]
        return [[0.0] * n, [1.0] * n, [0.0, -0.0, 0.0, -0.0][:n], [-0.0] * n, inside,
                [float(v) for v in rng.random(n)], [1.0 - 2.0 ** -53, 2.0 ** -60, 0.5, 1.0][:n]]

    for kind in (0, 1):
        for n in (2, 3, 4):
            for std in (0.0, 0.02, 1.0):
                for mu in mus(n):
                    for rep in range(2):
                        # (every single call starts from a zero Orn-Uhl state; the chains below carry it)
                        learner = make_learner(ac, kind, n, std, 0.15, 0, 0.01)
                        call(learner, kind, n, mu, std, -1, explicit_std=(kind == 0 and rep == 1))
    # Orn-Uhl chains: 24 successive calls on one learner, the state carried along
    chain = 0
    for n in (2, 3, 4):
        for std in (0.02, 1.0):
            for theta, ou_mu, dt in ((0.15, 0, 0.01), (0.3, 0.25, 0.5)):
                learner = make_learner(ac, 1, n, std, theta, ou_mu, dt)
                for _ in range(24):
                    call(learner, 1, n, [float(v) for v in rng.random(n)], std, chain, False)
                chain += 1
    data = {k: np.array(v, np.int64 if k in ("n", "kind", "cnt", "chain") else np.float64) for k, v in out.items()}
    # what the tests rely on
    assert rejections == {0, 1, 2, 3}, rejections
    vals = data["out"][~np.isnan(data["out"])]
    assert (vals == 0.0).any() and (vals == 1.0).any() and ((vals > 0.0) & (vals < 1.0)).any()
    assert np.signbit(vals[vals == 0.0]).any() and not np.signbit(vals[vals == 0.0]).all()  # numpy.clip keeps a -0.0
    return data


def main():
    ap = argparse.ArgumentParser()
    here = os.path.dirname(os.path.abspath(__file__))
    ap.add_argument("--out", default=os.path.join(here, "..", "..", "tests", "golden"))
    ap.add_argument("--ref", required=True, help="the reference's src directory (holds model/)")
    args = ap.parse_args()
    ac = import_reference(args.ref)
    data = run_cases(ac)
    path = os.path.join(args.out, "noise_cases.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in data.items()})


if __name__ == "__main__":
    main()
