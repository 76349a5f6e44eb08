#!/usr/bin/env python3
"""Golden vectors for the SPG learner's action search (aigar_spg*; tests/spg_model.py).

CPU-ONLY TEST INFRASTRUCTURE, on the model of gen_noise_golden.py (whose helpers and stub finder
it uses): this script imports the read-only reference (`model/actorCritic.py`) and writes numbers
only into `tests/golden/spg_cases.npz`.

An `ActorCritic.__new__` object runs the reference's own `train_actor_OCACLA`.  Its actor is a stub
whose `predict` returns the recorded row mu; its critic is a stub that evaluates the project's
model (net_model.forward on dpg_model.sa_rows) with recorded weights: the file pins the CONTROL
FLOW -- which candidate wins, the selection, `updated_actions` and `count` -- while the arithmetic
stays the project's own.  The stub actor's `train` records what the reference hands to
train_on_batch.

Draws.  The instance's `applyNoise` is wrapped: every call reseeds numpy's legacy generator, runs
the reference's own applyNoise, and records the uniforms it consumed (gen_noise_golden.consumed),
so no cached normal crosses calls: an odd action length drops its leftover normal, as the device
does.

File layout, spg_cases.npz (C cases of B rows each, R = C * B rows; N applyNoise calls):
  n_act, K, moving, replace [C];  noise [C]
  s [R][3]; a, extra, mu [R][4] (NaN padded); valid [R]; evals [R] (Q(s, a) from before the update)
  w0 [3][7][6], b0 [3][6], w1 [3][6][1], b1 [3][1]   the critic of n_act = 2 / 3 / 4 (rows beyond
                                                      3 + n_act are zero)
  cnt [N][2]      attempts pair 0 / pair 1 of call consumed (calls in row order, then sample order)
  att [sum cnt][2]  the attempts, in that order
  selected [R]; updated [R][4] (NaN padded); count [C]
  pick [R]        0 stored action, 1 stored extra, 2 mu, 3 + x sample x -- from the reference's
                  outputs: an unselected row ended on mu's value, a selected row's target is matched
                  against its candidates

Usage:  python tools/golden/gen_spg_golden.py --ref SRC [--out tests/golden]
"""
import argparse
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "..", "tests"))
import gen_noise_golden as gng  # noqa: E402
import dpg_model as DM  # noqa: E402
import net_model as M  # noqa: E402

N_S, B, HID = 3, 6, 6


class _Actor:
    def __init__(self, n_act):
        self.num_outputs = n_act
        self.rows = {}
        self.trained = None

    def predict(self, state):
        return np.array(self.rows[state.tobytes()], np.float64)

    def train(self, inputs, targets, weights):
        self.trained = (np.array(inputs), np.array(targets), np.array(weights))


class _Critic:
    def __init__(self, weights):
        self.weights = weights
        self.seen = []  # (state bytes, action) of every evaluation, in order

    def predict(self, state, actions):
        act = np.asarray(actions[0], np.float64)
        self.seen.append((state.tobytes(), act.copy()))
        return float(M.forward(DM.sa_rows(state[None, :], act[None, :]), self.weights, "relu", "linear")[0, 0])


def run_cases(ac):
    rng = np.random.default_rng(20241021)
    crit = {n: M.make_weights(rng, N_S + n, (HID, 1), hi=1) for n in (2, 3, 4)}
    keys = ("n_act", "K", "moving", "replace", "noise", "s", "a", "extra", "mu", "valid", "evals", "cnt", "att",
            "selected", "updated", "count", "pick")
    out = {k: [] for k in keys}
    seed_box = [5000]
    pad = lambda v: [float(x) for x in v] + [np.nan] * (4 - len(v))

    for n_act in (2, 3, 4):
        for K in (0, 1, 5):
            for moving in (0, 1):
                for replace in (0, 1):
                    noise = float(rng.choice([0.05, 0.3]))
                    learner = ac.ActorCritic.__new__(ac.ActorCritic)
                    learner.parameters = types.SimpleNamespace(
                        NOISE_TYPE="Gaussian", CNN_REPR=False, PRIORITIZED_EXP_REPLAY_ENABLED=False, OCACLA_EXPL_SAMPLES=K,
                        OCACLA_MOVING_GAUSSIAN=bool(moving), OCACLA_REPLACE_TRANSITIONS=bool(replace))
                    learner.actor, learner.critic = _Actor(n_act), _Critic(crit[n_act])
                    learner.input_len, learner.counts, learner.ocacla_noise, learner.std = N_S, [], noise, 99.0
                    calls = []

                    def apply_noise(action, std=None, learner=learner, calls=calls):
                        seed_box[0] += 1
                        np.random.seed(seed_box[0])
                        noisy = ac.ActorCritic.applyNoise(learner, action, std)
                        att = gng.consumed(seed_box[0])
                        k0 = next(i for i, a in enumerate(att) if gng.accepted(a)) + 1
                        pairs = [att[:k0], att[k0:]]
                        assert (len(pairs[1]) > 0) == (len(action) > 2) and all(len(p) <= gng.T for p in pairs)
                        calls.append((pairs, np.array(noisy, np.float64)))
                        return noisy

                    learner.applyNoise = apply_noise
                    s = rng.random((B, N_S)).astype(np.float32).astype(np.float64)
                    a = [rng.random(n_act) for _ in range(B)]
                    mu = rng.random((B, n_act))
                    valid = rng.random(B) < 0.5
                    extra = [rng.random(n_act) if v else None for v in valid]
                    q_a = np.array([learner.critic.predict(s[r], np.array([a[r]])) for r in range(B)])
                    # Q(s, a) from before an update: near the current value, so that every source wins somewhere
                    evals = q_a + rng.choice([-0.5, -0.05, 0.0, 0.05, 0.5], B) * (1.0 + np.abs(q_a))
                    for r in range(B):
                        learner.actor.rows[s[r].tobytes()] = mu[r]
                    learner.critic.seen = []
                    batch = [list(s), [x.copy() for x in a], list(range(B)), None, extra, np.ones(B)]
                    updated = learner.train_actor_OCACLA(batch, list(evals))
                    count = learner.counts[-1]
                    assert len(calls) == B * K
                    # the selected rows are those whose states the reference handed to the actor, in order (a
                    # selected row whose best is the stored action itself keeps a's value in updated_actions)
                    tr = learner.actor.trained
                    assert (tr is not None) == (count > 0) and (tr is None or len(tr[0]) == count)
                    sel = np.array([tr is not None and any(np.array_equal(s[r], x) for x in tr[0]) for r in range(B)])
                    tgt = iter(tr[1]) if tr is not None else iter(())
                    assert int(sel.sum()) == count
                    for r in range(B):
                        cands = [(0, a[r])] + ([(1, extra[r])] if (K and replace and valid[r]) else [])
                        cands += [(3 + x, calls[r * K + x][1]) for x in range(K)]
                        if sel[r]:
                            t = next(tgt)
                            assert np.array_equal(t, updated[r])
                            pick = [k for k, c in cands if np.array_equal(c, t)]
                            assert pick, "a selected row's target is none of its candidates"
                            pick = pick[0]
                        else:
                            assert np.array_equal(updated[r], a[r])
                            pick = 2 if K else 0
                        out["pick"].append(pick)
                        out["s"].append(s[r])
                        out["a"].append(pad(a[r]))
                        out["extra"].append(pad(extra[r]) if valid[r] else [np.nan] * 4)
                        out["mu"].append(pad(mu[r]))
                        out["valid"].append(int(valid[r]))
                        out["evals"].append(float(evals[r]))
                        out["selected"].append(int(sel[r]))
                        out["updated"].append(pad(updated[r]))
                    for pairs, _ in calls:
                        out["cnt"].append([len(pairs[0]), len(pairs[1])])
                        out["att"] += [list(x) for p in pairs for x in p]
                    for k, v in (("n_act", n_act), ("K", K), ("moving", moving), ("replace", replace), ("noise", noise),
                                 ("count", count)):
                        out[k].append(v)
    ints = ("n_act", "K", "moving", "replace", "valid", "cnt", "selected", "count", "pick")
    data = {k: np.array(v, np.int64 if k in ints else np.float64) for k, v in out.items()}
    for i, n in enumerate((2, 3, 4)):
        (w0, b0), (w1, b1) = crit[n]
        data.setdefault("w0", np.zeros((3, N_S + 4, HID), np.float32))[i, :N_S + n] = w0
        data.setdefault("b0", np.zeros((3, HID), np.float32))[i] = b0
        data.setdefault("w1", np.zeros((3, HID, 1), np.float32))[i] = w1
        data.setdefault("b1", np.zeros((3, 1), np.float32))[i] = b1
    # what the tests rely on
    pick, sel = data["pick"], data["selected"].astype(bool)
    rowK = np.repeat(data["K"], B)
    assert (pick[sel] == 0).any() and (pick == 1).any() and (pick[rowK > 0] == 2).any() and (pick == 3).any()
    assert (pick > 3).any(), "no later sample won"
    assert (~sel).any() and sel.any()
    assert (data["valid"] == 1).any() and (data["valid"] == 0).any()
    return data


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "..", "..", "tests", "golden"))
    ap.add_argument("--ref", required=True, help="the reference's src directory (holds model/)")
    args = ap.parse_args()
    ac = gng.import_reference(args.ref)
    data = run_cases(ac)
    path = os.path.join(args.out, "spg_cases.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in data.items()})


if __name__ == "__main__":
    main()
