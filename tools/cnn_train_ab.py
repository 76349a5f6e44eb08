#!/usr/bin/env python3
"""The CNN Q-learning trainer on the device against the torch loop it replaces:
C3 with 4096 NN bots, pixel states 42 x 42 x 1 in float32, the reference's default CNN
((8, 4, 32), (4, 2, 64)) -> 576 -> 100 -> 100 -> 25, memory=True (prioritized), batch 32 and batch
256 (the handle's largest); STEPS training steps after WARMUP, three interleaved rounds, three
variants:

  (a) torch    env.sample() -> a float32 torch CNN forward / backward / torch.optim.Adam ->
               env.update_priorities() -> env.set_weights() (which re-packs the filters)
  (b) train1   env.train(1), STEPS times
  (c) trainN   env.train(STEPS)

Prints one JSON line: ms per step of every round and variant, the median and the spread
(max - min).  Every phase runs under its own time limit (SIGALRM): a phase that exceeds it ends
the tool with an error.
--kernel-only: nothing but 20 env.train(1) calls at batch 32, for a kernel trace.
--large: the 84 x 84, batch 256 step alone, timed once over 10 steps after 2."""
import json
import os
import signal
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BOTS, STEPS, WARMUP, ROUNDS = 4096, 200, 20, 3
PHASE_LIMIT = 120  # seconds


class limit:
    def __init__(self, what, seconds=PHASE_LIMIT):
        self.what, self.seconds = what, seconds

    def __enter__(self):
        def over(*_):
            raise TimeoutError("cnn_train_ab: phase %r ran over %d s" % (self.what, self.seconds))
        signal.signal(signal.SIGALRM, over)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


def parameters(batch, side=42):
    return types.SimpleNamespace(VIRUS_SPAWN=True, ENABLE_SPLIT=False, PELLET_GRID=True, SELF_GRID=True, WALL_GRID=True,
                                 ENEMY_GRID=True, VIRUS_GRID=True, SELF_GRID_LF=True, ENEMY_GRID_LF=True,
                                 USE_FOVSIZE=True, USE_TOTALMASS=True, USE_LAST_ACTION=True, USE_LAST_FOVSIZE=True,
                                 GRID_SQUARES_PER_FOV=11, EXTRA_INPUT=True, FRAME_SKIP_RATE=7, NUM_ACTIONS=25,
                                 SQUARE_ACTIONS=True, EXPLORATION_STRATEGY="e-Greedy", EPSILON=0.1, Q_LAYERS=(100, 100),
                                 CNN_INPUT_DIM_1=side, RESET_LIMIT=0, MEMORY_CAPACITY=40000 if side == 42 else 8192,
                                 PRIORITIZED_EXP_REPLAY_ENABLED=True, MEMORY_BATCH_LEN=batch, ALPHA=1e-4, DISCOUNT=0.9,
                                 TARGET_NETWORK_STEPS=1500, NUM_EXPS_BEFORE_TRAIN=32)


def make_env(batch, train, side=42, bots=BOTS):
    import torch
    from aigar_amd.env import AgarVecEnv
    env = AgarVecEnv(bots, parameters(batch, side), field_size=4800, max_pellets=100000.0, discrete=True, memory=True,
                     network=True, train=train or None, seed=1, pixels=(side, False, False), pixel_dtype=torch.float32)
    env.reset(1)
    return env


class TorchTrainer:
    """The parent's loop: the caller's float32 torch CNN, trained from env.sample()."""

    def __init__(self, env, torch):
        self.env, self.torch = env, torch
        spec = env.network
        nn = torch.nn

        def mk():
            layers, cin = [], spec.channels
            for k, s, f in spec.convs:
                layers += [nn.Conv2d(cin, f, k, s), nn.ReLU()]
                cin = f
            layers.append(nn.Flatten())
            n = spec.n_flat
            for i, u in enumerate(spec.units):
                layers += [nn.Linear(n, u)] + ([nn.ReLU()] if i + 1 < len(spec.units) else [])
                n = u
            return nn.Sequential(*layers).to("cuda")
        self.net, self.target = mk(), mk()
        self.target.load_state_dict(self.net.state_dict())
        self.opt = torch.optim.Adam(self.net.parameters(), lr=1e-4, eps=1e-7)
        self.t = 0

    def step(self):
        torch, env = self.torch, self.env
        b = env.sample()
        n_out = env.network.units[-1]
        q = self.net(b.s.to(torch.float32).permute(0, 3, 1, 2))
        with torch.no_grad():
            q2 = self.target(torch.nan_to_num(b.s2).to(torch.float32).permute(0, 3, 1, 2)).max(dim=1).values.to(torch.float64)
            tgt = torch.where(b.done, b.r, b.r + 0.9 * q2)
        qa = q.gather(1, b.a[:, :1].to(torch.int64)).squeeze(1).to(torch.float64)
        td = tgt - qa
        loss = (b.w * td * td / n_out).mean()
        self.opt.zero_grad(set_to_none=True)
        loss.backward()
        self.opt.step()
        env.update_priorities(b.idx, td.detach())
        env.set_weights(self.net)
        self.t += 1
        if self.t % 1500 == 0:
            self.target.load_state_dict(self.net.state_dict())


def measure(batch, torch, np):
    with limit("setup batch %d" % batch, 240):
        e_t, e_d, e_n = make_env(batch, False), make_env(batch, True), make_env(batch, True)
        tt = TorchTrainer(e_t, torch)
        for e in (e_d, e_n):
            e.set_weights(tt.net)
            e.sync_target()
        for e in (e_t, e_d, e_n):
            e.collect(3)  # 4096 live bots: thousands of transitions

    def loop1(n):
        for _ in range(n):
            e_d.train(1)

    def torch_loop(n):
        for _ in range(n):
            tt.step()

    run = {"torch": torch_loop, "train1": loop1, "trainN": lambda n: e_n.train(n)}
    ms = {k: [] for k in run}
    for r in range(ROUNDS):
        for k, f in run.items():
            with limit("%s round %d batch %d" % (k, r, batch)):
                f(WARMUP)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f(STEPS)
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) / STEPS * 1e3)
    out = {"ms_per_step": {k: {"rounds": [round(v, 4) for v in vs], "median": round(float(np.median(vs)), 4),
                               "spread": round(max(vs) - min(vs), 4)} for k, vs in ms.items()},
           "info": e_n.train_info(), "memory_size": e_n.memory_size()}
    for e in (e_t, e_d, e_n):
        e.close()
    return out


def main():
    import numpy as np
    import torch
    torch.manual_seed(1)
    if "--kernel-only" in sys.argv:
        with limit("kernel-only", 240):
            env = make_env(32, True)
            env.collect(2)
            for _ in range(20):
                env.train(1)
            torch.cuda.synchronize()
            print(json.dumps({"kernel_only": True, "steps": 20, "info": env.train_info()}))
            env.close()
        return
    if "--large" in sys.argv:
        with limit("large", 240):
            env = make_env(256, True, side=84, bots=512)
            env.collect(2)
            env.train(2)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            env.train(10)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / 10 * 1e3
            print(json.dumps({"large": "84 x 84 x 1, batch 256", "ms_per_step": round(ms, 3), "info": env.train_info()}))
            env.close()
        return
    res = {"workload": "C3 AgarVecEnv: 4096 NN bots, pixels 42x42x1 float32, CNN (8,4,32),(4,2,64)-576-100-100-25, "
                       "prioritized memory of 40000, %d steps after %d, %d interleaved rounds" % (STEPS, WARMUP, ROUNDS)}
    for batch in (32, 256):
        res["batch_%d" % batch] = measure(batch, torch, np)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
