#!/usr/bin/env python3
"""The acting network on the device against the torch detour: C3 with 4096 NN
bots, the reference's default Q network (854 -> 100 -> 100 -> 25, relu), FRAME_SKIP_RATE 7,
memory=True; 200 decisions after 20 warm-up, three interleaved rounds, three variants:

  (a) torch   q = torch_mlp(obs) in float32 on the env's stream, then env.step_q(q)
  (b) step    env.step_net()
  (c) collect env.collect(200)

Prints one JSON line: ms per decision of every round and variant, the median and the spread
(max - min), and k_net alone (device events around 50 aigar_net_forward calls on the states).
--kernel-only: nothing but 20 aigar_net_forward calls on C3's states, for a kernel trace."""
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BOTS, DECISIONS, WARMUP, ROUNDS = 4096, 200, 20, 3


def parameters():
    return types.SimpleNamespace(VIRUS_SPAWN=True, ENABLE_SPLIT=False, PELLET_GRID=True, SELF_GRID=True, WALL_GRID=True,
                                 ENEMY_GRID=True, VIRUS_GRID=True, SELF_GRID_LF=True, ENEMY_GRID_LF=True,
                                 USE_FOVSIZE=True, USE_TOTALMASS=True, USE_LAST_ACTION=True, USE_LAST_FOVSIZE=True,
                                 GRID_SQUARES_PER_FOV=11, EXTRA_INPUT=True, FRAME_SKIP_RATE=7, NUM_ACTIONS=25,
                                 SQUARE_ACTIONS=True, EXPLORATION_STRATEGY="e-Greedy", EPSILON=0.1, Q_LAYERS=(100, 100),
                                 RESET_LIMIT=0)


def make_env(network):
    from aigar_amd.env import AgarVecEnv
    env = AgarVecEnv(BOTS, parameters(), field_size=4800, max_pellets=100000.0, discrete=True, memory=True,
                     network=network or None, seed=1)
    env.reset(1)
    return env


def main():
    import numpy as np
    import torch
    from aigar_amd.net import weights_from_torch
    torch.manual_seed(1)
    envs = {"torch": make_env(False), "step": make_env(True), "collect": make_env(True)}
    spec = envs["step"].network
    sizes = [spec.n_in] + list(spec.units)
    layers = []
    for i in range(len(spec.units)):
        layers.append(torch.nn.Linear(sizes[i], sizes[i + 1]))
        if i + 1 < len(spec.units):
            layers.append(torch.nn.ReLU())
    mlp = torch.nn.Sequential(*layers).to("cuda")
    w = weights_from_torch(mlp)
    for k in ("step", "collect"):
        envs[k].set_weights(w)
    state = {"obs": envs["torch"].obs.clone()}

    def torch_loop(n):
        env = envs["torch"]
        with torch.no_grad():
            for _ in range(n):
                q = mlp(state["obs"].to(torch.float32))
                state["obs"] = env.step_q(q)[0]

    def step_loop(n):
        for _ in range(n):
            envs["step"].step_net()

    run = {"torch": torch_loop, "step": step_loop, "collect": lambda n: envs["collect"].collect(n)}
    if "--kernel-only" in sys.argv:
        env = envs["step"]
        out = torch.empty((BOTS, spec.units[-1]), dtype=torch.float64, device="cuda")
        for _ in range(20):
            env.stepper.net_forward(env.obs, out)
        torch.cuda.synchronize()
        print(json.dumps({"kernel_only": True, "calls": 20}))
        return
    ms = {k: [] for k in run}
    for r in range(ROUNDS):
        for k, f in run.items():
            f(WARMUP)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f(DECISIONS)
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) / DECISIONS * 1e3)
    env = envs["step"]
    out = torch.empty((BOTS, spec.units[-1]), dtype=torch.float64, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(5):
        env.stepper.net_forward(env.obs, out)
    e0.record()
    for _ in range(50):
        env.stepper.net_forward(env.obs, out)
    e1.record()
    torch.cuda.synchronize()
    with torch.no_grad():
        x = env.obs.clone()
        for _ in range(5):
            mlp(x.to(torch.float32))
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(50):
            mlp(x.to(torch.float32))
        t1.record()
        torch.cuda.synchronize()
    alive = int((~torch.isnan(env.obs[:, 0])).sum())
    res = {"workload": "C3 AgarVecEnv: 4096 NN bots, Q network %s, FRAME_SKIP_RATE 7, memory=True, %d decisions after %d, "
                       "%d interleaved rounds" % ("-".join(map(str, sizes)), DECISIONS, WARMUP, ROUNDS),
           "ms_per_decision": {k: {"rounds": [round(v, 4) for v in vs], "median": round(float(np.median(vs)), 4),
                                   "spread": round(max(vs) - min(vs), 4)} for k, vs in ms.items()},
           "k_net_us_per_call_back_to_back": round(e0.elapsed_time(e1) / 50 * 1e3, 2),
           "torch_mlp_us_per_call_back_to_back": round(t0.elapsed_time(t1) / 50 * 1e3, 2),
           "live_rows": alive}
    print(json.dumps(res))
    for e in envs.values():
        e.close()


if __name__ == "__main__":
    main()
