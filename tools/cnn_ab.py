#!/usr/bin/env python3
"""The CNN acting network on the device against the torch detour: C3 with 4096
NN bots, pixel states 42 x 42 x 1 in float32, the reference's default CNN ((8, 4, 32), (4, 2, 64)
-> 576 -> 100 -> 100 -> 25, relu), FRAME_SKIP_RATE 7, memory=True; 200 decisions after 20
warm-up, three interleaved rounds, three variants:

  (a) torch   q = torch_cnn(obs) in float32 on the env's stream, then env.step_q(q)
  (b) step    env.step_net()
  (c) collect env.collect(200)

Prints one JSON line: ms per decision of every round and variant, the median and the spread
(max - min), and the network alone (device events around 50 aigar_net_forward calls on the
states, and around 50 calls of the torch module).
--kernel-only: nothing but 20 aigar_net_forward calls on C3's states, for a kernel trace."""
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BOTS, DECISIONS, WARMUP, ROUNDS, SIDE = 4096, 200, 20, 3, 42


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
                     network=network or None, pixels=(SIDE, False, False), seed=1)
    env.reset(1)
    return env


def main():
    import numpy as np
    import torch
    from aigar_amd.net import cnn_weights_from_torch
    torch.manual_seed(1)
    kernel_only = "--kernel-only" in sys.argv
    envs = {"step": make_env(True)}
    if not kernel_only:
        envs.update({"torch": make_env(False), "collect": make_env(True)})
    spec = envs["step"].network
    layers, cin = [], spec.channels
    for k, s, f in spec.convs:
        layers += [torch.nn.Conv2d(cin, f, k, stride=s), torch.nn.ReLU()]
        cin = f
    layers.append(torch.nn.Flatten())
    sizes = [spec.n_flat] + list(spec.units)
    for i in range(len(spec.units)):
        layers.append(torch.nn.Linear(sizes[i], sizes[i + 1]))
        if i + 1 < len(spec.units):
            layers.append(torch.nn.ReLU())
    cnn = torch.nn.Sequential(*layers).to("cuda")
    w = cnn_weights_from_torch(cnn, spec)
    for k in ("step", "collect"):
        if k in envs:
            envs[k].set_weights(w)
    env = envs["step"]
    out = torch.empty((BOTS, spec.units[-1]), dtype=torch.float64, device="cuda")
    if kernel_only:
        for _ in range(20):
            env.stepper.net_forward(env.obs, out)
        torch.cuda.synchronize()
        print(json.dumps({"kernel_only": True, "calls": 20}))
        return
    state = {"obs": envs["torch"].obs.clone()}

    def images(obs):  # [NP, side, side, C] -> torch's NCHW; a dead player's NaN frame as zeros
        return torch.nan_to_num(obs.to(torch.float32)).permute(0, 3, 1, 2)

    def torch_loop(n):
        e = envs["torch"]
        with torch.no_grad():
            for _ in range(n):
                q = cnn(images(state["obs"]))
                state["obs"] = e.step_q(q)[0]

    def step_loop(n):
        for _ in range(n):
            envs["step"].step_net()

    run = {"torch": torch_loop, "step": step_loop, "collect": lambda n: envs["collect"].collect(n)}
    ms = {k: [] for k in run}
    for r in range(ROUNDS):
        for k, f in run.items():
            f(WARMUP)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f(DECISIONS)
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) / DECISIONS * 1e3)
    # the two networks agree to float32 accuracy on the live rows (not bit for bit: torch's order of summation is its own)
    live = ~torch.isnan(env.obs[:, 0, 0, 0])
    env.stepper.net_forward(env.obs, out)
    with torch.no_grad():
        ref = cnn(images(env.obs)).to(torch.float64)
    torch.cuda.synchronize()
    err = float((out[live] - ref[live]).abs().max() / ref[live].abs().max())
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
            cnn(images(x))
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(50):
            cnn(images(x))
        t1.record()
        torch.cuda.synchronize()
    res = {"workload": "C3 AgarVecEnv: 4096 NN bots, pixels %d x %d x %d float32, CNN %s -> %s, FRAME_SKIP_RATE 7, "
                       "memory=True, %d decisions after %d, %d interleaved rounds"
                       % (SIDE, SIDE, spec.channels, list(spec.convs), "-".join(map(str, sizes)), DECISIONS, WARMUP, ROUNDS),
           "ms_per_decision": {k: {"rounds": [round(v, 4) for v in vs], "median": round(float(np.median(vs)), 4),
                                   "spread": round(max(vs) - min(vs), 4)} for k, vs in ms.items()},
           "device_cnn_us_per_call_back_to_back": round(e0.elapsed_time(e1) / 50 * 1e3, 2),
           "torch_cnn_us_per_call_back_to_back": round(t0.elapsed_time(t1) / 50 * 1e3, 2),
           "max_abs_difference_to_torch_over_max_abs": err,
           "live_rows": int(live.sum())}
    print(json.dumps(res))
    for e in envs.values():
        e.close()


if __name__ == "__main__":
    main()
