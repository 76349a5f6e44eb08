#!/usr/bin/env python3
"""Learner-loop throughput: AgarVecEnv decisions at C3
size with the reference's NN-bot frame skipping (FRAME_SKIP_RATE = 7,
networkParameters.py:33), one graph replay per decision (env.step) against the
same decision as separate calls (env.step_calls).  Prints one JSON line.
--memory: the replay memory's cost at the same shape instead (see memory()).
--discrete / --discrete-baseline: the Q-learning selection's cost (see discrete()).
--continuous / --continuous-baseline gaussian|ou: the exploration noise's cost (see continuous())."""
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parameters():
    return types.SimpleNamespace(VIRUS_SPAWN=True, ENABLE_SPLIT=True, PELLET_GRID=True, SELF_GRID=True, WALL_GRID=True,
                                 ENEMY_GRID=True, VIRUS_GRID=True, SELF_GRID_LF=True, ENEMY_GRID_LF=True,
                                 USE_FOVSIZE=True, USE_TOTALMASS=True, USE_LAST_ACTION=True, USE_LAST_FOVSIZE=True,
                                 GRID_SQUARES_PER_FOV=11, EXTRA_INPUT=True, FRAME_SKIP_RATE=7)


def main():
    import torch
    from aigar_amd.env import AgarVecEnv
    p = parameters()
    bots, n = 4096, 40
    out = {"workload": "C3 AgarVecEnv: 4096 NN bots, field 4800, 100k pellets, viruses, FRAME_SKIP_RATE 7",
           "ticks_per_decision": p.FRAME_SKIP_RATE + 1}
    for name in ("step", "step_calls"):
        env = AgarVecEnv(bots, p, field_size=4800, max_pellets=100000.0)
        env.reset(1)
        act = torch.rand((bots, 4), dtype=torch.float64, device="cuda")
        f = getattr(env, name)
        for _ in range(5):
            f(act)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            f(act)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out[name] = {"decisions_per_s": n / dt, "ms_per_decision": dt / n * 1e3,
                     "env_steps_per_s": bots * n * (p.FRAME_SKIP_RATE + 1) / dt}
        env.close()
    print(json.dumps(out))


def timed(torch, f, n):
    """ms per call of f over n calls, device events around the batch (after 3 warm-up calls)."""
    for _ in range(3):
        f()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def memory(rounds=3, n=40):
    """--memory: the cost of the replay memory at the same C3 shape.  Decisions with the
    memory off and on, alternated `rounds` times (same seed, so the envs of a round play
    the same world at the same age); the append's added time per round beside a plain device-to-device copy of the bytes it
    writes; one sample() of 32 and of 4096 rows, uniform and prioritized."""
    import torch
    from aigar_amd.env import AgarVecEnv
    p = parameters()
    bots = 4096
    envs = {"off": AgarVecEnv(bots, p, field_size=4800, max_pellets=100000.0),
            "on": AgarVecEnv(bots, p, field_size=4800, max_pellets=100000.0, memory=True),
            "on_prioritized": AgarVecEnv(bots, p, field_size=4800, max_pellets=100000.0,
                                         memory={"prioritized": True})}
    act = torch.rand((bots, 4), dtype=torch.float64, device="cuda")
    for env in envs.values():
        env.reset(1)
        for _ in range(5):
            env.step(act)
    ms = {k: [] for k in envs}
    for _ in range(rounds):
        for k, env in envs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                env.step(act)
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) / n * 1e3)
    L = envs["on"].stepper.obs_len
    wrote = 3 * bots * L * 8  # old state -> slot, new state -> slot, new state -> old state
    src, dst = torch.empty(wrote, dtype=torch.uint8, device="cuda"), torch.empty(wrote, dtype=torch.uint8, device="cuda")
    out = {"workload": "C3 AgarVecEnv, 4096 NN bots, FRAME_SKIP_RATE 7, MEMORY_CAPACITY 40000, state row %d float64" % L,
           "decisions": n, "rounds": rounds,
           "ms_per_decision": ms, "decisions_per_s_off": [1e3 / x for x in ms["off"]],
           # per round: the three envs play the same world, whose decisions get dearer as it matures
           "added_ms_per_decision": {k: [x - y for x, y in zip(ms[k], ms["off"])] for k in ("on", "on_prioritized")},
           "append_bytes_written": wrote, "d2d_copy_same_bytes_ms": timed(torch, lambda: dst.copy_(src), 200),
           "memory_size": envs["on"].memory_size(), "sample_ms": {}}
    for k in ("on", "on_prioritized"):
        for batch in (32, 4096):
            out["sample_ms"]["%s_%d" % (k, batch)] = timed(torch, lambda: envs[k].sample(batch), 200)
    for env in envs.values():
        env.close()
    print(json.dumps(out))


def discrete(baseline_only=False, rounds=3, n=40):
    """--discrete: a Q-learning decision at the C3 shape (4096 NN bots, 8 ticks per decision,
    NUM_ACTIONS 25 with split and eject: 75 outputs), both strategies: `step_q` (the selection
    inside the decision graph) against `step` with the selection written in torch on the same
    stream (argmax / multinomial plus a table gather), alternated `rounds` times on envs of the
    same seed.  --discrete-baseline: the torch variant alone -- it uses nothing of the selection,
    so it also runs on a build without it (the parent commit's side of the comparison)."""
    import torch
    from aigar_amd.env import AgarVecEnv
    p = parameters()
    p.ENABLE_EJECT, p.NUM_ACTIONS, p.SQUARE_ACTIONS, p.EPSILON, p.TEMPERATURE = True, 25, True, 0.1, 0.5
    bots, n_out = 4096, 75
    q = torch.randn((bots, n_out), dtype=torch.float32, device="cuda") * 2
    out = {"workload": "C3 AgarVecEnv: 4096 NN bots, FRAME_SKIP_RATE 7, Q rows [4096, 75] float32",
           "decisions": n, "rounds": rounds}
    for strategy in ("e-Greedy", "Boltzmann"):
        p.EXPLORATION_STRATEGY = strategy
        envs = {"torch": AgarVecEnv(bots, p, field_size=4800, max_pellets=100000.0)}
        if not baseline_only:
            envs["step_q"] = AgarVecEnv(bots, p, field_size=4800, max_pellets=100000.0, discrete=True)
            table = envs["step_q"].actions
        else:  # (network.py:46-65 for 25 square actions with split and eject)
            pts = [(c / 5 + 0.1, r / 5 + 0.1) for r in range(5) for c in range(5)]
            table = torch.tensor([[x, y, s, e] for x, y in pts for s, e in ((0, 0), (1, 0), (0, 1))],
                                 dtype=torch.float64, device="cuda")

        def torch_step(env):
            if strategy == "e-Greedy":
                coin = torch.rand(bots, device="cuda") < p.EPSILON
                idx = torch.where(coin, torch.randint(n_out, (bots,), device="cuda"), q.argmax(1))
            else:
                d = torch.exp((q.double() - q.double().max(1, keepdim=True).values) / p.TEMPERATURE)
                idx = torch.multinomial(d / d.sum(1, keepdim=True), 1).squeeze(1)
            return env.step(table[idx])

        run = {"torch": lambda: torch_step(envs["torch"])}
        if not baseline_only:
            run["step_q"] = lambda: envs["step_q"].step_q(q)
        for k, env in envs.items():
            env.reset(1)
            for _ in range(5):
                run[k]()
        ms = {k: [] for k in envs}
        for _ in range(rounds):
            for k in envs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(n):
                    run[k]()
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) / n * 1e3)
        out[strategy] = {"ms_per_decision": ms, "decisions_per_s": {k: [1e3 / x for x in v] for k, v in ms.items()}}
        for env in envs.values():
            env.close()
    print(json.dumps(out))


def continuous(kind, baseline_only=False, rounds=3, n=40):
    """--continuous gaussian|ou: an actor-critic decision at the C3 shape (4096 NN bots, 8 ticks
    per decision, 3 values per action): `step_ac` (the noise inside the decision graph) against
    `step` with the perturbation written in torch on the same stream (torch.randn, the Orn-Uhl
    update, clamp), alternated `rounds` times on envs of the same seed.  --continuous-baseline:
    the torch variant alone -- it uses nothing of the noise, so it also runs on a build without
    it (the parent commit's side of the comparison)."""
    import torch
    from aigar_amd.env import AgarVecEnv
    p = parameters()
    p.NOISE_TYPE = {"gaussian": "Gaussian", "ou": "Orn-Uhl"}[kind]
    p.GAUSSIAN_NOISE, p.ORN_UHL_THETA, p.ORN_UHL_MU, p.ORN_UHL_DT, p.ALGORITHM = 0.3, 0.15, 0.0, 0.01, "CACLA"
    bots, n_act = 4096, 3
    mu = torch.rand((bots, n_act), dtype=torch.float32, device="cuda")
    out = {"workload": "C3 AgarVecEnv: 4096 NN bots, FRAME_SKIP_RATE 7, actor rows [4096, 3] float32, %s noise" % p.NOISE_TYPE,
           "decisions": n, "rounds": rounds}
    envs = {"torch": AgarVecEnv(bots, p, field_size=4800, max_pellets=100000.0)}
    if not baseline_only:
        envs["step_ac"] = AgarVecEnv(bots, p, field_size=4800, max_pellets=100000.0, continuous=True)
    prev = torch.zeros((bots, n_act), dtype=torch.float64, device="cuda")
    std, sq = p.GAUSSIAN_NOISE, p.ORN_UHL_DT ** 0.5

    def torch_step(env):
        z = torch.randn((bots, n_act), dtype=torch.float64, device="cuda")
        if kind == "gaussian":
            a = mu.double() + std * z
        else:
            prev.add_(p.ORN_UHL_THETA * (p.ORN_UHL_MU - prev) * p.ORN_UHL_DT + std * sq * z)
            a = mu.double() + prev
        return env.step(a.clamp_(0.0, 1.0))

    run = {"torch": lambda: torch_step(envs["torch"])}
    if not baseline_only:
        run["step_ac"] = lambda: envs["step_ac"].step_ac(mu)
    for k, env in envs.items():
        env.reset(1)
        for _ in range(5):
            run[k]()
    ms = {k: [] for k in envs}
    for _ in range(rounds):
        for k in envs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                run[k]()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) / n * 1e3)
    out["ms_per_decision"] = ms
    out["decisions_per_s"] = {k: [1e3 / x for x in v] for k, v in ms.items()}
    for env in envs.values():
        env.close()
    print(json.dumps(out))


def _kind(flag):
    k = sys.argv[sys.argv.index(flag) + 1] if len(sys.argv) > sys.argv.index(flag) + 1 else ""
    if k not in ("gaussian", "ou"):
        sys.exit("%s takes gaussian or ou" % flag)
    return k


if __name__ == "__main__":
    if "--continuous" in sys.argv:
        continuous(_kind("--continuous"))
    elif "--continuous-baseline" in sys.argv:
        continuous(_kind("--continuous-baseline"), baseline_only=True)
    elif "--memory" in sys.argv:
        memory()
    elif "--discrete" in sys.argv or "--discrete-baseline" in sys.argv:
        discrete(baseline_only="--discrete-baseline" in sys.argv)
    else:
        main()
