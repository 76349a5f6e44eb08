#!/usr/bin/env python3
"""The CACLA trainer on the device against the torch loop it replaces: C3 with
4096 NN bots, the reference's default actor (854 -> 100 -> 100 -> n_act, sigmoid head) and critic
(854 -> 100 -> 100 -> 1), memory=True (prioritized), batch 32, var_epochs 0 (plain CACLA) and 8
(CACLA-Var's cap); STEPS training steps after WARMUP, three interleaved rounds, three variants:

  (a) torch    env.sample() -> two float32 torch MLPs, forward / backward / torch.optim.Adam on the
               critic, then on the actor once per epoch -> env.update_priorities() -> env.set_weights()
  (b) train1   env.train(1), STEPS times
  (c) trainN   env.train(STEPS)

Prints one JSON line: ms per step of every round and variant, the median and the spread
(max - min), and the device trainer's counters.  Every phase runs under its own time limit
(SIGALRM): a phase that exceeds it ends the tool with an error.
--kernel-only [E]: nothing but 20 env.train(1) calls with var_epochs E (default 8), for a kernel trace."""
import json
import math
import os
import signal
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BOTS, STEPS, WARMUP, ROUNDS, BATCH = 4096, 200, 20, 3, 32
PHASE_LIMIT = 120  # seconds


class limit:
    def __init__(self, what, seconds=PHASE_LIMIT):
        self.what, self.seconds = what, seconds

    def __enter__(self):
        def over(*_):
            raise TimeoutError("actrain_ab: phase %r ran over %d s" % (self.what, self.seconds))
        signal.signal(signal.SIGALRM, over)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


def parameters(var):
    return types.SimpleNamespace(VIRUS_SPAWN=True, ENABLE_SPLIT=False, PELLET_GRID=True, SELF_GRID=True, WALL_GRID=True,
                                 ENEMY_GRID=True, VIRUS_GRID=True, SELF_GRID_LF=True, ENEMY_GRID_LF=True,
                                 USE_FOVSIZE=True, USE_TOTALMASS=True, USE_LAST_ACTION=True, USE_LAST_FOVSIZE=True,
                                 GRID_SQUARES_PER_FOV=11, EXTRA_INPUT=True, FRAME_SKIP_RATE=7, ALGORITHM="CACLA",
                                 NOISE_TYPE="Gaussian", GAUSSIAN_NOISE=0.2, CACLA_ACTOR_LAYERS=(100, 100),
                                 CACLA_CRITIC_LAYERS=(100, 100), CACLA_VAR_ENABLED=bool(var), CACLA_VAR_START=1,
                                 CACLA_VAR_BETA=0.001, CACLA_CRITIC_ALPHA=0.000075, CACLA_ACTOR_ALPHA=0.0005,
                                 RESET_LIMIT=0, MEMORY_CAPACITY=40000, PRIORITIZED_EXP_REPLAY_ENABLED=True,
                                 MEMORY_BATCH_LEN=BATCH, DISCOUNT=0.9, TARGET_NETWORK_STEPS=1500, NUM_EXPS_BEFORE_TRAIN=32)


def make_env(var, train):
    from aigar_amd.env import AgarVecEnv
    env = AgarVecEnv(BOTS, parameters(var), field_size=4800, max_pellets=100000.0, continuous=True, memory=True,
                     network=True, train=train or None, seed=1)
    env.reset(1)
    return env


def mlp(torch, n_in, units, sigmoid):
    sizes = [n_in] + list(units)
    mods = []
    for i in range(len(units)):
        mods.append(torch.nn.Linear(sizes[i], sizes[i + 1]))
        if i + 1 < len(units):
            mods.append(torch.nn.ReLU())
    if sigmoid:
        mods.append(torch.nn.Sigmoid())
    return torch.nn.Sequential(*mods).to("cuda")


class TorchTrainer:
    """The parent's loop: the caller's float32 torch actor and critic, trained from env.sample()."""

    def __init__(self, env, torch, var):
        self.env, self.torch, self.E = env, torch, 8 if var else 0
        spec = env.network
        self.n_act = spec.units[-1]
        self.actor = mlp(torch, spec.n_in, spec.units, True)
        self.critic = mlp(torch, spec.n_in, tuple(spec.units[:-1]) + (1,), False)
        self.target = mlp(torch, spec.n_in, tuple(spec.units[:-1]) + (1,), False)
        self.target.load_state_dict(self.critic.state_dict())
        self.opt_c = torch.optim.Adam(self.critic.parameters(), lr=0.000075, eps=1e-7)
        self.opt_a = torch.optim.Adam(self.actor.parameters(), lr=0.0005, eps=1e-7)
        self.t, self.var = 0, 1.0

    def step(self):
        torch, env = self.torch, self.env
        b = env.sample()
        s = b.s.to(torch.float32)
        v = self.critic(s).squeeze(1).to(torch.float64)
        with torch.no_grad():
            v2 = self.target(torch.nan_to_num(b.s2).to(torch.float32)).squeeze(1).to(torch.float64)
            tgt = torch.where(b.done, b.r, b.r + 0.9 * v2)
        td = tgt - v
        self.opt_c.zero_grad(set_to_none=True)
        (b.w * td * td).mean().backward()
        self.opt_c.step()
        tdh = td.detach().cpu().tolist()  # (the reference's selection is host code too)
        count = []
        for x in tdh:
            if self.E:
                self.var = (1 - 0.001) * self.var + 0.001 * x * x
                c = math.ceil(x / math.sqrt(self.var)) if x > 0 else 0
                count.append(min(c, self.E))
            else:
                count.append(1 if x > 0 else 0)
        count = torch.tensor(count, device="cuda")
        a = b.a[:, :self.n_act].to(torch.float32)
        for e in range(int(count.max()) if len(tdh) else 0):
            rows = count > e
            mu = self.actor(s[rows])
            self.opt_a.zero_grad(set_to_none=True)
            ((mu - a[rows]) ** 2).mean().backward()
            self.opt_a.step()
        env.update_priorities(b.idx, td.detach())
        env.set_weights(self.actor)
        self.t += 1
        if self.t % 1500 == 0:
            self.target.load_state_dict(self.critic.state_dict())


def measure(var, torch, np):
    with limit("setup var %d" % var, 240):
        e_t, e_d, e_n = make_env(var, False), make_env(var, True), make_env(var, True)
        tt = TorchTrainer(e_t, torch, var)
        for e in (e_d, e_n):
            e.set_weights(tt.actor)
            e.set_critic_weights(tt.critic)
            e.stepper.actrain_sync_target()
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
            with limit("%s round %d var %d" % (k, r, var)):
                f(WARMUP)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f(STEPS)
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) / STEPS * 1e3)
    out = {"ms_per_step": {k: {"rounds": [round(v, 4) for v in vs], "median": round(float(np.median(vs)), 4),
                               "spread": round(max(vs) - min(vs), 4)} for k, vs in ms.items()},
           "info": e_n.train_info(), "var": e_n.cacla_var(), "memory_size": e_n.memory_size()}
    for e in (e_t, e_d, e_n):
        e.close()
    return out


def main():
    import numpy as np
    import torch
    torch.manual_seed(1)
    if "--kernel-only" in sys.argv:
        i = sys.argv.index("--kernel-only")
        var = int(sys.argv[i + 1]) if len(sys.argv) > i + 1 else 8
        with limit("kernel-only", 240):
            env = make_env(var, True)
            env.collect(2)
            for _ in range(20):
                env.train(1)
            torch.cuda.synchronize()
            print(json.dumps({"kernel_only": True, "var_epochs": env.training["var_epochs"], "steps": 20,
                              "info": env.train_info()}))
            env.close()
        return
    res = {"workload": "C3 AgarVecEnv: 4096 NN bots, CACLA actor 854-100-100-n_act and critic 854-100-100-1, prioritized "
                       "memory of 40000, batch %d, %d steps after %d, %d interleaved rounds" % (BATCH, STEPS, WARMUP, ROUNDS)}
    for var in (0, 8):
        res["var_epochs_%d" % var] = measure(var, torch, np)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
