#!/usr/bin/env python3
"""The SPG trainer on the device against the torch loop it replaces: C3 with 4096
NN bots, the reference's default actor (854 -> 100 -> 100 -> n_act, sigmoid head) and critic
(854 + n_act -> 100 -> 100 -> 1), memory=True (prioritized, 40000), batch 32, soft target updates
(tau 0.001), K = 5 samples a row around the moving best, the write-back on; STEPS training steps
after WARMUP, three interleaved rounds, five variants:

  (a) torch    this tree running the parent commit's call set (INTEGRATION.md's former recipe; the
               library under those calls is unchanged).  The networks are float32 torch modules, and a
               step without a selected row still runs the actor's optimiser on a zero gradient, where
               the device skips the half: env.sample() and
               env.sample_extra() -> two float32 torch MLPs with targets: the critic's TD update, then
               the search -- the critic on [s, mu], on [s, extra] and, K times, on [s, env.perturb(best)]
               -- the actor's regression towards the winners, torch.optim.Adam for each, the soft update
               of both targets -> env.update_priorities() -> env.update_actions() -> env.set_weights()
  (b) train1   env.train(1), STEPS times, fused = 0 (the search as a composition of launches)
  (c) trainN   env.train(STEPS), fused = 0
  (d) fused1   env.train(1), STEPS times, fused = 1 (the search in k_spg_search)
  (e) fusedN   env.train(STEPS), fused = 1

Prints one JSON line: ms per step of every round and variant, the median and the spread
(max - min), and the device trainer's counters.  Every phase runs under its own time limit
(SIGALRM): a phase that exceeds it ends the tool with an error.
--kernel-only [--fused]: nothing but 20 env.train(1) calls, for a kernel trace."""
import json
import os
import signal
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BOTS, STEPS, WARMUP, ROUNDS, BATCH = 4096, 200, 20, 3, 32
TAU, DISCOUNT, K, NOISE, DECAY = 0.001, 0.9, 5, 0.5, 0.999
PHASE_LIMIT = 120  # seconds


class limit:
    def __init__(self, what, seconds=PHASE_LIMIT):
        self.what, self.seconds = what, seconds

    def __enter__(self):
        def over(*_):
            raise TimeoutError("spg_ab: phase %r ran over %d s" % (self.what, self.seconds))
        signal.signal(signal.SIGALRM, over)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


def parameters():
    return types.SimpleNamespace(VIRUS_SPAWN=True, ENABLE_SPLIT=False, PELLET_GRID=True, SELF_GRID=True, WALL_GRID=True,
                                 ENEMY_GRID=True, VIRUS_GRID=True, SELF_GRID_LF=True, ENEMY_GRID_LF=True,
                                 USE_FOVSIZE=True, USE_TOTALMASS=True, USE_LAST_ACTION=True, USE_LAST_FOVSIZE=True,
                                 GRID_SQUARES_PER_FOV=11, EXTRA_INPUT=True, FRAME_SKIP_RATE=7, ALGORITHM="SPG",
                                 NOISE_TYPE="Gaussian", GAUSSIAN_NOISE=0.2, CACLA_ACTOR_LAYERS=(100, 100),
                                 DPG_CRITIC_LAYERS=(100, 100), DPG_CRITIC_FUNC="relu", DPG_CRITIC_ALPHA=0.0005,
                                 DPG_ACTOR_ALPHA=0.0001, DPG_TAU=TAU, SOFT_TARGET_UPDATES=True, OCACLA_EXPL_SAMPLES=K,
                                 OCACLA_MOVING_GAUSSIAN=True, OCACLA_REPLACE_TRANSITIONS=True, OCACLA_NOISE=NOISE,
                                 OCACLA_NOISE_DECAY=DECAY,
                                 RESET_LIMIT=0, MEMORY_CAPACITY=40000, PRIORITIZED_EXP_REPLAY_ENABLED=True,
                                 MEMORY_BATCH_LEN=BATCH, DISCOUNT=DISCOUNT, TARGET_NETWORK_STEPS=1500, NUM_EXPS_BEFORE_TRAIN=32)


def make_env(train, fused=False):
    from aigar_amd.env import AgarSpgEnv
    env = AgarSpgEnv(BOTS, parameters(), field_size=4800, max_pellets=100000.0, continuous=True, memory=True,
                     network=True, train="dpg" if train else None, search=dict(fused=fused) if train else None, seed=1)
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
    """The parent's loop: the caller's float32 torch actor and critic with targets, trained from env.sample()."""

    def __init__(self, env, torch):
        self.env, self.torch = env, torch
        spec = env.network
        self.n_act = spec.units[-1]
        hidden = tuple(spec.units[:-1])
        self.actor, self.actor_t = (mlp(torch, spec.n_in, spec.units, True) for _ in range(2))
        self.critic, self.critic_t = (mlp(torch, spec.n_in + self.n_act, hidden + (1,), False) for _ in range(2))
        self.actor_t.load_state_dict(self.actor.state_dict())
        self.critic_t.load_state_dict(self.critic.state_dict())
        self.opt_c = torch.optim.Adam(self.critic.parameters(), lr=0.0005, eps=1e-7)
        self.opt_a = torch.optim.Adam(self.actor.parameters(), lr=0.0001, eps=1e-7)
        self.noise = NOISE

    def soft(self, target, model):
        torch = self.torch
        with torch.no_grad():
            tp, mp = list(target.parameters()), list(model.parameters())
            torch._foreach_mul_(tp, 1.0 - TAU)
            torch._foreach_add_(tp, mp, alpha=TAU)

    def step(self):
        torch, env, n_act = self.torch, self.env, self.n_act
        b = env.sample()
        extra, valid = env.sample_extra(b.idx)
        s = b.s.to(torch.float32)
        a = b.a[:, :n_act].to(torch.float32)
        with torch.no_grad():
            s2 = torch.nan_to_num(b.s2).to(torch.float32)
            q2 = self.critic_t(torch.cat([s2, self.actor_t(s2)], 1)).squeeze(1).to(torch.float64)
            tgt = torch.where(b.done, b.r, b.r + DISCOUNT * q2)
        q = self.critic(torch.cat([s, a], 1)).squeeze(1).to(torch.float64)
        td = tgt - q
        self.opt_c.zero_grad(set_to_none=True)
        (b.w * td * td).mean().backward()
        self.opt_c.step()
        mu = self.actor(s)
        with torch.no_grad():  # the search: a chain of 2 + K dependent critic evaluations
            ev = lambda act: self.critic(torch.cat([s, act.to(torch.float32)], 1)).squeeze(1).to(torch.float64)
            qmu = ev(mu)
            best, best_eval = b.a[:, :n_act].clone(), q.detach()
            qe = ev(torch.nan_to_num(extra[:, :n_act]))
            win = valid & (qe > best_eval)
            best, best_eval = torch.where(win[:, None], extra[:, :n_act], best), torch.where(win, qe, best_eval)
            win = qmu > best_eval
            best, best_eval = torch.where(win[:, None], mu.to(torch.float64), best), torch.where(win, qmu, best_eval)
            for _ in range(K):
                cand = env.perturb(best, std=self.noise)
                e = ev(cand)
                win = e > best_eval
                best, best_eval = torch.where(win[:, None], cand, best), torch.where(win, e, best_eval)
            sel = best_eval > qmu
            count = sel.sum().clamp(min=1)
        self.opt_a.zero_grad(set_to_none=True)
        ((((mu - best.to(torch.float32)) ** 2) * sel[:, None]).sum() / (n_act * count)).backward()
        self.opt_a.step()  # (a step without a selected row is a zero gradient here: no host sync to skip it)
        self.soft(self.actor_t, self.actor)
        self.soft(self.critic_t, self.critic)
        self.noise *= DECAY
        env.update_priorities(b.idx, q.detach())
        rows = torch.where(sel[:, None], torch.nn.functional.pad(best, (0, 4 - n_act)), b.a)
        env.update_actions(b.idx, rows)
        env.set_weights(self.actor)


def measure(torch, np):
    with limit("setup", 240):
        e_t, e_d, e_n, f_d, f_n = make_env(False), make_env(True), make_env(True), make_env(True, True), make_env(True, True)
        tt = TorchTrainer(e_t, torch)
        for e in (e_d, e_n, f_d, f_n):
            e.set_weights(tt.actor)
            e.set_critic_weights(tt.critic)
            e.stepper.spg_sync_target()
        for e in (e_t, e_d, e_n, f_d, f_n):
            e.collect(3)  # 4096 live bots: 12288 transitions

    def loop1(n):
        for _ in range(n):
            e_d.train(1)

    def torch_loop(n):
        for _ in range(n):
            tt.step()

    def loopf(n):
        for _ in range(n):
            f_d.train(1)

    run = {"torch": torch_loop, "train1": loop1, "trainN": lambda n: e_n.train(n), "fused1": loopf,
           "fusedN": lambda n: f_n.train(n)}
    ms = {k: [] for k in run}
    for r in range(ROUNDS):
        for k, f in run.items():
            with limit("%s round %d" % (k, r)):
                f(WARMUP)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f(STEPS)
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) / STEPS * 1e3)
    out = {"ms_per_step": {k: {"rounds": [round(v, 4) for v in vs], "median": round(float(np.median(vs)), 4),
                               "spread": round(max(vs) - min(vs), 4)} for k, vs in ms.items()},
           "info": e_n.train_info(), "info_fused": f_n.train_info(), "memory_size": e_n.memory_size()}
    for e in (e_t, e_d, e_n, f_d, f_n):
        e.close()
    return out


def main():
    import numpy as np
    import torch
    torch.manual_seed(1)
    if "--kernel-only" in sys.argv:
        with limit("kernel-only", 240):
            env = make_env(True, "--fused" in sys.argv)
            env.collect(2)
            for _ in range(20):
                env.train(1)
            torch.cuda.synchronize()
            print(json.dumps({"kernel_only": True, "steps": 20, "info": env.train_info()}))
            env.close()
        return
    res = {"workload": "C3 AgarSpgEnv: 4096 NN bots, SPG actor 854-100-100-n_act and critic (854 + n_act)-100-100-1, "
                       "prioritized memory of 40000, batch %d, tau %g, K %d, moving, replace, %d steps after %d, %d "
                       "interleaved rounds" % (BATCH, TAU, K, STEPS, WARMUP, ROUNDS)}
    res.update(measure(torch, np))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
