#!/usr/bin/env python3
"""performAgarioTest on the device (aigar.py:523-538): one test episode per arena,
scored by the bots' mass over time (AIGAR_FLAG_SCORE).

Reset, `--ticks` Model.update()s, then per arena
  meanMass = mean over bots of (mean over time of the bot's mass)
  maxMass  = max over bots of (max over time)
and the number of deaths.  The world is the reference's default for the bot count
(field 75 * sqrt(bots), its pellet and virus densities, viruses on).

  --roles greedy | random      every bot that kind: the whole episode is replays of
                               aigar_run's step graph (random: the synthetic random
                               population of the benchmark, p_split 2.5e-3, p_eject 1e-2)
  --roles NN:16,Greedy:8,...   a mixed arena (counts must sum to --bots) through
                               AgarVecEnv with FRAME_SKIP_RATE 0: the NN players take
                               uniform random actions, the others their device policies
Prints one JSON line.  The same seed gives the same meanMass and maxMass, bit for bit.

    python tools/eval_episode.py --bots 4096 --roles greedy --ticks 500
"""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_roles(spec, bots):
    if spec.lower() in ("greedy", "random"):
        return spec.lower(), None
    roles = []
    for part in spec.split(","):
        name, _, n = part.partition(":")
        name = {"nn": "NN", "greedy": "Greedy", "random": "Random"}.get(name.strip().lower())
        if name is None or not n.strip().isdigit():
            raise SystemExit("--roles: greedy, random, or counts such as NN:16,Greedy:8,Random:8")
        roles += [name] * int(n)
    if len(roles) != bots:
        raise SystemExit("--roles names %d players, --bots is %d" % (len(roles), bots))
    return "mixed", roles


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bots", type=int, default=4096)
    ap.add_argument("--arenas", type=int, default=1)
    ap.add_argument("--ticks", type=int, default=500)
    ap.add_argument("--roles", default="greedy")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    kind, roles = parse_roles(args.roles, args.bots)
    import torch
    from aigar_amd import _abi, _lib
    dev = torch.device("cuda", 0)
    A, B = args.arenas, args.bots

    if kind == "mixed":
        from aigar_amd.env import AgarVecEnv
        p = types.SimpleNamespace(VIRUS_SPAWN=True, ENABLE_SPLIT=True, ENABLE_EJECT=False, ENABLE_GREEDY_SPLIT=True,
                                  PELLET_GRID=True, USE_FOVSIZE=True, USE_TOTALMASS=True, FRAME_SKIP_RATE=0,
                                  RESET_LIMIT=0)
        env = AgarVecEnv(B, p, n_arenas=A, roles=roles, reset_limit=0, desync=False, seed=args.seed, score=True)
        env.reset(args.seed)
        gen = torch.Generator(device=dev).manual_seed(args.seed)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(args.ticks):
            env.step(torch.rand((A * B, 3), dtype=torch.float64, device=dev, generator=gen))
        sc = env.score()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        env.close()
    else:
        c = _abi.Config()
        c.n_arenas, c.bots_per_arena, c.field_size = A, B, 0
        c.virus_enabled = 1
        c.max_pellets, c.max_viruses = -1.0, -1.0
        c.grid_squares, c.obs_channels, c.obs_extras = 11, _abi.OBS_PELLET, _abi.EX_FOV | _abi.EX_MASS
        c.rng_mode, c.device, c.flags = _abi.RNG_PHILOX, 0, _abi.FLAG_SCORE
        stp = _lib.Stepper(c)
        stp.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        stp.reset(args.seed)
        sc = torch.empty((A * B, 4), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if kind == "greedy":
            stp.run(args.ticks, policy="greedy", greedy_split=True)
        else:
            stp.run(args.ticks, policy="random", p_split=2.5e-3, p_eject=1e-2, seed=args.seed)
        stp.score(sc)
        stp.sync()  # (device error bits of the episode)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        stp.close()

    s = sc.view(A, B, 4)
    assert bool((s[:, :, 0] == args.ticks).all()), "every bot has one sample per tick"
    mean = (s[:, :, 1] / s[:, :, 0]).mean(dim=1)
    print(json.dumps({"bots": B, "arenas": A, "ticks": args.ticks, "roles": args.roles, "seed": args.seed,
                      "meanMass": mean.tolist(), "maxMass": s[:, :, 2].max(dim=1).values.tolist(),
                      "deaths": [int(x) for x in s[:, :, 3].sum(dim=1).tolist()],
                      "wall_s": round(wall, 4), "env_steps_per_s": round(A * B * args.ticks / wall, 1)}), flush=True)


if __name__ == "__main__":
    main()
