#!/usr/bin/env python3
"""Cost of resetting one arena of a batched handle (GPU box).

Shape: 8 arenas x 512 bots, the default field, viruses on, a learner's grids
(last-frame history included).  After 200 settled ticks, two ways of giving one
arena a fresh world, alternated for --reps repetitions each in one process:
  device: reset_arenas([a], [s])                         (aigar_reset_arenas)
  host:   a one-arena Stepper: reset(s), get_state, then load_state into arena a
          (what reset_arena did before aigar_reset_arenas existed)
Each repetition is a host clock around work that ends in sync().  Then one call
that resets all arenas together.  Prints one JSON line.

    python tools/reset_cost.py [--arenas 8] [--bots 512] [--reps 20]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arenas", type=int, default=8)
    ap.add_argument("--bots", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ticks", type=int, default=200)
    args = ap.parse_args()
    from aigar_amd import _abi, _lib
    ch = (_abi.OBS_PELLET | _abi.OBS_SELF | _abi.OBS_WALL | _abi.OBS_ENEMY | _abi.OBS_VIRUS | _abi.OBS_SELF_LF |
          _abi.OBS_ENEMY_LF)
    ex = _abi.EX_LAST_FOV | _abi.EX_FOV | _abi.EX_MASS | _abi.EX_LAST_ACT

    def cfg(arenas):
        c = _abi.Config()
        c.n_arenas, c.bots_per_arena, c.field_size = arenas, args.bots, 0
        c.virus_enabled = 1
        c.max_pellets, c.max_viruses = -1.0, -1.0
        c.grid_squares, c.obs_channels, c.obs_extras = 11, ch, ex
        c.rng_mode, c.device = _abi.RNG_PHILOX, 0
        return c

    g, one = _lib.Stepper(cfg(args.arenas)), _lib.Stepper(cfg(1))
    g.reset(1)
    for _ in range(args.ticks):
        g.policy_random(2.5e-3, 1e-2, 1)
        g.step(1)
    g.sync()

    def device(a, s):
        g.reset_arenas([a], [s])
        g.sync()

    def host(a, s):
        one.reset(s)
        g.load_state(one.get_state(0), a)
        g.sync()

    def clock(f, *xs):
        t0 = time.perf_counter()
        f(*xs)
        return (time.perf_counter() - t0) * 1e3

    device(0, 7)  # (first launches of the kernels, the helper handle's first use)
    host(0, 7)
    t = {"device": [], "host": []}
    for r in range(args.reps):
        a, s = r % args.arenas, 1000 + r
        t["device"].append(clock(device, a, s))
        t["host"].append(clock(host, a, s))

    def every():
        g.reset_arenas(list(range(args.arenas)), [2000 + a for a in range(args.arenas)])
        g.sync()

    t_all = [clock(every) for _ in range(5)]
    out = {"shape": "%d arenas x %d bots, default field, viruses on" % (args.arenas, args.bots), "reps": args.reps,
           "unit": "ms per reset of one arena (host clock, ends in sync)"}
    for k, v in t.items():
        out[k] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    out["device_all_arenas_one_call"] = {"median": round(statistics.median(t_all), 4), "min": round(min(t_all), 4),
                                         "max": round(max(t_all), 4)}
    out["host_over_device"] = round(out["host"]["median"] / out["device"]["median"], 1)
    print(json.dumps(out), flush=True)
    g.close()
    one.close()


if __name__ == "__main__":
    main()
