#!/usr/bin/env python3
"""Cost of AIGAR_FLAG_SCORE on the flagship step (GPU box).

C3 (4096 bots, field 4800, viruses on, the matured snapshot) stepped by aigar_run
with the benchmark's random policy and its observation, on three handles of one
build in one process:
  off:    no flag (the graphs of the benchmark)
  on:     AIGAR_FLAG_SCORE, no trace attached
  trace:  AIGAR_FLAG_SCORE and a trace buffer of --steps * --reps rows attached
The handles are warmed up, then timed alternately, --reps windows of --steps steps
each: a host clock around work that ends in a device synchronise.  Prints one JSON
line: median / min / max ms per step of each handle and the differences of the medians.

    python tools/score_cost.py [--steps 300] [--reps 7]
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
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=40)
    args = ap.parse_args()
    import torch
    import bench
    from aigar_amd import _abi, _lib
    _, _, _, _, ps, pe, _, _, _ = bench.WORKLOADS["c3"]
    hs = {}
    for name, flags in (("off", 0), ("on", _abi.FLAG_SCORE), ("trace", _abi.FLAG_SCORE)):
        stp = _lib.Stepper(bench.make_cfg("c3", flags=flags))
        stp.set_stream(torch.cuda.current_stream().cuda_stream)
        obs = torch.empty((stp.NP, stp.obs_len), dtype=torch.float64, device="cuda")
        start = bench.start_world(stp, "c3", 1, 1)
        buf = None
        if name == "trace":
            buf = torch.zeros((args.warmup + args.steps * args.reps, stp.NP), dtype=torch.float64, device="cuda")
            stp.score_trace(buf)
        hs[name] = (stp, obs, buf)
    run = lambda h, n: h[0].run(n, "random", h[1], p_split=ps, p_eject=pe, seed=1, greedy_split=True)
    for h in hs.values():
        run(h, args.warmup)
    torch.cuda.synchronize()
    ms = {k: [] for k in hs}
    for r in range(args.reps):
        for k, h in hs.items():
            t0 = time.perf_counter()
            run(h, args.steps)
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) / args.steps * 1e3)
    # the three worlds are one world: the sampler changes nothing it reads
    same = all(torch.equal(torch.nan_to_num(hs["off"][1]), torch.nan_to_num(hs[k][1])) for k in ("on", "trace"))
    n = args.warmup + args.steps * args.reps
    sc = hs["trace"][0].score()
    out = {"shape": "C3: 4096 bots, %s" % start, "steps_per_window": args.steps, "reps": args.reps,
           "unit": "ms per step (host clock, ends in a device synchronise)", "same_observations": bool(same),
           "samples_ok": bool((sc[:, 0] == n).all() and (hs["trace"][2][n - 1] == hs["trace"][2][n - 1]).all())}
    for k, v in ms.items():
        out[k] = {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}
    out["on_minus_off_us"] = round((out["on"]["median"] - out["off"]["median"]) * 1e3, 2)
    out["trace_minus_off_us"] = round((out["trace"]["median"] - out["off"]["median"]) * 1e3, 2)
    print(json.dumps(out), flush=True)
    for h in hs.values():
        h[0].sync()
        h[0].close()


if __name__ == "__main__":
    main()
