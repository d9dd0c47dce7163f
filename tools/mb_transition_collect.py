#!/usr/bin/env python3
"""Time per window of the two one-launch transition collectors, mm_moffq_collect (epsilon-greedy on Q) and
mm_maddpg_collect (Gumbel-softmax on the actor's logits), at the same (env, E, N, T) in one process: the variants
alternate inside every repetition, device events around the launch, warm-up, then median / min / max in ms.
maddpg at eps 1 draws no noise, so its gap to eps 0.3 is what the noise costs after the overlap with the env phase.
Prints one JSON line per shape. Needs an MI355X."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mini-marl_amd"))
from minimarl import MADDPG, MADDPGCollector, MOffQCollector  # noqa: E402
from minimarl.env import SwitchVecEnv, VecEnv  # noqa: E402
from minimarl.moffq import MOffQMix  # noqa: E402


def bench(kind, E, N, T, reps, warm):
    D = 3 if kind == "switch" else 47
    env = lambda: (SwitchVecEnv if kind == "switch" else VecEnv)(E, N, max_steps=T, device="cuda")   # noqa: E731
    q = MOffQCollector(env(), MOffQMix(N, D, 5, mixer="vdn", seed=7), T, 1)
    a = MADDPGCollector(env(), MADDPG(N, D, 5, seed=7), T, 1)
    g = MADDPGCollector(env(), MADDPG(N, D, 5, seed=7), T, 1, explore=False)
    variants = [("moffq eps 0.3", q, 0.3), ("maddpg eps 0.3", a, 0.3), ("moffq eps 1", q, 1.0), ("maddpg eps 1", a, 1.0),
                ("maddpg explore=0", g, 0.3)]
    times = {name: [] for name, _, _ in variants}
    for r in range(warm + reps):
        for name, col, eps in variants:
            col.set_epsilon(eps)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            col.launch()
            e1.record()
            e1.synchronize()
            if r >= warm:
                times[name].append(e0.elapsed_time(e1))
    return {name: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4),
                   "max_ms": round(float(np.max(v)), 4)} for name, v in times.items()}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="checkers:4096:8:100,checkers:4096:2:100,switch:4096:4:100",
                    help="comma list of env:E:N:T")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    for shape in args.shapes.split(","):
        kind, E, N, T = shape.split(":")
        print(json.dumps({"shape": shape, **bench(kind, int(E), int(N), int(T), args.reps, args.warmup)}), flush=True)
