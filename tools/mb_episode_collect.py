#!/usr/bin/env python3
"""Time per episode collect of the two one-launch episode collectors, mm_offq_collect (epsilon-greedy on the GRU Q-net)
and mm_rmaddpg_collect (Gumbel-softmax on the GRU actor's logits), at the same (env, E, N, T) in one process: the
variants alternate inside every repetition, device events around the launch, warm-up, then median / min / max in ms.
  rmaddpg eps 1        the warm-up shortcut: no net, no noise
  rmaddpg eps 1 +q     the same episode with q_out wanted: the net runs, so the gap to the line above is what the
                       shortcut saves
  rmaddpg explore=0    the net without noise: the gap of "rmaddpg eps 0.3" to it is what the noise still costs after its
                       overlap with the env phase
  gumbel x T           T launches of mm_maddpg_gumbel(B = E): the same draws made outside the collector, not overlapped
Prints one JSON line per shape. Needs an MI355X."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mini-marl_amd"))
from minimarl import RMADDPG, OffQCollector, RMADDPGCollector  # noqa: E402
from minimarl._lib import check, lib  # noqa: E402
from minimarl.env import SwitchVecEnv, VecEnv  # noqa: E402
from minimarl.offq import OffQMix  # noqa: E402
from minimarl.qnet import ptr, stream_handle  # noqa: E402


class GumbelOnly:
    """T launches of mm_maddpg_gumbel(B = E) behind the collectors' launch surface."""

    def __init__(self, policy, E, T):
        self.policy, self.E, self.T = policy, E, T
        self.g = torch.empty(policy.N, E, policy.A, device="cuda")

    def set_epsilon(self, eps):
        pass

    def launch(self):
        for t in range(self.T):
            check(lib().mm_maddpg_gumbel(ctypes.byref(self.policy.dims), ptr(self.g), self.E, 1, t,
                                         stream_handle(self.policy.device)), "maddpg_gumbel")


def bench(kind, E, N, T, reps, warm):
    D = 3 if kind == "switch" else 47
    env = lambda: (SwitchVecEnv if kind == "switch" else VecEnv)(E, N, max_steps=T, device="cuda")   # noqa: E731
    pol = RMADDPG(N, D, 5, T, 8, seed=7)
    q = OffQCollector(env(), OffQMix(N, D, 5, T, 8, mixer="vdn", seed=7), T, 1)
    a = RMADDPGCollector(env(), pol, T, 1)
    aq = RMADDPGCollector(env(), pol, T, 1, with_q=True)
    g = RMADDPGCollector(env(), pol, T, 1, explore=False)
    variants = [("offq eps 0.3", q, 0.3), ("rmaddpg eps 0.3", a, 0.3), ("offq eps 1", q, 1.0), ("rmaddpg eps 1", a, 1.0),
                ("rmaddpg eps 1 +q", aq, 1.0), ("rmaddpg explore=0", g, 0.3), ("gumbel x T", GumbelOnly(pol, E, T), 0.0)]
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
    ap.add_argument("--shapes", default="checkers:4096:2:100,checkers:4096:8:100,switch:4096:4:100",
                    help="comma list of env:E:N:T")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    for shape in args.shapes.split(","):
        kind, E, N, T = shape.split(":")
        print(json.dumps({"shape": shape, **bench(kind, int(E), int(N), int(T), args.reps, args.warmup)}), flush=True)
