"""MAPPO phase timing at BASELINE config 3 (4096 envs x 8 agents, T=100, L=5, 15 PPO epochs).

usage: python tools/mb_mappo.py [--envs E] [--epochs K] [--episodes n] [--centralized-v] [--minibatches M]
                                [--feed-forward] [--env checkers|switch]
Prints one JSON line: ms per rollout step, per compute (values + GAE), per train() and per epoch (medians over the
timed episodes; the first episode is warm-up). --centralized-v: the critic reads the env's share_obs.
--minibatches M: M PPO minibatches per epoch (num_mini_batch; an epoch is then M updates on 1 / M of the chunks each).
--feed-forward: the reference's algorithm_name "mappo" (nets without the GRU, minibatches over rows).
--env switch: the Switch2 corridor env (obs_dim 3; --agents defaults to 2 there, max_steps = T); also prints
us per rollout step.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mini-marl_amd"))
import torch  # noqa: E402
import minimarl._lib as _L  # noqa: E402

if os.environ.get("MB_LIB"):   # A/B: another build of libminimarl.so
    _L.LIB_PATH = os.path.abspath(os.environ["MB_LIB"])
from minimarl.env import make_env  # noqa: E402
from minimarl.mappo import MappoPolicy, MappoRunner  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--agents", type=int, default=None, help="default: 8 on checkers, 2 on switch")
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--epochs", type=int, default=15)
    ap.add_argument("--episodes", type=int, default=2)
    ap.add_argument("--centralized-v", action="store_true", help="centralized critic (use_centralized_V)")
    ap.add_argument("--minibatches", type=int, default=1, help="PPO minibatches per epoch (num_mini_batch)")
    ap.add_argument("--feed-forward", action="store_true", help="feed-forward nets (algorithm_name mappo)")
    ap.add_argument("--env", choices=("checkers", "switch"), default="checkers")
    a = ap.parse_args()
    if a.agents is None:
        a.agents = 2 if a.env == "switch" else 8
    env = make_env(a.env, a.envs, a.agents, max_steps=a.T if a.env == "switch" else 100, device="cuda")
    p = MappoPolicy(env.obs_dim, 5, 32, "cuda", seed=0, **({"cent_agents": a.agents} if a.centralized_v else {}),
                    **({"recurrent": False} if a.feed_forward else {}))
    r = MappoRunner(env, p, T=a.T, L=5, ppo_epoch=a.epochs, seed=1, num_mini_batch=a.minibatches)
    r.warmup()
    ev = lambda: torch.cuda.Event(enable_timing=True)
    res = []
    for ep in range(a.episodes + 1):
        e0, e1, e2, e3 = ev(), ev(), ev(), ev()
        e0.record()
        r.rollout()
        e1.record()
        r.compute()
        e2.record()
        info = r.train()
        e3.record()
        torch.cuda.synchronize()
        if ep > 0:
            res.append((e0.elapsed_time(e1), e1.elapsed_time(e2), e2.elapsed_time(e3)))
    med = lambda v: sorted(v)[len(v) // 2] if len(v) % 2 else sum(sorted(v)[len(v) // 2 - 1:len(v) // 2 + 1]) / 2
    ro, co, tr = (med([x[i] for x in res]) for i in range(3))
    epi = med([sum(x) for x in res])   # (the median episode, not the sum of the phase medians)
    rows = a.envs * a.agents * a.T
    out = {"env": a.env, "obs_dim": env.obs_dim, "rollout_us_per_step": 1e3 * ro / a.T,
           "envs": a.envs, "agents": a.agents, "T": a.T, "epochs": a.epochs, "centralized_v": bool(a.centralized_v),
           "minibatches": a.minibatches, "feed_forward": bool(a.feed_forward),
           "train_ms_per_update": tr / (a.epochs * a.minibatches),
           "episodes": len(res),
           "rollout_ms_per_step": ro / a.T, "compute_ms": co, "train_ms": tr, "train_ms_per_epoch": tr / a.epochs,
           "episode_ms": epi, "agent_env_steps_per_s_incl_train": rows / (epi / 1e3),
           "rollout_agent_env_steps_per_s": rows / (ro / 1e3), "train_info": {k: float(v) for k, v in info.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
