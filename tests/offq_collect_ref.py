"""CPU restatement (test helper, imports ``oracle`` only) of the offpolicy episode collector's loop
(include/minimarl.h mm_offq_collect): E lockstep Checkers envs from reset, the shared AgentQFunction with the
hidden state carried from zero over all T steps (not reset at done), per-(env, agent) epsilon-greedy from the
device counter RNG, no env step after done (rewards 0, the observation repeats, dones stay 1)."""
import numpy as np
import torch

from oracle import rng
from oracle.env import VecEnvOracle
from oracle.offq import agent_q_seq

SALT = 0x5bd1e995


def draws(seed, ctr, E, N, A):
    """(u [E, N] f32, rand_act [E, N] int64) of step counter ``ctr``: one draw per (env, agent) row."""
    ee = np.repeat(np.arange(E, dtype=np.uint64)[:, None], N, 1)
    aa = np.tile(np.arange(N, dtype=np.uint64)[None], (E, 1))
    u = rng.rng_uniform(rng.rng_draw(np.uint64(seed), np.uint64(ctr), ee, aa))
    ra = rng.rng_draw(np.uint64(seed) ^ np.uint64(SALT), np.uint64(ctr), ee, aa) % np.uint64(A)
    return u, ra.astype(np.int64)


def common_sum(rew):
    """f32 sum over agents in agent order, [E, N] -> [E]."""
    s = rew[:, 0].astype(np.float32)
    for k in range(1, rew.shape[1]):
        s = (s + rew[:, k]).astype(np.float32)
    return s


def step_not_done(env, act, done):
    """env.step for the envs that are not done; a done env keeps its state, gets reward 0 and stays done."""
    keep = [a[done].copy() for a in (env.pos, env.prev, env.grid, env.steps, env.apples)]
    _, rew, dn = env.step(act)
    for a, k in zip((env.pos, env.prev, env.grid, env.steps, env.apples), keep):
        a[done] = k
    rew = np.where(done[:, None], np.float32(0), rew).astype(np.float32)
    return rew, dn | done


def collect_ref(P, spec, E, T, eps, seed, counter0, common_reward):
    """Returns a dict: the five episode fields in the insert layout, ``q`` [T, E, N, A], ``explore`` [T, E, N]
    bool, ``rand_act`` [T, E, N], ``agent_rewards`` [T, E, N] (each agent's own reward) and ``returns`` [E]."""
    N, D, A = spec.n_agents, spec.obs_dim, spec.n_actions
    env = VecEnvOracle(spec, E)
    out = {"obs": np.zeros((T + 1, E, N, D), np.float32), "acts": np.zeros((T, E, N, A), np.float32),
           "rewards": np.zeros((T, E, N, 1), np.float32), "dones": np.ones((T, E, N, 1), np.float32),
           "dones_env": np.ones((T, E, 1), np.float32), "q": np.zeros((T, E, N, A), np.float32),
           "explore": np.zeros((T, E, N), bool), "rand_act": np.zeros((T, E, N), np.int64),
           "agent_rewards": np.zeros((T, E, N), np.float32)}
    h = None
    done = np.zeros(E, bool)
    obs = env.observe()
    for t in range(T):
        out["obs"][t] = obs
        with torch.no_grad():
            q, h = agent_q_seq(P, torch.from_numpy(obs.reshape(1, E * N, D)), h)
        q = q[0].numpy().reshape(E, N, A)
        u, ra = draws(seed, counter0 + t, E, N, A)
        explore = u < np.float32(eps)
        act = np.where(explore, ra, q.argmax(-1))
        rew, done = step_not_done(env, act, done)
        obs = env.observe()
        out["q"][t], out["explore"][t], out["rand_act"][t], out["agent_rewards"][t] = q, explore, ra, rew
        out["acts"][t] = np.eye(A, dtype=np.float32)[act]
        out["rewards"][t, :, :, 0] = np.repeat(common_sum(rew)[:, None], N, 1) if common_reward else rew
        out["dones"][t] = done[:, None, None]
        out["dones_env"][t] = done[:, None]
    out["obs"][T] = obs
    out["returns"] = out["rewards"][:, :, 0, 0].sum(0)
    return out
