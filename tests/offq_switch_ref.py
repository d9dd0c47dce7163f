"""CPU restatement (test helper, imports ``oracle`` and tests/offq_collect_ref.py only) of the offpolicy episode
collector's loop on Switch (include/minimarl.h mm_offq_collect_switch): E lockstep Switch envs from reset with local
observations and the clock, the shared AgentQFunction with the hidden state carried from zero over all T steps,
per-(env, agent) epsilon-greedy from the device counter RNG, no env step once every agent is done (rewards 0, the
observation with its clock repeats, dones stay 1). ``dones`` is per agent; ``dones_env`` is their conjunction."""
import numpy as np
import torch

from offq_collect_ref import common_sum, draws
from oracle.offq import agent_q_seq
from oracle.switch import SwitchOracle, SwitchSpec

A = 5


def step_not_done(env, act, done):
    """env.step for the envs that are not done; a done env keeps pos / adone / steps, gets reward 0 and stays done.
    Returns (reward [E, N] f32, agent_done [E, N] bool, done [E] bool)."""
    keep = [a[done].copy() for a in (env.pos, env.adone, env.steps)]
    _, rew, _, _ = env.step(act)
    for a, k in zip((env.pos, env.adone, env.steps), keep):
        a[done] = k
    rew = np.where(done[:, None], np.float32(0), rew).astype(np.float32)
    return rew, env.adone.copy(), env.adone.all(1)


def replay(spec, E, act_of_step, T, common_reward, env=None):
    """The collect loop with the actions given: ``act_of_step(t, obs [E, N, D])`` -> [E, N] ints. Returns the five
    episode fields in the insert layout plus ``agent_rewards`` [T, E, N], ``pos`` [T+1, E, N, 2] (the cells behind each
    stored observation), ``stepped`` [T, E] (the env was stepped at t) and ``returns`` [E] (f32 running sum).
    ``env``: a SwitchOracle to continue from (default: E envs from reset, as the collector starts them)."""
    N, D = spec.n_agents, spec.obs_dim
    env = SwitchOracle(spec, E) if env is None else env
    out = {"obs": np.zeros((T + 1, E, N, D), np.float32), "acts": np.zeros((T, E, N, A), np.float32),
           "rewards": np.zeros((T, E, N, 1), np.float32), "dones": np.ones((T, E, N, 1), np.float32),
           "dones_env": np.ones((T, E, 1), np.float32), "agent_rewards": np.zeros((T, E, N), np.float32),
           "pos": np.zeros((T + 1, E, N, 2), np.int64), "stepped": np.zeros((T, E), bool)}
    done = env.adone.all(1)
    ret = np.zeros(E, np.float32)
    for t in range(T):
        obs = env.obs()
        out["obs"][t], out["pos"][t], out["stepped"][t] = obs, env.pos, ~done
        act = np.asarray(act_of_step(t, obs))
        rew, adone, done = step_not_done(env, act, done)
        out["agent_rewards"][t] = rew
        out["acts"][t] = np.eye(A, dtype=np.float32)[act]
        out["rewards"][t, :, :, 0] = np.repeat(common_sum(rew)[:, None], N, 1) if common_reward else rew
        out["dones"][t, :, :, 0] = adone
        out["dones_env"][t, :, 0] = done
        ret = (ret + out["rewards"][t, :, 0, 0]).astype(np.float32)
    out["obs"][T], out["pos"][T] = env.obs(), env.pos
    out["returns"] = ret
    return out


def collect_ref(P, spec, E, T, eps, seed, counter0, common_reward):
    """``replay`` with the policy's epsilon-greedy actions; adds ``q`` [T, E, N, A], ``explore`` [T, E, N] bool and
    ``rand_act`` [T, E, N]."""
    N, D = spec.n_agents, spec.obs_dim
    extra = {"q": np.zeros((T, E, N, A), np.float32), "explore": np.zeros((T, E, N), bool),
             "rand_act": np.zeros((T, E, N), np.int64)}
    state = {"h": None}

    def act_of_step(t, obs):
        with torch.no_grad():
            q, state["h"] = agent_q_seq(P, torch.from_numpy(obs.reshape(1, E * N, D)), state["h"])
        q = q[0].numpy().reshape(E, N, A)
        u, ra = draws(seed, counter0 + t, E, N, A)
        explore = u < np.float32(eps)
        extra["q"][t], extra["explore"][t], extra["rand_act"][t] = q, explore, ra
        return np.where(explore, ra, q.argmax(-1))

    out = replay(spec, E, act_of_step, T, common_reward)
    out.update(extra)
    return out


def random_episodes(seed, counter0, E, N, T, max_steps, common_reward=True, step_cost=-0.01):
    """``replay`` at eps = 1: the actions are the counter RNG's draws alone, so the episodes are facts of the RNG and
    the oracle (what the long GPU cases collect, whatever the net)."""
    spec = SwitchSpec(N, max_steps=max_steps, step_cost=step_cost)
    return replay(spec, E, lambda t, obs: draws(seed, counter0 + t, E, N, A)[1], T, common_reward)


def arrival_stats(o, max_steps):
    """Of a replayed episode set: ``home`` [E, N] bool = the agent reached its target before the last step (its +5
    step t < max_steps - 1), ``some`` = envs with some but not all agents home early, ``all`` = envs with all."""
    paid = o["agent_rewards"] == np.float32(5)                    # [T, E, N]
    home = paid[:max_steps - 1].any(0)
    n = home.sum(1)
    N = home.shape[1]
    return {"home": home, "some": int(((n > 0) & (n < N)).sum()), "agents": int(home.sum()), "all": int((n == N).sum())}


def ln0_variance(obs):
    """Biased variance over the D features of every observation row, in float64."""
    return obs.astype(np.float64).var(-1)
