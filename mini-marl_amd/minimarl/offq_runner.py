"""Offpolicy QMix / VDN end to end on the MI355X: the device episode collector and the training runner.

``OffQCollector`` stands in for ``collect_rollout`` (offpolicy/runner/shared/magym_runner.py:40-141): one
``mm_offq_collect`` / ``mm_offq_collect_switch`` launch (csrc/offq_collect.hip) runs a whole T-step episode of E
lockstep Checkers or Switch envs with the behavior agent net and per-(env, agent) epsilon-greedy, and leaves the
episode fields in HBM in the replay buffer's insert layout. ``OffQRunner`` is ``RecRunner.run`` / ``warmup`` / ``batch_train_q``
(runner/shared/base_runner.py:193-298) over it, ``RecReplayBuffer.insert_collected`` and ``OffQMix``.

Deviations from the reference:
* the stored ``acts`` are true one-hots (the reference stores the action index broadcast over the one-hot width,
  magym_runner.py:115, so its learner's argmax always reads action 0);
* the final observation is stored at index T (the reference's ``episode_obs[step] = obs`` after the loop overwrites
  index T - 1 and leaves index T zero, magym_runner.py:126);
* E envs per collect instead of 1, and the exploration draws come from the device counter RNG, one epsilon per
  episode (the schedule at ``total_env_steps`` when the collect starts; the reference re-evaluates it every step).
``share_obs`` is never materialised: it is the agents' observations concatenated, which the buffer builds on insert.
There is no CPU path.
"""
import ctypes
from dataclasses import replace

import torch

from ._lib import OffqCollectIO, check, lib
from .config import OffQTrainConfig
from .env import SwitchVecEnv, make_env
from .offq import OffQMix
from .qnet import ptr, stream_handle
from .recbuf import PrioritizedRecReplayBuffer, RecReplayBuffer


class DecayThenFlatSchedule:
    """utils/util.py:78-99, linear decay: max(finish, start - (start - finish) / time_length * T)."""

    def __init__(self, start, finish, time_length):
        self.start, self.finish, self.time_length = start, finish, time_length
        self.delta = (start - finish) / time_length

    def eval(self, T):
        return max(self.finish, self.start - self.delta * T)


class OffQCollector:
    """One-launch episode collection for ``env`` (a Checkers ``VecEnv`` with local observations, or a
    ``SwitchVecEnv`` with local observations and the clock) and ``policy`` (an ``OffQMix``: its behavior parameters
    ``policy.P`` are read in place, so updates show in the next collect). On Switch ``dones`` holds each agent's
    own done flag and differs from ``dones_env``.
    The env handle supplies the rules and the reset state; its live state is neither read nor written.
    Buffers are allocated once and overwritten by every ``collect``; the launch does not sync and reads epsilon
    and the RNG step counter from device memory, so a captured ``launch()`` replays with whatever ``set_epsilon``
    / ``counter`` hold at replay time."""

    def __init__(self, env, policy, T, seed, common_reward=True, with_q=False):
        self.env, self.policy = env, policy
        self.E, self.N, self.T = int(env.E), int(env.N), int(T)
        self.D, self.A = int(policy.D), int(policy.A)
        self.device = policy.device
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.common_reward = bool(common_reward)
        if isinstance(env, SwitchVecEnv):
            self._name, supported = "offq_collect_switch", lib().mm_offq_collect_switch_supported
        else:
            self._name, supported = "offq_collect", lib().mm_offq_collect_supported
        self._collect = getattr(lib(), "mm_" + self._name)
        if not supported(env.handle(), ctypes.byref(policy.dims), self.E, self.T):
            # the launch reports why
            check(self._collect(env.handle(), ctypes.byref(policy.dims), None, None, self.E, self.T, None), self._name)
        dev, E, N, T_ = self.device, self.E, self.N, self.T
        self.fields = {"obs": torch.zeros(T_ + 1, E, N, self.D, device=dev),
                       "acts": torch.zeros(T_, E, N, self.A, device=dev),
                       "rewards": torch.zeros(T_, E, N, 1, device=dev),
                       "dones": torch.zeros(T_, E, N, 1, device=dev),
                       "dones_env": torch.zeros(T_, E, 1, device=dev)}
        self.returns = torch.zeros(E, device=dev)
        self.q = torch.zeros(T_, E, N, self.A, device=dev) if with_q else None
        self.eps = torch.zeros(1, device=dev)
        self.counter = torch.zeros(1, dtype=torch.int64, device=dev)   # counter0 of the next collect
        io = OffqCollectIO()
        io.eps, io.counter, io.counter0, io.seed = ptr(self.eps), ptr(self.counter), 0, self.seed
        io.common_reward = int(self.common_reward)
        for k in ("obs", "acts", "rewards", "dones", "dones_env"):
            setattr(io, k, ptr(self.fields[k]))
        io.q_out, io.ret_out = ptr(self.q), ptr(self.returns)
        self._io = io

    @property
    def share_obs(self):
        """The episode's share_obs [T+1, E, N*D]: a view of ``fields["obs"]``."""
        return self.fields["obs"].view(self.T + 1, self.E, self.N * self.D)

    def set_epsilon(self, eps):
        """Stream-ordered write of the epsilon the next launch (or graph replay) reads."""
        self.eps.fill_(float(eps))

    def launch(self):
        """The collect launch and the counter advance (+T), nothing else: capturable in a HIP graph."""
        check(self._collect(self.env.handle(), ctypes.byref(self.policy.dims), ptr(self.policy.P),
                            ctypes.byref(self._io), self.E, self.T, stream_handle(self.device)), self._name)
        self.counter.add_(self.T)

    def collect(self, eps):
        """One episode of every env at exploration rate ``eps``: (fields dict of device tensors in the insert
        layout, per-env returns [E] = the reference's ``average_episode_rewards`` per env, one-hot actions
        [T, E, N, A])."""
        self.set_epsilon(eps)
        self.launch()
        return self.fields, self.returns, self.fields["acts"]


class OffQRunner:
    """``RecRunner`` for qmix / vdn on Checkers or Switch (``cfg.env``; base_runner.py:193-298): ``warmup()`` then
    ``run()`` per iteration. Per collect of E = ``n_envs`` episodes the counters advance as the reference's do with ``num_envs``:
    ``total_env_steps`` by E per step (T E per collect), ``num_episodes_collected`` by E; ``total_train_steps`` by
    one per gradient update."""

    def __init__(self, cfg=None, device="cuda", **overrides):
        cfg = replace(cfg if cfg is not None else OffQTrainConfig(), **overrides)
        assert cfg.algorithm_name in ("qmix", "vdn")
        self.cfg = cfg
        self.device = torch.device(device)
        E, N, T = cfg.n_envs, cfg.n_agents, cfg.episode_length
        self.num_envs, self.num_agents, self.episode_length = E, N, T
        self.env = make_env(cfg.env, E, N, max_steps=T, step_cost=cfg.step_cost, full_observable=False, device=device)
        D, A = self.env.obs_dim, self.env.n_actions
        self.trainer = OffQMix(N, D, A, T, cfg.batch_size, mixer=cfg.algorithm_name, hidden=cfg.hidden_size,
                               mixer_hidden=cfg.mixer_hidden_dim, hyper_hidden=cfg.hypernet_hidden_dim,
                               gamma=cfg.gamma, lr=cfg.lr, opti_eps=cfg.opti_eps, max_grad_norm=cfg.max_grad_norm,
                               use_double_q=cfg.use_double_q, use_per=cfg.use_per, use_huber_loss=cfg.use_huber_loss,
                               huber_delta=cfg.huber_delta, per_nu=cfg.per_nu, per_eps=cfg.per_eps, tau=cfg.tau,
                               device=device, seed=cfg.seed)
        self.collector = OffQCollector(self.env, self.trainer, T, cfg.seed, common_reward=cfg.use_common_reward)
        info = {"policy_0": {"obs_space": (D,), "share_obs_space": (N * D,), "act_space": (A,)}}
        agents = {"policy_0": list(range(N))}
        if cfg.use_per:
            self.buffer = PrioritizedRecReplayBuffer(cfg.per_alpha, info, agents, cfg.buffer_size, T,
                                                     cfg.use_same_share_obs, False, device=device, seed=cfg.seed)
        else:
            self.buffer = RecReplayBuffer(info, agents, cfg.buffer_size, T, cfg.use_same_share_obs, False,
                                          device=device, seed=cfg.seed)
        self.epsilon = DecayThenFlatSchedule(cfg.epsilon_start, cfg.epsilon_finish, cfg.epsilon_anneal_time)
        num_train_episodes = (cfg.num_env_steps / T) / cfg.train_interval_episode
        self.beta_anneal = DecayThenFlatSchedule(cfg.per_beta_start, 1.0, num_train_episodes)
        self.total_env_steps = 0
        self.num_episodes_collected = 0
        self.total_train_steps = 0
        self.last_train_episode = 0
        self.last_hard_update_episode = 0
        self.train_infos = []
        self.env_info = {}

    def _collect(self, eps):
        fields, returns, _ = self.collector.collect(eps)
        self.total_env_steps += self.num_envs * self.episode_length
        self.num_episodes_collected += self.num_envs
        self.buffer.insert_collected(self.num_envs, fields)
        self.env_info = {"average_episode_rewards": returns.mean()}   # device scalar: no sync here
        return self.env_info

    def warmup(self, num_warmup_episodes=None):
        """base_runner.py:225-238 with the random policy (eps = 1): (n // num_envs) + 1 collects."""
        n = num_warmup_episodes if num_warmup_episodes is not None else max(self.cfg.batch_size,
                                                                            self.cfg.num_random_episodes)
        for _ in range(n // self.num_envs + 1):
            self._collect(1.0)

    def run(self):
        """base_runner.py:193-223 without the save / log / eval branches: collect, insert, train when due."""
        self._collect(self.epsilon.eval(self.total_env_steps))
        if ((self.num_episodes_collected - self.last_train_episode) / self.cfg.train_interval_episode >= 1
                or self.last_train_episode == 0):
            self.batch_train_q()
            self.total_train_steps += 1
            self.last_train_episode = self.num_episodes_collected
        return self.total_env_steps

    def batch_train_q(self):
        """base_runner.py:273-298."""
        cfg = self.cfg
        if cfg.use_per:
            beta = self.beta_anneal.eval(self.total_train_steps)
            sample = self.buffer.sample(cfg.batch_size, beta, "policy_0")
        else:
            sample = self.buffer.sample(cfg.batch_size)
        train_info, new_priorities, idxes = self.trainer.train_policy_on_batch(sample)
        if cfg.use_per:
            self.buffer.update_priorities(idxes, new_priorities, "policy_0")
        self.train_infos = [train_info]
        if cfg.use_soft_update:
            self.trainer.soft_target_updates()
        elif (self.num_episodes_collected - self.last_hard_update_episode) / cfg.hard_update_interval_episode >= 1:
            self.trainer.hard_target_updates()
            self.last_hard_update_episode = self.num_episodes_collected


__all__ = ["OffQCollector", "OffQRunner", "DecayThenFlatSchedule"]
