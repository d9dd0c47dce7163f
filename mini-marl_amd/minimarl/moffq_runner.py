"""Offpolicy mqmix / mvdn end to end on the MI355X: the device transition collector and the training runner.

``MOffQCollector`` stands in for the MLP runner's collect loop: one ``mm_moffq_collect`` / ``mm_moffq_collect_switch``
launch (csrc/moffq_collect.hip) runs a window of T lockstep steps of E Checkers or Switch envs from reset with the
feed-forward behavior net and per-(env, agent) epsilon-greedy, resets an env inside the window when it is done, and
leaves T * E single transitions in HBM: in its own staging tensors, or in place in a replay ring.
``MOffQRunner`` is ``OffQRunner``'s ``warmup`` / ``run`` / ``batch_train_q`` over it,
``MlpReplayBuffer.insert_collected`` and ``MOffQMix``.

Deviations from the reference (those of ``offq_runner`` apply: true one-hot ``acts``, E envs per collect, device RNG,
one epsilon per window), and:
* a collect is a window of T steps from reset, not an episode: an env that finishes is reset inside it, and the window
  cuts the last episode of each env short (its last transition has ``dones_env`` 0 unless the env finished there);
  a window counts as E episodes and T * E env steps;
* ``buffer_size`` counts transitions; the buffer runs with ``leaf_mode="slots"`` and ``store_share=False``
  (``cent_obs`` is the agents' observations concatenated, never materialised);
* ``average_episode_rewards`` is the mean over envs of the window's summed reward (agent 0's stored reward).
There is no CPU path.
"""
import ctypes

import torch

from ._lib import MoffqCollectIO, check, lib
from .env import SwitchVecEnv
from .mlpbuf import MlpReplayBuffer, PrioritizedMlpReplayBuffer
from .moffq import MOffQMix
from .offq_runner import OffQRunner
from .qnet import ptr, stream_handle

STAGED = ("obs", "next_obs", "acts", "rewards", "dones", "dones_env", "valid_transition")


class MOffQCollector:
    """One-launch transition collection for ``env`` (a Checkers ``VecEnv`` with local observations, or a
    ``SwitchVecEnv`` with local observations and the clock) and ``policy`` (a ``MOffQMix``: ``policy.P`` is read in
    place). Transition j = t * E + e of a window; ``fields`` are the staging tensors [T * E, ...] that ``collect``
    fills, ``returns`` [E] the window's summed reward (agent 0's stored one), ``n_done`` [E] the episodes finished in
    it, ``q`` [T * E, N, A] with ``with_q``. The env handle supplies the rules and the reset state; its live state is
    neither read nor written. The launch does not sync and reads epsilon and the RNG step counter from device memory,
    so a captured ``launch()`` replays with whatever ``set_epsilon`` / ``counter`` hold at replay time."""

    # what a collector of another algorithm family replaces: the entry points (Checkers, Switch), their io struct and
    # the policy's parameter vector the launch reads
    _names, _io_type, _params = ("moffq_collect", "moffq_collect_switch"), MoffqCollectIO, "P"

    def __init__(self, env, policy, T, seed, common_reward=True, with_q=False):
        self.env, self.policy = env, policy
        self.E, self.N, self.T = int(env.E), int(env.N), int(T)
        self.D, self.A = int(policy.D), int(policy.A)
        self.device = policy.device
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.common_reward = bool(common_reward)
        self._name = self._names[isinstance(env, SwitchVecEnv)]
        self._collect, supported = getattr(lib(), "mm_" + self._name), getattr(lib(), "mm_" + self._name + "_supported")
        if not supported(env.handle(), ctypes.byref(policy.dims), self.E, self.T):
            # the launch reports why
            check(self._collect(env.handle(), ctypes.byref(policy.dims), None, None, self.E, self.T, None), self._name)
        dev, N, n = self.device, self.N, self.T * self.E
        self.fields = {"obs": torch.zeros(n, N, self.D, device=dev), "next_obs": torch.zeros(n, N, self.D, device=dev),
                       "acts": torch.zeros(n, N, self.A, device=dev), "rewards": torch.zeros(n, N, 1, device=dev),
                       "dones": torch.zeros(n, N, 1, device=dev), "dones_env": torch.zeros(n, 1, device=dev),
                       "valid_transition": torch.zeros(n, N, 1, device=dev)}
        self.returns = torch.zeros(self.E, device=dev)
        self.n_done = torch.zeros(self.E, dtype=torch.int32, device=dev)
        self.q = torch.zeros(n, N, self.A, device=dev) if with_q else None
        self.eps = torch.zeros(1, device=dev)
        self.counter = torch.zeros(1, dtype=torch.int64, device=dev)   # counter0 of the next collect
        self._io = self._make_io({k: ptr(v) for k, v in self.fields.items()}, 0, n)

    def _make_io(self, p, first, size):
        io = self._io_type()
        io.eps, io.counter, io.counter0, io.seed = ptr(self.eps), ptr(self.counter), 0, self.seed
        io.common_reward = int(self.common_reward)
        io.first, io.size = int(first), int(size)
        for k in STAGED:
            setattr(io, k, p[k])
        io.q_out, io.ret_out, io.n_done_out = ptr(self.q), ptr(self.returns), ptr(self.n_done)
        return io

    def set_epsilon(self, eps):
        """Stream-ordered write of the epsilon the next launch (or graph replay) reads."""
        self.eps.fill_(float(eps))

    def launch(self, stores=None, first=0, size=None):
        """The collect launch and the counter advance (+T), nothing else: capturable in a HIP graph. With ``stores``
        (an ``MlpbufFields`` of [size][row] device stores) the window goes to ring slots (first + j) % size of them
        instead of the staging tensors."""
        io = self._io if stores is None else self._make_io({k: getattr(stores, k) for k in STAGED}, first, size)
        check(self._collect(self.env.handle(), ctypes.byref(self.policy.dims), ptr(getattr(self.policy, self._params)),
                            ctypes.byref(io), self.E, self.T, stream_handle(self.device)), self._name)
        self.counter.add_(self.T)

    def collect(self, eps):
        """One window of every env at exploration rate ``eps``: (staging fields dict, per-env returns [E])."""
        self.set_epsilon(eps)
        self.launch()
        return self.fields, self.returns


class MOffQRunner(OffQRunner):
    """``OffQRunner`` for mqmix / mvdn on Checkers or Switch: the same ``warmup`` / ``run`` / ``batch_train_q`` and
    counters over ``MOffQCollector``, a transition ring and ``MOffQMix``. A collect window counts as E = ``n_envs``
    episodes and T * E env steps; ``buffer_size`` counts transitions."""

    ALGORITHMS = ("mqmix", "mvdn")

    def _make_trainer(self, D, A):
        return MOffQMix(self.num_agents, D, A, mixer=self.cfg.algorithm_name[1:], **self._trainer_args())

    def _make_collector(self):
        return MOffQCollector(self.env, self.trainer, self.episode_length, self.cfg.seed,
                              common_reward=self.cfg.use_common_reward)

    def _make_buffer(self, info, agents):
        cfg = self.cfg
        kw = dict(device=self.device, seed=cfg.seed, leaf_mode="slots", store_share=False)
        if cfg.use_per:
            return PrioritizedMlpReplayBuffer(cfg.per_alpha, info, agents, cfg.buffer_size, cfg.use_same_share_obs,
                                              False, **kw)
        return MlpReplayBuffer(info, agents, cfg.buffer_size, cfg.use_same_share_obs, False, **kw)

    def _collect(self, eps):
        self.collector.set_epsilon(eps)
        self.buffer.insert_collected(self.collector)   # the launch writes the ring at the cursor
        self.total_env_steps += self.num_envs * self.episode_length
        self.num_episodes_collected += self.num_envs
        self.env_info = {"average_episode_rewards": self.collector.returns.mean()}   # device scalar: no sync here
        return self.env_info


__all__ = ["MOffQCollector", "MOffQRunner"]
