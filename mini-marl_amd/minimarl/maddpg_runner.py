"""Offpolicy maddpg / matd3 end to end on the MI355X: the device transition collector and the training runner.

``MADDPGCollector`` stands in for the MLP runner's collect loop (``collecter``, runner/shared/magym_runner.py) with
``MADDPGPolicy.get_actions`` (algorithm/MADDPGPolicy.py:95-104, discrete branch): one ``mm_maddpg_collect`` /
``mm_maddpg_collect_switch`` launch (csrc/maddpg_collect.hip) runs a window of T lockstep steps of E Checkers or Switch
envs from reset with the actor, samples every (env, agent) action as the hard Gumbel-softmax of its logits, replaces it
by a uniform action with probability epsilon, resets an env inside the window when it is done, and leaves T * E single
transitions in HBM: in its own staging tensors, or in place in a replay ring. ``MADDPGRunner`` is ``OffQRunner``'s
``warmup`` / ``run`` with ``batch_train`` (runner/shared/base_runner.py:240-271) over it,
``MlpReplayBuffer.insert_collected`` and ``MADDPG``.

Deviations from the reference (those of ``moffq_runner`` apply: windows instead of episodes, E envs per collect, true
one-hot ``acts``, one epsilon per window, ``buffer_size`` in transitions, ``leaf_mode="slots"``), and:
* the noise is the project's counter RNG, not torch's: ``g = -log(-log(U + 1e-20) + 1e-20)`` with
  ``U = rng_uniform(rng_draw(noise_seed ^ COLLECT_GUMBEL_SALT, counter + t, e, n A + k))``, which is what
  ``mm_maddpg_gumbel(B = E, ...)`` leaves at ``g[n][e][k]``; the stored action is the argmax of ``logits + g``
  (``gumbel_softmax(hard=True)`` is that one-hot up to an ulp);
* warm-up is epsilon = 1 windows (the reference calls ``get_random_actions``): every action is the uniform one and
  no noise is drawn;
* ``explore=False`` takes the first maximum of the logits on an exact tie, where ``onehot_from_logits`` would be
  multi-hot.
There is no CPU path.
"""
from ._lib import MaddpgCollectIO
from .maddpg import COLLECT_GUMBEL_SALT, MADDPG
from .moffq_runner import MOffQCollector, MOffQRunner


class MADDPGCollector(MOffQCollector):
    """``MOffQCollector``'s surface (``fields``, ``returns``, ``n_done``, ``q``, ``eps``, ``counter``,
    ``set_epsilon``, ``launch``, ``collect``) for ``policy`` = a ``MADDPG``: ``policy.Pa`` is read in place, ``q``
    holds the actor's logits. ``seed`` drives the epsilon draws and the uniform actions, ``policy.noise_seed`` the
    Gumbel noise. ``explore=False`` is the reference's ``collecter(explore=False)``: greedy, epsilon ignored."""

    _names, _io_type, _params = ("maddpg_collect", "maddpg_collect_switch"), MaddpgCollectIO, "Pa"

    def __init__(self, env, policy, T, seed, common_reward=True, with_q=False, explore=True):
        self.explore = bool(explore)
        self.gumbel_seed = policy.noise_seed ^ COLLECT_GUMBEL_SALT
        super().__init__(env, policy, T, seed, common_reward=common_reward, with_q=with_q)

    def _make_io(self, p, first, size):
        io = super()._make_io(p, first, size)
        io.gumbel_seed, io.explore = self.gumbel_seed, int(self.explore)
        return io


class MADDPGRunner(MOffQRunner):
    """``OffQRunner`` for maddpg / matd3 on Checkers or Switch: ``warmup`` / ``run`` and the counters of
    ``MOffQRunner`` (a collect window counts as E = ``n_envs`` episodes and T * E env steps) over ``MADDPGCollector``,
    a transition ring and ``MADDPG``; the training step is ``batch_train``."""

    ALGORITHMS = ("maddpg", "matd3")

    def _make_trainer(self, D, A):
        cfg = self.cfg
        return MADDPG(self.num_agents, D, A, td3=cfg.algorithm_name == "matd3", hidden=cfg.hidden_size, gamma=cfg.gamma,
                      lr=cfg.lr, opti_eps=cfg.opti_eps, max_grad_norm=cfg.max_grad_norm, use_per=cfg.use_per,
                      use_huber_loss=cfg.use_huber_loss, huber_delta=cfg.huber_delta, per_eps=cfg.per_eps, tau=cfg.tau,
                      use_same_share_obs=cfg.use_same_share_obs, device=self.device, seed=cfg.seed, noise_seed=cfg.seed)

    def _make_collector(self):
        return MADDPGCollector(self.env, self.trainer, self.episode_length, self.cfg.seed,
                               common_reward=self.cfg.use_common_reward)

    def batch_train(self):
        """base_runner.py:240-271 for the one shared policy."""
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
        if cfg.use_soft_update and train_info.get("update_actor", False):
            self.trainer.soft_target_updates()
        elif (self.num_episodes_collected - self.last_hard_update_episode) / cfg.hard_update_interval_episode >= 1:
            self.trainer.hard_target_updates()
            self.last_hard_update_episode = self.num_episodes_collected

    batch_train_q = batch_train      # the training step ``OffQRunner.run`` calls


__all__ = ["MADDPGCollector", "MADDPGRunner"]
