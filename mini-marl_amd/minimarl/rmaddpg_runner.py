"""Offpolicy rmaddpg / rmatd3 end to end on the MI355X: the device episode collector and the training runner.

``RMADDPGCollector`` stands in for ``collect_rollout`` (offpolicy/runner/shared/magym_runner.py:40-141) with
``R_MADDPGPolicy.get_actions`` (algorithm/rMADDPGPolicy.py:62-133, discrete non-multidiscrete branch): one
``mm_rmaddpg_collect`` / ``mm_rmaddpg_collect_switch`` launch (csrc/rmaddpg_collect.hip) runs a whole T-step episode of
E lockstep Checkers or Switch envs with the recurrent actor (hidden state zero at t = 0, carried over all T steps, never
reset), samples every (env, agent) action as the hard Gumbel-softmax of its logits, replaces it by a uniform action with
probability epsilon, and leaves the episode fields in HBM in the replay buffer's insert layout. ``RMADDPGRunner`` is
``OffQRunner``'s ``warmup`` / ``run`` with ``batch_train`` (runner/shared/base_runner.py:240-271) over it,
``RecReplayBuffer.insert_collected`` and ``RMADDPG``.

Deviations from the reference (those of ``offq_runner`` apply: true one-hot ``acts``, the final observation at index T,
E envs per collect, one epsilon per episode), and:
* the noise is the project's counter RNG, not torch's: ``g = -log(-log(U + 1e-20) + 1e-20)`` with
  ``U = rng_uniform(rng_draw(noise_seed ^ COLLECT_GUMBEL_SALT, counter + t, e, n A + k))``, which is what
  ``mm_maddpg_gumbel(B = E, ...)`` leaves at ``g[n][e][k]``; the stored action is the argmax of ``logits + g``
  (``gumbel_softmax(hard=True)`` is that one-hot up to an ulp);
* warm-up is epsilon = 1 collects (the reference calls ``get_random_actions``): every action is the uniform one, no
  noise is drawn and the actor is not evaluated;
* ``explore=False`` takes the first maximum of the logits on an exact tie, where ``onehot_from_logits`` would be
  multi-hot;
* last actions are not an input of the actor (``prev_act_inp`` is not built in ``RMADDPG``).
There is no CPU path.
"""
from ._lib import RmaddpgCollectIO
from .maddpg import COLLECT_GUMBEL_SALT
from .maddpg_runner import MADDPGRunner
from .offq_runner import OffQCollector, OffQRunner
from .rmaddpg import RMADDPG


class RMADDPGCollector(OffQCollector):
    """``OffQCollector``'s surface (``fields``, ``returns``, ``q``, ``eps``, ``counter``, ``set_epsilon``, ``launch``,
    ``collect``, ``share_obs``) for ``policy`` = an ``RMADDPG``: ``policy.Pa`` is read in place, ``q`` holds the actor's
    logits. ``seed`` drives the epsilon draws and the uniform actions, ``policy.noise_seed`` the Gumbel noise.
    ``explore=False`` is the reference's ``collect_rollout(explore=False)``: greedy, epsilon ignored."""

    _names, _io_type, _params = ("rmaddpg_collect", "rmaddpg_collect_switch"), RmaddpgCollectIO, "Pa"

    def __init__(self, env, policy, T, seed, common_reward=True, with_q=False, explore=True):
        self.explore = bool(explore)
        self.gumbel_seed = policy.noise_seed ^ COLLECT_GUMBEL_SALT
        super().__init__(env, policy, T, seed, common_reward=common_reward, with_q=with_q)

    def _make_io(self):
        io = super()._make_io()
        io.gumbel_seed, io.explore = self.gumbel_seed, int(self.explore)
        return io


class RMADDPGRunner(OffQRunner):
    """``OffQRunner`` for rmaddpg / rmatd3 on Checkers or Switch: its ``warmup`` / ``run``, counters and episode buffer
    over ``RMADDPGCollector`` and ``RMADDPG``; the training step is ``MADDPGRunner``'s ``batch_train``."""

    ALGORITHMS = ("rmaddpg", "rmatd3")

    def _make_trainer(self, D, A):
        cfg = self.cfg
        return RMADDPG(self.num_agents, D, A, self.episode_length, cfg.batch_size, td3=cfg.algorithm_name == "rmatd3",
                       hidden=cfg.hidden_size, gamma=cfg.gamma, lr=cfg.lr, opti_eps=cfg.opti_eps,
                       max_grad_norm=cfg.max_grad_norm, use_per=cfg.use_per, per_nu=cfg.per_nu,
                       use_huber_loss=cfg.use_huber_loss, huber_delta=cfg.huber_delta, per_eps=cfg.per_eps, tau=cfg.tau,
                       use_same_share_obs=cfg.use_same_share_obs, device=self.device, seed=cfg.seed, noise_seed=cfg.seed)

    def _make_collector(self):
        return RMADDPGCollector(self.env, self.trainer, self.episode_length, self.cfg.seed,
                                common_reward=self.cfg.use_common_reward)

    batch_train = MADDPGRunner.batch_train      # base_runner.py:240-271 for the one shared policy
    batch_train_q = batch_train                 # the training step ``OffQRunner.run`` calls


__all__ = ["RMADDPGCollector", "RMADDPGRunner"]
