"""Recurrent MADDPG / MATD3 ("rmaddpg" / "rmatd3" of the reference's ``offpolicy/`` fork) on the MI355X.

Mirrors ``R_MADDPG.shared_train_policy_on_batch`` (offpolicy/algorithms/r_maddpg/r_maddpg.py:114-331; ``R_MATD3`` is
the same class with ``actor_update_interval = 2``) with its shared ``R_MADDPGPolicy`` (algorithm/rMADDPGPolicy.py) over
mm_rmaddpg_* (include/minimarl_rmaddpg.h, csrc/rmaddpg.hip) for discrete actions and one policy (``policy_0``).
Everything runs on the GPU; there is no CPU path.

Two flat parameter / Adam sets in the trunk layout of ``minimarl.maddpg`` (``_Trunk(D, A)`` and ``_Trunk(Dc, nq)``,
Dc = N (D + A)): LN -> Linear -> ReLU -> LN -> Linear -> ReLU -> LN -> GRU -> LN -> head(s). Unlike the feed-forward
``MADDPG``, the critic's 1 (rmaddpg) or 2 (rmatd3) ``q_outs`` heads are an ``nn.ModuleList`` in the reference: they are
trained, counted in the gradient norm, held in the state dict as ``q_outs.h.weight / bias`` and covered by the target
updates. ``num_updates`` is incremented on every call (r_maddpg.py:330), so rmatd3 updates the actor on every second
call. The priorities carry ``per_eps`` twice, as the reference's do (r_maddpg.py:217-218).
Gumbel noise: injected through ``train_policy_on_batch(..., gumbel=, target_gumbel=)`` or drawn by mm_maddpg_gumbel of
the project's counter RNG (row index t B + b, salts below).

Not built, raise ``ValueError`` before any allocation: prev_act_inp, use_popart, use_same_share_obs=False,
use_value_active_masks, available-action masks, multidiscrete or continuous actions, layer_N != 1, recurrent_N != 1,
weight_decay, more than one policy, H != 64, A != 5, D not in {3, 47, 94}, critic width N (D + A) > 416.
"""
import ctypes

import numpy as np
import torch

from ._lib import MaddpgDims, RmaddpgBatch, c_i64, check, lib
from .maddpg import MAX_CRITIC_WIDTH, _Trunk
from .offq import AGENT_KEYS, AGENT_REF
from .qnet import ptr, stream_handle

GUMBEL_SALT, TARGET_GUMBEL_SALT, ACT_GUMBEL_SALT = 0x67756D62656C0011, 0x67756D62656C0012, 0x67756D62656C0013
TRUNK_REF = {k: v for k, v in AGENT_REF.items() if k not in ("Wo", "bo")}
ACTOR_REF = dict(TRUNK_REF, Wo="act.action_out.weight", bo="act.action_out.bias")


class RMADDPG:
    """R_MADDPG / R_MATD3 (``td3=True``) trainer + shared recurrent policy (one policy, ``policy_0``)."""

    def __init__(self, n_agents, obs_dim, n_actions, episode_length, batch_size, td3=False, hidden=64, gamma=0.99,
                 lr=5e-4, opti_eps=1e-5, max_grad_norm=10.0, use_per=True, per_nu=0.9, use_huber_loss=False,
                 huber_delta=10.0, per_eps=1e-6, tau=0.005, actor_update_interval=None, device="cuda", seed=None,
                 noise_seed=0, grad_allreduce=None, prev_act_inp=False, use_popart=False, use_same_share_obs=True,
                 weight_decay=0.0, layer_N=1, recurrent_N=1, use_value_active_masks=False, multidiscrete=False,
                 continuous=False, n_policies=1):
        for name, bad in (("prev_act_inp", prev_act_inp), ("use_popart", use_popart),
                          ("use_same_share_obs=False", not use_same_share_obs), ("weight_decay", weight_decay != 0),
                          ("layer_N != 1", layer_N != 1), ("recurrent_N != 1", recurrent_N != 1),
                          ("use_value_active_masks", use_value_active_masks),
                          ("multidiscrete actions", multidiscrete), ("continuous actions", continuous),
                          ("more than one policy", n_policies != 1)):
            if bad:
                raise ValueError(f"RMADDPG: {name} is not built")
        N, D, A, H = int(n_agents), int(obs_dim), int(n_actions), int(hidden)
        T, B = int(episode_length), int(batch_size)
        if H != 64 or A != 5 or D not in (3, 47, 94) or N < 1 or T < 1 or B < 1:
            raise ValueError(f"RMADDPG: unsupported dims N={N} D={D} H={H} A={A} T={T} B={B} (supported: N, T, B >= 1, "
                             "D 3|47|94, H 64, A 5)")
        if N * (D + A) > MAX_CRITIC_WIDTH:
            raise ValueError(f"RMADDPG: critic input width N (D + A) = {N * (D + A)} is above the limit of "
                             f"{MAX_CRITIC_WIDTH}")
        self.N, self.D, self.A, self.H, self.T, self.B, self.td3 = N, D, A, H, T, B, bool(td3)
        self.S, self.Dc, self.nq = N * D, N * (D + A), 2 if td3 else 1
        self.gamma, self.lr, self.eps, self.max_norm = gamma, lr, opti_eps, max_grad_norm
        self.use_per, self.nu, self.huber, self.delta = use_per, per_nu, use_huber_loss, huber_delta
        self.per_eps, self.tau = per_eps, tau
        self.actor_update_interval = int(actor_update_interval or (2 if td3 else 1))
        self.num_updates, self.act_calls = 0, 0
        self.noise_seed = int(noise_seed) & 0xFFFFFFFFFFFFFFFF
        self.allreduce = grad_allreduce
        self.device = torch.device(device)
        self.dims = MaddpgDims(N, D, H, A, int(self.td3))
        na, nc = c_i64(), c_i64()
        check(lib().mm_rmaddpg_param_counts(ctypes.byref(self.dims), ctypes.byref(na), ctypes.byref(nc)),
              "rmaddpg_param_counts")
        self.actor, self.critic = _Trunk(D, A), _Trunk(self.Dc, self.nq)
        assert (self.actor.total, self.critic.total) == (na.value, nc.value)
        nbytes = int(lib().mm_rmaddpg_workspace_bytes(ctypes.byref(self.dims), T, B))
        check(0 if nbytes > 0 else -22, "rmaddpg_workspace_bytes")
        dev = self.device
        for s, n in (("a", self.actor.total), ("c", self.critic.total)):
            for name in ("P", "PT", "grad", "m", "v"):
                setattr(self, name + s, torch.zeros(n, device=dev))
            for name in ("step", "norm"):
                setattr(self, name + s, torch.zeros(1, device=dev))
            setattr(self, "stats" + s, torch.zeros(2, device=dev))
        self.partials = torch.zeros(512, device=dev)
        self.ws, self.ws_bytes = torch.empty((nbytes + 3) // 4, device=dev), nbytes
        self.prio = torch.zeros(B, device=dev)
        self.gbuf, self.tgbuf = torch.zeros(N, T, B, A, device=dev), torch.zeros(N, T, B, A, device=dev)
        if seed is not None:
            self.init_default(seed)

    # -- parameters --------------------------------------------------------------------------
    def actor_view(self, key, target=False):
        return self.actor.view(self.PTa if target else self.Pa, key)

    def critic_view(self, key, target=False):
        return self.critic.view(self.PTc if target else self.Pc, key)

    def init_default(self, seed):
        """The reference init: orthogonal weights (gain sqrt(2) in the ReLU MLPs, ``gain`` = 0.01 for the action head,
        1 for the GRU and the Q heads), zero biases, unit LayerNorms; targets = copies."""
        g = torch.Generator().manual_seed(int(seed))
        for tr, P in ((self.actor, self.Pa), (self.critic, self.Pc)):
            P.zero_()
            for key in AGENT_KEYS:
                shp = tr.shape(key)
                if key.startswith("ln") and key.endswith("_w"):
                    tr.view(P, key).fill_(1.0)
                elif len(shp) == 2:
                    actor_head = key == "Wo" and tr is self.actor
                    gain = float(np.sqrt(2.0)) if key in ("W1", "W2") else (0.01 if actor_head else 1.0)
                    parts = [shp] if (key != "Wo" or actor_head) else [(1, shp[1])] * shp[0]   # q_outs: one Linear each
                    ws = [torch.nn.init.orthogonal_(torch.empty(p), gain=gain, generator=g) for p in parts]
                    tr.view(P, key).copy_(torch.cat(ws))
        self.hard_target_updates()

    def load_reference_state(self, actor_sd, critic_sd, target_actor_sd=None, target_critic_sd=None):
        """R_MADDPG_Actor / R_MADDPG_Critic ``state_dict()``s (heads: ``q_outs.h.weight / bias``). Targets default to
        copies."""
        f32 = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.float32)
        for target, asd, csd in ((False, actor_sd, critic_sd),
                                 (True, target_actor_sd or actor_sd, target_critic_sd or critic_sd)):
            if sum(k.startswith("q_outs.") and k.endswith("weight") for k in csd) != self.nq:
                raise ValueError(f"RMADDPG: {self.nq} critic heads expected")
            for k, name in ACTOR_REF.items():
                self.actor_view(k, target).copy_(f32(asd[name]))
            for k, name in TRUNK_REF.items():
                self.critic_view(k, target).copy_(f32(csd[name]))
            for h in range(self.nq):
                self.critic_view("Wo", target)[h].copy_(f32(csd[f"q_outs.{h}.weight"]).reshape(self.H))
                self.critic_view("bo", target)[h] = float(np.asarray(csd[f"q_outs.{h}.bias"]).reshape(()))

    def state_dict(self, target=False):
        """(actor state dict, critic state dict) under the reference's names."""
        cpu = lambda t: t.detach().cpu().clone()
        a = {name: cpu(self.actor_view(k, target)) for k, name in ACTOR_REF.items()}
        c = {name: cpu(self.critic_view(k, target)) for k, name in TRUNK_REF.items()}
        for h in range(self.nq):
            c[f"q_outs.{h}.weight"] = cpu(self.critic_view("Wo", target)[h:h + 1])
            c[f"q_outs.{h}.bias"] = cpu(self.critic_view("bo", target)[h:h + 1])
        return a, c

    def hard_target_updates(self):
        self.PTa.copy_(self.Pa)
        self.PTc.copy_(self.Pc)

    def soft_target_updates(self):
        L, st = lib(), stream_handle(self.device)
        check(L.mm_offq_soft_update(ptr(self.PTa), ptr(self.Pa), self.actor.total, float(self.tau), st), "soft_update")
        check(L.mm_offq_soft_update(ptr(self.PTc), ptr(self.Pc), self.critic.total, float(self.tau), st), "soft_update")

    def checkpoint_tensors(self):
        ts = {k + s: getattr(self, k + s) for s in "ac" for k in ("P", "PT", "m", "v", "step")}
        return ts, {"td3": int(self.td3), "num_updates": self.num_updates, "act_calls": self.act_calls}

    def restore_tensors(self, ts, scalars):
        from .checkpoint import copy_into
        if int(scalars.get("td3", int(self.td3))) != int(self.td3):
            raise ValueError("RMADDPG checkpoint: td3 differs")
        for s in "ac":
            for k in ("P", "PT", "m", "v", "step"):
                copy_into(getattr(self, k + s), ts[k + s], k + s)
        self.num_updates, self.act_calls = int(scalars.get("num_updates", 0)), int(scalars.get("act_calls", 0))

    # -- training ----------------------------------------------------------------------------
    def _dev(self, x):
        t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
        return t.to(device=self.device, dtype=torch.float32).contiguous()

    def _noise(self, given, buf, salt):
        if given is not None:
            g = self._dev(given)
            assert g.numel() == buf.numel(), (g.shape, buf.shape)
            return g
        check(lib().mm_maddpg_gumbel(ctypes.byref(self.dims), ptr(buf), self.T * self.B, self.noise_seed ^ salt,
                                     self.num_updates, stream_handle(self.device)), "maddpg_gumbel")
        return buf

    def _clip_adam(self, s, n):
        scale = 1.0
        grad = getattr(self, "grad" + s)
        if self.allreduce is not None:
            scale = 1.0 / self.allreduce(grad)
        check(lib().mm_clip_adam(ptr(getattr(self, "P" + s)), ptr(grad), ptr(getattr(self, "m" + s)),
                                 ptr(getattr(self, "v" + s)), n, n, self.max_norm, self.lr, 0.9, 0.999, self.eps,
                                 ptr(getattr(self, "step" + s)), ptr(self.partials), ptr(getattr(self, "norm" + s)),
                                 scale, stream_handle(self.device)), "clip_adam")

    def train_policy_on_batch(self, batch, gumbel=None, target_gumbel=None):
        """R_MADDPG.shared_train_policy_on_batch. batch = the RecReplayBuffer.sample tuple (obs [N, T+1, B, D],
        share_obs [T+1, B, S], acts [N, T, B, A], rewards [N, T, B, 1], dones [N, T, B, 1], dones_env [T, B, 1],
        avail_acts (None), importance_weights [B] or None, idxes), arrays bare or {policy_id: array}. gumbel /
        target_gumbel [N, T, B, A]: injected Gumbel(0, 1) noise of the actor pass (obs step t) / of rmatd3's target
        actions (obs step t + 1). Returns (train_info {critic_loss, critic_grad_norm, actor_loss, actor_grad_norm,
        update_actor} as device scalars, new priorities [B] or None, idxes); no sync."""
        obs, share, acts, rew, dones, dones_env, avail, isw, idxes = batch
        pick = (lambda d: d["policy_0"] if isinstance(d, dict) else d)
        if pick(avail) is not None:
            raise ValueError("RMADDPG: available-action masks are not built")
        N, T, B = self.N, self.T, self.B
        o, s, a, r, dn, de = (self._dev(pick(x)) for x in (obs, share, acts, rew, dones, dones_env))
        assert tuple(o.shape) == (N, T + 1, B, self.D) and tuple(s.shape) == (T + 1, B, self.S), (o.shape, s.shape)
        assert a.numel() == N * T * B * self.A and r.numel() == N * T * B and dn.numel() == N * T * B
        assert de.numel() == T * B
        w = self._dev(isw) if (self.use_per and isw is not None) else None
        L, st = lib(), stream_handle(self.device)
        update_actor = self.num_updates % self.actor_update_interval == 0
        g = self._noise(gumbel, self.gbuf, GUMBEL_SALT) if update_actor else None
        tg = self._noise(target_gumbel, self.tgbuf, TARGET_GUMBEL_SALT) if self.td3 else None
        self._keep = (o, s, a, r, dn, de, w, g, tg)         # alive until the kernels ran
        bt = RmaddpgBatch()
        bt.obs, bt.share_obs, bt.acts, bt.rewards, bt.dones, bt.dones_env = (ptr(x) for x in (o, s, a, r, dn, de))
        bt.is_weight, bt.gumbel, bt.target_gumbel = ptr(w), ptr(g), ptr(tg)
        bt.T, bt.B, bt.huber, bt.gamma, bt.huber_delta = T, B, int(self.huber), self.gamma, self.delta
        bt.per_eps, bt.per_nu = self.per_eps, self.nu
        d = ctypes.byref(self.dims)
        check(L.mm_rmaddpg_critic_grad(d, ctypes.byref(bt), ptr(self.PTa), ptr(self.Pc), ptr(self.PTc), ptr(self.gradc),
                                       ptr(self.ws), self.ws_bytes, ptr(self.statsc), ptr(self.prio), st),
              "rmaddpg_critic_grad")
        self._clip_adam("c", self.critic.total)
        info = {"critic_loss": self.statsc[0], "critic_grad_norm": self.normc[0]}
        if update_actor:
            check(L.mm_rmaddpg_actor_grad(d, ctypes.byref(bt), ptr(self.Pa), ptr(self.Pc), ptr(self.grada),
                                          ptr(self.ws), self.ws_bytes, ptr(self.statsa), st), "rmaddpg_actor_grad")
            self._clip_adam("a", self.actor.total)
            info.update(actor_loss=self.statsa[0], actor_grad_norm=self.norma[0])
        info["update_actor"] = update_actor
        self.num_updates += 1
        return info, (self.prio.clone() if w is not None else None), idxes

    # -- acting ------------------------------------------------------------------------------
    def init_hidden(self, n_agents, batch_size):
        """R_MADDPGPolicy.init_hidden: zeros [n_agents, batch, H], or [batch, H] for n_agents = -1."""
        shp = (batch_size, self.H) if n_agents == -1 else (n_agents, batch_size, self.H)
        return torch.zeros(shp, device=self.device)

    def get_actions(self, obs, rnn_states, explore=False, use_target=False, use_gumbel=False, gumbel=None, eps=0.0,
                    return_logits=False):
        """R_MADDPGPolicy.get_actions for one step (discrete branch): obs [R, D], rnn_states [R, H] -> (one-hot
        actions [R, A], new rnn_states [R, H], eps or None). ``use_gumbel`` (or ``explore``, or ``use_target`` with
        rmatd3) takes the argmax of logits + Gumbel noise (``gumbel`` [R, A] if injected, else the counter RNG under
        ``ACT_GUMBEL_SALT``); otherwise logits == rowmax. ``explore`` replaces a row by a uniform random action with
        probability ``eps``."""
        x = self._dev(obs).reshape(-1, self.D)
        R = int(x.shape[0])
        h = self._dev(rnn_states).reshape(R, self.H)
        noisy = use_gumbel or explore or (use_target and self.td3)
        L, st = lib(), stream_handle(self.device)
        g = None
        if noisy:
            if gumbel is not None:
                g = self._dev(gumbel).reshape(R, self.A)
            else:
                g = torch.empty(R, self.A, device=self.device)
                one = MaddpgDims(1, self.D, self.H, self.A, int(self.td3))
                check(L.mm_maddpg_gumbel(ctypes.byref(one), ptr(g), R, self.noise_seed ^ ACT_GUMBEL_SALT,
                                         self.act_calls, st), "maddpg_gumbel")
        logits, hot = torch.empty(R, 8, device=self.device), torch.empty(R, self.A, device=self.device)
        hout, scratch = torch.empty(R, self.H, device=self.device), torch.empty(R, 192, device=self.device)
        check(L.mm_rmaddpg_step(ctypes.byref(self.dims), ptr(self.PTa if use_target else self.Pa), ptr(x), ptr(h),
                                ptr(g), ptr(logits), ptr(hot), ptr(hout), ptr(scratch), R, st), "rmaddpg_step")
        call, self.act_calls = self.act_calls, self.act_calls + int(noisy)
        used_eps = None
        if explore:
            gen = torch.Generator(device=self.device).manual_seed(((self.noise_seed ^ ACT_GUMBEL_SALT) + call) % 2 ** 63)
            take = (torch.rand(R, 1, device=self.device, generator=gen) < eps).float()
            hot, used_eps = (1 - take) * hot + take * self.get_random_actions(obs, gen), eps
        if return_logits:
            return hot, hout, used_eps, logits[:, :self.A]
        return hot, hout, used_eps

    def get_random_actions(self, obs, generator=None):
        R = int(np.prod(tuple(obs.shape)[:-1]))
        ra = torch.randint(0, self.A, (R,), device=self.device, generator=generator)
        return torch.nn.functional.one_hot(ra, self.A).float()


__all__ = ["RMADDPG"]
