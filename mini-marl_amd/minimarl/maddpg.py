"""Feed-forward transition-batch MADDPG / MATD3 ("maddpg" / "matd3" of the reference's ``offpolicy/`` fork) on the MI355X.

Mirrors ``MADDPG.shared_train_policy_on_batch`` (offpolicy/algorithms/maddpg/maddpg.py:90-249; ``MATD3`` is the same
trainer) with its shared ``MADDPGPolicy`` (algorithm/MADDPGPolicy.py:63-151) over mm_maddpg_* (include/minimarl.h,
csrc/maddpg.hip) for discrete actions and one policy (``policy_0``). Everything runs on the GPU; there is no CPU path.

Two flat parameter / Adam sets. The actor is the MLP agent net of ``MOffQMix`` in the 18-tensor trunk layout; the
critic is the same layout over ``[cent_obs | cent_act]`` (width N (D + A)) with its 1 (maddpg) or 2 (matd3) heads in
the 4-row ``Wo`` / ``bo`` slot at the end of the vector. Reference behaviour kept on purpose:
* the critic heads are a plain Python list in the reference (actor_critic.py:67): never trained, not in the gradient
  norm, not in a state dict, not touched by target updates; the target critic keeps its own independently initialised
  heads. Here their gradient is exactly zero, Adam and the target updates stop in front of the slot, and
  ``load_reference_state`` takes both head lists as explicit arguments;
* ``num_updates`` is never incremented in maddpg.py, so the actor is updated on every call and matd3's
  ``actor_update_interval = 2`` is dead. ``count_updates=False`` (default) reproduces that; with ``count_updates=True``
  the counter advances and a skipped actor update leaves the actor keys out of ``train_info``;
* matd3's target actions are ``gumbel_softmax(hard=True)`` of the target logits; its value ``(y_hard - y) + y``
  differs from a one-hot by at most an ulp, the kernel uses the exact one-hot.
Gumbel noise: ``g = -log(-log(U + 1e-20) + 1e-20)`` (f32; each log evaluated in f64 and rounded) with
``U = rng_uniform(rng_draw(seed ^ salt, counter, b, n A + a))`` of the project's counter RNG, or injected through
``train_policy_on_batch(..., gumbel=, target_gumbel=)``.

Not built, raise ``ValueError`` before any allocation: use_popart, use_same_share_obs=False, available-action masks,
multidiscrete or continuous actions, layer_N != 1, weight_decay, use_value_active_masks, more than one policy,
H != 64, A != 5, D not in {3, 47, 94}, critic width N (D + A) > 416.
"""
import ctypes

import numpy as np
import torch

from ._lib import MaddpgBatch, MaddpgDims, c_i64, check, lib
from .offq import AGENT_KEYS
from .qnet import ptr, stream_handle

MAX_CRITIC_WIDTH = 416          # MM_MADDPG_MAX_CRITIC_WIDTH (include/minimarl.h)
GUMBEL_SALT, TARGET_GUMBEL_SALT, ACT_GUMBEL_SALT = 0x67756D62656C0001, 0x67756D62656C0002, 0x67756D62656C0003
COLLECT_GUMBEL_SALT = 0x67756D62656C0004       # the device collector's exploration noise (minimarl.maddpg_runner)
TRUNK_REF = {
    "ln0_w": "mlp.feature_norm.weight", "ln0_b": "mlp.feature_norm.bias",
    "W1": "mlp.mlp.fc1.0.weight", "b1": "mlp.mlp.fc1.0.bias",
    "ln1_w": "mlp.mlp.fc1.2.weight", "ln1_b": "mlp.mlp.fc1.2.bias",
    "W2": "mlp.mlp.fc2.0.0.weight", "b2": "mlp.mlp.fc2.0.0.bias",
    "ln2_w": "mlp.mlp.fc2.0.2.weight", "ln2_b": "mlp.mlp.fc2.0.2.bias",
}
ACTOR_REF = dict(TRUNK_REF, Wo="act.action_out.weight", bo="act.action_out.bias")


class _Trunk:
    """Views into a flat vector in the trunk layout (MGeo): input width ``din``, ``nout`` rows in the Wo / bo slot."""

    def __init__(self, din, nout, H=64):
        self.din, self.nout, self.H = din, nout, H
        self.Dp, self.Op = (din + 3) // 4 * 4, (nout + 3) // 4 * 4
        Dp, Op = self.Dp, self.Op
        sz = [Dp, Dp, H * Dp, H, H, H, H * H, H, H, H, 3 * H * H, 3 * H * H, 3 * H, 3 * H, H, H, Op * H, Op]
        self.offs = [int(x) for x in np.concatenate([[0], np.cumsum(sz)])]
        self.total, self.heads = self.offs[-1], self.offs[AGENT_KEYS.index("Wo")]

    def shape(self, key):
        D, H, O = self.din, self.H, self.nout
        return {"ln0_w": (D,), "ln0_b": (D,), "W1": (H, D), "b1": (H,), "ln1_w": (H,), "ln1_b": (H,), "W2": (H, H),
                "b2": (H,), "ln2_w": (H,), "ln2_b": (H,), "Wih": (3 * H, H), "Whh": (3 * H, H), "bih": (3 * H,),
                "bhh": (3 * H,), "lnr_w": (H,), "lnr_b": (H,), "Wo": (O, H), "bo": (O,)}[key]

    def view(self, t, key):
        o = self.offs[AGENT_KEYS.index(key)]
        if key == "W1":
            return t[o:o + self.H * self.Dp].view(self.H, self.Dp)[:, :self.din]
        if key == "Wo":
            return t[o:o + self.Op * self.H].view(self.Op, self.H)[:self.nout]
        shp = self.shape(key)
        return t[o:o + int(np.prod(shp))].view(shp)


class MADDPG:
    """MADDPG / MATD3 (``td3=True``) trainer + shared feed-forward policy (one policy, ``policy_0``)."""

    def __init__(self, n_agents, obs_dim, n_actions, td3=False, hidden=64, gamma=0.99, lr=5e-4, opti_eps=1e-5,
                 max_grad_norm=10.0, use_per=True, use_huber_loss=False, huber_delta=10.0, per_eps=1e-6, tau=0.005,
                 actor_update_interval=None, count_updates=False, device="cuda", seed=None, noise_seed=0,
                 grad_allreduce=None, use_popart=False, use_same_share_obs=True, weight_decay=0.0, layer_N=1,
                 use_value_active_masks=False, multidiscrete=False, continuous=False, n_policies=1):
        for name, bad in (("use_popart", use_popart), ("use_same_share_obs=False", not use_same_share_obs),
                          ("weight_decay", weight_decay != 0), ("layer_N != 1", layer_N != 1),
                          ("use_value_active_masks", use_value_active_masks),
                          ("multidiscrete actions", multidiscrete), ("continuous actions", continuous),
                          ("more than one policy", n_policies != 1)):
            if bad:
                raise ValueError(f"MADDPG: {name} is not built")
        N, D, A, H = int(n_agents), int(obs_dim), int(n_actions), int(hidden)
        if H != 64 or A != 5 or D not in (3, 47, 94) or N < 1:
            raise ValueError(f"MADDPG: unsupported dims N={N} D={D} H={H} A={A} (supported: N >= 1, D 3|47|94, H 64, A 5)")
        if N * (D + A) > MAX_CRITIC_WIDTH:
            raise ValueError(f"MADDPG: critic input width N (D + A) = {N * (D + A)} is above the limit of "
                             f"{MAX_CRITIC_WIDTH}")
        self.N, self.D, self.A, self.H, self.td3 = N, D, A, H, bool(td3)
        self.S, self.Dc, self.nq = N * D, N * (D + A), 2 if td3 else 1
        self.gamma, self.lr, self.eps, self.max_norm = gamma, lr, opti_eps, max_grad_norm
        self.use_per, self.huber, self.delta, self.per_eps, self.tau = use_per, use_huber_loss, huber_delta, per_eps, tau
        self.actor_update_interval = int(actor_update_interval or (2 if td3 else 1))
        self.count_updates, self.num_updates, self.calls, self.act_calls = bool(count_updates), 0, 0, 0
        self.noise_seed = int(noise_seed) & 0xFFFFFFFFFFFFFFFF
        self.allreduce = grad_allreduce
        self.device = torch.device(device)
        self.dims = MaddpgDims(N, D, H, A, int(self.td3))
        na, nc, nh = c_i64(), c_i64(), c_i64()
        check(lib().mm_maddpg_param_counts(ctypes.byref(self.dims), ctypes.byref(na), ctypes.byref(nc),
                                           ctypes.byref(nh)), "maddpg_param_counts")
        self.actor, self.critic = _Trunk(D, A), _Trunk(self.Dc, self.nq)
        assert (self.actor.total, self.critic.total, self.critic.heads) == (na.value, nc.value, nh.value)
        dev = self.device
        for s, n in (("a", self.actor.total), ("c", self.critic.total)):
            for name in ("P", "PT", "grad", "m", "v"):
                setattr(self, name + s, torch.zeros(n, device=dev))
            setattr(self, "step" + s, torch.zeros(1, device=dev))
            setattr(self, "norm" + s, torch.zeros(1, device=dev))
            setattr(self, "stats" + s, torch.zeros(2, device=dev))
        self.partials = torch.zeros(512, device=dev)
        self._ws = {}
        if seed is not None:
            self.init_default(seed)

    # -- parameters --------------------------------------------------------------------------
    def actor_view(self, key, target=False):
        return self.actor.view(self.PTa if target else self.Pa, key)

    def critic_view(self, key, target=False):
        return self.critic.view(self.PTc if target else self.Pc, key)

    def init_default(self, seed):
        """The reference init: orthogonal weights (gain sqrt(2) in the ReLU MLPs, ``gain`` = 0.01 for the action
        head, 1 for the Q heads), zero biases, unit LayerNorms; targets = copies, except the target critic's heads,
        which are drawn on their own."""
        g = torch.Generator().manual_seed(int(seed))
        for tr, P in ((self.actor, self.Pa), (self.critic, self.Pc)):
            P.zero_()
            for key in TRUNK_REF:
                if key.endswith("_w"):
                    tr.view(P, key).fill_(1.0)
                elif key in ("W1", "W2"):
                    w = torch.empty(tr.shape(key))
                    torch.nn.init.orthogonal_(w, gain=float(np.sqrt(2.0)), generator=g)
                    tr.view(P, key).copy_(w)
        w = torch.empty(self.A, self.H)
        torch.nn.init.orthogonal_(w, gain=0.01, generator=g)
        self.actor_view("Wo").copy_(w)
        self.PTa.copy_(self.Pa)
        self.PTc.copy_(self.Pc)
        for target in (False, True):
            for h in range(self.nq):
                w = torch.empty(1, self.H)
                torch.nn.init.orthogonal_(w, generator=g)
                self.critic_view("Wo", target)[h].copy_(w[0])

    def load_reference_state(self, actor_sd, critic_sd, q_outs, target_actor_sd=None, target_critic_sd=None,
                             target_q_outs=None):
        """actor_sd / critic_sd: MADDPG_Actor / MADDPG_Critic ``state_dict()``; q_outs: the critic's ``q_outs`` list
        as (weight [1, H], bias [1]) pairs, which no state dict holds. Targets default to copies."""
        f32 = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.float32)
        for target, asd, csd, qo in ((False, actor_sd, critic_sd, q_outs),
                                     (True, target_actor_sd or actor_sd, target_critic_sd or critic_sd,
                                      target_q_outs or q_outs)):
            if len(qo) != self.nq:
                raise ValueError(f"MADDPG: {len(qo)} critic heads given, {self.nq} expected")
            for k, name in ACTOR_REF.items():
                self.actor_view(k, target).copy_(f32(asd[name]))
            for k, name in TRUNK_REF.items():
                self.critic_view(k, target).copy_(f32(csd[name]))
            for h, (w, b) in enumerate(qo):
                self.critic_view("Wo", target)[h].copy_(f32(w).reshape(self.H))
                self.critic_view("bo", target)[h] = float(np.asarray(b).reshape(()))

    def state_dict(self, target=False):
        """(actor state dict, critic state dict, q_outs [(weight [1, H], bias [1])]) under the reference's names."""
        cpu = lambda t: t.detach().cpu().clone()
        a = {name: cpu(self.actor_view(k, target)) for k, name in ACTOR_REF.items()}
        c = {name: cpu(self.critic_view(k, target)) for k, name in TRUNK_REF.items()}
        q = [(cpu(self.critic_view("Wo", target)[h:h + 1]), cpu(self.critic_view("bo", target)[h:h + 1]))
             for h in range(self.nq)]
        return a, c, q

    def hard_target_updates(self):
        """MADDPGPolicy.hard_target_updates: parameters() only, so the critic heads stay."""
        self.PTa.copy_(self.Pa)
        self.PTc[:self.critic.heads].copy_(self.Pc[:self.critic.heads])

    def soft_target_updates(self):
        L, st = lib(), stream_handle(self.device)
        check(L.mm_offq_soft_update(ptr(self.PTa), ptr(self.Pa), self.actor.total, float(self.tau), st), "soft_update")
        check(L.mm_offq_soft_update(ptr(self.PTc), ptr(self.Pc), self.critic.heads, float(self.tau), st), "soft_update")

    def checkpoint_tensors(self):
        ts = {k + s: getattr(self, k + s) for s in "ac" for k in ("P", "PT", "m", "v", "step")}
        return ts, {"td3": int(self.td3), "num_updates": self.num_updates, "calls": self.calls,
                    "act_calls": self.act_calls}

    def restore_tensors(self, ts, scalars):
        from .checkpoint import copy_into
        if int(scalars.get("td3", int(self.td3))) != int(self.td3):
            raise ValueError("MADDPG checkpoint: td3 differs")
        for s in "ac":
            for k in ("P", "PT", "m", "v", "step"):
                copy_into(getattr(self, k + s), ts[k + s], k + s)
        self.num_updates, self.calls = int(scalars.get("num_updates", 0)), int(scalars.get("calls", 0))
        self.act_calls = int(scalars.get("act_calls", 0))

    # -- training ----------------------------------------------------------------------------
    def _dev(self, x):
        t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
        return t.to(device=self.device, dtype=torch.float32).contiguous()

    def _noise(self, given, buf, salt):
        if given is not None:
            g = self._dev(given)
            assert g.numel() == buf.numel(), (g.shape, buf.shape)
            return g
        check(lib().mm_maddpg_gumbel(ctypes.byref(self.dims), ptr(buf), int(buf.shape[1]), self.noise_seed ^ salt,
                                     self.calls, stream_handle(self.device)), "maddpg_gumbel")
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
        """MADDPG.shared_train_policy_on_batch. batch = the MlpReplayBuffer.sample tuple (obs, cent_obs, acts,
        rewards, nobs, cent_nobs, dones, dones_env, valid_transition, avail_act, navail_act, importance_weights,
        idxes), arrays bare or {policy_id: array}. gumbel / target_gumbel [N, B, A]: injected Gumbel(0, 1) noise of
        the actor pass / of matd3's target actions. Returns (train_info {critic_loss, critic_grad_norm, actor_loss,
        actor_grad_norm, update_actor} as device scalars, new priorities [B] or None, idxes); no sync."""
        obs, cent, acts, rew, nobs, ncent, _dones, dones_env, valid, avail, navail, isw, idxes = batch
        pick = (lambda d: d["policy_0"] if isinstance(d, dict) else d)
        if pick(avail) is not None or pick(navail) is not None:
            raise ValueError("MADDPG: available-action masks are not built")
        o, no = self._dev(pick(obs)), self._dev(pick(nobs))
        B = int(o.shape[1])
        assert tuple(o.shape) == (self.N, B, self.D) and tuple(no.shape) == (self.N, B, self.D), (o.shape, no.shape)
        a, r, de, va = (self._dev(pick(x)) for x in (acts, rew, dones_env, valid))
        s, ns = self._dev(pick(cent)), self._dev(pick(ncent))
        assert a.numel() == self.N * B * self.A and r.numel() == self.N * B and de.numel() == B
        assert va.numel() == self.N * B and tuple(s.shape) == (B, self.S) and tuple(ns.shape) == (B, self.S)
        w = self._dev(isw) if (self.use_per and isw is not None) else None
        L, st = lib(), stream_handle(self.device)
        if B not in self._ws:
            nbytes = int(L.mm_maddpg_workspace_bytes(ctypes.byref(self.dims), B))
            check(0 if nbytes > 0 else -22, "maddpg_workspace_bytes")
            self._ws[B] = (torch.empty((nbytes + 3) // 4, device=self.device), nbytes,
                           torch.zeros(B, device=self.device), torch.zeros(self.N, B, self.A, device=self.device),
                           torch.zeros(self.N, B, self.A, device=self.device))
        ws, nbytes, prio, gbuf, tgbuf = self._ws[B]
        update_actor = self.num_updates % self.actor_update_interval == 0
        g = self._noise(gumbel, gbuf, GUMBEL_SALT) if update_actor else None
        tg = self._noise(target_gumbel, tgbuf, TARGET_GUMBEL_SALT) if self.td3 else None
        self._keep = (o, no, a, r, de, va, s, ns, w, g, tg)         # alive until the kernels ran
        bt = MaddpgBatch()
        bt.obs, bt.nobs, bt.cent_obs, bt.cent_nobs = ptr(o), ptr(no), ptr(s), ptr(ns)
        bt.acts, bt.rewards, bt.dones_env, bt.valid, bt.is_weight = ptr(a), ptr(r), ptr(de), ptr(va), ptr(w)
        bt.gumbel, bt.target_gumbel = ptr(g), ptr(tg)
        bt.B, bt.huber, bt.gamma, bt.huber_delta, bt.per_eps = B, int(self.huber), self.gamma, self.delta, self.per_eps
        d = ctypes.byref(self.dims)
        check(L.mm_maddpg_critic_grad(d, ctypes.byref(bt), ptr(self.PTa), ptr(self.Pc), ptr(self.PTc), ptr(self.gradc),
                                      ptr(ws), nbytes, ptr(self.statsc), ptr(prio), st), "maddpg_critic_grad")
        self._clip_adam("c", self.critic.heads)
        info = {"critic_loss": self.statsc[0], "critic_grad_norm": self.normc[0]}
        if update_actor:
            check(L.mm_maddpg_actor_grad(d, ctypes.byref(bt), ptr(self.Pa), ptr(self.Pc), ptr(self.grada), ptr(ws),
                                         nbytes, ptr(self.statsa), st), "maddpg_actor_grad")
            self._clip_adam("a", self.actor.total)
            info.update(actor_loss=self.statsa[0], actor_grad_norm=self.norma[0], update_actor=True)
        self.calls += 1
        if self.count_updates:
            self.num_updates += 1
        return info, (prio if w is not None else None), idxes

    # -- acting ------------------------------------------------------------------------------
    def get_logits(self, obs, use_target=False, gumbel=None):
        """Actor logits [R, A] and the action one-hot [R, A]: argmax of logits + gumbel, or logits == rowmax."""
        x = self._dev(obs).reshape(-1, self.D)
        R = int(x.shape[0])
        g = None if gumbel is None else self._dev(gumbel).reshape(R, self.A)
        logits, hot = torch.empty(R, self.A, device=self.device), torch.empty(R, self.A, device=self.device)
        check(lib().mm_maddpg_logits(ctypes.byref(self.dims), ptr(self.PTa if use_target else self.Pa), ptr(x), ptr(g),
                                     ptr(logits), ptr(hot), R, stream_handle(self.device)), "maddpg_logits")
        return logits, hot

    def get_actions(self, obs, explore=False, use_target=False, use_gumbel=False, gumbel=None, eps=0.0):
        """MADDPGPolicy.get_actions (discrete branch, :93-106): one-hot actions [R, A] and eps. ``use_gumbel`` (or
        ``use_target`` with matd3, or ``explore``) takes the argmax of logits + Gumbel noise: ``gumbel`` [R, A] if
        injected, else mm_maddpg_gumbel of the counter RNG (``noise_seed ^ ACT_GUMBEL_SALT``, one counter step per
        call, row r as b). ``explore`` replaces a row by a uniform random action with probability ``eps``, both drawn
        from a generator seeded by (noise_seed, the same counter): acting replays from ``noise_seed`` alone."""
        R = int(np.prod(tuple(obs.shape)[:-1]))
        noisy = use_gumbel or explore or (use_target and self.td3)
        if noisy and gumbel is None:
            gumbel = torch.empty(R, self.A, device=self.device)
            one = MaddpgDims(1, self.D, self.H, self.A, int(self.td3))
            check(lib().mm_maddpg_gumbel(ctypes.byref(one), ptr(gumbel), R, self.noise_seed ^ ACT_GUMBEL_SALT,
                                         self.act_calls, stream_handle(self.device)), "maddpg_gumbel")
        _, hot = self.get_logits(obs, use_target, gumbel if noisy else None)
        call, self.act_calls = self.act_calls, self.act_calls + int(noisy)
        if not explore:
            return hot, None
        gen = torch.Generator(device=self.device).manual_seed(((self.noise_seed ^ ACT_GUMBEL_SALT) + call) % 2 ** 63)
        take = (torch.rand(R, 1, device=self.device, generator=gen) < eps).float()
        return (1 - take) * hot + take * self.get_random_actions(obs, gen), eps

    def get_random_actions(self, obs, generator=None):
        R = int(np.prod(tuple(obs.shape)[:-1]))
        ra = torch.randint(0, self.A, (R,), device=self.device, generator=generator)
        return torch.nn.functional.one_hot(ra, self.A).float()


__all__ = ["MADDPG"]
