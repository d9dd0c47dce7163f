"""Feed-forward transition-batch QMix / VDN ("mqmix" / "mvdn" of the reference's ``offpolicy/`` fork) on the MI355X.

Mirrors ``M_QMix`` (offpolicy/algorithms/mqmix/mqmix.py:68-235: train_policy_on_batch, hard_target_updates,
soft_target_updates) with its shared ``M_QMixPolicy`` (algorithm/mQMixPolicy.py:35-113: get_q_values, greedy
get_actions) over mm_moffq_* (include/minimarl.h, csrc/moffq.hip). Everything runs on the GPU; there is no CPU path.

The flat [agent | mixer] parameter vector, the gradient, Adam and the target copy are exactly those of
``minimarl.offq.OffQMix`` (the agent net is the 18-tensor trunk layout; its six recurrent tensors are not read and
keep a zero gradient), so a checkpoint has the same tensor shapes.

Not built, raise ``ValueError``: use_popart, available-action masks, multidiscrete actions, layer_N != 1,
hypernet_layers = 1, use_conv1d, weight_decay.
"""
import ctypes

import numpy as np
import torch

from ._lib import MM_OFFQ_QMIX, MM_OFFQ_VDN, MoffqBatch, OffqDims, c_i64, check, lib
from .offq import MAX_MIXER_HIDDEN, MIXER_KEYS, OffQMix
from .qnet import ptr, stream_handle

RECURRENT_KEYS = ("Wih", "Whh", "bih", "bhh", "lnr_w", "lnr_b")
# AgentQFunction state_dict names of the MLP variant (mqmix/algorithm/agent_q_function.py: MLPBase + ACTLayer)
AGENT_REF = {
    "ln0_w": "mlp.feature_norm.weight", "ln0_b": "mlp.feature_norm.bias",
    "W1": "mlp.mlp.fc1.0.weight", "b1": "mlp.mlp.fc1.0.bias",
    "ln1_w": "mlp.mlp.fc1.2.weight", "ln1_b": "mlp.mlp.fc1.2.bias",
    "W2": "mlp.mlp.fc2.0.0.weight", "b2": "mlp.mlp.fc2.0.0.bias",
    "ln2_w": "mlp.mlp.fc2.0.2.weight", "ln2_b": "mlp.mlp.fc2.0.2.bias",
    "Wo": "q.action_out.weight", "bo": "q.action_out.bias",
}


class MOffQMix(OffQMix):
    """M_QMix / M_VDN trainer + shared feed-forward Q policy (one policy, ``policy_0``)."""

    def __init__(self, n_agents, obs_dim, n_actions, mixer="qmix", hidden=64, mixer_hidden=32, hyper_hidden=64,
                 state_dim=None, gamma=0.99, lr=5e-4, opti_eps=1e-5, max_grad_norm=10.0, use_double_q=True,
                 use_per=True, use_huber_loss=False, huber_delta=10.0, per_eps=1e-6, tau=0.005, device="cuda",
                 seed=None, grad_allreduce=None, use_popart=False, weight_decay=0.0, layer_N=1, hypernet_layers=2,
                 use_conv1d=False, multidiscrete=False):
        if mixer not in ("qmix", "vdn"):
            raise ValueError(f"MOffQMix: mixer {mixer!r} (qmix or vdn)")
        for name, bad in (("use_popart", use_popart), ("weight_decay", weight_decay != 0), ("layer_N != 1", layer_N != 1),
                          ("hypernet_layers != 2", hypernet_layers != 2), ("use_conv1d", use_conv1d),
                          ("multidiscrete actions", multidiscrete)):
            if bad:
                raise ValueError(f"MOffQMix: {name} is not built")
        if int(hidden) != 64 or int(n_actions) != 5 or int(obs_dim) not in (3, 47, 94) or int(n_agents) < 1:
            raise ValueError(f"MOffQMix: unsupported dims N={n_agents} D={obs_dim} H={hidden} A={n_actions} "
                             "(supported: N >= 1, D 3|47|94, H 64, A 5)")
        if mixer == "qmix" and int(mixer_hidden) > MAX_MIXER_HIDDEN:
            raise ValueError(f"MOffQMix: mixer_hidden {int(mixer_hidden)} is above the limit of {MAX_MIXER_HIDDEN}")
        if mixer == "qmix" and (int(n_agents) * int(mixer_hidden) > 4096 or int(mixer_hidden) < 1 or int(hyper_hidden) < 1):
            raise ValueError("MOffQMix: QMIX needs mixer_hidden, hyper_hidden >= 1 and N * mixer_hidden <= 4096")
        self.N, self.D, self.A, self.H = int(n_agents), int(obs_dim), int(n_actions), int(hidden)
        self.mixer_kind = mixer
        self.S = self.N * self.D if state_dim is None else int(state_dim)
        self.K, self.Hh = int(mixer_hidden), int(hyper_hidden)
        self.gamma, self.lr, self.eps, self.max_norm = gamma, lr, opti_eps, max_grad_norm
        self.double_q, self.use_per, self.huber, self.delta = use_double_q, use_per, use_huber_loss, huber_delta
        self.per_eps, self.tau = per_eps, tau
        self.allreduce = grad_allreduce
        self.device = torch.device(device)
        self.dims = OffqDims(self.N, self.D, self.H, self.A, MM_OFFQ_QMIX if mixer == "qmix" else MM_OFFQ_VDN,
                             self.S, self.K, self.Hh)
        L = lib()
        na, nm = c_i64(), c_i64()
        check(L.mm_offq_param_counts(ctypes.byref(self.dims), ctypes.byref(na), ctypes.byref(nm)), "offq_param_counts")
        self.n_agent, self.n_mixer = int(na.value), int(nm.value)
        self.total = self.n_agent + self.n_mixer
        mo = (c_i64 * 15)()
        check(L.mm_offq_mixer_offsets(ctypes.byref(self.dims), mo), "offq_mixer_offsets")
        self.moffs = list(mo)
        self.Dp, self.Ap = (self.D + 3) // 4 * 4, (self.A + 3) // 4 * 4
        H, Dp, Ap = self.H, self.Dp, self.Ap
        sz = [Dp, Dp, H * Dp, H, H, H, H * H, H, H, H, 3 * H * H, 3 * H * H, 3 * H, 3 * H, H, H, Ap * H, Ap]
        self.aoffs = list(np.concatenate([[0], np.cumsum(sz)]).astype(np.int64))
        assert self.aoffs[-1] == self.n_agent, (self.aoffs[-1], self.n_agent)
        dev = self.device
        for name in ("P", "PT", "grad", "m", "v"):
            setattr(self, name, torch.zeros(self.total, device=dev))
        self.step = torch.zeros(1, device=dev)
        self.partials = torch.zeros(512, device=dev)
        self.norm = torch.zeros(1, device=dev)
        self.stats = torch.zeros(2, device=dev)
        self._ws = {}
        if seed is not None:
            self.init_default(seed)
            self.hard_target_updates()

    def init_default(self, seed):
        """The reference init (OffQMix.init_default); the recurrent tensors, which this net does not have, stay 0."""
        super().init_default(seed)
        for k in RECURRENT_KEYS:
            self.agent_view(k).zero_()

    def load_reference_state(self, q_sd, m_sd=None, target_q_sd=None, target_m_sd=None):
        """q_sd: AgentQFunction.state_dict() of the MLP variant; m_sd: M_QMixer.state_dict(); targets default to copies."""
        for t, qs, ms in ((self.P, q_sd, m_sd), (self.PT, target_q_sd or q_sd, target_m_sd or m_sd)):
            for k, name in AGENT_REF.items():
                self.agent_view(k, t).copy_(torch.as_tensor(np.asarray(qs[name]), dtype=torch.float32))
            if self.mixer_kind == "qmix":
                for k in MIXER_KEYS:
                    self.mixer_view(k, t).copy_(torch.as_tensor(np.asarray(ms[k]), dtype=torch.float32))

    def state_dict(self, target=False):
        t = self.PT if target else self.P
        q = {name: self.agent_view(k, t).detach().cpu().clone() for k, name in AGENT_REF.items()}
        m = ({k: self.mixer_view(k, t).detach().cpu().clone() for k in MIXER_KEYS}
             if self.mixer_kind == "qmix" else {})
        return q, m

    # -- training ----------------------------------------------------------------------------
    def train_policy_on_batch(self, batch, use_same_share_obs=True):
        """M_QMix.train_policy_on_batch (mqmix.py:68-218). batch = the MlpReplayBuffer.sample tuple (obs, cent_obs,
        acts, rewards, nobs, cent_nobs, dones, dones_env, valid_transition, avail_act, navail_act,
        importance_weights, idxes); the arrays {policy_id: array} dicts or bare, numpy or device tensors. Returns
        (train_info {loss, grad_norm, Q_tot} as device scalars, new priorities [B] device tensor or None, idxes)."""
        obs, cent, acts, rew, nobs, ncent, _dones, dones_env, _valid, avail, navail, isw, idxes = batch
        pick = (lambda d: d["policy_0"] if isinstance(d, dict) else d)
        if pick(avail) is not None or pick(navail) is not None:
            raise ValueError("MOffQMix: available-action masks are not built")
        o, no = self._dev(pick(obs)), self._dev(pick(nobs))
        B = int(o.shape[1])
        assert tuple(o.shape) == (self.N, B, self.D) and tuple(no.shape) == (self.N, B, self.D), (o.shape, no.shape)
        a = self._dev(pick(acts))
        r = self._dev(pick(rew))
        de = self._dev(pick(dones_env))
        assert a.numel() == self.N * B * self.A and r.numel() == self.N * B and de.numel() == B
        s = ns = None
        if self.mixer_kind == "qmix":
            s, ns = self._dev(pick(cent)), self._dev(pick(ncent))
            if not use_same_share_obs:           # [N, B, S]: agent 0's (mqmix.py:78-84)
                s, ns = s[0].contiguous(), ns[0].contiguous()
            assert tuple(s.shape) == (B, self.S) and tuple(ns.shape) == (B, self.S), (s.shape, ns.shape)
        w = self._dev(isw) if (self.use_per and isw is not None) else None
        L, st = lib(), stream_handle(self.device)
        if B not in self._ws:
            nbytes = int(L.mm_moffq_workspace_bytes(ctypes.byref(self.dims), B))
            check(0 if nbytes > 0 else -22, "moffq_workspace_bytes")
            self._ws[B] = (torch.empty((nbytes + 3) // 4, device=self.device), nbytes,
                           torch.zeros(B, device=self.device))
        ws, nbytes, prio = self._ws[B]
        self._keep = (o, no, a, r, de, s, ns, w)         # alive until the kernels ran
        bt = MoffqBatch()
        bt.obs, bt.nobs, bt.cent_obs, bt.cent_nobs = ptr(o), ptr(no), ptr(s), ptr(ns)
        bt.acts, bt.rewards, bt.dones_env, bt.is_weight = ptr(a), ptr(r), ptr(de), ptr(w)
        bt.B, bt.double_q, bt.huber = B, int(self.double_q), int(self.huber)
        bt.gamma, bt.huber_delta, bt.per_eps = self.gamma, self.delta, self.per_eps
        check(L.mm_moffq_loss_grad(ctypes.byref(self.dims), ctypes.byref(bt), ptr(self.P), ptr(self.PT), ptr(self.grad),
                                   ptr(ws), nbytes, ptr(self.stats), ptr(prio), st), "moffq_loss_grad")
        scale = 1.0
        if self.allreduce is not None:
            scale = 1.0 / self.allreduce(self.grad)
        check(L.mm_clip_adam(ptr(self.P), ptr(self.grad), ptr(self.m), ptr(self.v), self.total, self.total,
                             self.max_norm, self.lr, 0.9, 0.999, self.eps, ptr(self.step), ptr(self.partials),
                             ptr(self.norm), scale, st), "clip_adam")
        info = {"loss": self.stats[0], "grad_norm": self.norm[0], "Q_tot": self.stats[1]}
        return info, (prio if w is not None else None), idxes

    # -- acting ------------------------------------------------------------------------------
    def init_hidden(self, num_agents, batch_size):
        raise NotImplementedError("MOffQMix: the feed-forward policy has no hidden state")

    def get_q_values(self, obs_batch, action_batch=None, target=False):
        """M_QMixPolicy.get_q_values: obs [R, D] -> q [R, A]; with action_batch (indices [R]) the gathered
        column [R, 1] (mQMixPolicy.py:35-59)."""
        x = self._dev(obs_batch).reshape(-1, self.D)
        R = int(x.shape[0])
        act = None
        if action_batch is not None:
            t = action_batch if torch.is_tensor(action_batch) else torch.as_tensor(np.asarray(action_batch))
            act = t.to(device=self.device, dtype=torch.int32).reshape(R).contiguous()
        q = torch.empty((R, 1) if act is not None else (R, self.A), device=self.device)
        check(lib().mm_moffq_q_values(ctypes.byref(self.dims), ptr(self.PT if target else self.P), ptr(x), ptr(act),
                                      ptr(q), R, stream_handle(self.device)), "moffq_q_values")
        return q

    def get_actions(self, obs_batch):
        """Greedy get_actions (explore=False, mQMixPolicy.py:99,109-111): one-hot actions [R, A], greedy Q [R, 1]."""
        gq, ga = self.get_q_values(obs_batch).max(-1)
        return torch.nn.functional.one_hot(ga, self.A).float(), gq.unsqueeze(-1)
