"""MAPPO (rmappo, shared policy) on the MI355X: policy, device rollout buffer, trainer, runner.

Mirrors the reference's MAPPO interface (mappo/algorithms/rmappo_policy.py R_MAPPOPolicy,
mappo/runner/shared/shared_buffer.py SharedReplayBuffer, mappo/algorithms/ramppo_network.py
R_MAPPO, mappo/runner/shared/magym_runner.py MAGYM_Runner) over the C ABI in
include/minimarl.h (csrc/mappo.hip). Everything runs on the GPU; there is no CPU path.

Deviations: E independent envs instead of one env stepped E times per timestep
(magym_runner.py:53-54); the rollout's Categorical sample uses the device counter RNG
(inverse CDF). PPO minibatches (train_batch_size = num_mini_batch, ramppo_network.py:245-271): with one
minibatch per epoch the chunks are processed in chunk order instead of a torch.randperm order (a
full-batch gradient: same value up to float summation order, pinned by
tests/test_mappo_oracle.py::test_ppo_train_golden[False]); with more, each epoch draws one permutation
of the chunks and takes num_mini_batch steps on its slices, the remainder chunks dropped, as the
reference's recurrent_generator does (shared_buffer.py:318-331) -- drawn by a device generator, since
torch's CPU randperm stream is not the device's (a recorded one replays through train(perms=...)).
Feed-forward nets (the reference's algorithm_name "mappo", main.py:62-65): MappoPolicy(recurrent=False); the buffer
then holds no hidden states, the minibatches are slices of a permutation of the T * EN buffer rows
(feed_forward_generator, shared_buffer.py:159-219) and the kernels are mm_mappo_ff_fwd / _ff_grad / _ff_insert.
Envs: Checkers (VecEnv, obs_dim 47 | 94) or Switch2 (SwitchVecEnv with local observations and the clock, obs_dim 3;
critic width 3, or 6 with cent_agents=2); MappoRunner steps either through env.step_into.
"""
import ctypes

import numpy as np
import torch

from ._lib import (MM_MAPPO_ROLLOUT, MM_MAPPO_TRAIN, MM_MAPPO_VALUES, MM_MLOSS_ENTROPY, MM_MLOSS_POLICY,
                   MM_MLOSS_RATIO, MM_MLOSS_VALUE, MappoBwdArgs, MappoDims, MappoFwdArgs, c_i64, check, lib)
from .qnet import ptr, stream_handle

KEYS = ["ln0_w", "ln0_b", "W1", "b1", "ln1_w", "ln1_b", "W2", "b2", "ln2_w", "ln2_b",
        "Wih", "Whh", "bih", "bhh", "lnr_w", "lnr_b", "Wo", "bo"]
# reference parameter names (mappo/algorithms/r_actor_critic.py, utils/algorithm_utils/*)
REF_NAMES = {
    "ln0_w": "base.feature_norm.weight", "ln0_b": "base.feature_norm.bias",
    "W1": "base.mlp.fc1.0.weight", "b1": "base.mlp.fc1.0.bias",
    "ln1_w": "base.mlp.fc1.2.weight", "ln1_b": "base.mlp.fc1.2.bias",
    "W2": "base.mlp.fc2.0.0.weight", "b2": "base.mlp.fc2.0.0.bias",
    "ln2_w": "base.mlp.fc2.0.2.weight", "ln2_b": "base.mlp.fc2.0.2.bias",
    "Wih": "rnn.rnn.weight_ih_l0", "Whh": "rnn.rnn.weight_hh_l0",
    "bih": "rnn.rnn.bias_ih_l0", "bhh": "rnn.rnn.bias_hh_l0",
    "lnr_w": "rnn.norm.weight", "lnr_b": "rnn.norm.bias",
}
RECURRENT_KEYS = ("Wih", "Whh", "bih", "bhh", "lnr_w", "lnr_b")   # the RNNLayer's tensors (rnn.py)
FF_KEYS = [k for k in KEYS if k not in RECURRENT_KEYS]
HEAD_NAMES = {0: ("act.action_out.linear.weight", "act.action_out.linear.bias"), 1: ("v_out.weight", "v_out.bias")}


def ref_name(key, net):
    if key in ("Wo", "bo"):
        return HEAD_NAMES[net][0 if key == "Wo" else 1]
    return REF_NAMES[key]


class MappoNet:
    """One net's parameters (net 0 = R_Actor, net 1 = R_Critic) in the kernel's flat layout.

    cent_agents n >= 2 (use_centralized_V): the critic's input is the env's share_obs, n obs rows wide; ``D`` is
    the net's own input width (the critic's n * obs_dim), ``dims`` keeps the per-agent obs_dim.

    recurrent=False (the reference's feed-forward nets, r_actor_critic.py:46,84,123,168,204): the same flat layout,
    whose six RNNLayer tensors stay zero and are neither read, initialised, loaded nor exported."""

    def __init__(self, net, obs_dim, n_actions=5, hidden=32, device="cuda", seed=None, cent_agents=None,
                 recurrent=True):
        self.net, self.A, self.H = int(net), int(n_actions), int(hidden)
        self.recurrent = bool(recurrent)
        self.keys = KEYS if self.recurrent else FF_KEYS
        self.cent_agents = int(cent_agents) if cent_agents and int(cent_agents) > 1 else None
        self.D = int(obs_dim) * (self.cent_agents if self.cent_agents and self.net == 1 else 1)
        self.O = self.A if self.net == 0 else 1
        self.device = torch.device(device)
        self.dims = MappoDims(int(obs_dim), self.H, self.A, self.cent_agents or 0)
        offs = (c_i64 * 19)()
        check(lib().mm_mappo_param_offsets(ctypes.byref(self.dims), self.net, offs), "mappo_param_offsets")
        self.offs = list(offs)
        self.total = self.offs[18]
        self.flat = torch.zeros(self.total, device=self.device)
        self.Dp, self.Op = (self.D + 3) // 4 * 4, (self.O + 3) // 4 * 4
        if seed is not None:
            self.init_default(seed)

    def shape(self, key):
        D, H, O = self.D, self.H, self.O
        return {"ln0_w": (D,), "ln0_b": (D,), "W1": (H, D), "b1": (H,), "ln1_w": (H,), "ln1_b": (H,),
                "W2": (H, H), "b2": (H,), "ln2_w": (H,), "ln2_b": (H,), "Wih": (3 * H, H), "Whh": (3 * H, H),
                "bih": (3 * H,), "bhh": (3 * H,), "lnr_w": (H,), "lnr_b": (H,), "Wo": (O, H), "bo": (O,)}[key]

    def view(self, key, t=None):
        """Logical view of one tensor inside ``t`` (default: the parameters); pads are excluded."""
        t = self.flat if t is None else t
        i = KEYS.index(key)
        o = self.offs[i]
        if key == "W1":
            return t[o:o + self.H * self.Dp].view(self.H, self.Dp)[:, :self.D]
        if key == "Wo":
            return t[o:o + self.Op * self.H].view(self.Op, self.H)[:self.O]
        n = int(np.prod(self.shape(key)))
        return t[o:o + n].view(self.shape(key))

    def init_default(self, seed):
        """The reference init (orthogonal weights, zero biases, unit LayerNorms; gain sqrt(2) for the
        ReLU MLP, 1 for the GRU and the value head, 0.01 for the policy head)."""
        g = torch.Generator().manual_seed(int(seed))
        self.flat.zero_()
        relu_gain = float(np.sqrt(2.0))
        for key in self.keys:
            shp = self.shape(key)
            if key.startswith("ln") and key.endswith("_w"):
                self.view(key).fill_(1.0)
            elif len(shp) == 2:
                w = torch.empty(shp)
                gain = relu_gain if key in ("W1", "W2") else (0.01 if (key == "Wo" and self.net == 0) else 1.0)
                torch.nn.init.orthogonal_(w, gain=gain, generator=g)
                self.view(key).copy_(w.to(self.device))

    def load_reference_state(self, sd, prefix=""):
        for k in self.keys:
            v = torch.as_tensor(np.asarray(sd[prefix + ref_name(k, self.net)]), dtype=torch.float32)
            self.view(k).copy_(v.to(self.device))

    def state_dict(self):
        return {ref_name(k, self.net): self.view(k).detach().cpu().clone() for k in self.keys}


def _ptrs(*ts):
    return [ptr(t) if t is not None else None for t in ts]


class MappoPolicy:
    """R_MAPPOPolicy (rmappo_policy.py:7-153): shared actor + critic for all agents."""

    def __init__(self, obs_dim, n_actions=5, hidden=32, device="cuda", seed=None, cent_agents=None, recurrent=True):
        """cent_agents = n (use_centralized_V, base_runner.py:70-85): the critic reads the env's share_obs, the
        concatenation of its n agents' obs rows (input width n * obs_dim); None: the row's own obs.

        recurrent=False: the reference's algorithm_name "mappo" (main.py:62-65), feed-forward nets without the
        RNNLayer (mm_mappo_ff_fwd). get_actions / get_values / rollout_args then take None for the hiddens and masks
        and hand back the hiddens they were given."""
        self.recurrent = bool(recurrent)
        self.actor = MappoNet(0, obs_dim, n_actions, hidden, device, None if seed is None else seed, cent_agents,
                              self.recurrent)
        self.critic = MappoNet(1, obs_dim, n_actions, hidden, device, None if seed is None else seed + 1,
                               cent_agents, self.recurrent)
        self.dims = self.actor.dims
        self.D, self.A, self.H = int(obs_dim), int(n_actions), int(hidden)
        self.cent_agents = self.actor.cent_agents
        self.Dc = self.critic.D
        self.device = self.actor.device

    def _critic_input(self, x):
        """(obs, cent_obs) pointers' tensors for the critic from either form of its input: [R, D] rows grouped by
        env (the n rows of an env adjacent: the critic gathers its share_obs from them) or explicit [R, n*D]."""
        x = x.contiguous()
        if self.cent_agents is None or x.shape[-1] == self.D:
            if x.shape[-1] != self.D:
                raise ValueError(f"critic input width {x.shape[-1]} != obs_dim {self.D}")
            return x, None
        if x.shape[-1] != self.Dc:
            raise ValueError(f"critic input width {x.shape[-1]}: expected {self.D} (rows grouped by env) or "
                             f"{self.Dc} (explicit cent_obs, {self.cent_agents} agents x {self.D})")
        return None, x

    def _fwd(self, args):
        if not self.recurrent:
            check(lib().mm_mappo_ff_fwd(ctypes.byref(self.dims), ctypes.byref(args), stream_handle(self.device)),
                  "mappo_ff_fwd")
            return
        check(lib().mm_mappo_fwd(ctypes.byref(self.dims), ctypes.byref(args), stream_handle(self.device)),
              "mappo_fwd")

    def rollout_args(self, obs, ha=None, hc=None, masks=None, ha_out=None, hc_out=None, logp_out=None,
                     value_out=None, act_out=None, act_in=None, u=None, seed=0, counter=0, counter_ptr=None,
                     cent_obs=None):
        a = MappoFwdArgs()
        a.cent_obs = None if cent_obs is None else ptr(cent_obs)
        a.net[0].P, a.net[0].h_in, a.net[0].h_out, a.net[0].out = _ptrs(self.actor.flat, ha, ha_out, logp_out)
        a.net[1].P, a.net[1].h_in, a.net[1].h_out, a.net[1].out = _ptrs(self.critic.flat, hc, hc_out, value_out)
        a.obs, a.mask, a.act_in, a.act_out, a.u = _ptrs(obs, masks, act_in, act_out, u)
        a.seed, a.counter, a.counter_ptr = int(seed), int(counter), counter_ptr
        a.rows = int(obs.shape[0])
        a.mode = MM_MAPPO_ROLLOUT
        return a

    def get_actions(self, obs, ha=None, hc=None, masks=None, actions=None, u=None, seed=0, counter=0, cent_obs=None):
        """obs [R,D], ha/hc [R,H], masks [R] -> values [R,1], actions [R,1], logp [R,1], ha', hc'.

        Centralized critic: cent_obs [R, n*D] is the reference's explicit critic input; None reads the share_obs
        from obs itself (rows grouped by env, R a multiple of n).

        The sample is drawn by the device RNG (or from injected uniforms u [R]); pass ``actions``
        to evaluate given actions (the reference's get_actions always samples, rmappo_policy.py:86)."""
        R = obs.shape[0]
        dev = self.device
        if self.recurrent:
            ha2, hc2 = torch.empty(R, self.H, device=dev), torch.empty(R, self.H, device=dev)
        lp, v = torch.empty(R, device=dev), torch.empty(R, device=dev)
        act_in = None if actions is None else actions.reshape(-1).to(torch.int32).contiguous()
        act = torch.empty(R, dtype=torch.int32, device=dev) if actions is None else act_in
        if cent_obs is not None:
            cent_obs = self._critic_input(cent_obs)[1]
        if not self.recurrent:   # (the nets read neither hiddens nor masks; the hiddens pass through)
            self._fwd(self.rollout_args(obs.contiguous(), None, None, None, None, None, lp, v,
                                        None if actions is not None else act, act_in, u, seed, counter,
                                        cent_obs=cent_obs))
            return v.view(R, 1), act.view(R, 1), lp.view(R, 1), ha, hc
        self._fwd(self.rollout_args(obs.contiguous(), ha.contiguous(), hc.contiguous(),
                                    None if masks is None else masks.reshape(-1).contiguous(), ha2, hc2, lp, v,
                                    None if actions is not None else act, act_in, u, seed, counter,
                                    cent_obs=cent_obs))
        return v.view(R, 1), act.view(R, 1), lp.view(R, 1), ha2, hc2

    def get_values(self, obs, hc=None, masks=None, hc_out=None):
        """obs: the critic's input, [R, D] (centralized: rows grouped by env) or an explicit cent_obs [R, n*D];
        hc_out [R, H] (optional) receives the critic's new hidden (a feed-forward policy reads and writes none)."""
        R = obs.shape[0]
        v = torch.empty(R, device=self.device)
        a = MappoFwdArgs()
        if not self.recurrent:
            hc = hc_out = masks = None
        a.net[1].P, a.net[1].h_in, a.net[1].out, a.net[1].h_out = _ptrs(self.critic.flat,
                                                                        None if hc is None else hc.contiguous(), v,
                                                                        hc_out)
        o, co = self._critic_input(obs)
        # (the kernel's obs pointer is required; with an explicit cent_obs the critic does not read it)
        a.obs, a.cent_obs, a.mask = _ptrs(co if o is None else o, co,
                                          None if masks is None else masks.reshape(-1).contiguous())
        a.rows, a.mode = R, MM_MAPPO_VALUES
        self._fwd(a)
        return v.view(R, 1)


def _rs(rows):
    return (rows + 63) // 64 * 64


class MappoBuffer:
    """SharedReplayBuffer (shared_buffer.py:15-129) in HBM: [T(+1), EN, ...] with EN = envs*agents."""

    def __init__(self, T, n_envs, n_agents, obs_dim, hidden=32, device="cuda", recurrent=True):
        """recurrent=False (a feed-forward policy): no rnn_states / rnn_states_critic arrays (both None)."""
        self.recurrent = bool(recurrent)
        self.T, self.E, self.N, self.D, self.H = int(T), int(n_envs), int(n_agents), int(obs_dim), int(hidden)
        self.EN = self.E * self.N
        dev = self.device = torch.device(device)
        T, EN = self.T, self.EN
        self.obs = torch.zeros(T + 1, EN, self.D, device=dev)
        self.rnn_states = torch.zeros(T + 1, EN, self.H, device=dev) if self.recurrent else None
        self.rnn_states_critic = torch.zeros(T + 1, EN, self.H, device=dev) if self.recurrent else None
        self.value_preds = torch.zeros(T + 1, EN, device=dev)
        self.returns = torch.zeros(T + 1, EN, device=dev)
        self.actions = torch.zeros(T, EN, dtype=torch.int32, device=dev)
        self.action_log_probs = torch.zeros(T, EN, device=dev)
        self.rewards = torch.zeros(T, EN, device=dev)
        self.masks = torch.ones(T + 1, EN, device=dev)
        self.active_masks = torch.ones(T + 1, EN, device=dev)

    def load_reference(self, data):
        """Fill from reference-shaped numpy arrays ([T(+1), E, N, ...], see make_golden_mappo.py)."""
        def put(dst, src, dtype=torch.float32):
            dst.copy_(torch.as_tensor(np.ascontiguousarray(src)).reshape(dst.shape).to(dtype))
        put(self.obs, data["obs"])
        if self.recurrent:
            put(self.rnn_states, data["rnn_states"])
            put(self.rnn_states_critic, data["rnn_states_critic"])
        put(self.value_preds, data["value_preds"])
        put(self.returns, data["returns"])
        put(self.actions, data["actions"], torch.int32)
        put(self.action_log_probs, data["action_log_probs"])
        put(self.rewards, data["rewards"])
        put(self.masks, data["masks"])
        put(self.active_masks, data["active_masks"])

    def after_update(self):
        """shared_buffer.py:119-129: last slot becomes the first."""
        for t in (self.obs, self.rnn_states, self.rnn_states_critic, self.masks, self.active_masks):
            if t is not None:
                t[0].copy_(t[-1])

    def compute_returns(self, vn, gamma=0.99, gae_lambda=0.95):
        """shared_buffer.py:131-153 with ValueNorm (value_preds[T] must hold the next value)."""
        check(lib().mm_mappo_gae(ptr(self.rewards), ptr(self.value_preds), ptr(self.masks), ptr(self.returns),
                                 ptr(vn), self.T, self.EN, float(gamma), float(gae_lambda),
                                 stream_handle(self.device)), "mappo_gae")


def chunks_ref_to_native(c, T, L, EN):
    """Chunk numbers of the reference's recurrent_generator (c = en * (T / L) + kc: the buffer cast to
    [E, N, T] and cut every L steps, shared_buffer.py:325-357) -> the buffer's native numbering kc * EN + en
    (include/minimarl.h mm_mappo_grad_mb). c: an integer numpy array or torch tensor."""
    K = int(T) // int(L)
    return (c % K) * int(EN) + c // K


def chunks_native_to_ref(c, T, L, EN):
    """The inverse of chunks_ref_to_native."""
    K = int(T) // int(L)
    return (c % int(EN)) * K + c // int(EN)


class MappoTrainer:
    """R_MAPPO (ramppo_network.py:9-287): train_batch_size = num_mini_batch, recurrent chunks of L steps."""

    def __init__(self, policy, T, EN, L=5, ppo_epoch=15, clip_param=0.2, huber_delta=10.0, entropy_coef=0.01,
                 value_loss_coef=0.5, max_grad_norm=0.5, actor_lr=1e-4, critic_lr=1e-4, opti_eps=1e-5,
                 grad_allreduce=None, fused=True, num_mini_batch=1, perm_seed=0):
        """fused: one mm_mappo_grad pass per epoch (forward recomputed in the backward, weight gradients
        reduced on MFMA in the same kernel); False: the TRAIN forward with saved activations, the BPTT
        kernel writing per-row operands and the separate weight-gradient reduction.

        num_mini_batch M (the reference's train_batch_size): 1 = one full-batch step per epoch in chunk order;
        M > 1 = per epoch one permutation of the T * EN / L chunks, M steps on its slices of
        (T * EN / L) // M chunks (mm_mappo_mb_stats + mm_mappo_vn_update + mm_mappo_grad_mb + mm_clip_adam each),
        the remainder dropped. perm_seed seeds the device generator of those permutations together with the
        number of train() calls so far and the epoch.

        A feed-forward policy (MappoPolicy(recurrent=False); feed_forward_generator, shared_buffer.py:159-219): L is
        ignored and the unit of permutation is the buffer row t * EN + en (the reference numbers rows the same way):
        n_chunks counts rows, a minibatch holds (T * EN) // M of them, perms is [epochs, T * EN]; one
        mm_mappo_ff_grad per update."""
        self.recurrent = bool(getattr(policy, "recurrent", True))
        if not self.recurrent:
            L = 1
            if not fused:
                raise NotImplementedError("fused=False with a feed-forward policy: only the fused gradient pass "
                                          "(mm_mappo_ff_grad) exists for it, the saves + wgrad path is recurrent")
            if int(num_mini_batch) > 1 and policy.cent_agents and policy.cent_agents >= 8:
                raise NotImplementedError(f"num_mini_batch={num_mini_batch} with a feed-forward policy and cent_agents="
                                          f"{policy.cent_agents}: mm_mappo_ff_grad refuses a row list for the "
                                          f"{policy.Dc}-wide critic; use num_mini_batch=1")
        assert T % L == 0, "episode length must be a multiple of data_chunk_length"
        self.fused = bool(fused)
        self.M, self.perm_seed, self.train_calls = int(num_mini_batch), int(perm_seed), 0
        self.n_chunks = int(T) * int(EN) // int(L)
        self.mbs = self.n_chunks // max(self.M, 1)
        if self.M < 1:
            raise ValueError(f"num_mini_batch={num_mini_batch} must be at least 1")
        if self.M > 1:
            if not self.fused:
                raise NotImplementedError(f"num_mini_batch={self.M} needs fused=True: only the fused gradient pass "
                                          "(mm_mappo_grad_mb) runs over a chunk list, the saves + wgrad path does not")
            if grad_allreduce is not None:
                raise NotImplementedError(f"num_mini_batch={self.M} with grad_allreduce: the per-minibatch statistics "
                                          "(active count, return moments) would need their own all-reduce")
            if self.mbs < 1:
                if not self.recurrent:
                    raise NotImplementedError(f"num_mini_batch={self.M} exceeds the {self.n_chunks} rows of the "
                                              f"buffer (T={T} x EN={EN}): a minibatch would hold no row")
                raise NotImplementedError(f"num_mini_batch={self.M} exceeds the {self.n_chunks} chunks of the buffer "
                                          f"(T={T} x EN={EN} / L={L}): a minibatch would hold no chunk")
        if not self.fused and policy.cent_agents:
            raise NotImplementedError(f"fused=False does not support a centralized critic (cent_agents="
                                      f"{policy.cent_agents}, critic input width {policy.Dc}): only the fused "
                                      "gradient pass (mm_mappo_grad) reads share_obs")
        if policy.cent_agents and int(EN) % policy.cent_agents:
            raise ValueError(f"EN={EN} is not a multiple of cent_agents={policy.cent_agents} (rows of an env must be "
                             "adjacent)")
        self.p = policy
        self.T, self.EN, self.L, self.epochs = int(T), int(EN), int(L), int(ppo_epoch)
        self.clip, self.huber, self.ent, self.vcoef = clip_param, huber_delta, entropy_coef, value_loss_coef
        self.max_norm, self.lrs, self.eps = max_grad_norm, (actor_lr, critic_lr), opti_eps
        self.allreduce = grad_allreduce
        dev = self.device = policy.device
        L_ = lib()
        d = ctypes.byref(policy.dims)
        self.rows = self.T * self.EN
        self.rs = _rs(self.rows)
        if not self.recurrent:
            n_scr = int(L_.mm_mappo_ff_grad_scratch_count(d))
            if n_scr <= 0:
                raise RuntimeError("mappo_ff_grad: unsupported dims for the feed-forward gradient pass")
            self.gscr = torch.zeros(n_scr, device=dev)
        elif self.fused:
            n_scr = int(L_.mm_mappo_grad_scratch_count(d, self.L, self.T, self.EN))
            if n_scr <= 0:
                raise RuntimeError("mappo_grad: unsupported dims for the fused gradient pass")
            self.gscr = torch.zeros(n_scr, device=dev)
        else:
            ns = [L_.mm_mappo_save_fields(d, n) for n in (0, 1)]
            ng = [L_.mm_mappo_grad_fields(d, n) for n in (0, 1)]
            self.save = [torch.zeros(self.rs * ns[n], device=dev) for n in (0, 1)]
            self.gsoa = [torch.zeros(self.rs * ng[n], device=dev) for n in (0, 1)]
            self.partial = torch.zeros(int(L_.mm_mappo_wgrad_partial_count(d, self.rs)), device=dev)
        nets = (policy.actor, policy.critic)
        self.grad = [torch.zeros_like(n.flat) for n in nets]
        self.m = [torch.zeros_like(n.flat) for n in nets]
        self.v = [torch.zeros_like(n.flat) for n in nets]
        self.step = [torch.zeros(1, device=dev) for _ in nets]
        self.norm_part = [torch.zeros(256, device=dev) for _ in nets]
        self.norms = torch.zeros(2, max(1, self.epochs * self.M), device=dev)
        self.perm_gen = torch.Generator(device=dev) if self.M > 1 else None
        self.vn = torch.zeros(3, device=dev)          # ValueNorm running mean, mean sq, debias (f32)
        self.stats = torch.zeros(8, device=dev)
        self.adv = torch.zeros(self.rows, device=dev)
        self.adv_part = torch.zeros(7 * 256 + 5, dtype=torch.float64, device=dev)
        self.loss_acc = torch.zeros(4, device=dev)

    # -- checkpoint (minimarl.checkpoint) ------------------------------------------------------
    def checkpoint_tensors(self):
        ts = {"actor": self.p.actor.flat, "critic": self.p.critic.flat, "vn": self.vn}
        for n in (0, 1):
            ts[f"m{n}"], ts[f"v{n}"], ts[f"step{n}"] = self.m[n], self.v[n], self.step[n]
        # (the number of train() calls seeds the minibatch permutations: a resumed run draws what the uninterrupted
        # run would have drawn)
        return ts, {"train_calls": self.train_calls, "recurrent": int(self.recurrent)}

    def restore_tensors(self, ts, scalars):
        from .checkpoint import copy_into
        saved = bool((scalars or {}).get("recurrent", 1))   # (absent in older files: recurrent)
        if saved != self.recurrent:
            name = {True: "recurrent (rmappo)", False: "feed-forward (mappo)"}
            raise ValueError(f"checkpoint of a {name[saved]} policy cannot be loaded into a {name[self.recurrent]} "
                             "trainer: the nets differ (RNNLayer present or not)")
        if tuple(ts["critic"].shape) != tuple(self.p.critic.flat.shape):
            # (centralized vs decentralized critic: name the widths, not the flat parameter counts)
            c, H = self.p.critic, self.p.H
            # total = (H + 2) * ceil4(Din) + the width-independent rest
            rest = c.total - (H + 2) * c.Dp
            dp, rem = divmod(int(ts["critic"].numel()) - rest, H + 2)
            if rem or dp <= 0 or ts["critic"].dim() != 1:   # not an input-width difference: the plain shape error
                copy_into(self.p.critic.flat, ts["critic"], "critic")
            raise ValueError(f"checkpoint critic input width {dp} (padded to 4) != this trainer's critic input width "
                             f"{c.D} (obs_dim {self.p.D}, cent_agents {self.p.cent_agents}): a decentralized and a "
                             "centralized critic (use_centralized_V) are not interchangeable")
        copy_into(self.p.actor.flat, ts["actor"], "actor")
        copy_into(self.p.critic.flat, ts["critic"], "critic")
        copy_into(self.vn, ts["vn"], "vn")
        for n in (0, 1):
            copy_into(self.m[n], ts[f"m{n}"], f"m{n}")
            copy_into(self.v[n], ts[f"v{n}"], f"v{n}")
            copy_into(self.step[n], ts[f"step{n}"], f"step{n}")
        self.train_calls = int((scalars or {}).get("train_calls", 0))   # (absent in older files)

    # -- ValueNorm (utils/valuenorm.py) ------------------------------------------------------
    def value_normalizer_state(self):
        v = self.vn.detach().cpu().numpy()
        return {"running_mean": v[0:1], "running_mean_sq": v[1:2], "debiasing_term": np.float32(v[2])}

    def load_value_normalizer(self, mean, mean_sq, debias):
        self.vn.copy_(torch.tensor([mean, mean_sq, debias], dtype=torch.float32))

    def denormalize(self, x):
        v = self.vn.detach().cpu().double()
        d = max(float(v[2]), 1e-5)
        mean, msq = float(np.float32(v[0] / d)), float(np.float32(v[1] / d))
        var = max(msq - mean * mean, 1e-2)
        return x * float(np.sqrt(var)) + mean

    # -- one train() ------------------------------------------------------------------------
    def fwd_args(self, buf):
        if self.fused:
            return None
        a = MappoFwdArgs()
        a.net[0].P, a.net[0].h_in, a.net[0].save = _ptrs(self.p.actor.flat, buf.rnn_states, self.save[0])
        a.net[1].P, a.net[1].h_in, a.net[1].save = _ptrs(self.p.critic.flat, buf.rnn_states_critic, self.save[1])
        a.obs, a.mask = _ptrs(buf.obs, buf.masks)
        a.en, a.T, a.L, a.rs, a.mode = self.EN, self.T, self.L, self.rs, MM_MAPPO_TRAIN
        return a

    def bwd_args(self, buf):
        b = MappoBwdArgs()
        b.P[0], b.P[1] = ptr(self.p.actor.flat), ptr(self.p.critic.flat)
        if not self.fused:
            b.save[0], b.save[1] = ptr(self.save[0]), ptr(self.save[1])
            b.gsoa[0], b.gsoa[1] = ptr(self.gsoa[0]), ptr(self.gsoa[1])
        (b.obs, b.mask, b.active, b.act, b.adv, b.old_logp, b.old_value, b.returns, b.stats,
         b.loss_acc) = _ptrs(buf.obs, buf.masks, buf.active_masks, buf.actions, self.adv, buf.action_log_probs,
                             buf.value_preds, buf.returns, self.stats, self.loss_acc)
        b.clip, b.huber_delta, b.entropy_coef, b.value_coef = self.clip, self.huber, self.ent, self.vcoef
        b.en, b.T, b.L, b.rs = self.EN, self.T, self.L, self.rs
        return b

    def prepare(self, buf):
        """Advantages (returns - denorm(V)), their masked mean/std and the return moments. Data
        parallel: the raw sums are all-reduced so every replica normalises with the global
        statistics and applies the same ValueNorm updates."""
        s = stream_handle(self.device)
        check(lib().mm_mappo_adv_stats(ptr(buf.returns), ptr(buf.value_preds), ptr(buf.active_masks), ptr(self.vn),
                                       ptr(self.adv), self.rows, ptr(self.adv_part), ptr(self.stats), s),
              "mappo_adv_stats")
        if self.allreduce is not None:
            sums = self.adv_part[7 * 256:7 * 256 + 5]
            world = self.allreduce(sums)
            check(lib().mm_mappo_stats_from_sums(ptr(sums), self.rows * world, ptr(self.stats), s),
                  "mappo_stats_from_sums")
        self.loss_acc.zero_()

    def gradients(self, buf, fa=None, ba=None):
        """This epoch's unclipped gradients of both nets into self.grad (loss seeds + chunked BPTT +
        weight-gradient reduction, ramppo_network.py:56-209)."""
        L_, s, d = lib(), stream_handle(self.device), ctypes.byref(self.p.dims)
        ba = ba or self.bwd_args(buf)
        if not self.recurrent:
            check(L_.mm_mappo_ff_grad(d, ctypes.byref(ba), None, 0, ptr(self.grad[0]), ptr(self.grad[1]),
                                      ptr(self.gscr), s), "mappo_ff_grad")
            return
        if self.fused:
            check(L_.mm_mappo_grad(d, ctypes.byref(ba), ptr(buf.rnn_states), ptr(buf.rnn_states_critic),
                                   ptr(self.grad[0]), ptr(self.grad[1]), ptr(self.gscr), s), "mappo_grad")
            return
        fa = fa or self.fwd_args(buf)
        check(L_.mm_mappo_fwd(d, ctypes.byref(fa), s), "mappo_fwd(train)")
        check(L_.mm_mappo_bwd(d, ctypes.byref(ba), s), "mappo_bwd")
        for n in (0, 1):
            check(L_.mm_mappo_wgrad(d, n, ptr(self.gsoa[n]), self.rs, ptr(self.grad[n]), ptr(self.partial), s),
                  "mappo_wgrad")

    def epoch(self, buf, ep, fa=None, ba=None):
        L_, s, d = lib(), stream_handle(self.device), ctypes.byref(self.p.dims)
        check(L_.mm_mappo_vn_update(ptr(self.vn), ptr(self.stats), 0.99999, s), "mappo_vn_update")
        self.gradients(buf, fa, ba)
        # data parallel: the loss seeds already divide by the GLOBAL active count (stats from the
        # all-reduced sums in prepare()), so the SUM over replicas is the global-batch gradient: no
        # further 1/world
        scale = 1.0
        if self.allreduce is not None:
            for n in (0, 1):
                self.allreduce(self.grad[n])
        self.clip_adam(ep % self.norms.shape[1], scale)

    def clip_adam(self, slot, scale=1.0):
        """clip_grad_norm_ + Adam of both nets on self.grad; the pre-clip norms go to self.norms[:, slot]."""
        L_, s = lib(), stream_handle(self.device)
        nets = (self.p.actor, self.p.critic)
        for n in (0, 1):
            check(L_.mm_clip_adam(ptr(nets[n].flat), ptr(self.grad[n]), ptr(self.m[n]), ptr(self.v[n]),
                                  nets[n].total, nets[n].total, self.max_norm, self.lrs[n], 0.9, 0.999, self.eps,
                                  ptr(self.step[n]), ptr(self.norm_part[n]), ptr(self.norms[n, slot]),
                                  scale, s), "clip_adam")

    # -- minibatches (num_mini_batch > 1) ------------------------------------------------------
    def draw_perms(self, call=None):
        """The permutations train() call number ``call`` (default: the next one) uses, [epochs, n_chunks] int64 on
        the device in the reference's chunk numbering: one torch.randperm per epoch from the device generator
        seeded by (perm_seed, call, epoch)."""
        call = self.train_calls if call is None else int(call)
        rows = []
        for ep in range(self.epochs):
            self.perm_gen.manual_seed(((self.perm_seed * 1000003 + call) * 1000003 + ep) & (2 ** 63 - 1))
            rows.append(torch.randperm(self.n_chunks, generator=self.perm_gen, device=self.device))
        return torch.stack(rows) if rows else torch.zeros(0, self.n_chunks, dtype=torch.int64, device=self.device)

    def native_chunks(self, perms):
        """Injected permutations ([epochs, n_chunks], the reference's numbering: a recorded torch.randperm), checked
        on the host -> the device int32 chunk lists in the native numbering."""
        pm = np.asarray(perms.detach().cpu() if torch.is_tensor(perms) else perms)
        if pm.shape != (self.epochs, self.n_chunks) or pm.dtype.kind not in "iu":
            raise ValueError(f"perms: expected integers of shape [epochs={self.epochs}, n_chunks={self.n_chunks}], "
                             f"got {pm.dtype} {tuple(pm.shape)}")
        want = np.arange(self.n_chunks)
        for ep in range(self.epochs):
            if not np.array_equal(np.sort(pm[ep].astype(np.int64)), want):
                raise ValueError(f"perms[{ep}] is not a permutation of the {self.n_chunks} "
                                 f"{'chunks' if self.recurrent else 'rows'}")
        return self._to_native(torch.as_tensor(pm.astype(np.int64), device=self.device))

    def _to_native(self, perms):
        if not self.recurrent:   # (rows: the reference's numbering is the buffer's)
            return perms.to(torch.int32).contiguous()
        return chunks_ref_to_native(perms, self.T, self.L, self.EN).to(torch.int32).contiguous()

    def mb_stats(self, buf, chunks):
        """The minibatch's active count and return moments into self.stats (chunks: device int32, native)."""
        check(lib().mm_mappo_mb_stats(ptr(buf.returns), ptr(buf.active_masks), ptr(chunks), int(chunks.numel()),
                                      self.L, self.T, self.EN, ptr(self.adv_part), ptr(self.stats),
                                      stream_handle(self.device)), "mappo_mb_stats")

    def gradients_mb(self, buf, chunks, ba=None):
        """gradients() over the chunks of one minibatch (device int32, native numbering)."""
        ba = ba or self.bwd_args(buf)
        if not self.recurrent:   # (chunks: the minibatch's buffer rows)
            check(lib().mm_mappo_ff_grad(ctypes.byref(self.p.dims), ctypes.byref(ba), ptr(chunks), int(chunks.numel()),
                                         ptr(self.grad[0]), ptr(self.grad[1]), ptr(self.gscr),
                                         stream_handle(self.device)), "mappo_ff_grad")
            return
        check(lib().mm_mappo_grad_mb(ctypes.byref(self.p.dims), ctypes.byref(ba), ptr(chunks), int(chunks.numel()),
                                     ptr(buf.rnn_states), ptr(buf.rnn_states_critic), ptr(self.grad[0]),
                                     ptr(self.grad[1]), ptr(self.gscr), stream_handle(self.device)), "mappo_grad_mb")

    def minibatch(self, buf, chunks, slot, ba=None):
        """One ppo_update (ramppo_network.py:56-209) on a minibatch: its moments, ValueNorm.update(return_batch),
        the gradients over its chunks, clip + Adam."""
        self.mb_stats(buf, chunks)
        check(lib().mm_mappo_vn_update(ptr(self.vn), ptr(self.stats), 0.99999, stream_handle(self.device)),
              "mappo_vn_update")
        self.gradients_mb(buf, chunks, ba)
        self.clip_adam(slot)

    def train(self, buf, perms=None):
        """R_MAPPO.train (ramppo_network.py:211-287). perms (num_mini_batch > 1 only): [epochs, n_chunks]
        permutations in the reference's chunk numbering c = en * (T / L) + kc replacing the drawn ones (a
        feed-forward policy: [epochs, T * EN] permutations of the buffer rows t * EN + en)."""
        if self.M == 1:
            if perms is not None:
                raise ValueError("perms needs num_mini_batch > 1: one minibatch per epoch holds every chunk, in "
                                 "chunk order")
            self.prepare(buf)
            fa, ba = self.fwd_args(buf), self.bwd_args(buf)
            for ep in range(self.epochs):
                self.epoch(buf, ep, fa, ba)
        else:
            native = self._to_native(self.draw_perms()) if perms is None else self.native_chunks(perms)
            self.prepare(buf)
            ba = self.bwd_args(buf)
            for ep in range(self.epochs):
                for i in range(self.M):
                    self.minibatch(buf, native[ep, i * self.mbs:(i + 1) * self.mbs], ep * self.M + i, ba)
        self.train_calls += 1
        return self.train_info()

    def train_info(self):
        la = self.loss_acc.detach().cpu().numpy().astype(np.float64)
        nrm = self.norms.detach().cpu().numpy().astype(np.float64)
        e = max(1, self.epochs * self.M)                                        # updates
        rows = self.rows if self.M == 1 else self.mbs * self.L                  # rows trained per update
        return {"value_loss": la[MM_MLOSS_VALUE] / e, "policy_loss": la[MM_MLOSS_POLICY] / e,
                "dist_entropy": la[MM_MLOSS_ENTROPY] / e, "actor_grad_norm": nrm[0].mean(),
                "critic_grad_norm": nrm[1].mean(), "ratio": la[MM_MLOSS_RATIO] / (e * rows)}


class MappoRunner:
    """MAGYM_Runner (magym_runner.py:30-195) on lockstep device envs: collect -> insert -> compute -> train."""

    def __init__(self, env, policy, T=100, L=5, ppo_epoch=15, gamma=0.99, gae_lambda=0.95, seed=0,
                 grad_allreduce=None, num_mini_batch=1):
        """num_mini_batch: PPO minibatches per epoch (MappoTrainer; their permutations are seeded with ``seed``)."""
        self.env, self.p = env, policy
        from .env import SwitchVecEnv
        if isinstance(env, SwitchVecEnv):   # the 3-wide kernels read the own agent's [row, col, clock]
            switch_cfg = env.cfg
            if switch_cfg.full_observable:
                raise ValueError("MappoRunner on Switch needs local observations: full_observable=True (obs_dim "
                                 f"{env.obs_dim}) has no MAPPO kernel; use_centralized_V gives the critic the env's "
                                 "joint observation instead (MappoPolicy(cent_agents=n_agents))")
            if not switch_cfg.clock:
                raise ValueError("MappoRunner on Switch needs the clock feature: clock=False (obs_dim "
                                 f"{env.obs_dim}) has no MAPPO kernel (the built width is 3: row, column, clock)")
        if policy.cent_agents not in (None, env.N):
            raise ValueError(f"policy.cent_agents={policy.cent_agents} != the env's {env.N} agents")
        if policy.D != env.obs_dim:
            raise ValueError(f"policy obs_dim {policy.D} != the env's obs_dim {env.obs_dim}")
        self.E, self.N, self.D = env.E, env.N, env.obs_dim
        self.T, self.gamma, self.gl = int(T), gamma, gae_lambda
        dev = self.device = policy.device
        self.recurrent = bool(getattr(policy, "recurrent", True))
        self.buf = MappoBuffer(T, self.E, self.N, self.D, policy.H, dev, recurrent=self.recurrent)
        self.trainer = MappoTrainer(policy, T, self.E * self.N, L, ppo_epoch, grad_allreduce=grad_allreduce,
                                    num_mini_batch=num_mini_batch, perm_seed=int(seed))
        self.seed = int(seed)
        self.counter = torch.zeros(1, dtype=torch.int64, device=dev)
        self.done = torch.zeros(self.E, dtype=torch.uint8, device=dev)
        self.args = []
        b = self.buf
        for t in range(self.T):
            if not self.recurrent:
                self.args.append(policy.rollout_args(b.obs[t], logp_out=b.action_log_probs[t],
                                                     value_out=b.value_preds[t], act_out=b.actions[t],
                                                     seed=self.seed, counter_ptr=ptr(self.counter)))
                continue
            a = policy.rollout_args(b.obs[t], b.rnn_states[t], b.rnn_states_critic[t], b.masks[t],
                                    b.rnn_states[t + 1], b.rnn_states_critic[t + 1], b.action_log_probs[t],
                                    b.value_preds[t], act_out=b.actions[t], seed=self.seed,
                                    counter_ptr=ptr(self.counter))
            self.args.append(a)

    def warmup(self):
        self.env.reset(out=self.buf.obs[0].view(self.E, self.N, self.D))

    def collect_step(self, t):
        L_, s, b = lib(), stream_handle(self.device), self.buf
        if not self.recurrent:
            self.p._fwd(self.args[t])
            check(self.env.step_into(ptr(b.actions[t]), ptr(b.obs[t + 1]), ptr(b.rewards[t]), ptr(self.done), s),
                  "env_step")
            check(L_.mm_mappo_ff_insert(ptr(self.done), self.N, self.E, ptr(b.masks[t + 1]),
                                        ptr(b.active_masks[t + 1]), ptr(self.counter), s), "mappo_ff_insert")
            return
        check(L_.mm_mappo_fwd(ctypes.byref(self.p.dims), ctypes.byref(self.args[t]), s), "mappo_fwd")
        # no terminal obs needed (MAPPO bootstraps through masks): only the auto-reset current obs. On Switch ``done``
        # is the env-level all(agent done): the reference's insert takes its masks from it and leaves active_masks at
        # one (magym_runner.py:151-195 builds active_masks but does not pass them on, shared_buffer.py:82-113)
        check(self.env.step_into(ptr(b.actions[t]), ptr(b.obs[t + 1]), ptr(b.rewards[t]), ptr(self.done), s),
              "env_step")
        check(L_.mm_mappo_insert(ptr(self.done), self.N, self.p.H, self.E, ptr(b.masks[t + 1]),
                                 ptr(b.active_masks[t + 1]), ptr(b.rnn_states[t + 1]), ptr(b.rnn_states_critic[t + 1]),
                                 ptr(self.counter), s), "mappo_insert")

    def rollout(self):
        for t in range(self.T):
            self.collect_step(t)

    def compute(self):
        b = self.buf
        a = MappoFwdArgs()
        a.net[1].P, a.net[1].h_in, a.net[1].out = _ptrs(self.p.critic.flat,
                                                        b.rnn_states_critic[self.T] if self.recurrent else None,
                                                        b.value_preds[self.T])
        a.obs, a.mask = _ptrs(b.obs[self.T], b.masks[self.T])
        a.rows, a.mode = b.EN, MM_MAPPO_VALUES
        self.p._fwd(a)
        b.compute_returns(self.trainer.vn, self.gamma, self.gl)

    def train(self):
        info = self.trainer.train(self.buf)
        self.buf.after_update()
        return info

    def run_episode(self):
        self.rollout()
        self.compute()
        return self.train()
