"""Offpolicy transition replay on the MI355X: ``MlpReplayBuffer`` / ``PrioritizedMlpReplayBuffer``.

Mirrors offpolicy/utils/mlp_buffer.py:10-340 (same constructor arguments, ``insert`` / ``sample`` /
``update_priorities`` / ``__len__``, the same 13-tuple from ``sample``) over the C ABI ``mm_mlpbuf_*``
(include/minimarl.h, csrc/mlpbuf.hip). The transitions, SumSegmentTree and MinSegmentTree live in HBM; a sampled
tuple holds device tensors (``{policy_id: tensor}``, the ``avail`` entries ``{policy_id: None}``, ``weights`` f32 and
``idxes`` int64 on the device) and goes into ``MOffQMix.train_policy_on_batch`` unchanged.

Differences from the reference, by necessity or by switch:
* the numpy draws come from the device counter RNG, or are injected (``fracs=`` / ``inds=``), as in ``recbuf``;
* ``leaf_mode="reference"`` (default) keeps the reference's prioritized insert, whose loop
  ``range(idx_range[0], idx_range[1])`` gives only the first written slot's leaf ``max_priority ** alpha`` (none when
  the second written slot wrapped to 0; ``n = 1`` is an IndexError there and a ValueError here); ``"slots"`` writes
  the leaf of every slot written;
* ``store_share=False`` (needs S == N * D) stores no share_obs: a sampled ``cent_obs`` row is the transition's obs
  row, the concatenation over agents. ``insert`` then ignores its share arguments;
* ``insert_collected(collector)`` lets a ``MOffQCollector`` write the ring in place at the cursor;
* device-side ``update_priorities`` inputs are checked by the kernel (``check_errors``);
* not built, raise: ``use_avail_acts``, ``use_reward_normalization``, ``use_same_share_obs=False``, more than one
  policy.
There is no CPU path.
"""
import ctypes

import numpy as np
import torch

from ._lib import MlpbufDims, MlpbufFields, check, lib, release
from .qnet import ptr, stream_handle
from .recbuf import _dim

FIELDS = ("obs", "share_obs", "acts", "rewards", "next_obs", "next_share_obs", "dones", "dones_env",
          "valid_transition")


class MlpReplayBuffer:
    """mlp_buffer.py:10-96 (uniform transition sampling)."""
    prioritized = False

    def __init__(self, policy_info, policy_agents, buffer_size, use_same_share_obs, use_avail_acts,
                 use_reward_normalization=False, device="cuda", seed=0, leaf_mode="reference", store_share=True,
                 _alpha=0.6):
        if use_avail_acts:
            raise NotImplementedError("use_avail_acts is not built (MOffQMix takes no available-action masks)")
        if use_reward_normalization:
            raise NotImplementedError("use_reward_normalization is not built (off in the reference's configs)")
        if not use_same_share_obs:
            raise NotImplementedError("use_same_share_obs=False is not built")
        if list(policy_info.keys()) != ["policy_0"]:
            raise NotImplementedError("more than one policy is not built (the trainer has one shared policy)")
        if leaf_mode not in ("reference", "slots"):
            raise ValueError(f"leaf_mode {leaf_mode!r}: 'reference' or 'slots'")
        info = policy_info["policy_0"]
        self.policy_info = policy_info
        self.buffer_size = int(buffer_size)
        self.device = torch.device(device)
        self.seed, self._draws = int(seed), 0
        self.N = len(policy_agents["policy_0"])
        self.D, self.S, self.A = _dim(info["obs_space"]), _dim(info["share_obs_space"]), _dim(info["act_space"])
        self.store_share, self.leaf_mode = bool(store_share), leaf_mode
        if not self.store_share and self.S != self.N * self.D:
            raise ValueError(f"store_share=False needs share_obs dim S ({self.S}) == N * D ({self.N * self.D})")
        dims = MlpbufDims(self.N, self.D, self.S, self.A, int(self.store_share), int(self.prioritized),
                          0 if leaf_mode == "reference" else 1)
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            check(lib().mm_mlpbuf_create(ctypes.byref(dims), self.buffer_size, float(_alpha), ctypes.byref(h)),
                  "mlpbuf_create")
        self._h = h
        N = self.N
        self.rows = {"obs": (N, self.D), "share_obs": (self.S,), "acts": (N, self.A), "rewards": (N, 1),
                     "next_obs": (N, self.D), "next_share_obs": (self.S,), "dones": (N, 1), "dones_env": (1,),
                     "valid_transition": (N, 1)}

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self._h = None
            try:
                release("mm_mlpbuf_destroy", h)   # deferred while a graph capture is running
            except Exception:   # interpreter shutdown: module globals already gone
                pass

    def __len__(self):
        return int(lib().mm_mlpbuf_len(self._h))

    @property
    def current_i(self):
        return int(lib().mm_mlpbuf_current(self._h))

    def stores(self):
        """The device stores as an ``MlpbufFields`` of pointers, [buffer_size][row] each (share: NULL without
        store_share)."""
        f = MlpbufFields()
        check(lib().mm_mlpbuf_stores(self._h, ctypes.byref(f)), "mlpbuf_stores")
        return f

    def _dev(self, x, shape):
        x = x["policy_0"] if isinstance(x, dict) else x
        t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
        t = t.to(device=self.device, dtype=torch.float32).contiguous()
        assert tuple(t.shape) == shape, ("different size!", tuple(t.shape), shape)
        return t

    def _check_n(self, n):
        if self.prioritized and self.leaf_mode == "reference" and n < 2:
            raise ValueError("leaf_mode='reference' needs at least 2 transitions per insert: the reference's "
                             "PrioritizedMlpReplayBuffer.insert reads idx_range[1]")

    def insert(self, num_insert_steps, obs, share_obs, acts, rewards, next_obs, next_share_obs, dones, dones_env,
               valid_transition, avail_acts=None, next_avail_acts=None):
        """mlp_buffer.py:39-69 / 161-208 from the step-major arrays ([n, N, X], share [n, S], dones_env [n, 1]):
        returns the ring slots written (np.ndarray)."""
        n = int(num_insert_steps)
        self._check_n(n)
        given = dict(zip(FIELDS, (obs, share_obs, acts, rewards, next_obs, next_share_obs, dones, dones_env,
                                  valid_transition)))
        src = {k: self._dev(given[k], (n,) + self.rows[k]) for k in FIELDS
               if self.store_share or k not in ("share_obs", "next_share_obs")}
        f = MlpbufFields(*[ptr(src.get(k)) for k in FIELDS])
        idx = np.zeros(n, np.int64)
        check(lib().mm_mlpbuf_insert(self._h, n, ctypes.byref(f), idx.ctypes.data_as(ctypes.c_void_p),
                                     stream_handle(self.device)), "mlpbuf_insert")
        self._keep = src           # alive until the copies ran (stream-ordered reuse is safe after)
        return idx

    def insert_collected(self, collector):
        """One window of ``collector`` (a ``minimarl.moffq_runner.MOffQCollector`` at its current epsilon) written
        by its launch straight into the ring at the cursor, then the leaf writes and the cursor advance by T * E.
        Needs store_share=False. Returns the ring slots written (np.ndarray)."""
        assert not self.store_share, "insert_collected: the collector writes no share_obs (store_share=False)"
        assert (collector.N, collector.D, collector.A) == (self.N, self.D, self.A)
        n = collector.T * collector.E
        assert n <= self.buffer_size, "a collect window must fit the buffer"
        self._check_n(n)
        # current_i is the reference's cursor, in (0, size] after an insert: size stands for slot 0
        collector.launch(self.stores(), self.current_i % self.buffer_size, self.buffer_size)
        idx = np.zeros(n, np.int64)
        check(lib().mm_mlpbuf_advance(self._h, n, idx.ctypes.data_as(ctypes.c_void_p), stream_handle(self.device)),
              "mlpbuf_advance")
        return idx

    def _next_counter(self):
        self._draws += 1
        return self._draws - 1

    def sample(self, batch_size, inds=None):
        """mlp_buffer.py:71-95: B transitions uniformly (device RNG, or the injected ``inds``)."""
        B = int(batch_size)
        if inds is None:
            idx = torch.empty(B, dtype=torch.int64, device=self.device)
            check(lib().mm_mlpbuf_sample_uniform(self._h, B, self.seed, self._next_counter(), ptr(idx),
                                                 stream_handle(self.device)), "mlpbuf_sample_uniform")
        else:
            idx = torch.as_tensor(inds).to(device=self.device, dtype=torch.int64).contiguous()
        return self.sample_inds(idx) + (None, None)

    def sample_inds(self, idx):
        """MlpPolicyBuffer.sample_inds (mlp_buffer.py:210-257) for device indices [B]: the eleven fields."""
        B, N = int(idx.numel()), self.N
        out = {}
        for k in FIELDS:
            r = self.rows[k]
            out[k] = torch.empty((N, B, r[1]) if len(r) == 2 else (B, r[0]), device=self.device)
        f = MlpbufFields(*[ptr(out[k]) for k in FIELDS])
        check(lib().mm_mlpbuf_gather(self._h, B, ptr(idx), ctypes.byref(f), stream_handle(self.device)),
              "mlpbuf_gather")
        self._keep_idx = idx
        return tuple({"policy_0": out[k]} for k in FIELDS) + ({"policy_0": None}, {"policy_0": None})

    # -- inspection (tests, checkpoints) -------------------------------------------------------
    def state(self):
        """Device copies (stream-ordered) of (sum tree f64 [2 itcap], min tree, max_priority f32 [1], error word)."""
        n = 2 * int(lib().mm_mlpbuf_it_capacity(self._h))
        st = (torch.empty(n, dtype=torch.float64, device=self.device),
              torch.empty(n, dtype=torch.float64, device=self.device),
              torch.empty(1, dtype=torch.float32, device=self.device),
              torch.empty(1, dtype=torch.int32, device=self.device))
        check(lib().mm_mlpbuf_copy_state(self._h, *[ptr(t) for t in st], stream_handle(self.device)),
              "mlpbuf_copy_state")
        return st

    def trees(self):
        s, m, _, _ = self.state()
        return s.cpu().numpy(), m.cpu().numpy()

    def max_priority(self):
        return float(self.state()[2].cpu()[0])

    def check_errors(self):
        """Raise AssertionError if a device-side update_priorities or gather hit the reference's asserts."""
        e = int(self.state()[3].cpu()[0])
        assert e & 1 == 0, "update_priorities: index outside [0, len)"
        assert e & 2 == 0, "update_priorities: priority <= 0"
        assert e & 4 == 0, "sample: transition index outside the buffer"


class PrioritizedMlpReplayBuffer(MlpReplayBuffer):
    """mlp_buffer.py:260-340 (proportional prioritisation over SumSegmentTree / MinSegmentTree)."""
    prioritized = True

    def __init__(self, alpha, policy_info, policy_agents, buffer_size, use_same_share_obs, use_avail_acts,
                 use_reward_normalization=False, device="cuda", seed=0, leaf_mode="reference", store_share=True):
        self.alpha = alpha
        super().__init__(policy_info, policy_agents, buffer_size, use_same_share_obs, use_avail_acts,
                         use_reward_normalization, device=device, seed=seed, leaf_mode=leaf_mode,
                         store_share=store_share, _alpha=alpha)

    def sample(self, batch_size, beta=0, p_id=None, fracs=None):
        """mlp_buffer.py:295-320: the eleven fields, weights (device f32 [B]) and batch_inds (device int64 [B]).
        ``fracs``: the uniform draws to use instead of the device RNG."""
        B = int(batch_size)
        assert len(self) > B, "Not enough samples in the buffer!"
        assert beta > 0
        idx = torch.empty(B, dtype=torch.int64, device=self.device)
        w = torch.empty(B, dtype=torch.float32, device=self.device)
        fr = None
        if fracs is not None:
            fr = torch.as_tensor(np.asarray(fracs, np.float64) if not torch.is_tensor(fracs) else fracs).to(
                device=self.device, dtype=torch.float64).contiguous()
        check(lib().mm_mlpbuf_sample_prioritized(self._h, B, float(beta), ptr(fr), self.seed,
                                                 self._next_counter() if fr is None else 0, ptr(idx), None, ptr(w),
                                                 stream_handle(self.device)), "mlpbuf_sample_prioritized")
        self._keep_fr = fr
        return self.sample_inds(idx) + (w, idx)

    def update_priorities(self, idxes, priorities, p_id=None):
        """mlp_buffer.py:322-340 (device or host inputs)."""
        if not torch.is_tensor(idxes) or not torch.is_tensor(priorities):
            pi = np.asarray(priorities if not torch.is_tensor(priorities) else priorities.cpu())
            ii = np.asarray(idxes if not torch.is_tensor(idxes) else idxes.cpu())
            assert len(ii) == len(pi)
            assert np.min(pi) > 0
            assert np.min(ii) >= 0
            assert np.max(ii) < len(self)
        idx = torch.as_tensor(idxes).to(device=self.device, dtype=torch.int64).contiguous()
        pr = torch.as_tensor(priorities).to(device=self.device, dtype=torch.float32).contiguous()
        assert idx.numel() == pr.numel()
        check(lib().mm_mlpbuf_update_priorities(self._h, ptr(idx), ptr(pr), int(idx.numel()),
                                                stream_handle(self.device)), "mlpbuf_update_priorities")
        self._keep_up = (idx, pr)


__all__ = ["MlpReplayBuffer", "PrioritizedMlpReplayBuffer"]
