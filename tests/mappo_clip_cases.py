"""Case builder shared by tests/test_mappo_clip_cases_cpu.py (CPU) and tests/test_gpu_mappo_clip.py (GPU): MAPPO
training inputs on which PPO's three branch points are ACTIVE -- the surrogate clip min(r A, clamp(r, 1 +- eps) A),
the clipped value loss max(huber(tgt - v), huber(tgt - v_clipped)) and Huber's quadratic / linear switch
(ramppo_network.py:56-101,150-166) -- plus the oracle's answers on them. Imports neither the library nor CUDA;
every case is built once per process and is read-only.

  golden16  tests/golden/mappo_clip_train.npz (the reference's own train() on the perturbed buffer): E 4, N 2, T 10,
            L 5, 16 chunks (less than one tile of 32), 80 row-steps; through oracle.mappo.ppo_train
  tiles70   synthetic, E 7, N 5, T 10, L 5: 70 chunks = 2 tiles + 6, clip_param 0.1; through oracle.mappo.ppo_train
  cent_n2   tests/golden/mappo_cv_train.npz case n2, perturbed here, centralized critic; mappo_cv_ref.ppo_train_cv
  mb16      tests/golden/mappo_mb_train.npz, perturbed here, its recorded perms, M 3 (5 chunks per update, updates 0
            and 1); through mappo_mb_ref.ppo_train_mb

Every case's old log-probs move by U(+-LP_AMP) and its old values by U(+-V_AMP), a KEEP share of each left bit for
bit as the rollout wrote it (so the in-range tie arm s1 == s2 stays covered). huber_delta is the median |tgt - v|
over the active rows of the float64 oracle's first update, after that update's ValueNorm step (mb16: the rows of
update 0). tiles70's buffer restates make_golden_mappo.train_fixture's loop with the float32 oracle
(om.get_actions on injected uniforms) in place of the reference: the same kind of observations, env-level dones
inside chunks, one agent-level done (active_masks has zeros), returns from om.compute_returns.

Conditions on the INPUTS, asserted when a case is built on the float64 oracle's first update (mb16: updates 0 and 1).
A seed that misses one is replaced (SEEDS), never the threshold:
  coverage   each (ratio range, advantage sign) class, ratio in range / > 1 + eps with A > 0 / > 1 + eps with A < 0 /
             < 1 - eps with A > 0 / < 1 - eps with A < 0, holds >= MIN_CLASS of the active rows, and so does each of
             dv < -eps and dv > +eps; among the value-clipped rows each of lo > lc and lc > lo holds >= MIN_SIDE;
             each of |tgt - v| > delta and |tgt - v_clipped| > delta holds >= MIN_LINEAR of the active rows; mb16:
             over the rows of updates 0 and 1 together, and every class non-empty in each update
  margins    no active row's ratio within RATIO_MARGIN of 1 +- eps, no active row's |dv| within DV_MARGIN of eps, no
             value-clipped row's two Huber values within SIDE_MARGIN of each other (float32 noise on these is ~1e-7;
             the Huber switch itself is continuous and needs no margin)
  stability  every active row keeps its class (ratio range, advantage sign, dv range, side of the max) across the
             three oracle runs of the tolerance rule (float32 in the given chunk order, float32 in another order,
             float64), in every update the GPU tests check: a branch that flips between two float32 runs would widen
             the spread and could hide a failure
"""
import contextlib
import functools
import os

import numpy as np
import torch

import mappo_cv_ref as cv
import mappo_mb_ref as mb
from oracle import mappo as om

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K_FP32 = 16
LP_AMP, V_AMP, KEEP = 0.5, 0.6, 0.3
MIN_CLASS, MIN_SIDE, MIN_LINEAR = 0.05, 0.20, 0.25
RATIO_MARGIN, DV_MARGIN, SIDE_MARGIN = 1e-4, 1e-4, 1e-5
D, A, H = 47, 5, 32
#            kind    clip  updates whose gradients the GPU tests check
CASES = {
    "golden16": ("full", 0.2, 1),
    "tiles70":  ("full", 0.1, 1),
    "cent_n2":  ("cent", 0.2, 1),
    "mb16":     ("mb",   0.2, 2),
}
# perturbation seed per case (golden16's is the generator's: its perturbed data is in the fixture)
# replaced seeds: golden16's 1 left two Huber values 7.1e-6 apart; mb16's 4 gave update 0 a mean ratio 3.9e-3 off 1,
# its 5 is fine too, 6 left a class empty in update 0
SEEDS = {"golden16": 7, "tiles70": 2, "cent_n2": 3, "mb16": 7}
TILES70 = dict(E=7, N=5, T=10, L=5, seed=6)
TRAIN_EPOCHS = 3          # golden16's train()


def perturb(data, seed, lp_amp=LP_AMP, v_amp=V_AMP, keep=KEEP):
    """A copy of a reference-layout buffer with action_log_probs and value_preds[:-1] moved by U(+-amp), a ``keep``
    share of each left untouched (bit for bit). Returns, rewards and everything else stay the rollout's."""
    rng = np.random.default_rng(seed)
    out = dict(data)
    for key, amp, sl in (("action_log_probs", lp_amp, slice(None)), ("value_preds", v_amp, slice(0, -1))):
        x = np.array(data[key], np.float32)
        u = rng.uniform(-amp, amp, x[sl].shape)
        u[rng.random(x[sl].shape) < keep] = 0.0
        x[sl] = (x[sl].astype(np.float64) + u).astype(np.float32)
        out[key] = x
    return out


@contextlib.contextmanager
def _default_dtype(dtype):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def _cast(data, dtype):
    npd = np.float64 if dtype == torch.float64 else np.float32
    return {k: (v.astype(npd) if v.dtype in (np.float32, np.float64) else v) for k, v in data.items()}


def huber_np(e, d):
    a = np.abs(e)
    return np.where(a <= d, e * e / 2, d * (a - d / 2))


class Case:
    """Inputs of one case and the three oracle runs of the tolerance rule on them."""

    def __init__(self, cid, PA, PC, data, vn0, L, perms=None, M=1, fx=None):
        self.cid = cid
        self.kind, self.clip, self.n_updates = CASES[cid]
        self.PA, self.PC, self.data, self.vn0, self.L = PA, PC, data, tuple(vn0), int(L)
        self.T, self.E, self.N = (int(x) for x in data["rewards"].shape[:3])
        self.n_chunks = self.T * self.E * self.N // self.L
        self.perms, self.M, self.fx = perms, int(M), fx
        self.huber_delta = None
        self._runs = {}

    # -- the oracle ------------------------------------------------------------------------------
    def train(self, dtype, alt, updates):
        """The case's oracle for ``updates`` updates -> (record, PA2, PC2, vn2). alt: the other chunk order of the
        tolerance rule (a fixed permutation of the chunks; mb16: the chunks shuffled within each minibatch)."""
        key = (dtype, bool(alt), int(updates))
        if key in self._runs:
            return self._runs[key]
        kw = dict(clip=self.clip, huber_delta=self.huber_delta)
        with torch.enable_grad():
            out = self._train(dtype, alt, updates, kw)
        self._runs[key] = out
        return out

    def _train(self, dtype, alt, updates, kw):
        if self.kind == "mb":
            out = mb.ppo_train_mb(self.PA, self.PC, self.data, self.vn0, int(self.fx["epochs"]), self.L, self.perms,
                                  self.M, dtype=dtype, shuffle=bool(alt), updates=updates, **kw)
        else:
            pm = np.stack([self.order(alt, u) for u in range(updates)]) if alt and updates else None
            if self.kind == "cent":
                out = cv.ppo_train_cv(self.PA, self.PC, self.data, self.vn0, updates, self.L, perms=pm, dtype=dtype,
                                      **kw)
            else:
                with _default_dtype(dtype):
                    pa = {k: torch.as_tensor(v).to(dtype) for k, v in self.PA.items()}
                    pc = {k: torch.as_tensor(v).to(dtype) for k, v in self.PC.items()}
                    rec = []
                    PA2, PC2, vn2 = om.ppo_train(pa, pc, _cast(self.data, dtype), om.ValueNorm(*self.vn0), updates,
                                                 self.L, perms=pm, record=rec, **kw)
                out = (rec, PA2, PC2, vn2)
        return out

    def order(self, alt, u):
        """The chunks of update u (the reference's numbering) in the order the run (alt) evaluates them."""
        if self.kind != "mb":
            return np.random.default_rng(123).permutation(self.n_chunks) if alt else np.arange(self.n_chunks)
        orders = [o for ep in range(len(self.perms)) for o in mb.minibatches(self.perms[ep], self.M)]
        if not alt:
            return np.asarray(orders[u])
        rng = np.random.default_rng(123)          # (mappo_mb_ref.ppo_train_mb's shuffle, replayed)
        for i in range(u + 1):
            o = rng.permutation(orders[i])
        return o

    def batch(self, dtype, alt, u):
        """(PA, PC, chunk batch, ValueNorm after update u's step, chunk order) at the start of update u of the run
        (dtype, alt); built under the caller's default dtype. A centralized case's batch holds 'cent_obs'."""
        _, PA, PC, vn = self.train(dtype, alt, u)
        vn = om.ValueNorm(float(vn.m), float(vn.msq), float(vn.d))
        order = self.order(alt, u)
        d = _cast(self.data, dtype)
        adv = om.normalized_advantages(d, om.ValueNorm(*self.vn0))
        b = om.chunk_batch(d, adv, self.L, order)
        if self.kind == "cent":
            b["cent_obs"] = om.chunk_batch(dict(d, obs=cv.share_obs(d["obs"])), adv, self.L, order)["obs"]
        vn.update(b["returns"])
        return PA, PC, b, vn, order

    def row_terms(self, dtype, alt, u):
        """Per-row quantities of update u's loss seed in the run (dtype, alt), as float64 arrays [L, n_chunks] in
        the chunks' own numbering (NaN where a chunk is not in the update): ratio, adv, dv, eo, ec, active."""
        with _default_dtype(dtype), torch.no_grad():
            PA, PC, b, vn, order = self.batch(dtype, alt, u)
            lp, _ = om.evaluate_chunks(PA, b["obs"], b["ha0"], b["masks"], self.L, "actor", b["actions"],
                                       b["active_masks"])
            v = om.evaluate_chunks(PC, b.get("cent_obs", b["obs"]), b["hc0"], b["masks"], self.L, "critic")
            dv = v - b["value_preds"]
            tgt = vn.normalize(b["returns"])
            t = dict(ratio=torch.exp(lp - b["action_log_probs"]), adv=b["adv"], dv=dv, eo=tgt - v,
                     ec=tgt - (b["value_preds"] + dv.clamp(-self.clip, self.clip)), active=b["active_masks"])
        out = {}
        for k, x in t.items():
            full = np.full((self.L, self.n_chunks), np.nan)
            full[:, order] = x.double().numpy().reshape(self.L, len(order))
            out[k] = full
        return out

    def classes(self, t):
        """(ratio range, advantage sign, dv range, side of the max) per row of row_terms' output; -1 where the row
        is inactive or not in the update."""
        c, act = self.clip, np.nan_to_num(t["active"]) > 0
        with np.errstate(invalid="ignore"):
            rr = np.where(t["ratio"] > 1 + c, 1, np.where(t["ratio"] < 1 - c, 2, 0))
            sg = (t["adv"] > 0).astype(int)
            dr = np.where(t["dv"] > c, 1, np.where(t["dv"] < -c, 2, 0))
            side = np.where(dr != 0, np.sign(huber_np(t["eo"], self.huber_delta) - huber_np(t["ec"], self.huber_delta)),
                            0).astype(int)
        out = {"ratio": rr, "adv_sign": sg, "dv": dr, "side": side}
        return {k: np.where(act, v, -1) for k, v in out.items()}

    # -- conditions on the inputs ----------------------------------------------------------------
    def check_inputs(self):
        ts = [self.row_terms(torch.float64, False, u) for u in range(self.n_updates)]
        per = [self._shares(t) for t in ts]
        both = self._shares({k: np.concatenate([t[k] for t in ts], 1) for k in ts[0]})
        for name, (share, bar) in both.items():
            assert share >= bar, f"{self.cid}: class '{name}' holds {share:.3f} < {bar} of its rows"
        for u, p in enumerate(per):
            for name, (share, _) in p.items():
                assert share > 0, f"{self.cid}: class '{name}' is empty in update {u}"
        c = self.clip
        for u, t in enumerate(ts):
            act = np.nan_to_num(t["active"]) > 0
            r, dv = t["ratio"][act], t["dv"][act]
            m = np.minimum(np.abs(r - (1 - c)), np.abs(r - (1 + c))).min()
            assert m >= RATIO_MARGIN, f"{self.cid} update {u}: a ratio lies {m:.2e} from 1 +- clip"
            m = np.abs(np.abs(dv) - c).min()
            assert m >= DV_MARGIN, f"{self.cid} update {u}: a |dv| lies {m:.2e} from clip"
            vc = act & (np.abs(np.nan_to_num(t["dv"])) > c)
            m = np.abs(huber_np(t["eo"][vc], self.huber_delta) - huber_np(t["ec"][vc], self.huber_delta)).min()
            assert m >= SIDE_MARGIN, f"{self.cid} update {u}: two Huber values lie {m:.2e} apart"
        self.shares = {k: v[0] for k, v in both.items()}
        self.check_stability(self.n_updates)

    def _shares(self, t):
        """{class: (share of its population, the bar)} on row_terms-shaped arrays."""
        c, hd = self.clip, self.huber_delta
        act = np.nan_to_num(t["active"]) > 0
        r, adv, dv, eo, ec = (t[k][act] for k in ("ratio", "adv", "dv", "eo", "ec"))
        n = float(act.sum())
        hi, lo_, pos = r > 1 + c, r < 1 - c, adv > 0
        out = {"ratio in range": ((~hi & ~lo_).sum() / n, MIN_CLASS),
               "ratio > 1+eps, A > 0": ((hi & pos).sum() / n, MIN_CLASS),
               "ratio > 1+eps, A < 0": ((hi & ~pos).sum() / n, MIN_CLASS),
               "ratio < 1-eps, A > 0": ((lo_ & pos).sum() / n, MIN_CLASS),
               "ratio < 1-eps, A < 0": ((lo_ & ~pos).sum() / n, MIN_CLASS),
               "dv < -eps": ((dv < -c).sum() / n, MIN_CLASS), "dv > +eps": ((dv > c).sum() / n, MIN_CLASS)}
        vc = np.abs(dv) > c
        lo, lc = huber_np(eo[vc], hd), huber_np(ec[vc], hd)
        out["lo > lc"] = ((lo > lc).sum() / max(1.0, float(vc.sum())), MIN_SIDE)
        out["lc > lo"] = ((lc > lo).sum() / max(1.0, float(vc.sum())), MIN_SIDE)
        out["|tgt - v| > delta"] = ((np.abs(eo) > hd).sum() / n, MIN_LINEAR)
        out["|tgt - v_clipped| > delta"] = ((np.abs(ec) > hd).sum() / n, MIN_LINEAR)
        return out

    def check_stability(self, n_updates):
        for u in range(n_updates):
            ref = self.classes(self.row_terms(torch.float64, False, u))
            for alt in (False, True):
                got = self.classes(self.row_terms(torch.float32, alt, u))
                for k in ref:
                    bad = np.argwhere(ref[k] != got[k])
                    assert len(bad) == 0, (f"{self.cid} update {u}: {len(bad)} rows change their '{k}' class between "
                                           f"the float64 run and the float32 run (alt={alt}), first (l, chunk) = "
                                           f"{tuple(bad[0])}")

    # -- the oracle's answers ----------------------------------------------------------------------
    def spread(self, f):
        """f(dtype, alt) -> {name: array}; -> (float64 values, {name: fp32 spread}), the project's tolerance rule
        (mappo_cv_ref.fp32_spread / mappo_mb_ref.fp32_spread, with this case's other chunk order)."""
        if self.kind == "mb":
            return mb.fp32_spread(f)
        return cv.fp32_spread(lambda dt, pm: f(dt, pm is not None), self.n_chunks)

    def update_grads(self, dtype, alt):
        """{(update, net, key): unclipped gradient} of the case's checked updates."""
        return mb.update_grads(self.train(dtype, alt, self.n_updates)[0], range(self.n_updates))

    def mean_ratio(self, n_updates):
        """The train() log's 'ratio' in float64: the mean over the updates of the mean over ALL rows of an update
        (ramppo_network.py:278, inactive rows included)."""
        rs = [self.row_terms(torch.float64, False, u)["ratio"] for u in range(n_updates)]
        return float(np.mean([np.nanmean(r) for r in rs]))


def gen_obs(rng, shape):
    """Checkers-like observations (make_golden_mappo.gen_obs): 2 coords in [0, 1], then {0, 1} bits (p = 0.2)."""
    o = (rng.random(shape) < 0.2).astype(np.float32)
    o[..., :2] = rng.random(shape[:-1] + (2,)).astype(np.float32)
    return o


def synth_buffer(PA, PC, E, N, T, seed, gamma=0.99, gae_lambda=0.95):
    """make_golden_mappo.train_fixture's rollout with the float32 oracle in place of the reference: a buffer in the
    reference layout [T(+1), E, N, ...] and the fresh ValueNorm's state."""
    rng = np.random.default_rng(seed)
    z = lambda *s: np.zeros(s, np.float32)  # noqa: E731
    d = dict(obs=z(T + 1, E, N, D), rnn_states=z(T + 1, E, N, 1, H), rnn_states_critic=z(T + 1, E, N, 1, H),
             actions=z(T, E, N, 1), action_log_probs=z(T, E, N, 1), value_preds=z(T + 1, E, N, 1),
             rewards=z(T, E, N, 1), masks=np.ones((T + 1, E, N, 1), np.float32),
             active_masks=np.ones((T + 1, E, N, 1), np.float32))
    d["obs"][0] = gen_obs(rng, (E, N, D))
    done_at = {3: [1], 6: [5], 7: [0, 2]}          # step -> envs whose episode ends (all agents done)
    agent_done = {5: [(3, 1)]}                     # step -> (env, agent) done while the env goes on
    t32 = lambda x: torch.from_numpy(np.ascontiguousarray(x))  # noqa: E731
    for t in range(T):
        u = t32(rng.random(E * N).astype(np.float32))
        with torch.no_grad():
            v, a, lp, ha, hc = om.get_actions(PA, PC, t32(d["obs"][t].reshape(E * N, D)),
                                              t32(d["rnn_states"][t].reshape(E * N, H)),
                                              t32(d["rnn_states_critic"][t].reshape(E * N, H)),
                                              t32(d["masks"][t].reshape(E * N, 1)), u=u)
        v, a, lp = (x.numpy().astype(np.float32).reshape(E, N, 1) for x in (v, a, lp))
        ha, hc = ha.numpy().reshape(E, N, 1, H).copy(), hc.numpy().reshape(E, N, 1, H).copy()
        nobs = gen_obs(rng, (E, N, D))
        rew = rng.choice([-0.01, 0.99, -1.01, 9.99], size=(E, N, 1)).astype(np.float32)
        dones = np.zeros((E, N), bool)
        for e in done_at.get(t, []):
            dones[e] = True
        for e, k in agent_done.get(t, []):
            dones[e, k] = True
        dones_env = dones.all(axis=1)
        ha[dones_env] = 0.0
        hc[dones_env] = 0.0
        masks = np.ones((E, N, 1), np.float32)
        masks[dones_env] = 0.0
        active = np.ones((E, N, 1), np.float32)
        active[dones] = 0.0
        active[dones_env] = 1.0
        d["obs"][t + 1], d["rnn_states"][t + 1], d["rnn_states_critic"][t + 1] = nobs, ha, hc
        d["actions"][t], d["action_log_probs"][t], d["value_preds"][t], d["rewards"][t] = a, lp, v, rew
        d["masks"][t + 1], d["active_masks"][t + 1] = masks, active
    with torch.no_grad():
        nv, _ = om.net_step(PC, t32(d["obs"][T].reshape(E * N, D)), t32(d["rnn_states_critic"][T].reshape(E * N, H)),
                            t32(d["masks"][T].reshape(E * N, 1)))
    vn0 = (0.0, 0.0, 0.0)
    d["returns"], d["value_preds"] = om.compute_returns(d["rewards"], d["value_preds"], d["masks"],
                                                        nv.numpy().reshape(E, N, 1), om.ValueNorm(*vn0), gamma,
                                                        gae_lambda)
    return d, vn0


def median_delta(case):
    """The median |tgt - v| over the active rows of the float64 oracle's first update (after its ValueNorm step)."""
    t = case.row_terms(torch.float64, False, 0)
    return float(np.median(np.abs(t["eo"][np.nan_to_num(t["active"]) > 0])))


def _load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


@functools.lru_cache(maxsize=None)
def case(cid):
    """The case: inputs, huber_delta, the input conditions asserted, and ``grads`` = (float64 unclipped gradients
    of its checked updates, fp32 spreads)."""
    if cid == "golden16":
        fx = _load("mappo_clip_train")
        PA, PC, data, vn0, _ = cv.train_inputs(fx)
        c = Case(cid, PA, PC, data, vn0, int(fx["L"]), fx=fx)
        assert float(fx["clip_param"]) == c.clip
        c.huber_delta = float(fx["huber_delta"])
        # (the generator chose it by the same rule; the reference's train() ran with the stored value)
        assert abs(c.huber_delta - median_delta(c)) <= 1e-9 * c.huber_delta, (c.huber_delta, median_delta(c))
    elif cid == "tiles70":
        PA, PC = cv.nets(_load("mappo_clip_train"), "before.")
        s = TILES70
        data, vn0 = synth_buffer(PA, PC, s["E"], s["N"], s["T"], s["seed"])
        assert (data["active_masks"] == 0).any() and (data["masks"][[4, 7, 8]] == 0).any()
        c = Case(cid, PA, PC, perturb(data, SEEDS[cid]), vn0, s["L"])
        assert c.n_chunks == 70
    elif cid == "cent_n2":
        fx = cv.case(_load("mappo_cv_train"), "n2")
        PA, PC, data, vn0, _ = cv.train_inputs(fx)
        c = Case(cid, PA, PC, perturb(data, SEEDS[cid]), vn0, int(fx["L"]), fx=fx)
    elif cid == "mb16":
        fx = _load("mappo_mb_train")
        PA, PC, data, vn0, _ = cv.train_inputs(fx)
        c = Case(cid, PA, PC, perturb(data, SEEDS[cid]), vn0, int(fx["L"]), perms=fx["perms"],
                 M=int(fx["train_batch_size"]), fx=fx)
    else:
        raise KeyError(cid)
    if c.huber_delta is None:
        c.huber_delta = 10.0            # (any value: the median does not depend on it)
        delta = median_delta(c)
        c._runs.clear()
        c.huber_delta = delta
    c.check_inputs()
    c.grads = c.spread(c.update_grads)
    c.ratio0 = c.mean_ratio(1)
    return c


@functools.lru_cache(maxsize=None)
def train_answers(cid="golden16"):
    """TRAIN_EPOCHS epochs of train() on a single-minibatch case: the class stability of every epoch asserted, then
    (float64 train outputs, fp32 spreads) in mappo_cv_ref.train_outputs' keys, and the float64 mean ratio."""
    c = case(cid)
    assert c.kind != "mb"
    c.check_stability(TRAIN_EPOCHS)
    o64, spread = c.spread(lambda dt, alt: cv.train_outputs(*c.train(dt, alt, TRAIN_EPOCHS)))
    return o64, spread, c.mean_ratio(TRAIN_EPOCHS)
