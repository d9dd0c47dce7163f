"""Case builder shared by tests/test_offq_switch_oracle_fp64.py (CPU) and tests/test_gpu_offq_switch_shapes.py (GPU):
the scheme of tests/offq_cases.py for the trainer at D = 3 (Switch with local observations and the clock, mixer
state S = 3 N = 6, 9, 12). One QMix / VDN train_policy_on_batch per case, inputs plus the CPU oracle's answer in
float64 (the reference) and in float32 (the yardstick for summation-order noise).

Batches are Switch episodes, not minimarl.synth: B random-walk episodes of oracle.switch.SwitchOracle through the
collector's loop (tests/offq_switch_ref.py replay, common reward), so the observations take the env's few values
(three row features, seven column features, the clock k / max_steps), LayerNorm-0 rows of tiny or zero variance
included, ``dones`` is per agent and differs from ``dones_env``, and a finished env repeats its observation with
reward 0. max_steps = max(T, 10); where T < max_steps (the T = 1 cases) episode b is taken after w_b in
[0, max_steps - T] random-walk steps, so that the rows of a one-step batch are not all the reset observation.
Parameters, is_weight, the three fixed dones_env episodes (done at t = 0, never done, done at the last step; where
B >= 4 a last episode that never ends), the kink margin, the top-2 gap and huber_delta are those of
tests/offq_cases.py, by import."""
import functools

import numpy as np
import torch

from offq_cases import (A, HYPER, MIN_KINK_MARGIN, MIN_TOP2_GAP, Case, center_bias, grad_keys, huber_fraction_above,
                        kink_inputs, random_agent, random_mixer, rel_l2)
from offq_switch_ref import replay, step_not_done
from oracle import offq as ref
from oracle.switch import SwitchOracle, SwitchSpec

D = 3
#                 N   T    B    K   Hh  mixer  dQ    PER    huber  max_norm
CASES = {
    "sw_one_row":   (2, 1, 1, 1, 1, "qmix", True, True, False, 10.0),        # S = 6
    "sw_n3_splitk": (3, 1, 257, 33, 64, "qmix", True, False, True, 10.0),    # S = 9, split-K
    "sw_n4_vdn":    (4, 12, 7, 32, 64, "vdn", True, True, False, 10.0),      # S = 12
    "sw_clip_1025": (2, 25, 41, 32, 64, "qmix", True, True, True, 0.05),     # second pass of the loss loops, active clip
    "sw_ref_shape": (2, 100, 32, 32, 64, "qmix", True, True, False, 10.0),   # reference shape
}
FIELDS = ("N", "T", "B", "K", "Hh", "mixer", "double_q", "use_per", "huber", "max_norm")
# (parameter seed, target seed, batch seed) per case; a seed that misses MIN_TOP2_GAP or MIN_KINK_MARGIN is replaced,
# never the margin
SEEDS = {cid: (303 + 10 * i, 304 + 10 * i, 305 + 10 * i) for i, cid in enumerate(CASES)}


def make_batch(seed, N, T, B, use_per):
    rng = np.random.default_rng(int(seed))
    ms = max(T, 10)
    spec = SwitchSpec(N, max_steps=ms)
    warm = rng.integers(0, ms - T + 1, B)                                        # random-walk steps before t = 0
    walk = rng.integers(0, A, (ms, B, N))                                        # episode b's action at its step k
    env = SwitchOracle(spec, B)
    for k in range(int(warm.max())):
        step_not_done(env, walk[k], warm <= k)                                   # steps the episodes with warm[b] > k
    o = replay(spec, B, lambda t, obs: walk[warm + t, np.arange(B)], T, True, env=env)
    obs = np.ascontiguousarray(o["obs"].transpose(2, 0, 1, 3))                   # [N, T+1, B, D]
    share = o["obs"].reshape(T + 1, B, N * D).copy()                             # [T+1, B, N*D]
    tr = lambda x: np.ascontiguousarray(x.transpose(2, 0, 1, 3))                 # noqa: E731  [T, B, N, X] -> [N, T, B, X]
    acts, rew, dones, dones_env = tr(o["acts"]), tr(o["rewards"]), tr(o["dones"]), o["dones_env"].copy()
    isw = (0.5 + rng.random(B)).astype(np.float32) if use_per else None
    if B >= 3:
        dones_env[:, 0] = 1.0           # done at t = 0: every later step is masked
        dones_env[:, 1] = 0.0           # never done
        dones_env[:, 2] = 0.0           # done only at the last step
        dones_env[T - 1, 2] = 1.0
        if B >= 4:
            dones_env[:, B - 1] = 0.0   # the last (t, b) entry, alone in the loss loops' second pass at T * B = 1025
    return {"obs": obs, "share_obs": share, "acts": acts, "rewards": rew, "dones": dones, "dones_env": dones_env,
            "is_weight": isw}


@functools.lru_cache(maxsize=None)
def build_case(cid):
    """Inputs and both oracle answers of one case (computed once per process; treat as read-only)."""
    c = Case()
    c.id, c.D = cid, D
    for k, v in zip(FIELDS, CASES[cid]):
        setattr(c, k, v)
    ps, ts, bs = SEEDS[cid]
    qm = c.mixer == "qmix"
    c.P, c.PT = random_agent(ps, D), random_agent(ts, D)
    c.M = random_mixer(ps, c.N, D, c.K, c.Hh) if qm else {}
    c.MT = random_mixer(ts, c.N, D, c.K, c.Hh) if qm else {}
    c.batch = make_batch(bs, c.N, c.T, c.B, c.use_per)
    kink_inputs(c.P, c.M, c.batch, adjust=True)
    c.kink_margin = kink_inputs(c.P, c.M, c.batch, adjust=False)
    assert c.kink_margin >= MIN_KINK_MARGIN, f"{cid}: a ReLU / |.| argument of {c.kink_margin:.3g}"
    kw = dict(mixer=c.mixer, double_q=c.double_q, use_per=c.use_per, huber=c.huber, K=c.K, max_norm=c.max_norm,
              gamma=HYPER["gamma"], per_nu=HYPER["per_nu"], per_eps=HYPER["per_eps"], lr=HYPER["lr"], eps=HYPER["eps"])
    c.huber_delta = 10.0
    if c.huber:
        _, _, fw = ref.train_batch(c.P, c.M, c.PT, c.MT, c.batch, dtype=torch.float64, update=False, **kw)
        c.huber_delta = float(fw["err"].abs()[fw["mask"] > 0].median())
    kw["huber_delta"] = c.huber_delta
    c.kw = kw
    c.P64, c.M64, c.info64 = ref.train_batch(c.P, c.M, c.PT, c.MT, c.batch, dtype=torch.float64, **kw)
    c.P32, c.M32, c.info32 = ref.train_batch(c.P, c.M, c.PT, c.MT, c.batch, dtype=torch.float32, **kw)
    # behavior Q over the episode's stacked rows [T+1, N*B, A] in float64 and float32
    xs = ref.stack_agents(torch.tensor(c.batch["obs"]))
    with torch.no_grad():
        c.q64, _ = ref.agent_q_seq(c.P, xs, dtype=torch.float64)
        c.q32, _ = ref.agent_q_seq(c.P, xs, dtype=torch.float32)
    top2 = c.q64.topk(2, dim=-1)[0]
    c.top2_gap = float((top2[..., 0] - top2[..., 1]).min())
    assert c.top2_gap >= MIN_TOP2_GAP, f"{cid}: top-2 gap {c.top2_gap:.3g} of the behavior Q; choose another seed"
    return c


def q_units(q, q64, rtol=1e-4, atol=1e-5):
    """u(q) = max |q - q64| / (rtol |q64| + atol): the Q error in units of the project's Q tolerance."""
    q, q64 = np.asarray(q, np.float64), np.asarray(q64, np.float64)
    return float((np.abs(q - q64) / (rtol * np.abs(q64) + atol)).max())


__all__ = ["A", "D", "CASES", "HYPER", "build_case", "center_bias", "grad_keys", "huber_fraction_above", "q_units",
           "rel_l2"]
