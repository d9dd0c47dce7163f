"""Plain torch restatement of the feed-forward transition-batch QMix / VDN update (reference lines
offpolicy/algorithms/mqmix/mqmix.py:68-218, algorithm/mQMixPolicy.py:35-59, mq_mixer.py:80-126, utils/util.py:103-110),
gradients from autograd, clip_grad_norm_ and torch.optim.Adam. Run in float64 it is the reference of
tests/test_gpu_moffq.py, in float32 the yardstick for summation-order noise. Also the case table."""
import functools

import numpy as np
import torch

from minimarl.synth import gen_obs
from offq_cases import random_agent, random_mixer

H, A = 64, 5
AGENT_KEYS = ["ln0_w", "ln0_b", "W1", "b1", "ln1_w", "ln1_b", "W2", "b2", "ln2_w", "ln2_b", "Wo", "bo"]
HYPER = dict(gamma=0.99, lr=5e-4, eps=1e-5, per_eps=1e-6)
TB = 16                   # transitions per tile of csrc/moffq.hip
#           N   B   D   K  Hh  mixer   dQ     PER    huber  max_norm  seed
CASES = {
    "one_row": (1, 1, 47, 1, 1, "qmix", True, True, False, 10.0, 11),
    "tile_m1": (2, TB - 1, 47, 32, 64, "qmix", True, True, False, 10.0, 25),
    "tile":    (2, TB, 47, 32, 64, "qmix", True, True, False, 10.0, 34),
    "tile_p1": (2, TB + 1, 47, 32, 64, "qmix", True, True, False, 0.05, 52),      # clip active
    "blocks3": (3, 2 * TB + 5, 94, 5, 17, "qmix", False, True, True, 1e6, 64),    # clip inactive
    "d3_vdn":  (2, 20, 3, 0, 0, "vdn", False, False, True, 10.0, 61),
    "n8_k33":  (8, 19, 47, 33, 64, "qmix", True, True, False, 10.0, 72),
}
FIELDS = ("N", "B", "D", "K", "Hh", "mixer", "double_q", "use_per", "huber", "max_norm", "seed")


def ln(x, w, b):
    return torch.nn.functional.layer_norm(x, x.shape[-1:], w, b, 1e-5)


def agent_q(P, x, pre=None):
    """x [R, D] -> q [R, A]; pre collects the ReLU pre-activations."""
    z1 = ln(x, P["ln0_w"], P["ln0_b"]) @ P["W1"].t() + P["b1"]
    z2 = ln(torch.relu(z1), P["ln1_w"], P["ln1_b"]) @ P["W2"].t() + P["b2"]
    if pre is not None:
        pre += [z1, z2]
    return ln(torch.relu(z2), P["ln2_w"], P["ln2_b"]) @ P["Wo"].t() + P["bo"]


def mixer(M, q, s, K, pre=None):
    """q [B, N], s [B, S] -> Q_tot [B] (VDN when M is empty)."""
    if not M:
        return q.sum(-1)
    B, N = q.shape

    def two(k):
        z = s @ M[k + ".0.weight"].t() + M[k + ".0.bias"]
        if pre is not None:
            pre.append(z)
        return torch.relu(z) @ M[k + ".2.weight"].t() + M[k + ".2.bias"]

    w1 = two("hyper_w1").abs().view(B, N, K)
    b1 = (s @ M["hyper_b1.weight"].t() + M["hyper_b1.bias"]).view(B, 1, K)
    hid = torch.nn.functional.elu(q.view(B, 1, N) @ w1 + b1)
    return (hid @ two("hyper_w2").abs().view(B, K, 1) + two("hyper_b2").view(B, 1, 1)).view(B)


def update(c, dtype, huber_delta=None, step=True):
    """One train_policy_on_batch of case c in ``dtype``."""
    cast = lambda d: {k: d[k].to(dtype) for k in d}
    P = {k: torch.nn.Parameter(c.P[k].to(dtype).clone()) for k in AGENT_KEYS}
    M = {k: torch.nn.Parameter(v.to(dtype).clone()) for k, v in c.M.items()}
    PT, MT, b = cast({k: c.PT[k] for k in AGENT_KEYS}), cast(c.MT), {k: torch.tensor(v).to(dtype) for k, v in c.batch.items()}
    N, B = c.N, c.B
    rows = lambda x: x.reshape(N * B, -1)                      # agent-major stacking (mqmix.py:102-104)
    pre = []
    q = agent_q(P, rows(b["obs"]), pre)
    qa = q.gather(1, rows(b["acts"]).max(-1)[1].unsqueeze(-1)).view(N, B).t()
    with torch.no_grad():
        qn, qtn = agent_q(P, rows(b["nobs"])), agent_q(PT, rows(b["nobs"]))
        nq = (qtn.gather(1, qn.max(-1)[1].unsqueeze(-1))[:, 0] if c.double_q else qtn.max(-1)[0]).view(N, B).t()
        target = b["rewards"][0, :, 0] + (1 - b["dones_env"][:, 0]) * HYPER["gamma"] * mixer(MT, nq, b["cent_nobs"], c.K)
    qtot = mixer(M, qa, b["cent_obs"], c.K, pre)
    err = qtot - target
    out = {"q": q.detach(), "err": err.detach(), "min_pre": min(float(z.detach().abs().min()) for z in pre),
           "gap": min(float((t.topk(2, -1)[0] @ t.new_tensor([1.0, -1.0])).min() / t.abs().max()) for t in (qn, qtn, q.detach())),
           "prio": (err.detach().abs() + HYPER["per_eps"]) if c.use_per else None}
    if not step:
        return out
    d = huber_delta
    le = torch.where(err.abs() <= d, err ** 2 / 2, d * (err.abs() - d / 2)) if c.huber else err ** 2
    loss = (le * b["is_weight"]).mean() if c.use_per else le.mean()
    params = list(P.values()) + list(M.values())
    opt = torch.optim.Adam(params, lr=HYPER["lr"], eps=HYPER["eps"])
    loss.backward()
    out["grads"] = {k: v.grad.clone() for k, v in {**P, **M}.items()}
    out["grad_norm"] = float(torch.nn.utils.clip_grad_norm_(params, c.max_norm))
    opt.step()
    out.update(loss=float(loss.detach()), q_tot=float(qtot.detach().mean()), new={k: v.detach() for k, v in {**P, **M}.items()})
    return out


class Case:
    pass


@functools.lru_cache(maxsize=None)
def build_case(cid):
    """Inputs and both reference answers of one case (computed once per process; treat as read-only)."""
    c = Case()
    for k, v in zip(FIELDS, CASES[cid]):
        setattr(c, k, v)
    N, B, D = c.N, c.B, c.D
    qm = c.mixer == "qmix"
    c.P, c.PT = random_agent(c.seed, D), random_agent(c.seed + 1, D)      # the target net: its own seed
    c.M = random_mixer(c.seed, N, D, c.K, c.Hh) if qm else {}
    c.MT = random_mixer(c.seed + 1, N, D, c.K, c.Hh) if qm else {}
    rng = np.random.default_rng(c.seed + 2)
    obs, nobs = gen_obs(rng, (N, B, D)), gen_obs(rng, (N, B, D))
    dn = (rng.random((B, 1)) < 0.3).astype(np.float32)
    if B > 1:
        dn[0], dn[1] = 1.0, 0.0
    c.batch = {"obs": obs, "nobs": nobs, "cent_obs": obs.transpose(1, 0, 2).reshape(B, N * D).copy(),
               "cent_nobs": nobs.transpose(1, 0, 2).reshape(B, N * D).copy(),
               "acts": np.eye(A, dtype=np.float32)[rng.integers(0, A, (N, B))],
               "rewards": rng.standard_normal((N, B, 1)).astype(np.float32), "dones_env": dn,
               "is_weight": (0.5 + rng.random(B)).astype(np.float32)}
    # Huber: delta = the median |err| of the float64 forward, so both branches of the loss carry weight
    c.huber_delta = float(update(c, torch.float64, step=False)["err"].abs().median()) if c.huber else 10.0
    c.r64, c.r32 = update(c, torch.float64, c.huber_delta), update(c, torch.float32, c.huber_delta)
    return c
