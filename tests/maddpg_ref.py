"""Plain torch restatement of one MADDPG / MATD3 update (maddpg.py:90-249 of the reference's offpolicy fork, shared
cent_obs, discrete actions): autograd, clip_grad_norm_, torch.optim.Adam, a Dc-wide feature LayerNorm, critic heads
outside the parameters, mask-and-replace of one agent's action columns, straight-through Gumbel-softmax with injected
noise. Run in float64 as the reference and in float32 as the summation-noise yardstick. Also the case table."""
import functools
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

A, H = 5, 64
TRUNK = ("ln0_w", "ln0_b", "W1", "b1", "ln1_w", "ln1_b", "W2", "b2", "ln2_w", "ln2_b")
Case = namedtuple("Case", "id N B D td3 per huber max_norm seed")
CASES = [
    Case("one_row", 1, 1, 47, False, False, False, 10.0, 1),
    Case("b15", 2, 15, 47, False, True, False, 10.0, 2),
    Case("b16", 2, 16, 47, False, True, False, 10.0, 3),
    Case("b17_clip", 2, 17, 47, False, True, False, 0.02, 4),
    Case("switch_td3_huber", 2, 37, 3, True, False, True, 10.0, 5),
    Case("d94_td3_per", 2, 19, 94, True, True, False, 10.0, 6),
    Case("n8", 8, 19, 47, False, False, False, 10.0, 7),
    Case("second_tile", 2, 256 * 16 + 5, 3, True, False, False, 10.0, 8),
]
PERIOD = 37
GAMMA, LR, OPTI_EPS, PER_EPS, DELTA = 0.99, 5e-4, 1e-5, 1e-6, 1.5


def random_net(rng, din, nout, head_scale):
    p = {"ln0_w": 1 + 0.1 * rng.standard_normal(din), "ln0_b": 0.1 * rng.standard_normal(din),
         "W1": rng.standard_normal((H, din)) * (1.4 / np.sqrt(din)), "b1": 0.1 * rng.standard_normal(H),
         "W2": rng.standard_normal((H, H)) * (1.4 / np.sqrt(H)), "b2": 0.1 * rng.standard_normal(H),
         "Wo": rng.standard_normal((nout, H)) * head_scale, "bo": 0.1 * rng.standard_normal(nout)}
    for k in ("ln1", "ln2"):
        p[k + "_w"], p[k + "_b"] = 1 + 0.1 * rng.standard_normal(H), 0.1 * rng.standard_normal(H)
    return {k: v.astype(np.float32) for k, v in p.items()}


def perturbed(rng, p, keys):
    return {k: (v + 0.05 * rng.standard_normal(v.shape).astype(np.float32) if k in keys else v.copy())
            for k, v in p.items()}


@functools.lru_cache(maxsize=None)
def make_case(cid):
    """Parameters (actor, target actor, critic, target critic with heads of its own), the batch and the noise."""
    c = next(x for x in CASES if x.id == cid)
    rng = np.random.default_rng(c.seed)
    # past PERIOD rows the observations, stored actions and noise repeat the first PERIOD transitions (period coprime
    # to the 16-row tile): millions of independent ReLU inputs and argmax gaps cannot all keep their margins, 37 rows'
    # worth can. Rewards, dones, weights and valid, which touch no ReLU and no argmax, are drawn per row.
    N, B, Bf, D, nq, full = c.N, min(c.B, PERIOD), c.B, c.D, 2 if c.td3 else 1, np.arange(c.B) % PERIOD
    actor, critic = random_net(rng, D, A, 0.5), random_net(rng, N * (D + A), nq, 0.3)
    nets = {"actor": actor, "target_actor": perturbed(rng, actor, TRUNK + ("Wo", "bo")), "critic": critic,
            "target_critic": dict(perturbed(rng, critic, TRUNK), Wo=random_net(rng, 4, nq, 0.3)["Wo"])}
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    obs, nobs = f(N, B, D)[:, full], f(N, B, D)[:, full]
    valid = (rng.random((N, Bf, 1)) > 0.3).astype(np.float32)
    valid[:, 0] = 1.0
    valid[-1, Bf // 2] = 0.0 if N * Bf > 1 else 1.0
    de = (rng.random((Bf, 1)) > 0.5).astype(np.float32)
    if Bf > 1:
        de[0], de[1] = 0.0, 1.0
    batch = {"obs": obs, "nobs": nobs, "cent_obs": obs.transpose(1, 0, 2).reshape(Bf, N * D).copy(),
             "cent_nobs": nobs.transpose(1, 0, 2).reshape(Bf, N * D).copy(),
             "acts": np.eye(A, dtype=np.float32)[rng.integers(0, A, (N, B))][:, full], "rewards": f(N, Bf, 1),
             "dones_env": de, "valid": valid,
             "isw": (0.5 + rng.random(Bf)).astype(np.float32) if c.per else None}
    u = lambda: rng.random((N, B, A)).astype(np.float32)[:, full]
    gum = [(-np.log(-np.log(x + np.float32(1e-20)) + np.float32(1e-20))).astype(np.float32) for x in (u(), u())]
    return c, nets, batch, gum[0], gum[1]


def ln(x, w, b):
    return F.layer_norm(x, (x.shape[-1],), w, b, 1e-5)


def net(p, x, kinks=None):
    x = ln(x, p["ln0_w"], p["ln0_b"])
    for i in ("1", "2"):
        z = x @ p["W" + i].T + p["b" + i]
        if kinks is not None:
            kinks.append(float(z.detach().abs().min()))
        x = ln(torch.relu(z), p["ln" + i + "_w"], p["ln" + i + "_b"])
    return x @ p["Wo"].T + p["bo"]


def top2_gap(z):
    t = z.detach().topk(2, -1).values
    return float((t[..., 0] - t[..., 1]).min())


def step(params, keys, loss, max_norm):
    """backward, clip_grad_norm_, Adam: (gradients before the clip, norm, parameters after the step)."""
    ps = [params[k] for k in keys]
    grads = torch.autograd.grad(loss, ps)
    for p, g in zip(ps, grads):
        p.grad = g.clone()
    norm = torch.nn.utils.clip_grad_norm_(ps, max_norm)
    torch.optim.Adam(ps, lr=LR, eps=OPTI_EPS).step()
    return dict(zip(keys, grads)), float(norm), {k: params[k].detach().clone() for k in keys}


def update(cid, dtype=torch.float64, stale_critic=False, delta=DELTA):
    """One update. stale_critic: the actor pass reads the critic from BEFORE its Adam step (what the reference does
    not do). Returns losses, norms, priorities, gradients, stepped parameters and the preconditions' margins."""
    c, nets, batch, g, tg = make_case(cid) if isinstance(cid, str) else cid       # a case id, or a case itself
    T = lambda x: None if x is None else torch.tensor(x, dtype=dtype)
    P = {n: {k: T(v).requires_grad_(n in ("actor", "critic") and k in TRUNK + (("Wo", "bo") if n == "actor" else ()))
             for k, v in p.items()} for n, p in nets.items()}
    b = {k: T(v) for k, v in batch.items()}
    g, tg = T(g), T(tg)
    N, B = c.N, c.B
    kinks, gaps, out = [], [], {}
    with torch.no_grad():
        nact = []
        for n in range(N):
            z = net(P["target_actor"], b["nobs"][n], kinks) + (tg[n] if c.td3 else 0)
            gaps.append(top2_gap(z))
            nact.append(F.one_hot(z.argmax(-1), A).to(dtype) if c.td3 else (z == z.max(-1, keepdim=True)[0]).to(dtype))
        nq = net(P["target_critic"], torch.cat([b["cent_nobs"]] + nact, -1), kinks).min(-1, keepdim=True)[0]
        tgt = b["rewards"][0] + GAMMA * (1 - b["dones_env"]) * nq
    stored = torch.cat([b["cent_obs"]] + list(b["acts"]), -1)
    err = tgt - net(P["critic"], stored, kinks)                       # [B, nq]
    f = (torch.where(err.abs() <= delta, err ** 2 / 2, delta * (err.abs() - delta / 2)) if c.huber else err ** 2)
    w = b["isw"].view(-1, 1) if c.per else torch.ones(B, 1, dtype=dtype)
    closs = (f * w).mean(0).sum()
    out["prio"] = (err.detach().abs().mean(-1) + PER_EPS).numpy() if c.per else None
    out["huber_share"] = float((err.detach().abs() > delta).double().mean())
    old = {k: v.detach().clone() for k, v in P["critic"].items()}
    out["critic_grad"], out["critic_grad_norm"], out["critic_new"] = step(P["critic"], TRUNK, closs, c.max_norm)
    out["critic_loss"] = float(closs.detach())
    C = old if stale_critic else {k: v.detach() for k, v in P["critic"].items()}
    aloss = 0
    for i in range(N):
        z = net(P["actor"], b["obs"][i], kinks) + g[i]
        gaps.append(top2_gap(z))
        y = torch.softmax(z, -1)
        hard = F.one_hot(z.argmax(-1), A).to(dtype) + (y - y.detach())      # exact one-hot forward, d hard := d y
        x = torch.cat([b["cent_obs"]] + [hard if n == i else b["acts"][n] for n in range(N)], -1)
        aloss = aloss - (net(C, x, kinks)[:, :1] * b["valid"][i]).sum()
    aloss = aloss / b["valid"].sum()
    out["actor_grad"], out["actor_grad_norm"], out["actor_new"] = step(P["actor"], TRUNK + ("Wo", "bo"), aloss,
                                                                       c.max_norm)
    out["actor_loss"] = float(aloss.detach())
    out["kink_margin"], out["top2_gap"] = min(kinks), min(gaps) if A > 1 else np.inf
    return out


@functools.lru_cache(maxsize=None)
def reference(cid):
    """(float64 update, float32 update) of a case, computed once."""
    return update(cid, torch.float64), update(cid, torch.float32)


def rel_l2(x, ref):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(x - ref) / max(np.linalg.norm(ref), 1e-300))
