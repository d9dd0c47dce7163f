"""Plain-torch restatement (autograd, no hand-written backward) of one R_MADDPG / R_MATD3 update
(offpolicy/algorithms/r_maddpg/r_maddpg.py:114-331), the case table of tests/test_gpu_rmaddpg.py and its seeded inputs.
float64 is the reference, float32 the noise yardstick."""
import functools
import os
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

A, H, GAMMA, LR, OPTI_EPS, PER_EPS, NU, DELTA = 5, 64, 0.99, 5e-4, 1e-5, 1e-6, 0.9, 1.0
KEYS = ["ln0_w", "ln0_b", "W1", "b1", "ln1_w", "ln1_b", "W2", "b2", "ln2_w", "ln2_b", "Wih", "Whh", "bih", "bhh",
        "lnr_w", "lnr_b", "Wo", "bo"]
Case = namedtuple("Case", "N D T B td3 per huber max_norm seed")
CASES = {
    "t1": Case(2, 3, 1, 1, False, False, False, 10.0, 2),       # no recurrence, one row
    "sw": Case(2, 3, 4, 5, True, False, True, 10.0, 2),         # Dc 16, partial tile
    "ck": Case(2, 47, 6, 17, False, True, False, 0.05, 20),     # Dc 104, two row tiles, clip active on both nets
    "d94": Case(2, 94, 5, 33, True, True, False, 10.0, 4),      # Dc 198, three tiles
    "n3": Case(3, 47, 7, 6, False, False, True, 10.0, 5),       # N B = 18, odd agent count
    "wide": Case(8, 47, 3, 4, True, True, False, 10.0, 6),      # Dc 416, the limit
    "long": Case(2, 47, 40, 2, False, True, True, 10.0, 7),     # BPTT depth
}
# recordings of the reference's own R_MADDPG / R_MATD3 (tests/golden/make_golden_rmaddpg.py): N 2, D 47, T 4, B 5
FIXTURES = {"rmaddpg": Case(2, 47, 4, 5, False, True, False, 10.0, 0),
            "rmatd3": Case(2, 47, 4, 5, True, False, True, 10.0, 0)}
ALL = dict(CASES, **FIXTURES)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TRUNK_REF = {
    "ln0_w": "rnn.feature_norm.weight", "ln0_b": "rnn.feature_norm.bias", "W1": "rnn.mlp.fc1.0.weight",
    "b1": "rnn.mlp.fc1.0.bias", "ln1_w": "rnn.mlp.fc1.2.weight", "ln1_b": "rnn.mlp.fc1.2.bias",
    "W2": "rnn.mlp.fc2.0.0.weight", "b2": "rnn.mlp.fc2.0.0.bias", "ln2_w": "rnn.mlp.fc2.0.2.weight",
    "ln2_b": "rnn.mlp.fc2.0.2.bias", "Wih": "rnn.rnn.rnn.weight_ih_l0", "Whh": "rnn.rnn.rnn.weight_hh_l0",
    "bih": "rnn.rnn.rnn.bias_ih_l0", "bhh": "rnn.rnn.rnn.bias_hh_l0", "lnr_w": "rnn.rnn.norm.weight",
    "lnr_b": "rnn.rnn.norm.bias"}


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def target_offsets(sds, seed):
    """The seeded offsets of the fixtures' target nets: {net: {state-dict name: array}}, names in sorted order."""
    rng = np.random.default_rng(seed)
    return {n: {k: (0.02 * rng.standard_normal(np.shape(sd[k]))).astype(np.float32) for k in sorted(sd)}
            for n, sd in sorted(sds.items())}


def from_ref(sd, net, prefix=""):
    """Reference names -> KEYS, float64; the critic's q_outs.h heads stacked into Wo / bo."""
    sd = {k[len(prefix):]: torch.as_tensor(np.asarray(v), dtype=torch.float64) for k, v in sd.items()
          if k.startswith(prefix)}
    p = {k: sd[n] for k, n in TRUNK_REF.items() if n in sd}
    if net == "actor":
        p["Wo"], p["bo"] = sd["act.action_out.weight"], sd["act.action_out.bias"]
    else:
        heads = sorted(k for k in sd if k.startswith("q_outs.") and k.endswith("weight"))
        p["Wo"] = torch.cat([sd[k] for k in heads])
        p["bo"] = torch.cat([sd[k.replace("weight", "bias")] for k in heads])
    return p


@functools.lru_cache(None)
def load_fixture(name):
    """(case inputs as make_case gives them, the npz, the live and target state dicts under the reference's names)."""
    z = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    assert np.allclose(z["hyper"], [GAMMA, LR, OPTI_EPS, ALL[name].max_norm, DELTA, PER_EPS, NU])
    sds = {n: {k[len(n) + 1:]: z[k].astype(np.float32) for k in z if k.startswith(n + ".")} for n in ("actor", "critic")}
    off = target_offsets(sds, int(z["target_seed"]))
    tsd = {n: {k: v + off[n][k] for k, v in sds[n].items()} for n in sds}
    P = {"actor": from_ref(sds["actor"], "actor"), "critic": from_ref(sds["critic"], "critic"),
         "target_actor": from_ref(tsd["actor"], "actor"), "target_critic": from_ref(tsd["critic"], "critic")}
    t64 = lambda k: torch.as_tensor(z[k], dtype=torch.float64)
    batch = (t64("obs"), t64("share_obs"), t64("acts"), t64("rewards"), t64("dones"), t64("dones_env"), None,
             t64("is_weight") if "is_weight" in z else None, np.arange(ALL[name].B))
    return (P, batch, t64("gumbel"), t64("target_gumbel")), z, sds, tsd


def net(g, din, nout):
    """One trunk net with every tensor away from its init value; heads at unit scale."""
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    shp = {"ln0_w": (din,), "ln0_b": (din,), "W1": (H, din), "b1": (H,), "W2": (H, H), "b2": (H,), "Wih": (3 * H, H),
           "Whh": (3 * H, H), "bih": (3 * H,), "bhh": (3 * H,), "Wo": (nout, H), "bo": (nout,)}
    p = {}
    for k in KEYS:
        s = shp.get(k, (H,))
        if len(s) == 2:
            p[k] = r(*s) * (1.0 if k == "Wo" else 1.4) / np.sqrt(s[1])
        else:
            p[k] = (1.0 if k.endswith("_w") else 0.0) + 0.1 * r(*s)
    return p


@functools.lru_cache(None)
def make_case(cid):
    """(params {actor, critic, target_actor, target_critic}, batch tuple, gumbel, target_gumbel), float64 on the CPU."""
    if cid in FIXTURES:
        return load_fixture(cid)[0]
    c = CASES[cid]
    g = torch.Generator().manual_seed(1000 + c.seed)
    N, D, T, B = c.N, c.D, c.T, c.B
    P = {"actor": net(g, D, A), "critic": net(g, N * (D + A), 2 if c.td3 else 1)}
    for k in ("actor", "critic"):   # targets: perturbed copies
        P["target_" + k] = {n: v + 0.05 * v.abs().mean() * torch.randn(v.shape, generator=g, dtype=torch.float64)
                            for n, v in P[k].items()}
    obs = torch.randn(N, T + 1, B, D, generator=g, dtype=torch.float64)
    share = obs.permute(1, 2, 0, 3).reshape(T + 1, B, N * D).clone()
    acts = F.one_hot(torch.randint(0, A, (N, T, B), generator=g), A).double()
    rew = 0.6 * torch.randn(N, T, B, 1, generator=g, dtype=torch.float64)
    de = torch.zeros(T, B, 1, dtype=torch.float64)
    for b in range(B):   # never ends | ends mid-way | ends at t = 0
        if b % 3:
            de[(T // 2 if b % 3 == 1 else 0):, b] = 1.0
    dones = de.unsqueeze(0).repeat(N, 1, 1, 1)
    dones[N - 1, T // 2:, 0] = 1.0      # one agent of the episode that never ends dies mid-way
    isw = (0.5 + torch.rand(B, generator=g, dtype=torch.float64)) if c.per else None
    gum = -torch.log(-torch.log(torch.rand(2, N, T, B, A, generator=g, dtype=torch.float64)))
    return P, (obs, share, acts, rew, dones, de, None, isw, np.arange(B)), gum[0], gum[1]


def front(p, x):
    x = F.layer_norm(x, x.shape[-1:], p["ln0_w"], p["ln0_b"])
    x = F.layer_norm(F.relu(F.linear(x, p["W1"], p["b1"])), (H,), p["ln1_w"], p["ln1_b"])
    return F.layer_norm(F.relu(F.linear(x, p["W2"], p["b2"])), (H,), p["ln2_w"], p["ln2_b"])


def cell(p, x, h):
    gi, gh = F.linear(front(p, x), p["Wih"], p["bih"]), F.linear(h, p["Whh"], p["bhh"])
    r, z = torch.sigmoid(gi[..., :H] + gh[..., :H]), torch.sigmoid(gi[..., H:2 * H] + gh[..., H:2 * H])
    n = torch.tanh(gi[..., 2 * H:] + r * gh[..., 2 * H:])
    return (1 - z) * n + z * h


def out(p, h):
    return F.linear(F.layer_norm(h, (H,), p["lnr_w"], p["lnr_b"]), p["Wo"], p["bo"])


def run(p, xs):
    h, ys = xs.new_zeros(xs.shape[1], H), []
    for x in xs:
        h = cell(p, x, h)
        ys.append(out(p, h))
    return torch.stack(ys)


def gap(z):
    top = z.topk(2, -1).values
    return float((top[..., 0] - top[..., 1]).min())


def step(p, max_norm):
    """clip_grad_norm_ + the first Adam step; returns (unclipped gradients, pre-clip norm, stepped parameters)."""
    grads = {k: v.grad.clone() for k, v in p.items()}
    opt = torch.optim.Adam(list(p.values()), lr=LR, eps=OPTI_EPS)
    norm = torch.nn.utils.clip_grad_norm_(list(p.values()), max_norm)
    opt.step()
    return grads, float(norm), {k: v.detach().clone() for k, v in p.items()}


@functools.lru_cache(None)
def update(cid, dtype=torch.float64, actor=True):
    c = ALL[cid]
    P, batch, gum, tgum = make_case(cid)
    cast = lambda t: t.to(dtype)
    PA, PC = ({k: cast(v).clone().requires_grad_() for k, v in P[n].items()} for n in ("actor", "critic"))
    PAT, PCT = ({k: cast(v) for k, v in P["target_" + n].items()} for n in ("actor", "critic"))
    obs, share, acts, rew, dones, de, _, isw, _ = batch
    obs, share, acts, rew, dones, de, gum, tgum = (cast(x) for x in (obs, share, acts, rew, dones, de, gum, tgum))
    N, D, T, B = c.N, c.D, c.T, c.B
    o = {}
    seq = lambda a: a.permute(1, 2, 0, 3).reshape(a.shape[1], B, -1)          # [N, L, B, A] -> [L, B, N A]
    with torch.no_grad():   # 1. target actions, 2. target Q
        lt = run(PAT, obs.permute(1, 0, 2, 3).reshape(T + 1, N * B, D))[1:].reshape(T, N, B, A).permute(1, 0, 2, 3)
        z = lt + tgum if c.td3 else lt
        o["gap_target"] = gap(z)
        nact = F.one_hot(z.argmax(-1), A).to(dtype) if c.td3 else (lt == lt.max(-1, keepdim=True).values).to(dtype)
        x, xn = torch.cat([share[:-1], seq(acts)], -1), torch.cat([share[1:], seq(nact)], -1)
        h, nq = x.new_zeros(B, H), []
        for t in range(T):
            h = cell(PCT, x[t], h)
            nq.append(out(PCT, cell(PCT, xn[t], h)).min(-1, keepdim=True).values)
        curr = torch.cat([torch.zeros_like(de[:1]), de[:-1]])
        target = (rew[0] + GAMMA * (1 - de) * torch.stack(nq)) * (1 - curr)
    err = run(PC, x) * (1 - curr) - target                                     # 3. critic loss
    f = torch.where(err.abs() <= DELTA, err ** 2 / 2, DELTA * (err.abs() - DELTA / 2)) if c.huber else err ** 2
    w = cast(isw) if c.per else torch.ones(B, dtype=dtype)
    loss = (f.sum(0) * w[:, None]).sum() / (1 - curr).sum()
    loss.backward()
    o["err"], o["mask"] = err.detach()[(1 - curr).expand_as(err) > 0], 1 - curr
    ae = err.detach().abs()
    o["prio"] = (((1 - NU) * ae.mean(0) + NU * ae.max(0).values + PER_EPS).mean(-1) + PER_EPS) if c.per else None
    o["critic_loss"] = float(loss.detach())
    o["critic_grad"], o["critic_grad_norm"], o["critic"] = step(PC, c.max_norm)
    if not actor:
        return o
    for v in PC.values():                                                      # 4. actor loss
        v.requires_grad_(False)
    y = torch.softmax(run(PA, obs[:, :-1].permute(1, 0, 2, 3).reshape(T, N * B, D)) + gum.permute(1, 0, 2, 3).reshape(T, N * B, A), -1)
    o["gap_actor"] = gap(y.detach().log())
    hard = (F.one_hot(y.argmax(-1), A).to(dtype) - y).detach() + y
    hard = hard.reshape(T, N, B, A)
    acurr = torch.cat([torch.zeros_like(dones[:, :1]), dones[:, :-1]], 1)      # [N, T, B, 1]
    h, qs = x.new_zeros(B, H), 0.0
    for t in range(T):
        for i in range(N):
            xi = torch.cat([x[t, :, :N * D + i * A], hard[t, i], x[t, :, N * D + (i + 1) * A:]], -1)
            qs = qs + (out(PC, cell(PC, xi, h))[:, :1] * (1 - acurr[i, t])).sum()
        h = cell(PC, x[t], h)
    aloss = -qs / (1 - acurr).sum()
    aloss.backward()
    o["actor_loss"] = float(aloss.detach())
    o["actor_grad"], o["actor_grad_norm"], o["actor"] = step(PA, c.max_norm)
    return o
