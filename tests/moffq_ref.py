"""Plain torch restatement of the feed-forward transition-batch QMix / VDN update (reference lines
offpolicy/algorithms/mqmix/mqmix.py:68-218, algorithm/mQMixPolicy.py:35-59, mq_mixer.py:80-126, utils/util.py:103-110),
gradients from autograd, clip_grad_norm_ and torch.optim.Adam. Run in float64 it is the reference of
tests/test_gpu_moffq.py, in float32 the yardstick for summation-order noise. Also the case table."""
import functools
import os
import sys

import numpy as np
import torch

from minimarl.synth import gen_obs
from offq_cases import mixer_shapes, random_agent, random_mixer

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
UNFILTERED = tuple(CASES)   # the seven cases above: B plain draws. Every later case draws candidates and filters them.
GRID = 256 * TB           # transitions of one pass of the largest grid: past it a block walks a second tile
CASES.update({
    # a block walks 2 and 3 tiles: the partial's += of a later tile, loss / Q sums carried, LDS and scratch reused
    "walk2_vdn":    (2, GRID + 5, 3, 0, 0, "vdn", True, True, True, 10.0, 81),       # block 0: a full, then a ragged tile
    "walk3_qmix":   (2, 2 * GRID + TB + 3, 3, 4, 8, "qmix", True, True, False, 10.0, 83),  # block 0: 3, block 1: ragged third
    "walk2_d47":    (2, GRID + 15, 47, 32, 64, "qmix", False, True, True, 10.0, 85),
    "walk2_n3_d94": (3, GRID + 1, 94, 5, 17, "qmix", True, False, False, 10.0, 87),  # a one-row second tile
    # the mixer at its stated limits
    "k64_h128":     (3, 21, 47, 64, 128, "qmix", True, True, False, 10.0, 93),       # the [16][64] LDS tile's last column
    "h100":         (2, 17, 3, 7, 100, "qmix", True, True, False, 10.0, 94),         # a ragged second column pass
    "nk4096":       (64, 17, 3, 64, 8, "qmix", True, True, False, 10.0, 433),        # the scratch slice at full size
    "own_state":    (2, 18, 47, 32, 64, "qmix", True, True, False, 10.0, 100),       # state_dim 29 != N D
})
STATE_DIM = {"own_state": 29}
# input edges (tests of their own, not in the case sweep)
EDGE_CASES = {
    "acts_edge":  (2, 19, 47, 32, 64, "qmix", True, True, False, 10.0, 101),
    "all_done":   (2, 19, 47, 32, 64, "qmix", True, True, False, 10.0, 106),
    "no_weights": (2, 18, 47, 32, 64, "qmix", True, False, True, 10.0, 105),
}
FIELDS = ("N", "B", "D", "K", "Hh", "mixer", "double_q", "use_per", "huber", "max_norm", "seed")
MIN_PRE, MIN_GAP, MAX_DROPPED = 2e-5, 2e-3, 0.15        # the candidate filter: twice the bars of the precondition test
STATE_IN = ("hyper_w1.0.weight", "hyper_w2.0.weight", "hyper_b1.weight", "hyper_b2.0.weight")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def acts_edge(b):
    """Action rows that are not one-hot: positive reals, an all-zero row (index 0) and a row with two equal maxima
    (the first wins, torch.max)."""
    rng = np.random.default_rng(7)
    b["acts"][:] = rng.random(b["acts"].shape).astype(np.float32)
    b["acts"][0, 0] = 0.0
    b["acts"][1, 1] = [0.25, 0.75, 0.5, 0.75, 0.0]
    b["acts"][1, 17] = [0.5, 0.5, 0.5, 0.5, 0.5]


def all_done(b):
    """The first tile's transitions all end their episode; the second tile is mixed."""
    b["dones_env"][:TB] = 1.0
    b["dones_env"][TB:, 0] = [0.0, 1.0, 0.0]


TWEAKS = {"acts_edge": acts_edge, "all_done": all_done}


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


def new_state(c, dtype):
    """Behavior parameters, target tensors and (made at the first step) the Adam instance of one trainer."""
    cast = lambda d: {k: d[k].to(dtype) for k in d}
    return {"P": {k: torch.nn.Parameter(c.P[k].to(dtype).clone()) for k in AGENT_KEYS},
            "M": {k: torch.nn.Parameter(v.to(dtype).clone()) for k, v in c.M.items()},
            "PT": cast({k: c.PT[k] for k in AGENT_KEYS}), "MT": cast(c.MT), "opt": None}


def update(c, dtype, huber_delta=None, step=True, state=None):
    """One train_policy_on_batch of case c in ``dtype``; ``state`` (new_state) carries a trainer over several."""
    st = new_state(c, dtype) if state is None else state
    P, M, PT, MT = st["P"], st["M"], st["PT"], st["MT"]
    b = {k: torch.tensor(v).to(dtype) for k, v in c.batch.items()}
    if b["cent_obs"].dim() == 3:                               # use_same_share_obs=False: agent 0's (mqmix.py:82-84)
        b["cent_obs"], b["cent_nobs"] = b["cent_obs"][0], b["cent_nobs"][0]
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
    out = {"q": q.detach(), "err": err.detach(), "target": target, "min_pre": min(float(z.detach().abs().min()) for z in pre),
           "gap": min(float((t.topk(2, -1)[0] @ t.new_tensor([1.0, -1.0])).min() / t.abs().max()) for t in (qn, qtn, q.detach())),
           "prio": (err.detach().abs() + HYPER["per_eps"]) if c.use_per else None}
    if not step:
        return out
    d = huber_delta
    le = torch.where(err.abs() <= d, err ** 2 / 2, d * (err.abs() - d / 2)) if c.huber else err ** 2
    loss = (le * b["is_weight"]).mean() if c.use_per else le.mean()
    params = list(P.values()) + list(M.values())
    if st["opt"] is None:
        st["opt"] = torch.optim.Adam(params, lr=HYPER["lr"], eps=HYPER["eps"])
    st["opt"].zero_grad()
    loss.backward()
    out["grads"] = {k: v.grad.clone() for k, v in {**P, **M}.items()}
    out["grad_norm"] = float(torch.nn.utils.clip_grad_norm_(params, c.max_norm))
    out["clipped"] = {k: v.grad.clone() for k, v in {**P, **M}.items()}
    st["opt"].step()
    out.update(loss=float(loss.detach()), q_tot=float(qtot.detach().mean()), new={k: v.detach() for k, v in {**P, **M}.items()})
    return out


class Case:
    same_share = True         # cent_obs [B, S] (False: [N, B, S], agent 0's slice is the state)
    dropped = 0.0             # share of the candidate transitions that the filter dropped


def mixer_of_state(seed, S, N, K, Hh):
    """random_mixer with a state width of its own (S != N D)."""
    g = torch.Generator().manual_seed(int(seed) + 1000)
    return {k: torch.randn(shp[:1] + ((S,) if k in STATE_IN else shp[1:]), generator=g) * 0.1
            for k, shp in mixer_shapes(N, 1, K, Hh).items()}


def draw(c, rng, B):
    """B transitions; the draws and their order are those of the first seven cases, the state of its own comes last."""
    N, D = c.N, c.D
    obs, nobs = gen_obs(rng, (N, B, D)), gen_obs(rng, (N, B, D))
    dn = (rng.random((B, 1)) < 0.3).astype(np.float32)
    share = lambda o: o.transpose(1, 0, 2).reshape(B, N * D).copy()
    b = {"obs": obs, "nobs": nobs, "cent_obs": share(obs), "cent_nobs": share(nobs),
         "acts": np.eye(A, dtype=np.float32)[rng.integers(0, A, (N, B))],
         "rewards": rng.standard_normal((N, B, 1)).astype(np.float32), "dones_env": dn,
         "is_weight": (0.5 + rng.random(B)).astype(np.float32)}
    if not c.same_share:
        b["cent_obs"], b["cent_nobs"] = gen_obs(rng, (N, B, c.S)), gen_obs(rng, (N, B, c.S))
    return b


def passes(c, b):
    """[B] bool, in float64: every ReLU argument of the behavior nets on obs / cent_obs at least MIN_PRE from 0 and
    every top-2 gap of q(obs), q(nobs), q_target(nobs) at least MIN_GAP of the largest |q| of its tensor."""
    N, B = c.N, b["obs"].shape[1]
    f64 = lambda d: {k: v.double() for k, v in d.items()}
    P, PT, M = f64(c.P), f64(c.PT), f64(c.M)
    rows = lambda x: torch.tensor(x).double().reshape(N * B, -1)
    per_b = lambda v: v.view(N, B).min(0)[0]
    with torch.no_grad():
        pre = []
        qs = [agent_q(P, rows(b["obs"]), pre), agent_q(P, rows(b["nobs"])), agent_q(PT, rows(b["nobs"]))]
        margin = per_b(torch.stack([z.abs().min(-1)[0] for z in pre]).min(0)[0])
        if M:
            s = torch.tensor(b["cent_obs"] if c.same_share else b["cent_obs"][0]).double()
            for net in ("hyper_w1", "hyper_w2", "hyper_b2"):
                z = s @ M[net + ".0.weight"].t() + M[net + ".0.bias"]
                margin = torch.minimum(margin, z.abs().min(-1)[0])
        gap = torch.stack([per_b((t.topk(2, -1)[0] @ t.new_tensor([1.0, -1.0])) / t.abs().max()) for t in qs]).min(0)[0]
    return ((margin >= MIN_PRE) & (gap >= MIN_GAP)).numpy()


def filtered(c, rng):
    """The first B of ceil(1.5 B) candidate transitions that pass ``passes``; c.dropped = the share that does not."""
    cand = draw(c, rng, -(-3 * c.B // 2))
    ok = passes(c, cand)
    c.dropped = float(1.0 - ok.mean())
    assert c.dropped <= MAX_DROPPED, f"{c.id}: {c.dropped:.3f} of the candidates dropped; choose another seed"
    keep = np.flatnonzero(ok)[:c.B]
    assert keep.size == c.B
    return {k: np.ascontiguousarray(v[:, keep] if v.ndim == 3 else v[keep]) for k, v in cand.items()}


@functools.lru_cache(maxsize=None)
def build_case(cid):
    """Inputs and both reference answers of one case (computed once per process; treat as read-only)."""
    c = Case()
    c.id = cid
    for k, v in zip(FIELDS, CASES[cid] if cid in CASES else EDGE_CASES[cid]):
        setattr(c, k, v)
    N, B, D = c.N, c.B, c.D
    qm = c.mixer == "qmix"
    c.S = STATE_DIM.get(cid, N * D)
    c.same_share = cid not in STATE_DIM
    c.P, c.PT = random_agent(c.seed, D), random_agent(c.seed + 1, D)      # the target net: its own seed
    mix = (lambda s: random_mixer(s, N, D, c.K, c.Hh)) if c.same_share else (lambda s: mixer_of_state(s, c.S, N, c.K, c.Hh))
    c.M = mix(c.seed) if qm else {}
    c.MT = mix(c.seed + 1) if qm else {}
    rng = np.random.default_rng(c.seed + 2)
    c.batch = draw(c, rng, B) if cid in UNFILTERED else filtered(c, rng)
    dn = c.batch["dones_env"]
    if B > 1:
        dn[0], dn[1] = 1.0, 0.0
    if cid in TWEAKS:
        TWEAKS[cid](c.batch)
    # Huber: delta = the median |err| of the float64 forward, so both branches of the loss carry weight
    c.huber_delta = float(update(c, torch.float64, step=False)["err"].abs().median()) if c.huber else 10.0
    c.r64, c.r32 = update(c, torch.float64, c.huber_delta), update(c, torch.float32, c.huber_delta)
    return c


@functools.lru_cache(maxsize=None)
def fixture_case(name):
    """tests/golden/moffq_<name>.npz (the reference's own train_policy_on_batch) as a Case, and the arrays the
    reference recorded (gradients after the clip). The target nets are rebuilt from the recorded seed."""
    from minimarl.moffq import AGENT_REF
    from minimarl.offq import MIXER_KEYS
    sys.path.insert(0, GOLD)
    from make_golden_offq import target_perturbation
    f = np.load(os.path.join(GOLD, f"moffq_{name}.npz"))
    d = {k: f[k] for k in f.files}
    c = Case()
    c.id = "fixture_" + name
    c.N, c.B, c.D, a, dq, per, hub, tseed = (int(x) for x in d["meta"])
    assert a == A
    c.double_q, c.use_per, c.huber = bool(dq), bool(per), bool(hub)
    gamma, lr, eps, c.max_norm, c.huber_delta, per_eps = (float(x) for x in d["hyper"])
    assert (gamma, lr, eps, per_eps) == tuple(HYPER[k] for k in ("gamma", "lr", "eps", "per_eps"))
    pert = target_perturbation([(k, d[k].shape) for k in f.files if k.startswith(("q.", "m."))], tseed)   # file order
    t = torch.tensor
    c.P = {k: t(d["q." + n]) for k, n in AGENT_REF.items()}
    c.PT = {k: t(d["q." + n] + pert["q." + n]) for k, n in AGENT_REF.items()}
    c.mixer = "qmix" if "m.hyper_b1.weight" in d else "vdn"
    c.K, c.Hh = (int(x) for x in d["mixer_dims"]) if c.mixer == "qmix" else (0, 0)
    c.M = {k: t(d["m." + k]) for k in MIXER_KEYS} if c.mixer == "qmix" else {}
    c.MT = {k: t(d["m." + k] + pert["m." + k]) for k in c.M}
    c.S = c.N * c.D
    c.batch = {k: d[k] for k in ("obs", "nobs", "cent_obs", "cent_nobs", "acts", "rewards", "dones_env")}
    c.batch["is_weight"] = d["is_weight"] if c.use_per else np.ones(c.B, np.float32)
    names = {**{k: "q." + n for k, n in AGENT_REF.items()}, **{k: "m." + k for k in c.M}}
    rec = {"grads": {k: d["grad." + n] for k, n in names.items()}, "new": {k: d["post." + n] for k, n in names.items()},
           "loss": float(d["loss"]), "grad_norm": float(d["grad_norm"]), "q_tot": float(d["q_tot"]),
           "prio": d["new_priorities"] if c.use_per else None, "files": list(f.files)}
    c.r64, c.r32 = update(c, torch.float64, c.huber_delta), update(c, torch.float32, c.huber_delta)
    return c, rec


SEQ = dict(N=2, D=3, K=4, Hh=8, Bs=(17, GRID + 5, 17), seed=121, tau=0.005)


@functools.lru_cache(maxsize=None)
def build_sequence():
    """Three updates of ONE float64 trainer (one Adam instance) at B = 17, 4101, 17 on different batches, a soft target
    update (utils/util.py:123-134) after the first and a hard one after the second. Each batch is filtered against the
    parameters it meets. Returns (the case that holds the initial parameters, [(case, answers)] per step)."""
    base = Case()
    base.id, base.N, base.D, base.K, base.Hh, base.seed = "seq", SEQ["N"], SEQ["D"], SEQ["K"], SEQ["Hh"], SEQ["seed"]
    base.mixer, base.double_q, base.use_per, base.huber, base.max_norm, base.huber_delta = "qmix", True, True, False, 10.0, 10.0
    base.S = base.N * base.D
    base.P, base.PT = random_agent(base.seed, base.D), random_agent(base.seed + 1, base.D)
    base.M = random_mixer(base.seed, base.N, base.D, base.K, base.Hh)
    base.MT = random_mixer(base.seed + 1, base.N, base.D, base.K, base.Hh)
    st = new_state(base, torch.float64)
    snap = lambda d: {k: v.detach().clone() for k, v in d.items()}
    steps = []
    for i, B in enumerate(SEQ["Bs"]):
        c = Case()
        c.__dict__.update(base.__dict__)
        c.id, c.B = f"seq{i}", B
        c.P, c.M, c.PT, c.MT = snap(st["P"]), snap(st["M"]), snap(st["PT"]), snap(st["MT"])
        c.batch = filtered(c, np.random.default_rng(base.seed + 2 + i))
        c.batch["dones_env"][0], c.batch["dones_env"][1] = 1.0, 0.0
        r = update(c, torch.float64, c.huber_delta, state=st)
        ans = {k: r[k] for k in ("loss", "grad_norm", "q_tot", "min_pre", "gap")}
        ans["new"] = snap(r["new"])
        with torch.no_grad():
            for tgt, src in ((st["PT"], st["P"]), (st["MT"], st["M"])):
                for k in tgt:
                    if i == 0:
                        tgt[k] = tgt[k] * (1.0 - SEQ["tau"]) + src[k].detach() * SEQ["tau"]
                    elif i == 1:
                        tgt[k] = src[k].detach().clone()
        ans["target"] = {**snap(st["PT"]), **snap(st["MT"])}
        steps.append((c, ans))
    return base, steps
