"""Restatement of MAPPO with a centralized critic (use_centralized_V) from oracle.mappo's primitives.

The critic's input is share_obs, derived here from obs exactly as the reference's obs_sharing does
(mappo/runner/shared/base_runner.py:155-161): the env's N agent observations concatenated, the same vector for
every agent. Everything else is oracle.mappo's R_MAPPO.train (ppo_train) with the critic evaluated on the
share_obs chunks. A plain helper module (not a conftest): the f32 / f64 yardstick of tests/test_mappo_cv_oracle.py
and tests/test_gpu_mappo_cv.py for shapes the golden fixtures (tests/golden/mappo_cv_*.npz) do not cover.
"""
import numpy as np
import torch

from oracle import mappo as om


def share_obs(obs):
    """[..., E, N, D] -> [..., E, N, N*D]."""
    obs = np.asarray(obs)
    *lead, E, N, D = obs.shape
    return np.ascontiguousarray(np.broadcast_to(obs.reshape(*lead, E, 1, N * D), (*lead, E, N, N * D)))


def case(fx, name):
    """The entries of one case ('n2' / 'n8') of a mappo_cv_*.npz fixture."""
    return {k[len(name) + 1:]: v for k, v in fx.items() if k.startswith(name + ".")}


def nets(fx, prefix=""):
    sd = {k[len(prefix):]: fx[k] for k in fx if k.startswith(prefix)}
    return om.net_from_state(sd, "actor.", "actor"), om.net_from_state(sd, "critic.", "critic")


def train_inputs(fx):
    """(PA, PC, data, vn0, n_chunks) of a mappo_cv_train case."""
    PA, PC = nets(fx, "before.")
    data = {k[5:]: fx[k] for k in fx if k.startswith("data.")}
    vn0 = (float(fx["vn0.running_mean"][0]), float(fx["vn0.running_mean_sq"][0]), float(fx["vn0.debiasing_term"]))
    return PA, PC, data, vn0, int(fx["T"]) * int(fx["E"]) * int(fx["N"]) // int(fx["L"])


def get_actions_cv(PA, PC, obs, cent_obs, ha, hc, masks, actions):
    """R_MAPPOPolicy.get_actions(obs, cent_obs, ...) with the given actions."""
    logits, ha2 = om.net_step(PA, obs, ha, masks)
    v, hc2 = om.net_step(PC, cent_obs, hc, masks)
    lp = om.categorical(logits)[0].gather(-1, actions.long().view(-1, 1))
    return v, lp, ha2, hc2


def ppo_losses_cv(PA, PC, b, L, vn, clip=0.2, huber_delta=10.0):
    """om.ppo_losses with the critic on the share_obs chunks b['cent_obs']."""
    lp, ent = om.evaluate_chunks(PA, b["obs"], b["ha0"], b["masks"], L, "actor", b["actions"], b["active_masks"])
    v = om.evaluate_chunks(PC, b["cent_obs"], b["hc0"], b["masks"], L, "critic")
    m = b["active_masks"]
    ratio = torch.exp(lp - b["action_log_probs"])
    s1 = ratio * b["adv"]
    s2 = torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * b["adv"]
    pol = (-torch.sum(torch.min(s1, s2), dim=-1, keepdim=True) * m).sum() / m.sum()
    vpc = b["value_preds"] + (v - b["value_preds"]).clamp(-clip, clip)
    tgt = vn.normalize(b["returns"])
    vl = torch.max(om.huber(tgt - v, huber_delta), om.huber(tgt - vpc, huber_delta))
    return pol, ent, (vl * m).sum() / m.sum(), ratio


def ppo_train_cv(PA, PC, data, vn0, epochs, L, perms=None, dtype=torch.float32, lr=1e-4, eps=1e-5, max_norm=0.5,
                 value_loss_coef=0.5, entropy_coef=0.01, clip=0.2, huber_delta=10.0):
    """R_MAPPO.train (one minibatch per epoch) in ``dtype``; data in the reference layout [T(+1), E, N, ...] without
    share_obs; vn0 = (mean, mean_sq, debias). -> (record per epoch, PA2, PC2, vn)."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        npd = np.float64 if dtype == torch.float64 else np.float32
        d = {k: (v.astype(npd) if v.dtype in (np.float32, np.float64) else v) for k, v in data.items()}
        dc = dict(d, obs=share_obs(d["obs"]))
        PA = {k: torch.as_tensor(v).to(dtype) for k, v in PA.items()}
        PC = {k: torch.as_tensor(v).to(dtype) for k, v in PC.items()}
        vn = om.ValueNorm(*vn0)
        adv = om.normalized_advantages(d, vn)
        sa, sc, rec = {}, {}, []
        for ep in range(epochs):
            order = None if perms is None else perms[ep]
            b = om.chunk_batch(d, adv, L, order)
            b["cent_obs"] = om.chunk_batch(dc, adv, L, order)["obs"]
            pa = {k: v.detach().clone().requires_grad_(True) for k, v in PA.items()}
            pc = {k: v.detach().clone().requires_grad_(True) for k, v in PC.items()}
            vn.update(b["returns"])
            pol, ent, vloss, _ = ppo_losses_cv(pa, pc, b, L, vn, clip=clip, huber_delta=huber_delta)
            ga = torch.autograd.grad(pol - ent * entropy_coef, [pa[k] for k in om.NET_KEYS])
            gc = torch.autograd.grad(vloss * value_loss_coef, [pc[k] for k in om.NET_KEYS])
            ga, na = om.clip_grads(list(ga), max_norm)
            gc, nc = om.clip_grads(list(gc), max_norm)
            rec.append(dict(ga=dict(zip(om.NET_KEYS, ga)), gc=dict(zip(om.NET_KEYS, gc)), na=float(na), nc=float(nc),
                            pol=float(pol.detach()), ent=float(ent.detach()), vloss=float(vloss.detach())))
            PA = om.adam(PA, dict(zip(om.NET_KEYS, ga)), sa, lr, eps)
            PC = om.adam(PC, dict(zip(om.NET_KEYS, gc)), sc, lr, eps)
    finally:
        torch.set_default_dtype(old)
    return rec, PA, PC, vn


def unclipped_grads(rec, ep=0, max_norm=0.5):
    """{(net, key): gradient before clip_grad_norm_} of epoch ep of a ppo_train_cv record."""
    out = {}
    for n, tag, nk in ((0, "ga", "na"), (1, "gc", "nc")):
        coef = min(1.0, max_norm / (rec[ep][nk] + 1e-6))
        for k in om.NET_KEYS:
            out[(n, k)] = rec[ep][tag][k].double().numpy() / coef
    return out


def train_outputs(rec, PA2, PC2, vn2):
    """Post-train parameters and the train() log (R_MAPPO.train averages the per-epoch losses / norms)."""
    out = {("actor", k): PA2[k].double().numpy() for k in om.NET_KEYS}
    out.update({("critic", k): PC2[k].double().numpy() for k in om.NET_KEYS})
    E = len(rec)
    for key, f in (("value_loss", "vloss"), ("policy_loss", "pol"), ("dist_entropy", "ent"),
                   ("actor_grad_norm", "na"), ("critic_grad_norm", "nc")):
        out[key] = np.array(sum(r[f] for r in rec) / E)
    out["vn_mean"] = vn2.m.double().numpy()
    out["vn_mean_sq"] = vn2.msq.double().numpy()
    return out


def fp32_spread(f, n_chunks):
    """f(dtype, perms) -> {name: array}; -> (f64 values, {name: fp32 spread}): per tensor
    max(|fp32 chunk order - fp32 permuted order|, |fp32 - f64|, 2^-23 max|f64|), the distance two legitimate fp32
    evaluations of the same sums land from each other and from the exact value (tests/test_gpu_mappo.py)."""
    a = f(torch.float32, None)
    b = f(torch.float32, np.random.default_rng(123).permutation(n_chunks)[None].repeat(64, 0))
    c = f(torch.float64, None)
    sp = {}
    for k in c:
        x, y, z = (np.asarray(v[k], np.float64) for v in (a, b, c))
        sp[k] = max(np.abs(x - y).max(), np.abs(x - z).max(), 2.0 ** -23 * np.abs(z).max(), 1e-30)
    return c, sp
