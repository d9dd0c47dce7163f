"""Restatement of feed-forward MAPPO (algorithm_name "mappo": no RNNLayer, minibatches over single rows) from
oracle.mappo's primitives, shared by tests/test_mappo_ff_cpu.py and tests/test_gpu_mappo_ff.py.

The reference (mappo/main.py:62-65, r_actor_critic.py:46,84,123,168,204, ramppo_network.py:245-261,
shared_buffer.py:159-219): the nets are the LN-MLP trunk x2 = LN2(ReLU(W2 LN1(ReLU(W1 LN0(obs) + b1)) + b2))
(mlp.py:31-55) followed directly by the head Wo x2 + bo -- no GRU and no post-GRU LayerNorm (that norm belongs to
RNNLayer, rnn.py:79); hidden states pass through untouched and the nets never read the masks. R_MAPPO.train draws,
per epoch, one torch.randperm of the T * E * N rows (row = t * E * N + e * N + n: reshape(-1) of [T, E, N]), cuts it
into train_batch_size slices of rows // train_batch_size (the remainder dropped) and runs one ppo_update per slice:
ValueNorm.update(return_batch), the losses over the slice's rows divided by the slice's active count,
clip_grad_norm_, Adam. Advantages are normalised once per train() over the whole buffer.

A net is a dict over FF_KEYS (the 12 tensors the reference's feed-forward nets hold). Tolerances: the rule of
tests/mappo_mb_ref.py's docstring (K_FP32 = 16 spreads of fp32 in order / fp32 shuffled within each minibatch / f64),
whose fp32_spread / assert_within / golden_grad are used as they are.
"""
import numpy as np
import torch

import mappo_cv_ref as cv
from oracle import mappo as om

RECURRENT_KEYS = ("Wih", "Whh", "bih", "bhh", "lnr_w", "lnr_b")
FF_KEYS = [k for k in om.NET_KEYS if k not in RECURRENT_KEYS]


def nets(fx, prefix=""):
    """(actor, critic) parameter dicts from reference-named arrays under ``prefix``."""
    def one(kind):
        return {k: torch.tensor(np.asarray(fx[f"{prefix}{kind}.{om.ref_name(k, kind)}"]), dtype=torch.float32)
                for k in FF_KEYS}
    return one("actor"), one("critic")


def net_out(P, obs):
    """Head output [R, O] of one feed-forward net."""
    f = om.layer_norm(obs, P["ln0_w"], P["ln0_b"])
    f = om.layer_norm(torch.relu(f @ P["W1"].t() + P["b1"]), P["ln1_w"], P["ln1_b"])
    f = om.layer_norm(torch.relu(f @ P["W2"].t() + P["b2"]), P["ln2_w"], P["ln2_b"])
    return f @ P["Wo"].t() + P["bo"]


def get_actions(PA, PC, obs, cent_obs=None, actions=None, u=None, deterministic=False):
    """R_MAPPOPolicy.get_actions without hiddens: the sample given (actions), drawn from u (the build's inverse CDF)
    or the mode (first argmax). -> values [R, 1], actions [R, 1], log-probs [R, 1]."""
    logits = net_out(PA, obs)
    v = net_out(PC, obs if cent_obs is None else cent_obs)
    logp_all, _ = om.categorical(logits)
    if actions is None:
        actions = logits.argmax(-1) if deterministic else om.sample_actions(logits, u)
    return v, actions.view(-1, 1), logp_all.gather(-1, actions.long().view(-1, 1))


def train_inputs(fx):
    """(PA, PC, data, vn0, rows) of a mappo_ff_train fixture."""
    PA, PC = nets(fx, "before.")
    data = {k[5:]: fx[k] for k in fx if k.startswith("data.")}
    vn0 = (float(fx["vn0.running_mean"][0]), float(fx["vn0.running_mean_sq"][0]), float(fx["vn0.debiasing_term"]))
    return PA, PC, data, vn0, int(fx["T"]) * int(fx["E"]) * int(fx["N"])


def row_batch(d, adv, rows, dc=None):
    """feed_forward_generator's batch of the listed rows (shared_buffer.py:180-219)."""
    T = d["rewards"].shape[0]
    flat = lambda x: x[:T].reshape(T * x.shape[1] * x.shape[2], *x.shape[3:])  # noqa: E731
    rows = np.asarray(rows)
    b = {k: torch.from_numpy(np.ascontiguousarray(flat(d[k])[rows]))
         for k in ("obs", "actions", "action_log_probs", "value_preds", "returns", "active_masks")}
    b["adv"] = torch.from_numpy(np.ascontiguousarray(flat(adv)[rows]))
    if dc is not None:
        b["cent_obs"] = torch.from_numpy(np.ascontiguousarray(flat(dc)[rows]))
    return b


def ppo_losses(PA, PC, b, vn, clip=0.2, huber_delta=10.0):
    """ramppo_network.py:103-200 on one minibatch of rows; vn already updated by the caller."""
    logp_all, ent = om.categorical(net_out(PA, b["obs"]))
    lp = logp_all.gather(-1, b["actions"].long().view(-1, 1))
    m = b["active_masks"]
    ent = (ent * m.view(-1)).sum() / m.sum()
    v = net_out(PC, b.get("cent_obs", b["obs"]))
    ratio = torch.exp(lp - b["action_log_probs"])
    s1 = ratio * b["adv"]
    s2 = torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * b["adv"]
    pol = (-torch.sum(torch.min(s1, s2), dim=-1, keepdim=True) * m).sum() / m.sum()
    vpc = b["value_preds"] + (v - b["value_preds"]).clamp(-clip, clip)
    tgt = vn.normalize(b["returns"])
    vl = torch.max(om.huber(tgt - v, huber_delta), om.huber(tgt - vpc, huber_delta))
    return pol, ent, (vl * m).sum() / m.sum(), ratio


def minibatches(perm, M):
    perm = np.asarray(perm)
    mbs = len(perm) // M
    return [perm[i * mbs:(i + 1) * mbs] for i in range(M)]


def ppo_train_ff(PA, PC, data, vn0, epochs, perms, M, dtype=torch.float32, shuffle=False, cent=False, updates=None,
                 lr=1e-4, eps=1e-5, max_norm=0.5, value_loss_coef=0.5, entropy_coef=0.01, clip=0.2, huber_delta=10.0):
    """R_MAPPO.train of the feed-forward nets with M minibatches per epoch in ``dtype``. data: the reference layout
    [T(+1), E, N, ...]; perms [epochs, T*E*N] row permutations (None: every epoch takes the rows in buffer order);
    vn0 = (mean, mean_sq, debias). shuffle: the rows of every minibatch in a fixed random order. cent: centralized
    critic on share_obs. updates: stop after that many. -> (record per update, PA2, PC2, vn)."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        npd = np.float64 if dtype == torch.float64 else np.float32
        d = {k: (v.astype(npd) if v.dtype in (np.float32, np.float64) else v) for k, v in data.items()}
        dc = cv.share_obs(d["obs"]) if cent else None
        PA = {k: torch.as_tensor(v).to(dtype) for k, v in PA.items() if k in FF_KEYS}
        PC = {k: torch.as_tensor(v).to(dtype) for k, v in PC.items() if k in FF_KEYS}
        vn = om.ValueNorm(*vn0)
        adv = om.normalized_advantages(d, vn)
        T, E, N = d["rewards"].shape[:3]
        rng = np.random.default_rng(123)
        sa, sc, rec = {}, {}, []
        for ep in range(epochs):
            for order in minibatches(np.arange(T * E * N) if perms is None else perms[ep], M):
                if updates is not None and len(rec) >= updates:
                    break
                if shuffle:
                    order = rng.permutation(order)
                b = row_batch(d, adv, order, dc)
                pa = {k: v.detach().clone().requires_grad_(True) for k, v in PA.items()}
                pc = {k: v.detach().clone().requires_grad_(True) for k, v in PC.items()}
                vn.update(b["returns"])
                pol, ent, vloss, ratio = ppo_losses(pa, pc, b, vn, clip=clip, huber_delta=huber_delta)
                ga = torch.autograd.grad(pol - ent * entropy_coef, [pa[k] for k in FF_KEYS])
                gc = torch.autograd.grad(vloss * value_loss_coef, [pc[k] for k in FF_KEYS])
                ga, na = om.clip_grads(list(ga), max_norm)
                gc, nc = om.clip_grads(list(gc), max_norm)
                rec.append(dict(ga=dict(zip(FF_KEYS, ga)), gc=dict(zip(FF_KEYS, gc)), na=float(na), nc=float(nc),
                                pol=float(pol.detach()), ent=float(ent.detach()), vloss=float(vloss.detach()),
                                ratio_sum=float(ratio.detach().double().sum()), rows=int(ratio.numel()),
                                active=float(b["active_masks"].sum())))
                PA = om.adam(PA, dict(zip(FF_KEYS, ga)), sa, lr, eps)
                PC = om.adam(PC, dict(zip(FF_KEYS, gc)), sc, lr, eps)
    finally:
        torch.set_default_dtype(old)
    return rec, PA, PC, vn


def train_outputs(rec, PA2, PC2, vn2):
    """Post-train parameters, ValueNorm state and the train() log (averages over the updates)."""
    out = {("actor", k): PA2[k].double().numpy() for k in FF_KEYS}
    out.update({("critic", k): PC2[k].double().numpy() for k in FF_KEYS})
    n = len(rec)
    for key, f in (("value_loss", "vloss"), ("policy_loss", "pol"), ("dist_entropy", "ent"),
                   ("actor_grad_norm", "na"), ("critic_grad_norm", "nc")):
        out[key] = np.array(sum(r[f] for r in rec) / n)
    out["vn_mean"] = vn2.m.double().numpy()
    out["vn_mean_sq"] = vn2.msq.double().numpy()
    out["ratio"] = np.array(sum(r["ratio_sum"] for r in rec) / sum(r["rows"] for r in rec))
    out["norms"] = np.array([x for r in rec for x in (r["na"], r["nc"])])
    return out


def update_grads(rec, updates, max_norm=0.5):
    """{(update, net, key): gradient before clip_grad_norm_} of the listed updates of a record."""
    out = {}
    for u in updates:
        for n, tag, nk in ((0, "ga", "na"), (1, "gc", "nc")):
            coef = min(1.0, max_norm / (rec[u][nk] + 1e-6))
            for k in FF_KEYS:
                out[(u, n, k)] = rec[u][tag][k].double().numpy() / coef
    return out
