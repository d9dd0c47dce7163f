"""Restatement of R_MAPPO.train with train_batch_size > 1 (PPO minibatches over shuffled chunks) from oracle.mappo's
primitives, and the tolerance rule of the tests that use it.

The reference (mappo/algorithms/ramppo_network.py:245-271, runner/shared/shared_buffer.py:318-331): per epoch one
torch.randperm of the T*E*N/L chunks (numbered c = (e*N + n) * (T/L) + kc, the buffer cast to [E, N, T]), cut into
train_batch_size slices of n_chunks // train_batch_size chunks, the remainder dropped; each slice is one ppo_update:
ValueNorm.update(return_batch), the losses over the slice's rows divided by the slice's active count, clip_grad_norm_,
Adam. Advantages are normalised once per train() over the whole buffer. Here that is a loop over
``om.chunk_batch(data, adv, L, order=<slice>)``, ``vn.update``, ``om.ppo_losses`` (a centralized critic:
``mappo_cv_ref.ppo_losses_cv`` on the share_obs chunks), ``om.clip_grads`` and ``om.adam``. A plain helper module
(not a conftest), shared by tests/test_mappo_mb_cpu.py and tests/test_gpu_mappo_mb.py.

Tolerance (the project's rule, tests/test_gpu_mappo.py's docstring): the loop is run three times -- fp32 with the
chunks of each minibatch in the given order, fp32 with the chunks shuffled WITHIN each minibatch (membership fixed:
the same sums in another order), and float64. Per tensor the fp32 spread is
max(|fp32 - fp32 shuffled|, |fp32 - f64|, 2^-23 max|f64|), the distance two legitimate fp32 evaluations of the same
sums land from each other and from the exact value. A value under test must land within K_FP32 = 16 spreads of the
f64 value; against a golden value the golden's own distance to the f64 run is added. No other constant.
"""
import numpy as np
import torch

import mappo_cv_ref as cv
from oracle import mappo as om

K_FP32 = 16


def minibatches(perm, M):
    """One epoch's permutation -> its M chunk slices (the tail dropped), shared_buffer.py:328-331."""
    perm = np.asarray(perm)
    mbs = len(perm) // M
    return [perm[i * mbs:(i + 1) * mbs] for i in range(M)]


def ppo_train_mb(PA, PC, data, vn0, epochs, L, perms, M, dtype=torch.float32, shuffle=False, cent=False,
                 updates=None, lr=1e-4, eps=1e-5, max_norm=0.5, value_loss_coef=0.5, entropy_coef=0.01,
                 clip=0.2, huber_delta=10.0):
    """R_MAPPO.train with M minibatches per epoch in ``dtype``. data: the reference layout [T(+1), E, N, ...];
    perms [epochs, n_chunks] in the reference's chunk numbering; vn0 = (mean, mean_sq, debias). shuffle: the chunks
    of every minibatch in a fixed random order. cent: centralized critic on share_obs. updates: stop after that many.
    -> (record per update, PA2, PC2, vn); a record also holds 'ratio_sum' and 'rows'."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        npd = np.float64 if dtype == torch.float64 else np.float32
        d = {k: (v.astype(npd) if v.dtype in (np.float32, np.float64) else v) for k, v in data.items()}
        dc = dict(d, obs=cv.share_obs(d["obs"])) if cent else None
        PA = {k: torch.as_tensor(v).to(dtype) for k, v in PA.items()}
        PC = {k: torch.as_tensor(v).to(dtype) for k, v in PC.items()}
        vn = om.ValueNorm(*vn0)
        adv = om.normalized_advantages(d, vn)
        rng = np.random.default_rng(123)
        sa, sc, rec = {}, {}, []
        for ep in range(epochs):
            for order in minibatches(perms[ep], M):
                if updates is not None and len(rec) >= updates:
                    break
                if shuffle:
                    order = rng.permutation(order)
                b = om.chunk_batch(d, adv, L, order)
                pa = {k: v.detach().clone().requires_grad_(True) for k, v in PA.items()}
                pc = {k: v.detach().clone().requires_grad_(True) for k, v in PC.items()}
                vn.update(b["returns"])
                if cent:
                    b["cent_obs"] = om.chunk_batch(dc, adv, L, order)["obs"]
                    pol, ent, vloss, ratio = cv.ppo_losses_cv(pa, pc, b, L, vn, clip=clip, huber_delta=huber_delta)
                else:
                    pol, ent, vloss, ratio = om.ppo_losses(pa, pc, b, L, vn, clip=clip, huber_delta=huber_delta,
                                                           entropy_coef=entropy_coef)
                ga = torch.autograd.grad(pol - ent * entropy_coef, [pa[k] for k in om.NET_KEYS])
                gc = torch.autograd.grad(vloss * value_loss_coef, [pc[k] for k in om.NET_KEYS])
                ga, na = om.clip_grads(list(ga), max_norm)
                gc, nc = om.clip_grads(list(gc), max_norm)
                rec.append(dict(ga=dict(zip(om.NET_KEYS, ga)), gc=dict(zip(om.NET_KEYS, gc)), na=float(na),
                                nc=float(nc), pol=float(pol.detach()), ent=float(ent.detach()),
                                vloss=float(vloss.detach()), ratio_sum=float(ratio.detach().double().sum()),
                                rows=int(ratio.numel()), active=float(b["active_masks"].sum()),
                                ret_mean=float(b["returns"].double().mean()),
                                ret_sq_mean=float((b["returns"].double() ** 2).mean())))
                PA = om.adam(PA, dict(zip(om.NET_KEYS, ga)), sa, lr, eps)
                PC = om.adam(PC, dict(zip(om.NET_KEYS, gc)), sc, lr, eps)
    finally:
        torch.set_default_dtype(old)
    return rec, PA, PC, vn


def train_outputs(rec, PA2, PC2, vn2):
    """Post-train parameters, ValueNorm state and the train() log (averages over the epochs * M updates)."""
    out = cv.train_outputs(rec, PA2, PC2, vn2)
    out["ratio"] = np.array(sum(r["ratio_sum"] for r in rec) / sum(r["rows"] for r in rec))
    return out


def update_grads(rec, updates):
    """{(update, net, key): unclipped gradient} of the listed updates of a record."""
    out = {}
    for u in updates:
        for (n, k), g in cv.unclipped_grads(rec, u).items():
            out[(u, n, k)] = g
    return out


def fp32_spread(f):
    """f(dtype, shuffle) -> {name: array}; -> (f64 values, {name: fp32 spread}) (module docstring)."""
    a, b, c = f(torch.float32, False), f(torch.float32, True), f(torch.float64, False)
    sp = {}
    for k in c:
        x, y, z = (np.asarray(v[k], np.float64) for v in (a, b, c))
        sp[k] = max(np.abs(x - y).max(), np.abs(x - z).max(), 2.0 ** -23 * np.abs(z).max(), 1e-30)
    return c, sp


def assert_within(got, want, spread, what, extra=0.0):
    """|got - want| <= K_FP32 spreads (+ extra: a golden value's own distance to the f64 run); prints the figures."""
    err = float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max())
    print(f"{what}: err = {err:.3e}, bar = {K_FP32} x {spread:.3e} + {extra:.3e}")
    assert err <= K_FP32 * spread + extra, f"{what}: err {err:.3e} > {K_FP32} x spread {spread:.3e} + {extra:.3e}"


def golden_grad(fx, u, n, k):
    """The reference's own unclipped gradient of update u (recorded clipped -> divided by its clip coefficient)."""
    kind, tag = ("actor", "a") if n == 0 else ("critic", "c")
    coef = min(1.0, 0.5 / (float(fx["norms"][2 * u + n]) + 1e-6))
    return fx[f"grad{tag}{u}.{om.ref_name(k, kind)}"] / coef
