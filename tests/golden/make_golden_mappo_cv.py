"""Generate golden vectors for MAPPO with a centralized critic (use_centralized_V=True) by importing the reference.

Runs ONLY in the build container (needs the reference checkout, read-only; see make_golden_mappo.py, whose
helpers this script reuses). The critic is built on cent_obs_space = Box(N*D) (rmappo_policy.py:29-33) and fed
share_obs, the concatenation of the env's N agent observations tiled to every agent
(runner/shared/base_runner.py:155-161, obs_sharing). share_obs is NOT stored: tests derive it from obs.

  mappo_cv_fwd.npz    per case n2 / n8 (D 47, N agents, E 3): get_actions and get_values on the same inputs
                      (critic hiddens distinct per agent, some masks zero); evaluate_actions on one minibatch
                      of n = 7 chunks of L = 5 steps with in-chunk mask zeros and an explicit cent_obs
  mappo_cv_train.npz  n2: R_MAPPO.train on a synthetic rollout (E 5, T 10, L 5, 3 epochs; train_fixture's done
                      pattern): gradients fed to Adam, norms, post-train parameters, ValueNorm, info
                      n8: E 3, T 5, L 5, one epoch: gradients and norms only

Usage (from the repository root):  python tests/golden/make_golden_mappo_cv.py
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden_mappo import (OUT, Box, Discrete, SampleRecorder, gen_obs, load, make_args, sd,  # noqa: E402
                               seed_all)

D, A, H = 47, 5, 32


def share(obs):
    """obs_sharing (base_runner.py:155-161): [..., E, N, D] -> [..., E, N, N*D], the env's obs concatenated over
    its agents, the same vector for every agent."""
    *lead, E, N, d = obs.shape
    flat = obs.reshape(*lead, E, 1, N * d)
    return np.ascontiguousarray(np.broadcast_to(flat, (*lead, E, N, N * d)))


def policy(m, N, **kw):
    args = make_args(m, use_centralized_V=True, **kw)
    pol = m.policy.R_MAPPOPolicy(args, Box(np.zeros(D)), Box(np.zeros(N * D)), Discrete(A), torch.device("cpu"))
    return args, pol


def fwd_case(m, N, seed):
    seed_all(seed)
    E = 3
    _, pol = policy(m, N)
    rng = np.random.default_rng(seed)
    R = E * N
    obs = gen_obs(rng, (E, N, D))
    cent = share(obs).reshape(R, N * D)
    obs = obs.reshape(R, D)
    ha = (rng.standard_normal((R, 1, H)) * 0.5).astype(np.float32)
    hc = (rng.standard_normal((R, 1, H)) * 0.5).astype(np.float32)    # distinct per agent
    masks = np.ones((R, 1), np.float32)
    masks[[1, R - 2]] = 0.0
    with torch.no_grad(), SampleRecorder():
        v, a, lp, ha2, hc2 = pol.get_actions(obs, cent, ha, hc, masks)
        v2 = pol.get_values(cent, hc, masks)
    out = dict(obs=obs, ha=ha, hc=hc, masks=masks, values=v.numpy(), actions=a.numpy(), logp=lp.numpy(),
               ha_out=ha2.numpy(), hc_out=hc2.numpy(), values_only=v2.numpy(), N=np.int64(N), E=np.int64(E))
    # one minibatch of n chunks of L steps (rows (l, j)), explicit cent_obs: chunk j's steps are steps of one agent
    # row, so its cent_obs rows are whole-env share_obs vectors of an env of N agents drawn per (l, j)
    L, n = 5, 7
    sobs_env = gen_obs(rng, (L * n, N, D))                  # the env of every (l, j) row
    sobs = np.ascontiguousarray(sobs_env[:, 0])             # the row's own agent: agent 0 of that env
    scent = sobs_env.reshape(L * n, N * D)
    sh = (rng.standard_normal((n, 1, H)) * 0.5).astype(np.float32)
    shc = (rng.standard_normal((n, 1, H)) * 0.5).astype(np.float32)
    smask = np.ones((L * n, 1), np.float32)
    smask[[0 * n + 2, 2 * n + 1, 2 * n + 5, 3 * n + 1]] = 0.0
    sact = rng.integers(0, A, (L * n, 1)).astype(np.float32)
    sactive = np.ones((L * n, 1), np.float32)
    sactive[[4, 11]] = 0.0
    with torch.no_grad():
        sv, slp, sent = pol.evaluate_actions(scent, sobs, sh, shc, sact, smask, None, sactive)
    out.update(seq_obs=sobs, seq_cent_obs=scent, seq_ha=sh, seq_hc=shc, seq_masks=smask, seq_actions=sact,
               seq_active=sactive, seq_values=sv.numpy(), seq_logp=slp.numpy(), seq_entropy=np.float32(sent.item()),
               seq_L=np.int64(L), seq_n=np.int64(n))
    out.update(sd("actor.", pol.actor))
    out.update(sd("critic.", pol.critic))
    return out


def train_case(m, N, E, T, L, EPOCHS, seed, full):
    seed_all(seed)
    args, pol = policy(m, N, batch_size=E, max_step=T, ppo_epoch=EPOCHS, data_chunk_length=L)
    tr = m.trainer.R_MAPPO(args, pol, torch.device("cpu"))
    buf = m.buffer.SharedReplayBuffer(args, N, Box(np.zeros(D)), Box(np.zeros(N * D)), Discrete(A))
    rng = np.random.default_rng(seed)
    buf.obs[0] = gen_obs(rng, (E, N, D))
    buf.share_obs[0] = share(buf.obs[0])
    done_at = {3: [1], 7: [0, 2]}          # step -> envs whose episode ends (all agents done)
    agent_done = {5: [(E - 1, 1)]}         # step -> (env, agent) done while the env goes on
    for t in range(T):
        with torch.no_grad():
            v, a, lp, ha, hc = pol.get_actions(np.concatenate(buf.obs[t]), np.concatenate(buf.share_obs[t]),
                                               np.concatenate(buf.rnn_states[t]),
                                               np.concatenate(buf.rnn_states_critic[t]),
                                               np.concatenate(buf.masks[t]))
        sp = lambda x: np.array(np.split(x.numpy(), E))
        v, a, lp, ha, hc = sp(v), sp(a), sp(lp), sp(ha), sp(hc)
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
        buf.insert(share(nobs), nobs, ha, hc, a, lp, v, rew, masks, active_masks=active)
    with torch.no_grad():
        nv = pol.get_values(np.concatenate(buf.share_obs[-1]), np.concatenate(buf.rnn_states_critic[-1]),
                            np.concatenate(buf.masks[-1]))
    buf.compute_returns(np.array(np.split(nv.numpy(), E)), tr.value_normalizer)
    assert np.array_equal(buf.share_obs, share(buf.obs)), "share_obs is derivable from obs"
    before = {}
    before.update(sd("actor.", pol.actor))
    before.update(sd("critic.", pol.critic))
    vn0 = {k: v.detach().numpy().copy() for k, v in tr.value_normalizer.state_dict().items()}
    data = dict(obs=buf.obs.copy(), rnn_states=buf.rnn_states.copy(), rnn_states_critic=buf.rnn_states_critic.copy(),
                actions=buf.actions.copy(), action_log_probs=buf.action_log_probs.copy(),
                value_preds=buf.value_preds.copy(), returns=buf.returns.copy(), masks=buf.masks.copy(),
                active_masks=buf.active_masks.copy(), rewards=buf.rewards.copy())
    perms, grads, norms = [], [], []
    orig_perm, orig_clip = torch.randperm, torch.nn.utils.clip_grad_norm_

    def perm(*a, **k):
        p = orig_perm(*a, **k)
        perms.append(p.numpy().copy())
        return p

    def clip(params, *a, **k):
        n = orig_clip(list(params), *a, **k)
        norms.append(float(n))
        return n

    for opt, tag in ((pol.actor_optimizer, "a"), (pol.critic_optimizer, "c")):
        step0 = opt.step

        def wrapped(*a, _s=step0, _o=opt, _t=tag, **k):
            grads.append((_t, [p.grad.detach().numpy().copy() if p.grad is not None else None
                               for g in _o.param_groups for p in g["params"]]))
            return _s(*a, **k)
        opt.step = wrapped
    torch.randperm, torch.nn.utils.clip_grad_norm_ = perm, clip
    try:
        info = tr.train(buf)
    finally:
        torch.randperm, torch.nn.utils.clip_grad_norm_ = orig_perm, orig_clip
    out = {f"data.{k}": v for k, v in data.items()}
    out.update({f"before.{k}": v for k, v in before.items()})
    out.update({f"vn0.{k}": v for k, v in vn0.items()})
    out["perms"] = np.stack(perms)
    out["norms"] = np.array(norms, np.float64)
    names = {"a": [n for n, _ in pol.actor.named_parameters()], "c": [n for n, _ in pol.critic.named_parameters()]}
    idx = {"a": 0, "c": 0}
    for tag, gl in grads:
        for n, g in zip(names[tag], gl):
            if g is not None:
                out[f"grad{tag}{idx[tag]}.{n}"] = g
        idx[tag] += 1
    if full:
        after = {}
        after.update(sd("actor.", pol.actor))
        after.update(sd("critic.", pol.critic))
        out.update({f"after.{k}": v for k, v in after.items()})
        vn1 = {k: v.detach().numpy().copy() for k, v in tr.value_normalizer.state_dict().items()}
        out.update({f"vn1.{k}": v for k, v in vn1.items()})
        for k in ("value_loss", "policy_loss", "dist_entropy", "actor_grad_norm", "critic_grad_norm"):
            out[f"info.{k}"] = np.float64(info[k])
        out["info.ratio"] = np.float64(float(info["ratio"]))
    out.update(dict(E=np.int64(E), N=np.int64(N), T=np.int64(T), L=np.int64(L), epochs=np.int64(EPOCHS),
                    gamma=np.float32(args.gamma), gae_lambda=np.float32(args.gae_lambda)))
    return out


def save(name, cases):
    np.savez(os.path.join(OUT, name), **{f"{c}.{k}": v for c, d in cases.items() for k, v in d.items()})


if __name__ == "__main__":
    m = load()
    save("mappo_cv_fwd.npz", {"n2": fwd_case(m, 2, 11), "n8": fwd_case(m, 8, 12)})
    save("mappo_cv_train.npz", {"n2": train_case(m, 2, 5, 10, 5, 3, 21, True),
                                "n8": train_case(m, 8, 3, 5, 5, 1, 22, False)})
    print("wrote mappo_cv_fwd.npz, mappo_cv_train.npz")
