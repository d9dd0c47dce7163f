"""Generate the golden vectors of MAPPO at the Switch2 observation width (obs_space Box(3): row, column, clock;
cent_obs_space Box(3) or, with use_centralized_V, Box(6) for 2 agents) by importing the reference.

Runs ONLY in the build container (needs the reference checkout, read-only; see make_golden_mappo.py, whose loader,
gym stand-in and recorders this script reuses); the GPU box only reads the fixtures written next to this script.
ma_gym is absent, so the observations are synthetic, drawn from the value set Switch emits (oracle/switch.py):
round(r / 2, 2) for r < 3, round(c / 6, 2) for c < 7 and a clock k / 100 shared by the agents of an env. Rewards are
Switch's two values, step_cost -0.01 and +5.

  mappo_sw_fwd.npz       cases rec_d / rec_c / ff_d / ff_c (recurrent | feed-forward, critic width 3 | 6), E 6, N 2:
                         get_actions (drawn actions recorded) and get_values on the same inputs
  mappo_sw_train.npz     case d: recurrent, decentralized critic
  mappo_sw_cv_train.npz  case c: recurrent, centralized critic over 2 agents
  mappo_sw_ff_train.npz  cases d, c: feed-forward, critic width 3 | 6
Every train case is R_MAPPO.train on one synthetic rollout (E 4, N 2, T 10, L 5, 3 epochs; make_golden_mappo.py's
done pattern) run twice from equal seeds: m1 (train_batch_size 1: the clipped gradients of the first update, the
pre-clip norms, post-train parameters, ValueNorm state, info) and m2 (train_batch_size 2: the recorded permutations
-- chunks for the recurrent nets, rows for the feed-forward ones --, norms, post-train parameters, ValueNorm, info).

Usage (from the repository root):  python tests/golden/make_golden_mappo_switch.py
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden_mappo import (OUT, Box, Discrete, SampleRecorder, load, make_args, sd, seed_all)  # noqa: E402

D, A, H, N = 3, 5, 32, 2
FF = dict(use_recurrent_policy=False, use_naive_recurrent_policy=False)
ROW = np.array([round(r / 2, 2) for r in range(3)], np.float32)
COL = np.array([round(c / 6, 2) for c in range(7)], np.float32)


def gen_obs(rng, E):
    """[E, N, 3] Switch-like observations: a row and a column feature per agent, one clock per env."""
    o = np.empty((E, N, D), np.float32)
    o[..., 0] = ROW[rng.integers(0, 3, (E, N))]
    o[..., 1] = COL[rng.integers(0, 7, (E, N))]
    o[..., 2] = (rng.integers(0, 101, (E, 1)) / 100.0).astype(np.float32)
    return o


def share(obs):
    """obs_sharing (base_runner.py:155-161): [..., E, N, D] -> [..., E, N, N*D]."""
    *lead, E, n, d = obs.shape
    return np.ascontiguousarray(np.broadcast_to(obs.reshape(*lead, E, 1, n * d), (*lead, E, n, n * d)))


def keep(k):
    return ".base.mlp.fc_h." not in "." + k      # built but unused by the feed-forward nets (mlp.py:20-27)


def policy(m, cent, ff, **kw):
    args = make_args(m, use_centralized_V=cent, **dict(kw, **(FF if ff else {})))
    cs = Box(np.zeros(N * D if cent else D))
    return args, cs, m.policy.R_MAPPOPolicy(args, Box(np.zeros(D)), cs, Discrete(A), torch.device("cpu"))


def fwd_case(m, cent, ff, seed):
    seed_all(seed)
    E = 6
    _, _, pol = policy(m, cent, ff)
    rng = np.random.default_rng(seed)
    R = E * N
    obs3 = gen_obs(rng, E)
    cent_obs = share(obs3).reshape(R, N * D) if cent else obs3.reshape(R, D)
    obs = obs3.reshape(R, D)
    ha = (rng.standard_normal((R, 1, H)) * 0.5).astype(np.float32)
    hc = (rng.standard_normal((R, 1, H)) * 0.5).astype(np.float32)
    masks = np.ones((R, 1), np.float32)
    masks[[1, 4, R - 2]] = 0.0
    with torch.no_grad(), SampleRecorder():
        v, a, lp, ha2, hc2 = pol.get_actions(obs, cent_obs, ha, hc, masks)
        v2 = pol.get_values(cent_obs, hc, masks)
    out = dict(obs=obs, ha=ha, hc=hc, masks=masks, values=v.numpy(), actions=a.numpy(), logp=lp.numpy(),
               ha_out=ha2.numpy(), hc_out=hc2.numpy(), get_values=v2.numpy(), E=np.int64(E), N=np.int64(N))
    if ff:
        np.testing.assert_array_equal(out["ha_out"], ha)
        np.testing.assert_array_equal(out["hc_out"], hc)
    out.update({k: v for k, v in sd("actor.", pol.actor).items() if keep(k)})
    out.update({k: v for k, v in sd("critic.", pol.critic).items() if keep(k)})
    return out


def train_run(m, cent, ff, M, seed, E=4, T=10, L=5, EPOCHS=3):
    seed_all(seed)
    args, cs, pol = policy(m, cent, ff, batch_size=E, max_step=T, ppo_epoch=EPOCHS, data_chunk_length=L,
                           train_batch_size=M)
    tr = m.trainer.R_MAPPO(args, pol, torch.device("cpu"))
    buf = m.buffer.SharedReplayBuffer(args, N, Box(np.zeros(D)), cs, Discrete(A))
    rng = np.random.default_rng(seed)
    sh = share if cent else (lambda x: x)
    buf.obs[0] = gen_obs(rng, E)
    buf.share_obs[0] = sh(buf.obs[0])
    done_at = {3: [1], 7: [0, 2]}          # step -> envs whose episode ends (all agents done)
    agent_done = {5: [(E - 1, 1)]}         # step -> (env, agent) done while the env goes on
    for t in range(T):
        with torch.no_grad():
            v, a, lp, ha, hc = pol.get_actions(np.concatenate(buf.obs[t]), np.concatenate(buf.share_obs[t]),
                                               np.concatenate(buf.rnn_states[t]),
                                               np.concatenate(buf.rnn_states_critic[t]),
                                               np.concatenate(buf.masks[t]))
        sp = lambda x: np.array(np.split(np.asarray(x), E))  # noqa: E731
        v, a, lp, ha, hc = sp(v), sp(a), sp(lp), sp(ha), sp(hc)
        nobs = gen_obs(rng, E)
        rew = rng.choice(np.array([-0.01, 5.0], np.float32), size=(E, N, 1), p=[0.85, 0.15]).astype(np.float32)
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
        buf.insert(sh(nobs), nobs, ha, hc, a, lp, v, rew, masks, active_masks=active)
    with torch.no_grad():
        nv = pol.get_values(np.concatenate(buf.share_obs[-1]), np.concatenate(buf.rnn_states_critic[-1]),
                            np.concatenate(buf.masks[-1]))
    buf.compute_returns(np.array(np.split(nv.numpy(), E)), tr.value_normalizer)
    assert np.array_equal(buf.share_obs, sh(buf.obs)), "share_obs is derivable from obs"
    before = {}
    before.update(sd("actor.", pol.actor))
    before.update(sd("critic.", pol.critic))
    vn0 = {k: v.detach().numpy().copy() for k, v in tr.value_normalizer.state_dict().items()}
    data = dict(obs=buf.obs.copy(), actions=buf.actions.copy(), action_log_probs=buf.action_log_probs.copy(),
                value_preds=buf.value_preds.copy(), returns=buf.returns.copy(), masks=buf.masks.copy(),
                active_masks=buf.active_masks.copy(), rewards=buf.rewards.copy())
    if ff:
        assert not buf.rnn_states.any() and not buf.rnn_states_critic.any()
    else:
        data.update(rnn_states=buf.rnn_states.copy(), rnn_states_critic=buf.rnn_states_critic.copy())
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
    shared = {f"data.{k}": v for k, v in data.items()}
    shared.update({f"before.{k}": v for k, v in before.items() if keep(k)})
    shared.update({f"vn0.{k}": v for k, v in vn0.items()})
    shared.update(dict(E=np.int64(E), N=np.int64(N), T=np.int64(T), L=np.int64(L), epochs=np.int64(EPOCHS),
                       gamma=np.float32(args.gamma), gae_lambda=np.float32(args.gae_lambda)))
    run = {"perms": np.stack(perms), "norms": np.array(norms, np.float64), "train_batch_size": np.int64(M)}
    assert run["norms"].shape == (2 * EPOCHS * M,), run["norms"].shape
    names = {"a": [n for n, _ in pol.actor.named_parameters()], "c": [n for n, _ in pol.critic.named_parameters()]}
    seen = {"a": 0, "c": 0}
    for tag, gl in grads:
        if M == 1 and seen[tag] == 0:          # the first update's clipped gradients
            for n, g in zip(names[tag], gl):
                if g is not None and keep(n):
                    run[f"grad{tag}0.{n}"] = g
        seen[tag] += 1
    after = {}
    after.update(sd("actor.", pol.actor))
    after.update(sd("critic.", pol.critic))
    run.update({f"after.{k}": v for k, v in after.items() if keep(k)})
    run.update({f"vn1.{k}": v.detach().numpy().copy() for k, v in tr.value_normalizer.state_dict().items()})
    for k in ("value_loss", "policy_loss", "dist_entropy", "actor_grad_norm", "critic_grad_norm"):
        run[f"info.{k}"] = np.float64(info[k])
    run["info.ratio"] = np.float64(float(info["ratio"]))
    return shared, run


def train_case(m, cent, ff, seed):
    s1, m1 = train_run(m, cent, ff, 1, seed)
    s2, m2 = train_run(m, cent, ff, 2, seed)
    assert s1.keys() == s2.keys() and all(np.array_equal(s1[k], s2[k]) for k in s1), "equal seeds, equal rollouts"
    out = dict(s1)
    out.update({f"m1.{k}": v for k, v in m1.items()})
    out.update({f"m2.{k}": v for k, v in m2.items()})
    return out


def save(name, cases):
    np.savez(os.path.join(OUT, name), **{f"{c}.{k}": v for c, d in cases.items() for k, v in d.items()})


if __name__ == "__main__":
    m = load()
    save("mappo_sw_fwd.npz", {"rec_d": fwd_case(m, False, False, 31), "rec_c": fwd_case(m, True, False, 32),
                              "ff_d": fwd_case(m, False, True, 33), "ff_c": fwd_case(m, True, True, 34)})
    save("mappo_sw_train.npz", {"d": train_case(m, False, False, 41)})
    save("mappo_sw_cv_train.npz", {"c": train_case(m, True, False, 42)})
    save("mappo_sw_ff_train.npz", {"d": train_case(m, False, True, 43), "c": train_case(m, True, True, 44)})
    print("wrote mappo_sw_fwd.npz, mappo_sw_train.npz, mappo_sw_cv_train.npz, mappo_sw_ff_train.npz")
