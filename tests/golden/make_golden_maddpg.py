"""Golden vectors for the offpolicy actor-critic trainers of ``offpolicy/``: ONE
``MADDPG.shared_train_policy_on_batch`` (offpolicy/algorithms/maddpg/maddpg.py:90-249) of the reference's own
``MADDPG`` / ``MATD3`` trainer and ``MADDPGPolicy`` / ``MATD3Policy`` classes at N 2, B 19, D 47, A 5 on CPU.

Runs ONLY in the build container (imports /root/reference, read-only); everything else reads ``maddpg.npz`` /
``matd3.npz``. Stand-ins as in make_golden_moffq.py (``gym``; ``algorithms.utils.mlp`` / ``.act`` aliased to
``utils/algorithm_utils``), and:
  * ``utils.util.sample_gumbel`` is replaced by a function that hands out recorded Gumbel(0, 1) noise, call by call
    (matd3: the target actions first, then the actor pass; maddpg: the actor pass only);
  * ``config.py`` has no ``target_action_noise_std``, which ``MATD3Policy`` reads: it is set to 0.2 (any value that is
    not None selects the Gumbel branch for discrete actions);
  * the critic optimizer's ``step`` is wrapped to copy the critic gradients (after clip_grad_norm_) before it steps:
    the actor pass zeroes them afterwards.
  maddpg.npz  MADDPG: one head, use_per, MSE
  matd3.npz   MATD3: two heads, Gumbel target actions, no PER, Huber with huber_delta 1.0
Recorded: actor / critic state dicts before the update and those of the perturbed targets
(make_golden_offq.target_perturbation), BOTH ``q_outs`` lists (no state dict holds them), the noise, gradients after
clip_grad_norm_, parameters after Adam, losses, norms, priorities, the batch and the hyperparameters.

Usage (from the repository root):  python tests/golden/make_golden_maddpg.py
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden_offq import OUT, REF, Box, Discrete, gen_obs, install_gym, target_perturbation  # noqa: E402

PID = "policy_0"


def load():
    install_gym()
    sys.path.insert(0, REF)
    try:
        m = types.SimpleNamespace()
        m.config = importlib.import_module("config")
        importlib.import_module("algorithms")
        au = types.ModuleType("algorithms.utils")
        au.mlp = importlib.import_module("utils.algorithm_utils.mlp")
        au.act = importlib.import_module("utils.algorithm_utils.act")
        sys.modules.update({"algorithms.utils": au, "algorithms.utils.mlp": au.mlp, "algorithms.utils.act": au.act})
        m.util = importlib.import_module("utils.util")
        m.maddpg = importlib.import_module("algorithms.maddpg.maddpg")
        m.matd3 = importlib.import_module("algorithms.matd3.matd3")
        m.policy = importlib.import_module("algorithms.maddpg.algorithm.MADDPGPolicy")
        m.td3_policy = importlib.import_module("algorithms.matd3.algorithm.MATD3Policy")
    finally:
        sys.path.pop(0)
    return m


def run_variant(m, name, td3, use_per, huber, N=2, B=19, D=47, A=5, seed=5):
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed + 7)
    args = m.config.get_config().parse_known_args([])[0]
    args.use_per, args.use_huber_loss, args.huber_delta, args.target_action_noise_std = use_per, huber, 1.0, 0.2
    dev = torch.device("cpu")
    cfg = {"args": args, "device": dev}
    pcfg = {"obs_space": Box(shape=(D,)), "act_space": Discrete(A), "cent_obs_dim": N * D, "cent_act_dim": N * A}
    pol = (m.td3_policy.MATD3Policy if td3 else m.policy.MADDPGPolicy)(cfg, pcfg)
    trainer = (m.matd3.MATD3 if td3 else m.maddpg.MADDPG)(args, N, {PID: pol}, lambda a: PID, device=dev)
    nets = {"actor": pol.actor, "critic": pol.critic, "target_actor": pol.target_actor,
            "target_critic": pol.target_critic}
    tseed = seed + 1000
    pert = target_perturbation([(n + "." + k, tuple(v.shape)) for n in ("target_actor", "target_critic")
                                for k, v in nets[n].state_dict().items()], tseed)
    with torch.no_grad():
        for n in ("target_actor", "target_critic"):
            for k, p in nets[n].state_dict().items():
                p.add_(torch.from_numpy(pert[n + "." + k]))
    out = {}
    for n, net in nets.items():
        for k, v in net.state_dict().items():
            out[f"{n}.{k}"] = v.numpy().copy()
    for n in ("critic", "target_critic"):
        for h, q in enumerate(nets[n].q_outs):
            out[f"{n}.q_outs.{h}.weight"], out[f"{n}.q_outs.{h}.bias"] = (q.weight.detach().numpy().copy(),
                                                                         q.bias.detach().numpy().copy())
    # recorded noise, [N * B, A] per call in the reference's row order (agent-major)
    u = rng.random((2, N * B, A)).astype(np.float32)
    noise = (-np.log(-np.log(u + np.float32(1e-20)) + np.float32(1e-20))).astype(np.float32)
    out["target_gumbel"], out["gumbel"] = noise[0].reshape(N, B, A), noise[1].reshape(N, B, A)
    queue = [noise[0], noise[1]] if td3 else [noise[1]]
    m.util.sample_gumbel = lambda shape, eps=1e-20, tens_type=torch.FloatTensor: torch.from_numpy(queue.pop(0))
    step = pol.critic_optimizer.step

    def recording_step(*a, **k):
        for key, p in pol.critic.named_parameters():
            if p.grad is not None:              # mlp.mlp.fc_h.* is built and never used
                out["grad.critic." + key] = p.grad.numpy().copy()
        return step(*a, **k)

    pol.critic_optimizer.step = recording_step
    obs, nobs = gen_obs(rng, (N, B, D)), gen_obs(rng, (N, B, D))
    share = lambda o: o.transpose(1, 0, 2).reshape(B, N * D).copy()
    dones_env = (rng.random((B, 1)) < 0.3).astype(np.float32)
    dones_env[0], dones_env[1] = 1.0, 0.0
    valid = (rng.random((N, B, 1)) > 0.3).astype(np.float32)
    valid[:, 0], valid[1, 3] = 1.0, 0.0
    b = {"obs": obs, "nobs": nobs, "cent_obs": share(obs), "cent_nobs": share(nobs),
         "acts": np.eye(A, dtype=np.float32)[rng.integers(0, A, (N, B))],
         "rewards": rng.standard_normal((N, B, 1)).astype(np.float32), "dones_env": dones_env, "valid": valid,
         "is_weight": (0.5 + rng.random(B)).astype(np.float32)}
    d = lambda k: {PID: b[k]}
    batch = (d("obs"), d("cent_obs"), d("acts"), d("rewards"), d("nobs"), d("cent_nobs"),
             {PID: np.broadcast_to(dones_env[None], (N, B, 1)).copy()}, d("dones_env"), d("valid"), {PID: None},
             {PID: None}, b["is_weight"] if use_per else None, np.arange(B))
    info, prios, _ = trainer.train_policy_on_batch(PID, batch)
    assert not queue and info["update_actor"]
    for key, p in pol.actor.named_parameters():
        if p.grad is not None:
            out["grad.actor." + key] = p.grad.numpy().copy()
    for n in ("actor", "critic"):
        for key, p in nets[n].named_parameters():
            out[f"post.{n}.{key}"] = p.detach().numpy().copy()
    for n in ("critic", "target_critic"):       # the heads after the update: unchanged, whatever the optimizer did
        for h, q in enumerate(nets[n].q_outs):
            assert np.array_equal(q.weight.detach().numpy(), out[f"{n}.q_outs.{h}.weight"])
    out.update({k: v for k, v in b.items() if use_per or k != "is_weight"})
    out.update({k: np.float32(float(info[k])) for k in ("critic_loss", "critic_grad_norm", "actor_loss",
                                                        "actor_grad_norm")})
    out["meta"] = np.array([N, B, D, A, int(td3), int(use_per), int(huber), tseed], np.int64)
    out["hyper"] = np.array([args.gamma, args.lr, args.opti_eps, args.max_grad_norm, args.huber_delta, args.per_eps],
                            np.float64)
    if use_per:
        out["new_priorities"] = np.asarray(prios, np.float64)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(f"wrote {name}.npz:", {k: float(out[k]) for k in ("critic_loss", "critic_grad_norm", "actor_loss",
                                                           "actor_grad_norm")})


def main():
    torch.set_num_threads(1)
    m = load()
    run_variant(m, "maddpg", False, True, False, seed=5)
    run_variant(m, "matd3", True, False, True, seed=6)


if __name__ == "__main__":
    main()
