"""Golden vectors for the recurrent offpolicy actor-critic trainers of ``offpolicy/``: ONE
``R_MADDPG.shared_train_policy_on_batch`` (offpolicy/algorithms/r_maddpg/r_maddpg.py:114-331) of the reference's own
``R_MADDPG`` / ``R_MATD3`` trainer and ``R_MADDPGPolicy`` / ``R_MATD3Policy`` classes at N 2, D 47, T 4, B 5 on CPU.

Runs ONLY in the build container (imports /root/reference, read-only); everything else reads ``rmaddpg.npz`` /
``rmatd3.npz``. Stand-ins as in make_golden_maddpg.py (``gym``; ``algorithms.utils.rnn`` / ``.mlp`` / ``.act`` aliased
to ``utils/algorithm_utils``; ``utils.util.sample_gumbel`` hands out recorded noise call by call: rmatd3 the target
actions over T + 1 steps first, then the actor pass; the critic optimizer's ``step`` copies the critic gradients after
clip_grad_norm_), and ``args.gain = 1`` so that the action head's logits are not all within 1e-2 of each other.
  rmaddpg.npz  R_MADDPG: one head, use_per, MSE
  rmatd3.npz   R_MATD3: two heads, Gumbel target actions, no PER, Huber with huber_delta 1.0
Recorded: the live state dicts before the update, rounded to float16 values and kept as float16 (the nets run with
exactly those values), the seed of the target nets' offsets (tests/rmaddpg_ref.py: target_offsets), the noise, the
batch, gradients after clip_grad_norm_, parameters after Adam, losses, norms, priorities, the hyperparameters.

Usage (from the repository root):  python tests/golden/make_golden_rmaddpg.py
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")]
from make_golden_offq import OUT, REF, Box, Discrete, gen_obs, install_gym  # noqa: E402
from rmaddpg_ref import target_offsets  # noqa: E402

PID = "policy_0"


def load():
    install_gym()
    sys.path.insert(0, REF)
    try:
        m = types.SimpleNamespace()
        m.config = importlib.import_module("config")
        importlib.import_module("algorithms")
        au = types.ModuleType("algorithms.utils")
        mods = {"algorithms.utils": au}
        for k in ("mlp", "rnn", "act"):
            mods["algorithms.utils." + k] = importlib.import_module("utils.algorithm_utils." + k)
            setattr(au, k, mods["algorithms.utils." + k])
        sys.modules.update(mods)
        m.util = importlib.import_module("utils.util")
        m.trainer = {False: importlib.import_module("algorithms.r_maddpg.r_maddpg").R_MADDPG,
                     True: importlib.import_module("algorithms.r_matd3.r_matd3").R_MATD3}
        m.policy = {False: importlib.import_module("algorithms.r_maddpg.algorithm.rMADDPGPolicy").R_MADDPGPolicy,
                    True: importlib.import_module("algorithms.r_matd3.algorithm.rMATD3Policy").R_MATD3Policy}
    finally:
        sys.path.pop(0)
    return m


def run_variant(m, name, td3, use_per, huber, N=2, D=47, T=4, B=5, A=5, seed=5):
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed + 7)
    args = m.config.get_config().parse_known_args([])[0]
    args.use_per, args.use_huber_loss, args.huber_delta, args.gain, args.episode_length = use_per, huber, 1.0, 1.0, T
    dev = torch.device("cpu")
    pcfg = {"obs_space": Box(shape=(D,)), "act_space": Discrete(A), "cent_obs_dim": N * D, "cent_act_dim": N * A}
    pol = m.policy[td3]({"args": args, "device": dev}, pcfg)
    trainer = m.trainer[td3](args, N, {PID: pol}, lambda a: PID, device=dev, episode_length=T)
    out, live = {}, {"actor": pol.actor, "critic": pol.critic}
    with torch.no_grad():
        for n, net in live.items():
            for k, p in net.state_dict().items():
                p.copy_(p.half().float())
                out[f"{n}.{k}"] = p.numpy().astype(np.float16)
        sds = {n: {k: v.numpy() for k, v in net.state_dict().items()} for n, net in live.items()}
        for n, off in target_offsets(sds, seed + 1000).items():
            for k, p in getattr(pol, "target_" + n).state_dict().items():
                p.copy_(torch.from_numpy(sds[n][k] + off[k]))
    # recorded noise in the reference's row order [steps, N * B, A]; target step 0 is discarded by the reference
    u = rng.random((2, T + 1, N * B, A)).astype(np.float32)
    noise = (-np.log(-np.log(u + np.float32(1e-20)) + np.float32(1e-20))).astype(np.float32)
    agents = lambda x: x.reshape(T, N, B, A).transpose(1, 0, 2, 3).copy()
    out["target_gumbel"], out["gumbel"] = agents(noise[0, 1:]), agents(noise[1, :T])
    queue = ([noise[0]] if td3 else []) + [noise[1, :T]]
    m.util.sample_gumbel = lambda shape, eps=1e-20, tens_type=torch.FloatTensor: torch.from_numpy(queue.pop(0))
    step = pol.critic_optimizer.step

    def recording_step(*a, **k):
        out.update({"grad.critic." + key: p.grad.numpy().copy() for key, p in pol.critic.named_parameters()
                    if p.grad is not None})
        return step(*a, **k)

    pol.critic_optimizer.step = recording_step
    obs = gen_obs(rng, (N, T + 1, B, D))
    de = np.zeros((T, B, 1), np.float32)
    de[0:, 1], de[2:, 2], de[3:, 4] = 1.0, 1.0, 1.0           # ends at t = 0, mid-way, at the last step, never
    dones = np.broadcast_to(de[None], (N, T, B, 1)).copy()
    dones[1, 1:, 0] = 1.0                                      # one agent of an episode that never ends
    b = {"obs": obs, "share_obs": obs.transpose(1, 2, 0, 3).reshape(T + 1, B, N * D).copy(),
         "acts": np.eye(A, dtype=np.float32)[rng.integers(0, A, (N, T, B))],
         "rewards": rng.standard_normal((N, T, B, 1)).astype(np.float32), "dones": dones, "dones_env": de,
         "is_weight": (0.5 + rng.random(B)).astype(np.float32)}
    d = lambda k: {PID: b[k]}
    batch = (d("obs"), d("share_obs"), d("acts"), d("rewards"), d("dones"), d("dones_env"), {PID: None},
             b["is_weight"] if use_per else None, np.arange(B))
    info, prios, _ = trainer.train_policy_on_batch(PID, batch)
    assert not queue and info["update_actor"]
    out.update({"grad.actor." + key: p.grad.numpy().copy() for key, p in pol.actor.named_parameters()
                if p.grad is not None})
    for n, net in live.items():
        out.update({f"post.{n}.{key}": p.detach().numpy().copy() for key, p in net.named_parameters()})
    out.update({k: v for k, v in b.items() if use_per or k != "is_weight"})
    out.update({k: np.float32(float(info[k])) for k in ("critic_loss", "critic_grad_norm", "actor_loss",
                                                        "actor_grad_norm")})
    out["target_seed"] = np.int64(seed + 1000)
    out["hyper"] = np.array([args.gamma, args.lr, args.opti_eps, args.max_grad_norm, args.huber_delta, args.per_eps,
                             args.per_nu], np.float64)
    if use_per:
        out["new_priorities"] = np.asarray(prios, np.float64)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(f"wrote {name}.npz:", {k: float(out[k]) for k in ("critic_loss", "critic_grad_norm", "actor_loss",
                                                           "actor_grad_norm")})


def main():
    torch.set_num_threads(1)
    m = load()
    run_variant(m, "rmaddpg", False, True, False, seed=5)
    run_variant(m, "rmatd3", True, False, True, seed=5)


if __name__ == "__main__":
    main()
