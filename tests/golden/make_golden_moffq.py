"""Golden vectors for the feed-forward transition-batch QMix / VDN trainer of ``offpolicy/``:
``M_QMix.train_policy_on_batch`` (offpolicy/algorithms/mqmix/mqmix.py:68-218) with the shared
``M_QMixPolicy`` (algorithm/mQMixPolicy.py: AgentQFunction = MLPBase + ACTLayer) and ``M_QMixer`` or, through the
``M_VDN`` trainer class (algorithms/mvdn/mvdn.py), ``M_VDNMixer``.

Runs ONLY in the build container (imports /root/reference, read-only); everything else reads the
``moffq_*.npz`` fixtures only. Two things the reference needs before it imports:
  * ``utils/util.py`` imports ``gym`` / ``gym.spaces``: the in-memory stand-in of make_golden_offq.py;
  * ``mqmix/algorithm/agent_q_function.py`` imports ``algorithms.utils.mlp`` / ``algorithms.utils.act``, which live at
    ``utils/algorithm_utils/``: both are aliased in ``sys.modules``.
And one while it runs: ``train_policy_on_batch`` calls ``self.mixer(agent_qs, cent_obs)``, but ``M_VDNMixer.forward``
takes the agent Qs alone, so the ``M_VDN`` trainer raises a TypeError as it stands. ``TwoArgMixer`` below (ours) hands
the first argument on to the reference's own forward; the arithmetic stays the reference's.

One fixture per variant, each ONE train_policy_on_batch (use_same_share_obs=True) at N 2, B 19, D 47 on a gen_obs batch
(layout of MlpReplayBuffer.sample) with mixed dones_env:
  moffq_qmix.npz  M_QMix: M_QMixer, use_double_q, use_per, MSE
  moffq_vdn.npz   M_VDN: M_VDNMixer, max-Q target, no PER, Huber with huber_delta = the median |err| (float32) of a
                  probe run of the same trainer, so both branches occur (asserted: share above delta in [0.25, 0.75])
Recorded: the state dicts before (``q.*`` with the unused ``mlp.mlp.fc_h.*``, ``m.*``), gradients after
clip_grad_norm_ (only of tensors that have one), parameters after Adam, loss / grad_norm / Q_tot, the new priorities,
the hyperparameters of the reference's config. The target nets are the behavior nets plus a seeded perturbation
(make_golden_offq.target_perturbation) that the tests rebuild from ``target_seed``.

Usage (from the repository root):  python tests/golden/make_golden_moffq.py
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
        m.mqmix = importlib.import_module("algorithms.mqmix.mqmix")
        m.mvdn = importlib.import_module("algorithms.mvdn.mvdn")
        m.policy = importlib.import_module("algorithms.mqmix.algorithm.mQMixPolicy")
        m.vdn_policy = importlib.import_module("algorithms.mvdn.algorithm.mVDNPolicy")
        m.vdn_mixer = importlib.import_module("algorithms.mvdn.algorithm.mvdn_mixer")
    finally:
        sys.path.pop(0)

    class TwoArgMixer(m.vdn_mixer.M_VDNMixer):
        def forward(self, agent_q_inps, states=None):
            return super().forward(agent_q_inps)

    m.TwoArgMixer = TwoArgMixer
    return m


def make_batch(seed, N, B, D, A):
    rng = np.random.default_rng(seed)
    obs, nobs = gen_obs(rng, (N, B, D)), gen_obs(rng, (N, B, D))
    dones_env = (rng.random((B, 1)) < 0.3).astype(np.float32)
    dones_env[0], dones_env[1] = 1.0, 0.0
    share = lambda o: o.transpose(1, 0, 2).reshape(B, N * D).copy()
    return {"obs": obs, "nobs": nobs, "cent_obs": share(obs), "cent_nobs": share(nobs),
            "acts": np.eye(A, dtype=np.float32)[rng.integers(0, A, (N, B))],
            "rewards": rng.standard_normal((N, B, 1)).astype(np.float32), "dones_env": dones_env,
            "dones": np.broadcast_to(dones_env[None], (N, B, 1)).copy(),
            "is_weight": (0.5 + rng.random(B)).astype(np.float32)}


def make_trainer(m, vdn, double_q, use_per, huber, huber_delta, N, D, A, seed):
    """A fresh trainer from ``seed`` with its perturbed target nets; returns (args, policy, trainer, tseed)."""
    torch.manual_seed(seed)
    args = m.config.get_config().parse_known_args([])[0]
    args.use_double_q, args.use_per, args.use_huber_loss = double_q, use_per, huber
    if huber_delta is not None:
        args.huber_delta = huber_delta
    cfg = {"args": args, "device": torch.device("cpu"), "num_agents": N}
    pcfg = {"obs_space": Box(shape=(D,)), "act_space": Discrete(A), "cent_obs_dim": N * D}
    policies = {PID: (m.vdn_policy.M_VDNPolicy if vdn else m.policy.M_QMixPolicy)(cfg, pcfg)}
    if vdn:
        trainer = m.mvdn.M_VDN(args, N, policies, lambda a: PID, device=torch.device("cpu"))
        trainer.mixer = m.TwoArgMixer(args, N, N * D, torch.device("cpu"))
        trainer.target_mixer = m.TwoArgMixer(args, N, N * D, torch.device("cpu"))
    else:
        trainer = m.mqmix.M_QMix(args, N, policies, lambda a: PID, device=torch.device("cpu"))
    q_sd, m_sd = policies[PID].q_network.state_dict(), trainer.mixer.state_dict()
    tseed = seed + 1000
    pert = target_perturbation([("q." + k, tuple(v.shape)) for k, v in q_sd.items()] +
                               [("m." + k, tuple(v.shape)) for k, v in m_sd.items()], tseed)
    with torch.no_grad():
        for k, p in trainer.target_policies[PID].q_network.state_dict().items():
            p.add_(torch.from_numpy(pert["q." + k]))
        for k, p in trainer.target_mixer.state_dict().items():
            p.add_(torch.from_numpy(pert["m." + k]))
    return args, policies[PID], trainer, tseed


def sample_tuple(b, use_per):
    d = lambda k: {PID: b[k]}
    return (d("obs"), d("cent_obs"), d("acts"), d("rewards"), d("nobs"), d("cent_nobs"), d("dones"), d("dones_env"),
            {PID: None}, {PID: None}, {PID: None}, b["is_weight"] if use_per else None, np.arange(b["obs"].shape[1]))


def run_variant(m, name, vdn, double_q, use_per, huber, N=2, B=19, D=47, A=5, seed=5):
    b = make_batch(seed + 7, N, B, D, A)
    delta, above = None, -1.0
    if huber:
        # probe: the same trainer with PER on returns |err| + per_eps as its priorities; delta = their median
        args, _, probe, _ = make_trainer(m, vdn, double_q, True, True, None, N, D, A, seed)
        _, prio, _ = probe.train_policy_on_batch(sample_tuple(b, True), True)
        ae = np.asarray(prio, np.float64) - args.per_eps
        delta = float(np.float32(np.median(ae)))
        above = float((ae > delta).mean())
        assert 0.25 <= above <= 0.75, above
    args, policy, trainer, tseed = make_trainer(m, vdn, double_q, use_per, huber, delta, N, D, A, seed)
    out = {}
    for k, v in policy.q_network.state_dict().items():
        out["q." + k] = v.numpy().copy()
    for k, v in trainer.mixer.state_dict().items():
        out["m." + k] = v.numpy().copy()
    info, prios, _ = trainer.train_policy_on_batch(sample_tuple(b, use_per), True)
    for pre, net in (("q.", policy.q_network), ("m.", trainer.mixer)):
        for k, p in net.named_parameters():
            if p.grad is not None:
                out["grad." + pre + k] = p.grad.numpy().copy()
            out["post." + pre + k] = p.detach().numpy().copy()
    out.update({k: b[k] for k in ("obs", "nobs", "cent_obs", "cent_nobs", "acts", "rewards", "dones_env")})
    out.update({"loss": np.float32(info["loss"].item()), "grad_norm": np.float32(float(info["grad_norm"])),
                "q_tot": np.float32(info["Q_tot"].item()),
                "meta": np.array([N, B, D, A, int(double_q), int(use_per), int(huber), tseed], np.int64),
                "hyper": np.array([args.gamma, args.lr, args.opti_eps, args.max_grad_norm, args.huber_delta,
                                   args.per_eps], np.float64),
                "mixer_dims": np.array([args.mixer_hidden_dim, args.hypernet_hidden_dim], np.int64)})
    if use_per:
        out["is_weight"] = b["is_weight"]
        out["new_priorities"] = np.asarray(prios, np.float64)
    np.savez_compressed(os.path.join(OUT, f"moffq_{name}.npz"), **out)
    print(f"wrote moffq_{name}.npz: loss {out['loss']:.6f} grad_norm {out['grad_norm']:.6f} q_tot {out['q_tot']:.6f} "
          f"done rows {int(b['dones_env'].sum())}/{B} huber_delta {args.huber_delta:.6g} (above: {above:.3f})")


def main():
    torch.set_num_threads(1)
    m = load()
    # The seed is chosen for two things that tests/test_moffq_ref_cpu.py asks of a float32 rerun on another machine.
    # No priority is a cancelling difference: the smallest |err| is 0.13 (seed 5: one |err| of 0.006, whose float32
    # value is 2e-5 off the float64 one, against a bar of 5e-6). And Adam's first step, lr g / (|g| + eps), does not
    # magnify float32 summation noise dg of a near-zero gradient element past atol 1e-7: the worst
    # lr eps |g32 - g64| / (|g64| + eps)^2 over all elements is 4.6e-8 (seeds 5..74: 3e-8 .. 1e-6; seed 8 had 8e-7 and
    # one element of hyper_w2.0.weight came out 5e-7 off on a second CPU)
    run_variant(m, "qmix", False, True, True, False, seed=19)
    run_variant(m, "vdn", True, False, False, True, seed=6)


if __name__ == "__main__":
    main()
