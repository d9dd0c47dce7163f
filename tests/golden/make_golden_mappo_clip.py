"""Generate the golden vectors of R_MAPPO.train with PPO's branches ACTIVE by importing the reference.

Runs ONLY in the build container (needs the reference checkout, read-only; see make_golden_mappo.py, whose loader,
gym stand-in and train fixture this script reuses); the GPU box only reads the fixture written next to this script.

  mappo_clip_train.npz  R_MAPPO.train (mappo/algorithms/ramppo_network.py:56-287) on the synthetic rollout of
                        mappo_train.npz (E 4, N 2, T 10, L 5, 3 epochs) whose old log-probs and old values were
                        moved before train(): buf.action_log_probs by U(+-0.5) and buf.value_preds[:-1] by U(+-0.6),
                        30 % of each left untouched (tests/mappo_clip_cases.perturb, seed SEEDS["golden16"]). Returns
                        stay those of the unperturbed rollout; the advantages the reference computes inside train()
                        see the perturbed values, as they would with such a buffer. clip_param is the default 0.2;
                        huber_delta is the median |tgt - v| over the active rows of the float64 oracle's epoch 0
                        (tests/mappo_clip_cases.median_delta), so the surrogate clip, the value clip, both sides of
                        the max and both arms of Huber carry rows. Recorded as in mappo_train.npz (the perturbed
                        data, before / after parameters, ValueNorm before / after, the clipped gradients and
                        pre-clip norms of every epoch, info.*) plus the scalars clip_param and huber_delta.

Usage (from the repository root):  python tests/golden/make_golden_mappo_clip.py
"""
import os
import sys
import tempfile

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE), HERE):
    sys.path.insert(0, p)
import make_golden_mappo as g  # noqa: E402
import mappo_clip_cases as cc  # noqa: E402
from oracle import mappo as om  # noqa: E402


def main():
    m = g.load()
    Buffer, Trainer = m.buffer.SharedReplayBuffer, m.trainer.R_MAPPO
    compute_returns, train = Buffer.compute_returns, Trainer.train
    chosen = {}

    def compute_returns_then_perturb(self, next_value, value_normalizer=None):
        compute_returns(self, next_value, value_normalizer)
        moved = cc.perturb(dict(action_log_probs=self.action_log_probs, value_preds=self.value_preds),
                           cc.SEEDS["golden16"])
        self.action_log_probs[:] = moved["action_log_probs"]
        self.value_preds[:] = moved["value_preds"]

    def train_with_median_delta(self, buffer, *a, **k):
        sd = {}
        sd.update(g.sd("actor.", self.policy.actor))
        sd.update(g.sd("critic.", self.policy.critic))
        data = {key: getattr(buffer, key).copy() for key in
                ("obs", "rnn_states", "rnn_states_critic", "actions", "action_log_probs", "value_preds", "returns",
                 "masks", "active_masks", "rewards")}
        vn = {key: v.detach().numpy() for key, v in self.value_normalizer.state_dict().items()}
        vn0 = (float(vn["running_mean"][0]), float(vn["running_mean_sq"][0]), float(vn["debiasing_term"]))
        case = cc.Case("golden16", om.net_from_state(sd, "actor.", "actor"), om.net_from_state(sd, "critic.", "critic"),
                       data, vn0, self.data_chunk_length)
        case.huber_delta = 10.0            # (any value: the median does not depend on it)
        chosen["huber_delta"] = self.huber_delta = cc.median_delta(case)
        chosen["clip_param"] = float(self.clip_param)
        return train(self, buffer, *a, **k)

    with tempfile.TemporaryDirectory() as tmp:
        Buffer.compute_returns, Trainer.train, g.OUT = compute_returns_then_perturb, train_with_median_delta, tmp
        try:
            g.train_fixture(m)
        finally:
            Buffer.compute_returns, Trainer.train, g.OUT = compute_returns, train, HERE
        out = dict(np.load(os.path.join(tmp, "mappo_train.npz")))
    assert chosen["clip_param"] == cc.CASES["golden16"][1], chosen
    out["clip_param"] = np.float64(chosen["clip_param"])
    out["huber_delta"] = np.float64(chosen["huber_delta"])
    np.savez(os.path.join(HERE, "mappo_clip_train.npz"), **out)
    print(f"wrote mappo_clip_train.npz (huber_delta {chosen['huber_delta']:.6f}, "
          f"mean ratio {float(out['info.ratio']):.6f})")


if __name__ == "__main__":
    main()
