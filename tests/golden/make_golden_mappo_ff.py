"""Generate the golden vectors of feed-forward MAPPO (algorithm_name "mappo": use_recurrent_policy and
use_naive_recurrent_policy False, mappo/main.py:62-65) by importing the reference.

Runs ONLY in the build container (needs the reference checkout, read-only; see make_golden_mappo.py, whose loader,
gym stand-in and fixtures this script reuses with the two recurrent flags off); the GPU box only reads the fixtures
written next to this script. Without the flags R_Actor / R_Critic hold no RNNLayer (r_actor_critic.py:46,84,123,168,
204): 12 tensors per net (the built but unused base.mlp.fc_h is dropped here), rnn_states pass through unchanged, and
R_MAPPO.train draws its minibatches from feed_forward_generator (shared_buffer.py:159-219): one torch.randperm of the
T * E * N rows (numbered by reshape(-1) of [T, E, N]: row = t * E * N + e * N + n, the buffer's own numbering) per
epoch, cut into train_batch_size slices, the remainder dropped.

  mappo_ff_fwd.npz    R_MAPPOPolicy.get_actions / get_values (rmappo_policy.py:57-99) on mappo_fwd.npz's inputs with
                      the drawn actions recorded
  mappo_ff_train.npz  R_MAPPO.train with train_batch_size 3 on the E 4, N 2, T 10 synthetic rollout (3 epochs): 80
                      rows, 9 updates of 26 rows (less than one 32-row tile), 2 rows dropped per epoch. Recorded:
                      perms [3, 80], the 18 pre-clip norms, before / after parameters, the ValueNorm state, info.* and
                      the clipped gradients of updates 0, 1 and 2 (the only inactive row, row 55, first appears in
                      update 2, whose active count 25 therefore differs from its 26 rows).

Usage (from the repository root):  python tests/golden/make_golden_mappo_ff.py
"""
import os
import sys
import tempfile

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_mappo as g  # noqa: E402

TRAIN_BATCH_SIZE = 3
KEEP_GRAD_UPDATES = 3
FF = dict(use_recurrent_policy=False, use_naive_recurrent_policy=False)


def keep(k):
    return ".base.mlp.fc_h." not in "." + k


def main():
    m = g.load()
    make_args, policy_cls = g.make_args, m.policy.R_MAPPOPolicy
    made = []

    def policy(*a, **k):
        made.append(policy_cls(*a, **k))
        return made[-1]

    with tempfile.TemporaryDirectory() as tmp:
        g.OUT = tmp
        m.policy.R_MAPPOPolicy = policy
        try:
            g.make_args = lambda mod, **kw: make_args(mod, **dict(kw, **FF))
            g.fwd_fixture(m)
            fwd = dict(np.load(os.path.join(tmp, "mappo_fwd.npz")))
            with torch.no_grad():
                gv = made[-1].get_values(fwd["obs"], fwd["hc"], fwd["masks"]).numpy()
            g.make_args = lambda mod, **kw: make_args(mod, **dict(kw, train_batch_size=TRAIN_BATCH_SIZE, **FF))
            g.train_fixture(m)
            fx = dict(np.load(os.path.join(tmp, "mappo_train.npz")))
        finally:
            g.make_args, g.OUT, m.policy.R_MAPPOPolicy = make_args, HERE, policy_cls

    # ---- forward
    assert not any(".rnn." in "." + k for k in fwd), "the feed-forward nets hold no RNNLayer"
    np.testing.assert_array_equal(fwd["ha_out"], fwd["ha"])
    np.testing.assert_array_equal(fwd["hc_out"], fwd["hc"])
    out = {k: v for k, v in fwd.items() if not k.startswith("seq_") and keep(k)}
    out["get_values"] = gv
    np.savez(os.path.join(HERE, "mappo_ff_fwd.npz"), **out)

    # ---- train
    rows = int(fx["T"]) * int(fx["E"]) * int(fx["N"])
    updates = int(fx["epochs"]) * TRAIN_BATCH_SIZE
    assert fx["perms"].shape == (int(fx["epochs"]), rows), fx["perms"].shape
    assert fx["norms"].shape == (2 * updates,), fx["norms"].shape
    assert not fx["data.rnn_states"].any() and not fx["data.rnn_states_critic"].any()
    out = {}
    for k, v in fx.items():
        if not keep(k) or k in ("data.rnn_states", "data.rnn_states_critic"):
            continue
        if k.startswith("grad"):
            idx = int(k.split(".", 1)[0][5:])      # grada<i>.<name> / gradc<i>.<name>
            assert idx < updates, k
            if idx >= KEEP_GRAD_UPDATES:
                continue
        out[k] = v
    out["train_batch_size"] = np.int64(TRAIN_BATCH_SIZE)
    np.savez(os.path.join(HERE, "mappo_ff_train.npz"), **out)
    inactive = np.flatnonzero(fx["data.active_masks"][:-1].reshape(-1) == 0)
    mbs = rows // TRAIN_BATCH_SIZE
    first = [int(np.flatnonzero(fx["perms"][0] == r)[0]) // mbs for r in inactive]
    print("wrote mappo_ff_fwd.npz, mappo_ff_train.npz; inactive rows", inactive.tolist(), "first in updates", first,
          "norms", np.round(fx["norms"], 3).tolist())


if __name__ == "__main__":
    main()
