"""Generate the golden vectors of MAPPO's PPO minibatches (train_batch_size > 1) by importing the reference.

Runs ONLY in the build container (needs the reference checkout, read-only; see make_golden_mappo.py, whose loader,
gym stand-in and train fixture this script reuses); the GPU box only reads the fixture written next to this script.

  mappo_mb_train.npz  R_MAPPO.train (mappo/algorithms/ramppo_network.py:211-287) with train_batch_size 3 on the
                      synthetic rollout of mappo_train.npz (E 4, N 2, T 10, L 5, 3 epochs): 16 chunks, per epoch one
                      torch.randperm (shared_buffer.py:318-331) cut into 3 minibatches of 5 chunks, 1 chunk dropped;
                      9 ppo_updates, each with its own ValueNorm.update(return_batch) (ramppo_network.py:72-73).
                      Recorded: perms [3, 16] (the reference's chunk numbering), the 18 pre-clip norms (actor,
                      critic per update), before / after parameters, the ValueNorm state, info.*, and the clipped
                      gradients of the first two updates only (all nine would double the file).

Usage (from the repository root):  python tests/golden/make_golden_mappo_mb.py
"""
import os
import sys
import tempfile

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_mappo as g  # noqa: E402

TRAIN_BATCH_SIZE = 3
KEEP_GRAD_UPDATES = 2


def main():
    m = g.load()
    make_args = g.make_args
    with tempfile.TemporaryDirectory() as tmp:
        # train_fixture with one more argument for the reference, written to a scratch directory
        g.make_args = lambda mod, **kw: make_args(mod, **dict(kw, train_batch_size=TRAIN_BATCH_SIZE))
        g.OUT = tmp
        try:
            g.train_fixture(m)
        finally:
            g.make_args, g.OUT = make_args, HERE
        fx = dict(np.load(os.path.join(tmp, "mappo_train.npz")))
    n_chunks = int(fx["T"]) * int(fx["E"]) * int(fx["N"]) // int(fx["L"])
    updates = int(fx["epochs"]) * TRAIN_BATCH_SIZE
    assert fx["perms"].shape == (int(fx["epochs"]), n_chunks), fx["perms"].shape
    assert fx["norms"].shape == (2 * updates,), fx["norms"].shape
    out = {}
    for k, v in fx.items():
        if k.startswith("grad"):
            idx = int(k.split(".", 1)[0][5:])      # grada<i>.<name> / gradc<i>.<name>
            assert idx < updates, k
            if idx >= KEEP_GRAD_UPDATES:
                continue
        out[k] = v
    out["train_batch_size"] = np.int64(TRAIN_BATCH_SIZE)
    np.savez(os.path.join(HERE, "mappo_mb_train.npz"), **out)
    print("wrote mappo_mb_train.npz")


if __name__ == "__main__":
    main()
