"""Golden vectors for the offpolicy transition replay (``MlpReplayBuffer`` / ``PrioritizedMlpReplayBuffer``,
offpolicy/utils/mlp_buffer.py:10-340 over offpolicy/utils/segment_tree.py).

Runs only where the reference checkout is present (``REF`` below, read-only); the tests read ``mlpbuf_*.npz`` only. A
fixed op sequence is run through the reference classes with the numpy draws of each ``sample`` read off beforehand
from a saved RNG state, so tests can inject them: size 10 (tree capacity 16), N 2, D 3, A 5, S 6; inserts of 4, 4, 4
(the third wraps) and 3, a sample of 5, update_priorities with a duplicate index and a new maximum, a second sample.
Recorded after every op: the nine stores, both trees, max_priority, the length; per insert its inputs and idx_range;
per sample the indices, weights and the eleven fields.

  mlpbuf_per.npz  PrioritizedMlpReplayBuffer      mlpbuf_uni.npz  MlpReplayBuffer (uniform)
  mlpbuf_per_full.npz  PrioritizedMlpReplayBuffer, inserts of 5, 5, 2 and a sample: after the second insert the
                       reference's cursor is current_i = size, and the third writes slots 0, 1 and leaf 0

Usage (from the repository root):  python tests/golden/make_golden_mlpbuf.py
"""
import importlib
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_offq import Box, Discrete, install_gym  # noqa: E402

REF = "/root/reference/offpolicy"
SIZE, N, D, A = 10, 2, 3, 5
S = N * D
FIELDS = ["obs", "share_obs", "acts", "rewards", "next_obs", "next_share_obs", "dones", "dones_env",
          "valid_transition"]
SCRIPT = [("insert", 4), ("insert", 4), ("insert", 4), ("insert", 3), ("sample", 5, 0.5), ("update",),
          ("sample", 5, 0.7)]
# the second insert leaves the cursor at current_i = size: the third starts at slot 0 and writes leaf 0
SCRIPT_FULL = [("insert", 5), ("insert", 5), ("insert", 2), ("sample", 5, 0.5)]


def load():
    install_gym()
    sys.path.insert(0, REF)
    try:
        return importlib.import_module("utils.mlp_buffer")
    finally:
        sys.path.pop(0)


def transitions(rng, n):
    f32 = np.float32
    flag = lambda *s: (rng.random(s) < 0.3).astype(f32)   # noqa: E731
    return [rng.standard_normal((n, N, D)).astype(f32), rng.standard_normal((n, S)).astype(f32),
            np.eye(A, dtype=f32)[rng.integers(0, A, (n, N))], rng.standard_normal((n, N, 1)).astype(f32),
            rng.standard_normal((n, N, D)).astype(f32), rng.standard_normal((n, S)).astype(f32),
            flag(n, N, 1), flag(n, 1), flag(n, N, 1)]


def run(mod, prioritized, seed, script=SCRIPT):
    np.random.seed(seed)
    rng = np.random.default_rng(seed + 1)
    pinfo = {"policy_0": {"obs_space": Box(shape=(D,)), "share_obs_space": Box(shape=(S,)), "act_space": Discrete(A)}}
    pagents = {"policy_0": list(range(N))}
    if prioritized:
        buf = mod.PrioritizedMlpReplayBuffer(0.6, pinfo, pagents, SIZE, True, False)
    else:
        buf = mod.MlpReplayBuffer(pinfo, pagents, SIZE, True, False)
    pb = buf.policy_buffers["policy_0"]
    none = {"policy_0": None}
    out, ops, last_idx = {}, [], None
    for i, op in enumerate(script):
        p = f"op{i}_"
        if op[0] == "insert":
            tr = transitions(rng, op[1])
            out[p + "idx_range"] = np.asarray(buf.insert(op[1], *[{"policy_0": x} for x in tr], none, none), np.int64)
            for k, x in zip(FIELDS, tr):
                out[p + k] = x
            ops.append([0, op[1], i])
        elif op[0] == "sample":
            B = op[1]
            st = np.random.get_state()
            draw = np.random.random(size=B) if prioritized else np.random.choice(len(buf), B)
            np.random.set_state(st)
            res = buf.sample(B, op[2], "policy_0") if prioritized else buf.sample(B)
            if prioritized:
                out[p + "fracs"], out[p + "beta"] = draw, np.float64(op[2])
                out[p + "weights"] = np.asarray(res[11], np.float64)
                last_idx = np.asarray(res[12], np.int64)
            out[p + "idx"] = last_idx if prioritized else np.asarray(draw, np.int64)
            for k, x in zip(FIELDS, res[:9]):
                out[p + "out_" + k] = np.asarray(x["policy_0"], np.float32)
            assert res[9]["policy_0"] is None and res[10]["policy_0"] is None
            ops.append([1, B, i])
        elif prioritized:
            prio = (0.2 + 0.7 * rng.random(len(last_idx))).astype(np.float32)
            prio[1] = 3.5                                      # a new maximum
            idx = last_idx.copy()
            idx[-1] = idx[0]                                   # a duplicate index: last write wins
            buf.update_priorities(idx, prio, "policy_0")
            out[p + "idx"], out[p + "prio"] = idx, prio
            ops.append([2, len(idx), i])
        else:
            continue
        for k in FIELDS:
            out[p + "store_" + k] = getattr(pb, k).copy()
        if prioritized:
            out[p + "sum"] = np.asarray(buf._it_sums["policy_0"]._value, np.float64).copy()
            out[p + "min"] = np.asarray(buf._it_mins["policy_0"]._value, np.float64).copy()
            out[p + "max_p"] = np.float64(buf.max_priorities["policy_0"])
        out[p + "len"] = np.int64(len(buf))
    out["ops"] = np.asarray(ops, np.int64)
    out["meta"] = np.array([SIZE, N, D, S, A, int(prioritized)], np.int64)
    return out


def main():
    mod = load()
    for name, pri, seed, script in (("per", True, 21, SCRIPT), ("uni", False, 22, SCRIPT),
                                    ("per_full", True, 23, SCRIPT_FULL)):
        out = run(mod, pri, seed, script)
        np.savez_compressed(os.path.join(HERE, f"mlpbuf_{name}.npz"), **out)
        print(f"wrote mlpbuf_{name}.npz ({len(out['ops'])} ops)")


if __name__ == "__main__":
    main()
