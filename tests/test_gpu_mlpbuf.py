"""Device transition replay (mm_mlpbuf_*, minimarl.mlpbuf) vs the reference's own op sequence
(tests/golden/mlpbuf_*.npz from offpolicy/utils/mlp_buffer.py + segment_tree.py) and a plain numpy ring.

Tolerances, those of tests/test_gpu_recbuf.py for the same quantities: stores, gathered fields, indices and ring slots
bit-exact (byte movement); tree nodes within 4e-7 relative (a leaf is float32 prio ** alpha: numpy's powf vs the
device's correctly rounded f64 pow can differ by one float32 ulp); IS weights within 1e-6 relative."""
import os

import numpy as np
import pytest
import torch

from test_gpu_recbuf import Box, Discrete, tree_close

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
FIELDS = ["obs", "share_obs", "acts", "rewards", "next_obs", "next_share_obs", "dones", "dones_env", "valid_transition"]
PID = "policy_0"


def make(pri, size, N, D, S, A, **kw):
    from minimarl.mlpbuf import MlpReplayBuffer, PrioritizedMlpReplayBuffer
    pinfo = {PID: {"obs_space": Box((D,)), "share_obs_space": Box((S,)), "act_space": Discrete(A)}}
    pag = {PID: list(range(N))}
    kw = dict(dict(use_same_share_obs=True, use_avail_acts=False, device="cuda"), **kw)
    return PrioritizedMlpReplayBuffer(0.6, pinfo, pag, size, **kw) if pri else MlpReplayBuffer(pinfo, pag, size, **kw)


def stores(buf):
    """Every slot of the ring, never-written ones included, as host arrays [size, row] (the stored fields only)."""
    res, f = buf.sample_inds(torch.arange(buf.buffer_size, device="cuda")), buf.stores()
    out = {k: x[PID].cpu().numpy() for k, x in zip(FIELDS, res[:9]) if getattr(f, k)}
    return {k: x.transpose(1, 0, 2) if len(buf.rows[k]) == 2 else x for k, x in out.items()}


@pytest.mark.parametrize("name", ["per", "uni", "per_full"])   # per_full: an insert that starts at current_i = size
def test_replays_reference_sequence(name):
    z = np.load(os.path.join(GOLD, f"mlpbuf_{name}.npz"))
    SIZE, N, D, S, A, pri = [int(x) for x in z["meta"]]
    buf = make(bool(pri), SIZE, N, D, S, A)
    for kind, n, i in z["ops"]:
        p = f"op{i}_"
        if kind == 0:
            got = buf.insert(int(n), *[{PID: z[p + k]} for k in FIELDS], {PID: None}, {PID: None})
            np.testing.assert_array_equal(got, z[p + "idx_range"])
            assert buf.current_i == int(z[p + "idx_range"][-1]) + 1      # the reference's cursor, in (0, size]
        elif kind == 1:
            if pri:
                res = buf.sample(int(n), float(z[p + "beta"]), PID, fracs=z[p + "fracs"])
                np.testing.assert_array_equal(res[12].cpu().numpy(), z[p + "idx"], err_msg=p)
                assert res[11].dtype == torch.float32
                np.testing.assert_allclose(res[11].cpu().numpy(), z[p + "weights"], rtol=1e-6, err_msg=p)
            else:
                res = buf.sample(int(n), inds=z[p + "idx"])
                assert res[11] is None and res[12] is None
            for k, x in zip(FIELDS, res[:9]):
                np.testing.assert_array_equal(x[PID].cpu().numpy(), z[p + "out_" + k], err_msg=p + k)
            assert res[9][PID] is None and res[10][PID] is None
        else:
            buf.update_priorities(torch.as_tensor(z[p + "idx"]).cuda(), torch.as_tensor(z[p + "prio"]).cuda(), PID)
        for k, x in stores(buf).items():
            np.testing.assert_array_equal(x, z[p + "store_" + k], err_msg=p + k)
        if pri:
            s, m = buf.trees()
            tree_close(s, z[p + "sum"], p + "sum")
            tree_close(m, z[p + "min"], p + "min")
            assert np.float32(buf.max_priority()) == np.float32(z[p + "max_p"]), p
        assert len(buf) == int(z[p + "len"])
    buf.check_errors()


def test_slots_ring_without_share_store():
    """leaf_mode="slots", store_share=False against a numpy ring: inserts of 5, 9 (wraps) and 1 into 12 slots."""
    SIZE, N, D, A = 12, 3, 4, 5
    rng = np.random.default_rng(4)
    buf = make(True, SIZE, N, D, N * D, A, leaf_mode="slots", store_share=False)
    ring = {k: np.zeros((SIZE,) + buf.rows[k], np.float32) for k in FIELDS if "share" not in k}
    ring["dones"][:], ring["dones_env"][:] = 1, 1
    cur, written = 0, set()
    for n in (5, 9, 1):
        tr = {k: rng.standard_normal((n,) + buf.rows[k]).astype(np.float32) for k in FIELDS}
        slots = (cur + np.arange(n)) % SIZE
        np.testing.assert_array_equal(buf.insert(n, *[tr[k] for k in FIELDS]), slots)   # the share arguments are ignored
        for k in ring:
            ring[k][slots] = tr[k]
        cur, written = int(slots[-1]) + 1, written | set(slots.tolist())
        assert buf.current_i == cur and len(buf) == len(written)
        s, m = buf.trees()
        leaves = s[16:16 + SIZE]
        assert set(np.nonzero(leaves)[0].tolist()) == written and (leaves[sorted(written)] == 1.0).all()
        assert m[1] == 1.0 and s[1] == len(written)
    f = buf.stores()
    assert not f.share_obs and not f.next_share_obs
    for k, x in stores(buf).items():
        np.testing.assert_array_equal(x, ring[k], err_msg=k)
    idx = np.array([11, 0, 3, 3, 7, 10, 2])
    res = buf.sample_inds(torch.as_tensor(idx).cuda())
    for k, x in zip(FIELDS, res[:9]):
        src = ring[k.replace("share_", "")][idx]
        want = src.reshape(len(idx), -1) if "share" in k or k == "dones_env" else src.transpose(1, 0, 2)
        np.testing.assert_array_equal(x[PID].cpu().numpy(), want, err_msg=k)
    buf.check_errors()
    out = buf.sample_inds(torch.tensor([1, SIZE, -1], device="cuda"))         # out of range: zeros and the error word
    assert float(out[0][PID][:, 1:].abs().sum()) == 0.0 and float(out[7][PID][1:].abs().sum()) == 0.0
    np.testing.assert_array_equal(out[0][PID][:, 0].cpu().numpy(), ring["obs"][1])
    with pytest.raises(AssertionError, match="outside the buffer"):
        buf.check_errors()


def test_options_that_are_not_built_raise():
    from minimarl.mlpbuf import MlpReplayBuffer
    info = {"obs_space": Box((3,)), "share_obs_space": Box((6,)), "act_space": Discrete(5)}
    for kw in (dict(use_avail_acts=True), dict(use_reward_normalization=True), dict(use_same_share_obs=False)):
        with pytest.raises(NotImplementedError):
            make(False, 8, 2, 3, 6, 5, **kw)
    with pytest.raises(NotImplementedError, match="one policy"):
        MlpReplayBuffer({PID: info, "policy_1": info}, {PID: [0], "policy_1": [1]}, 8, True, False)
    with pytest.raises(ValueError, match="N \\* D"):
        make(False, 8, 2, 3, 7, 5, store_share=False)
    buf = make(True, 8, 2, 3, 6, 5)                               # leaf_mode reference: the reference reads idx_range[1]
    one = [np.zeros((1,) + buf.rows[k], np.float32) for k in FIELDS]
    with pytest.raises(ValueError, match="at least 2"):
        buf.insert(1, *one)
    assert len(buf) == 0
