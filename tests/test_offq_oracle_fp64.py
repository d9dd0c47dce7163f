"""CPU: the offpolicy oracle's float64 mode (oracle.offq.train_batch(dtype=torch.float64), the reference of
tests/test_gpu_offq_shapes.py) against its float32 mode on cases of tests/offq_cases.py, and the
mixer_hidden <= 64 limit on both sides of the C ABI (no device is touched)."""
import ctypes

import numpy as np
import pytest
import torch

from offq_cases import build_case, grad_keys, huber_fraction_above, rel_l2
from oracle import offq as ref

# fp32 vs fp64 of the same arithmetic: 2e-7 .. 8e-7 measured per tensor at these shapes
GRAD_REL_L2 = 5e-6


@pytest.mark.parametrize("cid", ["one_row", "odd_d94", "loss_1025", "ref_shape"])
def test_offq_oracle_fp32_vs_fp64(cid):
    c = build_case(cid)
    assert c.info64["raw_grads"]["W1"].dtype == torch.float64 and c.P64["W1"].dtype == torch.float64
    assert c.info32["raw_grads"]["W1"].dtype == torch.float32 and c.P32["W1"].dtype == torch.float32
    if c.use_per:
        assert c.info64["priorities"].dtype == np.float64 and c.info32["priorities"].dtype == np.float32
    # greedy actions of the behavior net over every row-step
    with torch.no_grad():
        q32, _ = ref.agent_q_seq(c.P, ref.stack_agents(torch.tensor(c.batch["obs"])))
    assert q32.dtype == torch.float32 and c.q64.dtype == torch.float64
    assert torch.equal(q32.argmax(-1), c.q64.argmax(-1))
    gmax = max(float(g.abs().max()) for g in c.info64["raw_grads"].values())
    worst = 0.0
    for kind, k in grad_keys(c):
        g64, g32 = c.info64["raw_grads"][k].numpy(), c.info32["raw_grads"][k].numpy()
        if not np.any(g64):
            assert np.abs(g32).max() <= 2e-6 * gmax, k
            continue
        e = rel_l2(g32, g64)
        worst = max(worst, e)
        assert e <= GRAD_REL_L2, (k, e)
    print(f"{cid}: worst fp32-vs-fp64 gradient rel L2 {worst:.3g}, top-2 gap {c.top2_gap:.3g}, "
          f"kink margin {c.kink_margin:.3g}")
    np.testing.assert_allclose(c.info32["loss"], c.info64["loss"], rtol=2e-5)
    np.testing.assert_allclose(c.info32["grad_norm"], c.info64["grad_norm"], rtol=2e-5)
    # the post-update bound of the GPU test must hold for the fp32 oracle itself
    for kind, k in grad_keys(c):
        new32, new64 = (c.P32, c.P64) if kind == "agent" else (c.M32, c.M64)
        np.testing.assert_allclose(new32[k].numpy(), new64[k].numpy(), rtol=1e-5, atol=2e-6, err_msg=k)
    if c.use_per:
        np.testing.assert_allclose(c.info32["priorities"], c.info64["priorities"], rtol=2e-5)


def test_offq_case_preconditions():
    """What the cases are for holds in the float64 oracle: Huber cases use both branches, the clip is
    active in loss_1025 and inactive in odd_d94, W_hh gets an exactly zero gradient at T = 1."""
    for cid in ("odd_d94", "loss_1025"):
        c = build_case(cid)
        assert c.huber and 0.25 <= huber_fraction_above(c) <= 0.75, (cid, huber_fraction_above(c))
    assert build_case("loss_1025").info64["grad_norm"] > 2 * 0.05
    assert build_case("odd_d94").info64["grad_norm"] < 0.5e6
    assert not bool(build_case("one_row").info64["raw_grads"]["Whh"].any())


@pytest.mark.parametrize("K", [65, 128])
def test_offq_mixer_hidden_above_64_rejected(K):
    from minimarl._lib import MM_OFFQ_QMIX, OffqBatch, OffqDims, c_i64, lib
    from minimarl.offq import OffQMix
    with pytest.raises(ValueError, match="64"):
        OffQMix(2, 47, 5, 4, 4, mixer="qmix", mixer_hidden=K)
    L = lib()
    d = OffqDims(2, 47, 64, 5, MM_OFFQ_QMIX, 94, K, 64)
    na, nm, offs = c_i64(), c_i64(), (c_i64 * 15)()
    assert L.mm_offq_param_counts(ctypes.byref(d), ctypes.byref(na), ctypes.byref(nm)) == -22
    assert b"64" in L.mm_last_error()
    assert L.mm_offq_mixer_offsets(ctypes.byref(d), offs) == -22
    assert L.mm_offq_workspace_bytes(ctypes.byref(d), 4, 4) == -1
    bt = OffqBatch()
    assert L.mm_offq_loss_grad(ctypes.byref(d), ctypes.byref(bt), None, None, None, None, 0, None, None, None) == -22
    assert b"mixer_hidden" in L.mm_last_error()


def test_offq_mixer_hidden_64_accepted_by_abi():
    from minimarl._lib import MM_OFFQ_QMIX, OffqDims, c_i64, lib
    d = OffqDims(2, 47, 64, 5, MM_OFFQ_QMIX, 94, 64, 100)
    na, nm = c_i64(), c_i64()
    assert lib().mm_offq_param_counts(ctypes.byref(d), ctypes.byref(na), ctypes.byref(nm)) == 0
    assert lib().mm_offq_workspace_bytes(ctypes.byref(d), 8, 32) > 0
