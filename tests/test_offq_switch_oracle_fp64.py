"""CPU: the cases of tests/offq_switch_cases.py (the trainer at D = 3 on Switch episodes) in the offpolicy oracle's
float64 mode against its float32 mode, and what the cases are for: per-agent dones that the loss ignores, degenerate
LayerNorm-0 rows, the fixed dones_env episodes, both Huber branches, the active clip (no device is touched)."""
import numpy as np
import pytest
import torch

from offq_switch_cases import CASES, build_case, grad_keys, huber_fraction_above, q_units, rel_l2
from offq_switch_ref import ln0_variance
from oracle import offq as ref

# fp32 vs fp64 of the same arithmetic. Measured per tensor: 2e-7 .. 8e-7, but 1.2e-5 for the one-element
# hyper_w2.2.weight of sw_one_row (K = Hh = 1)
GRAD_REL_L2 = {"sw_one_row": 5e-5}
GRAD_REL_L2_DEFAULT = 5e-6


@pytest.mark.parametrize("cid", list(CASES))
def test_offq_switch_oracle_fp32_vs_fp64(cid):
    c = build_case(cid)
    assert c.info64["raw_grads"]["W1"].dtype == torch.float64 and c.info32["raw_grads"]["W1"].dtype == torch.float32
    assert tuple(c.info64["raw_grads"]["W1"].shape) == (64, 3)
    if c.mixer == "qmix":
        assert tuple(c.info64["raw_grads"]["hyper_w1.0.weight"].shape) == (c.Hh, 3 * c.N)
    assert torch.equal(c.q32.argmax(-1), c.q64.argmax(-1))
    u32 = q_units(c.q32.numpy(), c.q64.numpy())
    gmax = max(float(g.abs().max()) for g in c.info64["raw_grads"].values())
    worst = (0.0, None)
    for kind, k in grad_keys(c):
        g64, g32 = c.info64["raw_grads"][k].numpy(), c.info32["raw_grads"][k].numpy()
        if not np.any(g64):
            assert np.abs(g32).max() <= 2e-6 * gmax, k
            continue
        e = rel_l2(g32, g64)
        worst = max(worst, (e, k))
        assert e <= GRAD_REL_L2.get(cid, GRAD_REL_L2_DEFAULT), (k, e)
        assert 8 * e <= 1e-3, (k, e)          # no tensor's yardstick makes the GPU bound 8 x e32 meaningless
    print(f"{cid}: worst fp32-vs-fp64 gradient rel L2 {worst[0]:.3g} ({worst[1]}), u(q32) {u32:.3g}, "
          f"top-2 gap {c.top2_gap:.3g}, kink margin {c.kink_margin:.3g}")
    np.testing.assert_allclose(c.info32["loss"], c.info64["loss"], rtol=2e-5)
    np.testing.assert_allclose(c.info32["grad_norm"], c.info64["grad_norm"], rtol=2e-5)
    for kind, k in grad_keys(c):
        new32, new64 = (c.P32, c.P64) if kind == "agent" else (c.M32, c.M64)
        np.testing.assert_allclose(new32[k].numpy(), new64[k].numpy(), rtol=1e-5, atol=2e-6, err_msg=k)
    if c.use_per:
        np.testing.assert_allclose(c.info32["priorities"], c.info64["priorities"], rtol=2e-5)


def test_offq_switch_case_preconditions():
    for cid in CASES:
        c = build_case(cid)
        b = c.batch
        assert b["obs"].shape == (c.N, c.T + 1, c.B, 3) and b["share_obs"].shape == (c.T + 1, c.B, 3 * c.N)
        # share_obs is the agents' observations concatenated; the observations take the env's values only
        np.testing.assert_array_equal(b["share_obs"], np.concatenate(list(b["obs"]), -1))
        assert set(np.unique(b["obs"][..., 0])) <= {0.0, 0.5, 1.0}
        assert set(np.unique(b["obs"][..., 1])) <= {np.float32(round(k / 6, 2)) for k in range(7)}
        if c.huber:
            assert 0.25 <= huber_fraction_above(c) <= 0.75, (cid, huber_fraction_above(c))
        if c.T == 1:
            assert not bool(c.info64["raw_grads"]["Whh"].any())
    c = build_case("sw_clip_1025")
    assert c.info64["grad_norm"] > 2 * c.max_norm                      # clip active
    e = c.info64["err"].reshape(-1)[1024:]
    assert e.numel() == 1 and float(c.info64["mask"].reshape(-1)[1024]) == 1.0 and abs(float(e)) > 0.1
    c = build_case("sw_ref_shape")
    var = ln0_variance(c.batch["obs"])
    assert var.min() == 0.0 and (var < 1e-4).sum() >= 10               # degenerate LayerNorm-0 rows
    de = c.batch["dones_env"]
    assert (de[:, 0] == 1).all() and (de[:, 1] == 0).all() and de[:, 2, 0].tolist() == [0.0] * (c.T - 1) + [1.0]
    assert (c.batch["dones"] != de[None]).any()                        # per agent, not the env's


@pytest.mark.parametrize("cid", ["sw_n4_vdn", "sw_ref_shape"])
def test_offq_switch_loss_ignores_agent_dones(cid):
    c = build_case(cid)
    b2 = dict(c.batch)
    b2["dones"] = 1.0 - c.batch["dones"]
    _, _, info = ref.train_batch(c.P, c.M, c.PT, c.MT, b2, dtype=torch.float64, **c.kw)
    assert info["loss"] == c.info64["loss"]
    for k, g in c.info64["raw_grads"].items():
        assert torch.equal(g, info["raw_grads"][k]), k
