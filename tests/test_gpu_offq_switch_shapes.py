"""GPU: one OffQMix.train_policy_on_batch (csrc/offq.hip) at D = 3 per case of tests/offq_switch_cases.py against
the CPU oracle in float64, in the scheme of tests/test_gpu_offq_shapes.py: Switch episodes as the batch (the env's
few observation values, LayerNorm-0 rows of zero variance, per-agent dones), the mixer state S = 3 N = 6, 9, 12
(ragged against every GEMM tile), the MFMA weight-gradient jobs with K = 3 (dW1) and M = 3 (LayerNorm 0), split-K,
the second pass of the loss loops, an active clip, and N = 2, T = B = 1.

Gradient bound: relative L2 against float64 <= max(8 x e32, 2e-6), e32 = the float32 oracle's relative L2 for the same
tensor and case. Q bound (get_q_values, the trainer's forward at D = 3): with u(x) = max |x - q64| / (1e-4 |q64| +
1e-5), u(q_hip) <= max(1, 8 u(q32)); LayerNorm 0 over three nearly equal features multiplies rounding by up to
1 / sqrt(1e-5), so the project's fixed Q tolerance is not the float32 oracle's own error here.
Measured worst err_hip / e32 per case (tensor, its err_hip) and u(q_hip) / u(q32), MI355X:
  sw_one_row   1.47 (ln0_b, 1.2e-6)             Q 0.03 / 0.09    sw_n3_splitk 2.14 (hyper_b2.0.bias, 2.6e-7)  Q 0.10 / 0.15
  sw_n4_vdn    4.16 (ln0_w, 2.9e-7)             Q 0.12 / 0.09    sw_clip_1025 17.5 (hyper_b2.2.bias, 1.8e-7)  Q 0.13 / 0.17
  sw_ref_shape 1.59 (hyper_b2.2.bias, 2.0e-7)   Q 0.30 / 0.44
No tensor of any case is off by more than 1.3e-6, so every one passes on the 2e-6 floor alone; the ratio 17.5 is the
one-element hyper_b2.2.bias (the plain sum of dQ_tot), whose e32 of 1e-8 is the rounding of a single float32 sum.
No tensor's 8 x e32 exceeds 1e-3: the largest e32 is 1.2e-5, the one-element hyper_w2.2.weight of sw_one_row
(K = Hh = 1; tests/test_offq_switch_oracle_fp64.py asserts it). get_q_values alone: u(q_hip) / u(q32) = 0.005 / 0.012
(1 x 1 rows), 0.44 / 0.37 (7 x 300), 0.50 / 0.38 (3 x 5500): D = 3 with the oracle's N(0, 0.2) weights stays inside
the fixed bound; the head scaled by 10 over 100 steps (tests/test_gpu_offq_switch_collect.py) does not.
"""
import functools

import numpy as np
import pytest
import torch

from offq_switch_cases import CASES, build_case, grad_keys, q_units, rel_l2
from oracle import offq as ref
from test_gpu_offq_shapes import FLOOR, RATIO, one_update, sample

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def run_case(cid):
    return one_update(build_case(cid), True)


def q_bound(c):
    """(u(q32), the bound on u(q_hip))."""
    u32 = q_units(c.q32.numpy(), c.q64.numpy())
    return u32, max(1.0, RATIO * u32)


@pytest.mark.parametrize("cid", list(CASES))
def test_offq_switch_q_loss_priorities(cid):
    c, o = build_case(cid), run_case(cid)
    q64 = c.q64.numpy()
    u32, bound = q_bound(c)
    u = q_units(o["q"].numpy(), q64)
    print(f"{cid} Q: u(q_hip) {u:.3g} u(q32) {u32:.3g} bound {bound:.3g} max |q64| {np.abs(q64).max():.3g}")
    assert u <= bound
    assert np.array_equal(o["q"].numpy().argmax(-1), q64.argmax(-1))
    for k, k64 in (("loss", "loss"), ("Q_tot", "q_tot"), ("grad_norm", "grad_norm")):
        print(f"{cid} {k}: hip {o[k]:.9g} fp64 {c.info64[k64]:.9g} rel {abs(o[k] / c.info64[k64] - 1):.3g}")
    np.testing.assert_allclose(o["loss"], c.info64["loss"], rtol=2e-5)
    np.testing.assert_allclose(o["Q_tot"], c.info64["q_tot"], rtol=2e-5)
    np.testing.assert_allclose(o["grad_norm"], c.info64["grad_norm"], rtol=2e-5)
    if c.use_per:
        np.testing.assert_allclose(o["prio"].numpy(), c.info64["priorities"], rtol=2e-5)
    else:
        assert o["prio"] is None


@pytest.mark.parametrize("cid", list(CASES))
def test_offq_switch_gradients(cid):
    c, o = build_case(cid), run_case(cid)
    g64, g32 = c.info64["raw_grads"], c.info32["raw_grads"]
    gmax = max(float(g.abs().max()) for g in g64.values())
    bad, worst, above = [], (0.0, None, 0.0), (0.0, None, 0.0)
    for kind, k in grad_keys(c):
        g = o["grad_of"][kind, k]
        assert g.shape == tuple(g64[k].shape)
        if not bool(g64[k].any()):
            if not np.abs(g).max() <= FLOOR * gmax:
                bad.append(f"{k}: fp64 gradient is 0, hip max |g| {np.abs(g).max():.3g} > {FLOOR * gmax:.3g}")
            continue
        e32, e = rel_l2(g32[k].numpy(), g64[k].numpy()), rel_l2(g, g64[k].numpy())
        if e / e32 > worst[0]:
            worst = (e / e32, k, e)
        if e > FLOOR and e / e32 > above[0]:
            above = (e / e32, k, e)
        if not e <= max(RATIO * e32, FLOOR):
            bad.append(f"{k}: rel L2 {e:.3g} > max({RATIO:g} x {e32:.3g}, {FLOOR:g})")
    print(f"{cid}: worst err_hip / e32 = {worst[0]:.2f} ({worst[1]}, err {worst[2]:.3g}); "
          f"among errors above the floor: {above[0]:.2f} ({above[1]}, err {above[2]:.3g})")
    assert not bad, "\n".join(bad)
    # the pad column of W1 (rows of Dp = 4 floats at offset 2 Dp of the flat MGeo<3, 64, 5> layout) gets no gradient
    assert float(o["grad"][8:8 + 64 * 4].view(64, 4)[:, 3].abs().max()) == 0.0


@pytest.mark.parametrize("cid", list(CASES))
def test_offq_switch_updated_parameters(cid):
    c, o = build_case(cid), run_case(cid)
    for kind, k in grad_keys(c):
        new64 = (c.P64 if kind == "agent" else c.M64)[k].numpy()
        np.testing.assert_allclose(o["P_of"][kind, k], new64, rtol=1e-5, atol=2e-6, err_msg=k)


@pytest.mark.parametrize("cid", list(CASES))
def test_offq_switch_deterministic_and_ignores_agent_dones(cid):
    """A second trainer on the same inputs gives the same bits (split-K and the row-block partials sum in a fixed
    order), also with every per-agent done flag inverted: the loss reads dones_env only."""
    c, o = build_case(cid), run_case(cid)
    c2 = type(c)()
    c2.__dict__.update(c.__dict__)
    c2.batch = dict(c.batch, dones=1.0 - c.batch["dones"])
    assert len(sample(c2)) == 9
    o2 = one_update(c2, False)
    assert torch.equal(o["grad"], o2["grad"]) and torch.equal(o["P"], o2["P"])
    assert (o["prio"] is None and o2["prio"] is None) or torch.equal(o["prio"], o2["prio"])


def test_offq_switch_unsupported_dims_message():
    from minimarl.offq import OffQMix
    with pytest.raises(RuntimeError, match=r"D 3\|47\|94"):
        OffQMix(2, 4, 5, 4, 4, mixer="vdn")


@pytest.mark.parametrize("L,R,target", [(1, 1, False), (7, 300, False), (3, 5500, True)])
def test_offq_switch_q_values_vs_fp64(L, R, target):
    """get_q_values on its own at D = 3, non-zero h0, Switch observation values; 3 x 5500 rows are past the one-net
    cap of 256 blocks of 64 rows."""
    from minimarl.offq import OffQMix
    from offq_cases import A, H, random_agent
    from test_gpu_offq_shapes import agent_sd
    P, PT = random_agent(211, 3), random_agent(212, 3)
    tr = OffQMix(2, 3, A, 2, 2, mixer="vdn")
    tr.load_reference_state(agent_sd(P), None, agent_sd(PT), None)
    rng = np.random.default_rng(213)
    x = np.stack([rng.integers(0, 3, (L, R)) / 2.0, np.round(rng.integers(0, 7, (L, R)) / 6.0, 2),
                  rng.integers(0, 101, (L, R)) / 100.0], -1).astype(np.float32)
    x = torch.tensor(x)
    h0 = torch.tensor(rng.standard_normal((R, H)).astype(np.float32) * 0.3)
    with torch.no_grad():
        q64, h64 = ref.agent_q_seq(PT if target else P, x, h0, dtype=torch.float64)
        q32, _ = ref.agent_q_seq(PT if target else P, x, h0, dtype=torch.float32)
    q, h = tr.get_q_values(x.cuda(), h0.cuda(), target=target)
    assert q.shape == (L, R, A) and h.shape == (R, H)
    u32, u = q_units(q32.numpy(), q64.numpy()), q_units(q.cpu().numpy(), q64.numpy())
    print(f"L{L} R{R}: u(q_hip) {u:.3g} u(q32) {u32:.3g}")
    assert u <= max(1.0, RATIO * u32)
    np.testing.assert_allclose(h.cpu().numpy(), h64.numpy(), rtol=1e-4, atol=1e-5)
