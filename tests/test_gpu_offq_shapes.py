"""GPU: one OffQMix.train_policy_on_batch (csrc/offq.hip) per case of tests/offq_cases.py against the CPU
oracle in float64, at the sizes where the host code changes path: split-K of the mixer weight gradients
(T*B > 256), the stride loops of the one-block loss kernel (T*B > 1024), the grid caps of the LDS and
wave kernels, TrunkWgrad::rows_per_block above 128, D = 94, the mixer's lane packing (K = 1, 5, 33, 64),
ragged GEMM tiles, the Huber linear branch, an active and an inactive clip, and N = T = B = 1.

Gradient bound: relative L2 against float64 <= max(8 x e32, 2e-6), e32 = the float32 oracle's relative L2
for the same tensor and case (same arithmetic and precision; the kernels differ in summation order only).
Measured worst err_hip / e32 per case (tensor, its err_hip), MI355X:
  one_row 4.21 (hyper_w2.2.bias, 2.0e-7)    odd_d94 1.76 (hyper_w1.0.bias, 8.1e-7)
  splitk_257 1.08 (hyper_w1.0.bias, 2.7e-7) splitk_256 4.23 (hyper_b2.2.bias, 2.0e-7)
  loss_1025 1.56 (hyper_b2.2.bias, 6.7e-7)  vdn_per 1.12 (bih, 5.1e-7)
  ref_shape 1.21 (hyper_w2.0.bias, 1.1e-7)  wgrad_step 8.58 (hyper_b2.2.bias, 7.5e-7)
No tensor of any case is off by more than 8.1e-7, so every one passes on the 2e-6 floor alone. The ratios above 4
are one- to K-element tensors (hyper_b2.2.bias is the plain sum of dQ_tot) whose e32 is the rounding of a single
float32 sum (2e-8 .. 9e-8), not a spread over many elements; the agent tensors stay below 1.6.

Before the cases kept ReLU inputs away from 0 (offq_cases.MIN_KINK_MARGIN), wgrad_step missed the bound in W2, b2,
ln1_w and ln1_b by 2e-5 .. 7e-5: a layer-2 input of -5.3e-7 in float64 was positive in the kernel (unit 10 of one
row of 52000), and the float32 oracle had flipped a layer-1 input of -2.4e-7 itself. Float32 noise at a kink, not a
summation fault; no kernel was changed for it.
"""
import functools

import numpy as np
import pytest
import torch

from offq_cases import A, CASES, H, HYPER, build_case, grad_keys, huber_fraction_above, random_agent, rel_l2
from oracle import offq as ref

pytestmark = pytest.mark.gpu
FLOOR = 2e-6          # the gradient atol of tests/test_gpu_offq.py, read as a relative value
RATIO = 8.0


def agent_sd(P):
    return {ref.AGENT_REF[k]: v.numpy() for k, v in P.items()}


def make_trainer(c):
    from minimarl.offq import OffQMix
    tr = OffQMix(c.N, c.D, A, c.T, c.B, mixer=c.mixer, mixer_hidden=c.K, hyper_hidden=c.Hh, gamma=HYPER["gamma"],
                 lr=HYPER["lr"], opti_eps=HYPER["eps"], max_grad_norm=c.max_norm, use_double_q=c.double_q,
                 use_per=c.use_per, use_huber_loss=c.huber, huber_delta=c.huber_delta, per_nu=HYPER["per_nu"],
                 per_eps=HYPER["per_eps"])
    qm = c.mixer == "qmix"
    tr.load_reference_state(agent_sd(c.P), {k: v.numpy() for k, v in c.M.items()} if qm else None,
                            agent_sd(c.PT), {k: v.numpy() for k, v in c.MT.items()} if qm else None)
    return tr


def sample(c):
    pid, b = "policy_0", c.batch
    return ({pid: b["obs"]}, {pid: b["share_obs"]}, {pid: b["acts"]}, {pid: b["rewards"]}, {pid: b["dones"]},
            {pid: b["dones_env"]}, {pid: None}, b["is_weight"], np.arange(c.B))


def one_update(c, with_q):
    """Behavior Q over the stacked rows (before the update), then one update; everything copied to the host."""
    tr = make_trainer(c)
    out = {}
    if with_q:
        xs = ref.stack_agents(torch.tensor(c.batch["obs"]))
        out["q"] = tr.get_q_values(xs.cuda())[0].cpu()
    info, prio, _ = tr.train_policy_on_batch(sample(c))
    torch.cuda.synchronize()
    out.update({k: float(v) for k, v in info.items()})
    out["prio"] = None if prio is None else prio.cpu().clone()
    out["grad"], out["P"] = tr.grad.cpu().clone(), tr.P.cpu().clone()     # flat, pads included
    for name in ("grad", "P"):
        out[name + "_of"] = {(kind, k): (tr.agent_view if kind == "agent" else tr.mixer_view)(k, out[name]).numpy()
                             for kind, k in grad_keys(c)}
    return out


@functools.lru_cache(maxsize=None)
def run_case(cid):
    return one_update(build_case(cid), True)


@pytest.mark.parametrize("cid", list(CASES))
def test_offq_case_preconditions(cid):
    c = build_case(cid)
    if c.huber:
        f = huber_fraction_above(c)
        assert 0.25 <= f <= 0.75, f
    gn = c.info64["grad_norm"]
    if cid == "odd_d94":
        assert gn < 0.5 * c.max_norm            # clip inactive
    if cid == "loss_1025":
        assert gn > 2 * c.max_norm              # clip active
        # the one entry of the loss loops' second pass is unmasked and its error is not small
        e = c.info64["err"].reshape(-1)[1024:]
        assert e.numel() == 1 and float(c.info64["mask"].reshape(-1)[1024]) == 1.0 and abs(float(e)) > 0.1
    if c.T == 1:
        assert not bool(c.info64["raw_grads"]["Whh"].any())


@pytest.mark.parametrize("cid", list(CASES))
def test_offq_case_q_loss_priorities(cid):
    c, o = build_case(cid), run_case(cid)
    q64 = c.q64.numpy()
    assert np.array_equal(o["q"].numpy().argmax(-1), q64.argmax(-1))
    np.testing.assert_allclose(o["q"].numpy(), q64, rtol=1e-4, atol=1e-5)
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
def test_offq_case_gradients(cid):
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


@pytest.mark.parametrize("cid", list(CASES))
def test_offq_case_updated_parameters(cid):
    c, o = build_case(cid), run_case(cid)
    for kind, k in grad_keys(c):
        new64 = (c.P64 if kind == "agent" else c.M64)[k].numpy()
        np.testing.assert_allclose(o["P_of"][kind, k], new64, rtol=1e-5, atol=2e-6, err_msg=k)


@pytest.mark.parametrize("cid", list(CASES))
def test_offq_case_deterministic(cid):
    """A second trainer on the same inputs: split-K and the row-block partials sum in a fixed order."""
    c, o = build_case(cid), run_case(cid)
    o2 = one_update(c, False)
    assert torch.equal(o["grad"], o2["grad"]) and torch.equal(o["P"], o2["P"])
    assert (o["prio"] is None and o2["prio"] is None) or torch.equal(o["prio"], o2["prio"])


def test_offq_mixer_hidden_above_64_rejected_before_allocation():
    from minimarl.offq import OffQMix
    before = torch.cuda.memory_allocated()
    for K in (65, 128):
        with pytest.raises(ValueError, match="64"):
            OffQMix(2, 47, A, 4, 4, mixer="qmix", mixer_hidden=K)
    assert torch.cuda.memory_allocated() == before


@pytest.mark.parametrize("L,R,D,target", [(1, 1, 47, False), (7, 300, 94, False), (3, 5500, 47, False),
                                          (2, 70, 94, True)])
def test_offq_q_values_vs_fp64(L, R, D, target):
    """get_q_values on its own, non-zero h0; 3 x 5500 rows are past the one-net cap of 256 blocks of 64 rows."""
    from minimarl.offq import OffQMix
    from minimarl.synth import gen_obs
    P, PT = random_agent(201, D), random_agent(202, D)
    tr = OffQMix(2, D, A, 2, 2, mixer="vdn")
    tr.load_reference_state(agent_sd(P), None, agent_sd(PT), None)
    rng = np.random.default_rng(203)
    x = torch.tensor(gen_obs(rng, (L, R, D)))
    h0 = torch.tensor(rng.standard_normal((R, H)).astype(np.float32) * 0.3)
    with torch.no_grad():
        q64, h64 = ref.agent_q_seq(PT if target else P, x, h0, dtype=torch.float64)
    q, h = tr.get_q_values(x.cuda(), h0.cuda(), target=target)
    assert q.shape == (L, R, A) and h.shape == (R, H)
    np.testing.assert_allclose(q.cpu().numpy(), q64.numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(h.cpu().numpy(), h64.numpy(), rtol=1e-4, atol=1e-5)
