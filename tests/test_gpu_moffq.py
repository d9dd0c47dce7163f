"""GPU: one MOffQMix.train_policy_on_batch (csrc/moffq.hip) per case of tests/moffq_ref.py against its float64
restatement: one row, the 16-transition tile's edge, three blocks of partials, D = 94 and 3, N = 8 with K = 33 and
S = 376, VDN / no PER / Huber / max-Q target, QMIX / PER / MSE / double Q, an active and an inactive clip.

Gradient bound: relative L2 against float64 <= max(8 x e32, 2e-6), e32 = the float32 restatement's relative L2 for
the same tensor and case (the kernels differ from it in summation order only)."""
import functools

import numpy as np
import pytest
import torch

from moffq_ref import A, AGENT_KEYS, CASES, HYPER, build_case
from offq_cases import MIN_KINK_MARGIN, random_agent, rel_l2

pytestmark = pytest.mark.gpu
FLOOR, RATIO = 2e-6, 8.0


def make_trainer(c):
    from minimarl.moffq import AGENT_REF, MOffQMix
    tr = MOffQMix(c.N, c.D, A, mixer=c.mixer, mixer_hidden=max(c.K, 1), hyper_hidden=max(c.Hh, 1), gamma=HYPER["gamma"],
                  lr=HYPER["lr"], opti_eps=HYPER["eps"], max_grad_norm=c.max_norm, use_double_q=c.double_q,
                  use_per=c.use_per, use_huber_loss=c.huber, huber_delta=c.huber_delta, per_eps=HYPER["per_eps"])
    sd = lambda P: {AGENT_REF[k]: P[k].numpy() for k in AGENT_KEYS}
    tr.load_reference_state(sd(c.P), {k: v.numpy() for k, v in c.M.items()}, sd(c.PT),
                            {k: v.numpy() for k, v in c.MT.items()})
    return tr


def one_update(c):
    tr, b, pid = make_trainer(c), c.batch, "policy_0"
    out = {"q": tr.get_q_values(b["obs"].reshape(c.N * c.B, c.D)).cpu()}
    info, prio, _ = tr.train_policy_on_batch((
        {pid: b["obs"]}, {pid: b["cent_obs"]}, {pid: b["acts"]}, {pid: b["rewards"]}, {pid: b["nobs"]},
        {pid: b["cent_nobs"]}, {pid: None}, {pid: b["dones_env"]}, {pid: None}, {pid: None}, {pid: None},
        b["is_weight"] if c.use_per else None, np.arange(c.B)))
    torch.cuda.synchronize()
    out.update({k: float(v) for k, v in info.items()})
    out["prio"] = None if prio is None else prio.cpu().clone()
    out["grad"], out["P"] = tr.grad.cpu().clone(), tr.P.cpu().clone()
    view = lambda k, t: (tr.agent_view if k in AGENT_KEYS else tr.mixer_view)(k, t).numpy()
    out["grad_of"] = {k: view(k, out["grad"]) for k in c.r64["grads"]}
    out["P_of"] = {k: view(k, out["P"]) for k in c.r64["grads"]}
    out["rec_grads"] = [tr.agent_view(k, out["grad"]) for k in ("Wih", "Whh", "bih", "bhh", "lnr_w", "lnr_b")]
    return out


@functools.lru_cache(maxsize=None)
def run_case(cid):
    return one_update(build_case(cid))


@pytest.mark.parametrize("cid", list(CASES))
def test_moffq_case_preconditions(cid):
    c = build_case(cid)
    assert c.r64["min_pre"] >= MIN_KINK_MARGIN                   # no ReLU input at the kink
    assert c.r64["gap"] >= 1e-3                                  # no argmax on a near tie
    if c.B > 1:
        assert set(np.unique(c.batch["dones_env"])) == {0.0, 1.0}
    if c.huber:
        assert 0.25 <= float((c.r64["err"].abs() > c.huber_delta).double().mean()) <= 0.75
    # no checked scalar is a cancelling sum: the float32 restatement itself stays within a quarter of the rtol 2e-5 bar
    for k in ("loss", "q_tot", "grad_norm") + (("prio",) if c.use_per else ()):
        np.testing.assert_allclose(np.asarray(c.r32[k]), np.asarray(c.r64[k]), rtol=5e-6, err_msg=k)
    if cid == "tile_p1":
        assert c.r64["grad_norm"] > 2 * c.max_norm
    if cid == "blocks3":
        assert c.r64["grad_norm"] < 0.5 * c.max_norm


@pytest.mark.parametrize("cid", list(CASES))
def test_moffq_case_q_loss_priorities(cid):
    c, o = build_case(cid), run_case(cid)
    q64 = c.r64["q"].numpy()
    assert np.array_equal(o["q"].numpy().argmax(-1), q64.argmax(-1))
    np.testing.assert_allclose(o["q"].numpy(), q64, rtol=1e-4, atol=1e-5)
    for k, k64 in (("loss", "loss"), ("Q_tot", "q_tot"), ("grad_norm", "grad_norm")):
        print(f"{cid} {k}: hip {o[k]:.9g} fp64 {c.r64[k64]:.9g}")
        np.testing.assert_allclose(o[k], c.r64[k64], rtol=2e-5)
    if c.use_per:
        np.testing.assert_allclose(o["prio"].numpy(), c.r64["prio"].numpy(), rtol=2e-5)
    else:
        assert o["prio"] is None


@pytest.mark.parametrize("cid", list(CASES))
def test_moffq_case_gradients(cid):
    c, o = build_case(cid), run_case(cid)
    g64, g32 = c.r64["grads"], c.r32["grads"]
    gmax = max(float(g.abs().max()) for g in g64.values())
    bad, worst = [], (0.0, None, 0.0)
    for k in g64:
        g = o["grad_of"][k]
        assert g.shape == tuple(g64[k].shape)
        if not bool(g64[k].any()):
            if not np.abs(g).max() <= FLOOR * gmax:
                bad.append(f"{k}: fp64 gradient is 0, hip max |g| {np.abs(g).max():.3g}")
            continue
        e32, e = rel_l2(g32[k].numpy(), g64[k].numpy()), rel_l2(g, g64[k].numpy())
        if e32 > 0 and e / e32 > worst[0]:
            worst = (e / e32, k, e)
        if not e <= max(RATIO * e32, FLOOR):
            bad.append(f"{k}: rel L2 {e:.3g} > max({RATIO:g} x {e32:.3g}, {FLOOR:g})")
    print(f"{cid}: worst err_hip / e32 = {worst[0]:.2f} ({worst[1]}, err {worst[2]:.3g})")
    assert not bad, "\n".join(bad)
    assert all(not bool(g.any()) for g in o["rec_grads"])         # the unread recurrent tensors: exactly zero


@pytest.mark.parametrize("cid", list(CASES))
def test_moffq_case_updated_parameters(cid):
    c, o = build_case(cid), run_case(cid)
    for k, new64 in c.r64["new"].items():
        np.testing.assert_allclose(o["P_of"][k], new64.numpy(), rtol=1e-5, atol=2e-6, err_msg=k)


@pytest.mark.parametrize("cid", list(CASES))
def test_moffq_case_deterministic(cid):
    c, o = build_case(cid), run_case(cid)
    o2 = one_update(c)
    assert torch.equal(o["grad"], o2["grad"]) and torch.equal(o["P"], o2["P"])
    assert (o["prio"] is None and o2["prio"] is None) or torch.equal(o["prio"], o2["prio"])


@pytest.mark.parametrize("R,D,target,gather", [(1, 47, False, False), (1, 3, True, True), (4133, 94, False, True),
                                               (4133, 47, True, False)])
def test_moffq_q_values_vs_fp64(R, D, target, gather):
    """get_q_values on its own; 4133 rows are past one grid's worth (256 blocks of 16 rows) and end in a ragged tile."""
    from minimarl.moffq import AGENT_REF, MOffQMix
    from minimarl.synth import gen_obs
    from moffq_ref import agent_q
    P, PT = random_agent(301, D), random_agent(302, D)
    tr = MOffQMix(2, D, A, mixer="vdn")
    tr.load_reference_state({AGENT_REF[k]: P[k].numpy() for k in AGENT_KEYS}, None,
                            {AGENT_REF[k]: PT[k].numpy() for k in AGENT_KEYS}, None)
    rng = np.random.default_rng(303)
    x, act = torch.tensor(gen_obs(rng, (R, D))), torch.tensor(rng.integers(0, A, R))
    with torch.no_grad():
        q64 = agent_q({k: v.double() for k, v in (PT if target else P).items()}, x.double())
    if gather:
        q64 = q64.gather(1, act.unsqueeze(-1))
    q = tr.get_q_values(x.numpy(), act.numpy() if gather else None, target=target)
    assert q.shape == q64.shape
    np.testing.assert_allclose(q.cpu().numpy(), q64.numpy(), rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("kw", [dict(mixer_hidden=65), dict(obs_dim=48)])
def test_moffq_unsupported_rejected_before_allocation(kw):
    from minimarl.moffq import MOffQMix
    before = torch.cuda.memory_allocated()
    args = dict(n_agents=2, obs_dim=47, n_actions=A, mixer="qmix")
    with pytest.raises(ValueError):
        MOffQMix(**{**args, **kw})
    assert torch.cuda.memory_allocated() == before
