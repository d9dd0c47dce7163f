"""GPU: one MOffQMix.train_policy_on_batch (csrc/moffq.hip) per case of tests/moffq_ref.py against its float64
restatement: one row, the 16-transition tile's edge, three blocks of partials, D = 94 and 3, N = 8 with K = 33 and
S = 376, VDN / no PER / Huber / max-Q target, QMIX / PER / MSE / double Q, an active and an inactive clip; batches past
one grid's worth of tiles (a block walks a second and a third tile, full then ragged), the mixer at K = 64, Hh = 100 and
128, N K = 4096 and a state of its own width; the reference's own recorded update (tests/golden/moffq_*.npz); three
updates of one trainer; input edges.

Gradient bound: relative L2 against float64 <= max(8 x e32, 2e-6), e32 = the float32 restatement's relative L2 for
the same tensor and case (the kernels differ from it in summation order only)."""
import functools

import numpy as np
import pytest
import torch

from moffq_ref import (A, AGENT_KEYS, CASES, GRID, HYPER, SEQ, TB, UNFILTERED, agent_q, build_case, build_sequence,
                       fixture_case)
from offq_cases import MIN_KINK_MARGIN, random_agent, rel_l2

pytestmark = pytest.mark.gpu
FLOOR, RATIO = 2e-6, 8.0
PID = "policy_0"


def make_trainer(c, S=None, **kw):
    from minimarl.moffq import AGENT_REF, MOffQMix
    args = dict(mixer=c.mixer, mixer_hidden=max(c.K, 1), hyper_hidden=max(c.Hh, 1), state_dim=S, gamma=HYPER["gamma"],
                lr=HYPER["lr"], opti_eps=HYPER["eps"], max_grad_norm=c.max_norm, use_double_q=c.double_q,
                use_per=c.use_per, use_huber_loss=c.huber, huber_delta=c.huber_delta, per_eps=HYPER["per_eps"])
    tr = MOffQMix(c.N, c.D, A, **{**args, **kw})
    sd = lambda P: {AGENT_REF[k]: P[k].numpy() for k in AGENT_KEYS}
    tr.load_reference_state(sd(c.P), {k: v.numpy() for k, v in c.M.items()}, sd(c.PT),
                            {k: v.numpy() for k, v in c.MT.items()})
    return tr


def sample_tuple(c, weights=True):
    b = c.batch
    return ({PID: b["obs"]}, {PID: b["cent_obs"]}, {PID: b["acts"]}, {PID: b["rewards"]}, {PID: b["nobs"]},
            {PID: b["cent_nobs"]}, {PID: None}, {PID: b["dones_env"]}, {PID: None}, {PID: None}, {PID: None},
            b["is_weight"] if (c.use_per and weights) else None, np.arange(c.B))


def one_update(c, tr=None, weights=True):
    tr = tr or make_trainer(c, None if c.same_share else c.S)
    out = {"q": tr.get_q_values(c.batch["obs"].reshape(c.N * c.B, c.D)).cpu()}
    info, prio, _ = tr.train_policy_on_batch(sample_tuple(c, weights), use_same_share_obs=c.same_share)
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


def check_kinks_and_scalars(c):
    assert c.r64["min_pre"] >= MIN_KINK_MARGIN                   # no ReLU input at the kink
    assert c.r64["gap"] >= 1e-3                                  # no argmax on a near tie
    if c.huber:
        assert 0.25 <= float((c.r64["err"].abs() > c.huber_delta).double().mean()) <= 0.75
    # no checked scalar is a cancelling sum: the float32 restatement itself stays within a quarter of the rtol 2e-5 bar.
    # Past one grid (B > 4096) some |err| is about 1e-3 and its float32 value 5e-4 off: there the priorities are
    # checked against the float32 restatement's own worst error instead (check_q_loss_priorities)
    for k in ("loss", "q_tot", "grad_norm") + (("prio",) if c.use_per and c.B <= GRID else ()):
        np.testing.assert_allclose(np.asarray(c.r32[k]), np.asarray(c.r64[k]), rtol=5e-6, err_msg=k)


@pytest.mark.parametrize("cid", list(CASES))
def test_moffq_case_preconditions(cid):
    c = build_case(cid)
    check_kinks_and_scalars(c)
    if c.B > 1:
        assert set(np.unique(c.batch["dones_env"])) == {0.0, 1.0}
    if cid == "tile_p1":
        assert c.r64["grad_norm"] > 2 * c.max_norm
    if cid == "blocks3":
        assert c.r64["grad_norm"] < 0.5 * c.max_norm
    if cid not in UNFILTERED:
        print(f"{cid}: dropped {c.dropped:.4f} of the candidates, min |pre| {c.r64['min_pre']:.3g}, gap {c.r64['gap']:.3g}")
    if cid == "own_state":
        s = c.batch["cent_obs"]
        assert s.shape == (c.N, c.B, 29) and c.S != c.N * c.D and not np.array_equal(s[0], s[1])


def check_q_loss_priorities(c, o, strict_prio):
    q64 = c.r64["q"].numpy()
    assert np.array_equal(o["q"].numpy().argmax(-1), q64.argmax(-1))
    np.testing.assert_allclose(o["q"].numpy(), q64, rtol=1e-4, atol=1e-5)
    for k, k64 in (("loss", "loss"), ("Q_tot", "q_tot"), ("grad_norm", "grad_norm")):
        print(f"{c.id} {k}: hip {o[k]:.9g} fp64 {c.r64[k64]:.9g}")
        np.testing.assert_allclose(o[k], c.r64[k64], rtol=2e-5)
    if not c.use_per:
        assert o["prio"] is None
    elif strict_prio:
        np.testing.assert_allclose(o["prio"].numpy(), c.r64["prio"].numpy(), rtol=2e-5)
    else:
        # an element passes at rtol 2e-5, or within 8 x the float32 restatement's own worst absolute error
        p64, p = c.r64["prio"].numpy(), o["prio"].numpy().astype(np.float64)
        e32 = float(np.abs(c.r32["prio"].numpy().astype(np.float64) - p64).max())
        d = np.abs(p - p64)
        fail = (d > 2e-5 * p64) & (d > RATIO * e32)
        print(f"{c.id}: worst priority |hip - p64| / max_b |p32 - p64| = {d.max() / e32:.2f} (max_b |p32 - p64| = "
              f"{e32:.3g}); worst relative {float((d / p64).max()):.3g}")
        assert not fail.any(), (int(fail.sum()), float(d[fail].max()), e32)


def check_gradients(c, o):
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
    print(f"{c.id}: worst err_hip / e32 = {worst[0]:.2f} ({worst[1]}, err {worst[2]:.3g})")
    assert not bad, "\n".join(bad)
    assert all(not bool(g.any()) for g in o["rec_grads"])         # the unread recurrent tensors: exactly zero


def check_updated_parameters(c, o):
    for k, new64 in c.r64["new"].items():
        np.testing.assert_allclose(o["P_of"][k], new64.numpy(), rtol=1e-5, atol=2e-6, err_msg=k)


@pytest.mark.parametrize("cid", list(CASES))
def test_moffq_case_q_loss_priorities(cid):
    check_q_loss_priorities(build_case(cid), run_case(cid), strict_prio=cid in UNFILTERED)


@pytest.mark.parametrize("cid", list(CASES))
def test_moffq_case_gradients(cid):
    check_gradients(build_case(cid), run_case(cid))


@pytest.mark.parametrize("cid", list(CASES))
def test_moffq_case_updated_parameters(cid):
    check_updated_parameters(build_case(cid), run_case(cid))


@pytest.mark.parametrize("cid", list(CASES))
def test_moffq_case_deterministic(cid):
    c, o = build_case(cid), run_case(cid)
    o2 = one_update(c)
    assert torch.equal(o["grad"], o2["grad"]) and torch.equal(o["P"], o2["P"])
    assert (o["prio"] is None and o2["prio"] is None) or torch.equal(o["prio"], o2["prio"])


@pytest.mark.parametrize("name", ["qmix", "vdn"])
def test_moffq_reference_fixture(name):
    """One update from the reference's state dicts against the arrays the reference itself recorded (float32; its
    gradients are those after clip_grad_norm_, the kernels' are unclipped and get the recorded norm's factor)."""
    c, rec = fixture_case(name)
    o = one_update(c)
    for k, kr in (("loss", "loss"), ("Q_tot", "q_tot"), ("grad_norm", "grad_norm")):
        print(f"{c.id} {k}: hip {o[k]:.9g} reference {rec[kr]:.9g}")
        np.testing.assert_allclose(o[k], rec[kr], rtol=2e-5)
    if c.use_per:
        np.testing.assert_allclose(o["prio"].numpy(), rec["prio"], rtol=2e-5)
    else:
        assert o["prio"] is None
    coef = min(1.0, c.max_norm / (rec["grad_norm"] + 1e-6))
    bad = []
    for k, g in rec["grads"].items():
        e32 = rel_l2(c.r32["clipped"][k].numpy(), c.r64["clipped"][k].numpy())
        e = rel_l2(o["grad_of"][k].astype(np.float64) * coef, g)
        if not e <= max(RATIO * e32, FLOOR):
            bad.append(f"{k}: rel L2 {e:.3g} > max({RATIO:g} x {e32:.3g}, {FLOOR:g})")
    assert not bad, "\n".join(bad)
    for k, new in rec["new"].items():
        np.testing.assert_allclose(o["P_of"][k], new, rtol=1e-5, atol=2e-6, err_msg=k)


def test_moffq_three_updates_of_one_trainer():
    """B = 17, 4101, 17 through one trainer: the workspace cached per B, Adam's moments and step carried, a grid of 2
    blocks after one of 256, the target nets after a soft and a hard update."""
    base, steps = build_sequence()
    tr = make_trainer(base, tau=SEQ["tau"])
    view = lambda k, t: (tr.agent_view if k in AGENT_KEYS else tr.mixer_view)(k, t).cpu().numpy()
    assert [c.B for c, _ in steps] == [17, GRID + 5, 17]
    for i, (c, ans) in enumerate(steps):
        assert ans["min_pre"] >= MIN_KINK_MARGIN and ans["gap"] >= 1e-3
        info, prio, _ = tr.train_policy_on_batch(sample_tuple(c))
        (tr.soft_target_updates, tr.hard_target_updates, lambda: None)[i]()
        torch.cuda.synchronize()
        assert prio.shape == (c.B,)
        for k, k64 in (("loss", "loss"), ("grad_norm", "grad_norm"), ("Q_tot", "q_tot")):
            print(f"step {i} {k}: hip {float(info[k]):.9g} fp64 {ans[k64]:.9g}")
            np.testing.assert_allclose(float(info[k]), ans[k64], rtol=2e-5, err_msg=f"step {i} {k}")
        for k, new64 in ans["new"].items():
            np.testing.assert_allclose(view(k, tr.P), new64.numpy(), rtol=1e-5, atol=2e-6, err_msg=f"step {i} {k}")
            np.testing.assert_allclose(view(k, tr.PT), ans["target"][k].numpy(), rtol=1e-5, atol=2e-6,
                                       err_msg=f"step {i} target {k}")
    assert float(tr.step[0]) == 3.0 and sorted(tr._ws) == [17, GRID + 5]


def check_edge(cid, o=None):
    c = build_case(cid)
    o = o or one_update(c)
    check_kinks_and_scalars(c)
    check_q_loss_priorities(c, o, strict_prio=True)
    check_gradients(c, o)
    check_updated_parameters(c, o)
    return c, o


def test_moffq_action_rows_that_are_not_one_hot():
    """The action index is the first maximum of the row (torch.max): 0 for an all-zero or all-equal row."""
    c = build_case("acts_edge")
    a = c.batch["acts"]
    assert not a[0, 0].any() and a[1, 1].argmax() == 1 and a[1, 1, 3] == a[1, 1, 1] and len(set(a[1, 17])) == 1
    assert ((a > 0) & (a < 1)).sum(-1).max() == A
    q = c.r64["q"].view(c.N, c.B, A)
    assert abs(float(q[1, 1, 1] - q[1, 1, 3])) > 1e-2 and abs(float(q[0, 0, 0] - q[0, 0].max())) > 1e-2
    check_edge("acts_edge")


def test_moffq_tile_of_finished_episodes():
    """dones_env = 1 over a whole tile: the target is the reward alone."""
    c = build_case("all_done")
    dn = c.batch["dones_env"][:, 0]
    assert dn[:TB].all() and set(dn[TB:]) == {0.0, 1.0} and c.B > TB
    assert torch.equal(c.r64["target"][:TB], torch.tensor(c.batch["rewards"][0, :TB, 0]).double())
    assert not torch.equal(c.r64["target"][TB:], torch.tensor(c.batch["rewards"][0, TB:, 0]).double())
    check_edge("all_done")


def test_moffq_per_without_importance_weights():
    """use_per with importance_weights=None: the unweighted loss, no priorities, the bits of the use_per=False run."""
    c = build_case("no_weights")
    assert not c.use_per
    plain = one_update(c)
    per = one_update(c, make_trainer(c, use_per=True), weights=False)
    assert per["prio"] is None and plain["prio"] is None
    assert torch.equal(per["grad"], plain["grad"]) and torch.equal(per["P"], plain["P"])
    assert all(per[k] == plain[k] for k in ("loss", "grad_norm", "Q_tot"))
    check_edge("no_weights", per)


@pytest.mark.parametrize("R", [1, 33])
def test_moffq_get_actions_vs_fp64(R):
    from minimarl.synth import gen_obs
    c = build_case("tile")
    x = torch.tensor(gen_obs(np.random.default_rng(400 + R), (R, c.D)))
    with torch.no_grad():
        q64 = agent_q({k: v.double() for k, v in c.P.items()}, x.double())
    top = q64.topk(2, -1)[0]
    assert float((top[:, 0] - top[:, 1]).min() / q64.abs().max()) >= 1e-3
    onehot, gq = make_trainer(c).get_actions(x.numpy())
    assert onehot.shape == (R, A) and gq.shape == (R, 1) and onehot.dtype == torch.float32
    assert np.array_equal(onehot.cpu().numpy(), np.eye(A, dtype=np.float32)[q64.argmax(-1).numpy()])
    np.testing.assert_allclose(gq.cpu().numpy()[:, 0], q64.max(-1)[0].numpy(), rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("R,D,target,gather", [(1, 47, False, False), (1, 3, True, True), (4133, 94, False, True),
                                               (4133, 47, True, False)])
def test_moffq_q_values_vs_fp64(R, D, target, gather):
    """get_q_values on its own; 4133 rows are past one grid's worth (256 blocks of 16 rows) and end in a ragged tile."""
    from minimarl.moffq import AGENT_REF, MOffQMix
    from minimarl.synth import gen_obs
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
