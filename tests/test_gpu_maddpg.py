"""MADDPG / MATD3 trainer (minimarl.maddpg.MADDPG over csrc/maddpg.hip) against the float64 restatement of
tests/maddpg_ref.py, with the float32 restatement as the summation-noise yardstick. Bars as in test_gpu_moffq.py."""
import functools
import os

import numpy as np
import pytest
import torch

import maddpg_ref as R
from conftest import GOLDEN
from offq_cases import MIN_KINK_MARGIN

IDS = [c.id for c in R.CASES]
RECURRENT = ("Wih", "Whh", "bih", "bhh", "lnr_w", "lnr_b")


def grad_bar(e32):
    return max(8 * e32, 2e-6)


def make_trainer(cid, huber_delta=R.DELTA, **kw):
    from minimarl.maddpg import MADDPG
    c, nets, batch, g, tg = R.make_case(cid) if isinstance(cid, str) else cid
    tr = MADDPG(c.N, c.D, R.A, td3=c.td3, gamma=R.GAMMA, lr=R.LR, opti_eps=R.OPTI_EPS, max_grad_norm=c.max_norm,
                use_per=c.per, use_huber_loss=c.huber, huber_delta=huber_delta, per_eps=R.PER_EPS, **kw)
    for name, target in (("", False), ("target_", True)):
        for k, v in nets[name + "actor"].items():
            tr.actor_view(k, target).copy_(torch.as_tensor(v))
        for k, v in nets[name + "critic"].items():
            tr.critic_view(k, target).copy_(torch.as_tensor(v))
    b = batch
    tup = (b["obs"], b["cent_obs"], b["acts"], b["rewards"], b["nobs"], b["cent_nobs"], None, b["dones_env"],
           b["valid"], None, None, b["isw"], None)
    return tr, tup, g, tg


@pytest.mark.parametrize("cid", IDS)
def test_preconditions(cid):
    c = R.make_case(cid)[0]
    o = R.reference(cid)[0]
    assert o["top2_gap"] >= 1e-3 and o["kink_margin"] >= MIN_KINK_MARGIN
    if c.huber:
        assert 0.25 <= o["huber_share"] <= 0.75
    b = R.make_case(cid)[2]
    assert b["valid"].min() == 0 or c.B == 1
    assert (b["valid"].sum((1, 2)) > 0).all() and (c.B == 1 or set(np.unique(b["dones_env"])) == {0.0, 1.0})


def test_actor_pass_needs_the_updated_critic():
    """The float64 actor gradient taken through the critic from before its Adam step misses the bar somewhere."""
    miss = False
    for cid in IDS[1:4]:
        o64, o32 = R.reference(cid)
        stale = R.update(cid, stale_critic=True)
        for k, ref in o64["actor_grad"].items():
            miss |= R.rel_l2(stale["actor_grad"][k], ref) > grad_bar(R.rel_l2(o32["actor_grad"][k], ref))
    assert miss


@pytest.mark.gpu
@pytest.mark.parametrize("cid", IDS)
def test_update_matches_float64(cid):
    c = R.make_case(cid)[0]
    o64, o32 = R.reference(cid)
    tr, tup, g, tg = make_trainer(cid)
    heads = [tr.critic_view(k, t).clone() for k in ("Wo", "bo") for t in (False, True)]
    info, prio, _ = tr.train_policy_on_batch(tup, gumbel=g, target_gumbel=tg)
    first = [t.clone() for t in (tr.Pa, tr.Pc, tr.grada, tr.gradc, tr.statsa, tr.statsc)]
    for k in ("critic_loss", "critic_grad_norm", "actor_loss", "actor_grad_norm"):
        np.testing.assert_allclose(float(info[k]), o64[k], rtol=2e-5, err_msg=k)
    assert info["update_actor"] is True
    if c.per:
        np.testing.assert_allclose(prio.cpu().numpy(), o64["prio"], rtol=2e-5)
    else:
        assert prio is None
    for net, view, grad in (("actor", tr.actor, tr.grada), ("critic", tr.critic, tr.gradc)):
        for k, ref in o64[net + "_grad"].items():
            e32 = R.rel_l2(o32[net + "_grad"][k], ref)
            e = R.rel_l2(view.view(grad, k).cpu().numpy(), ref.numpy())
            assert e <= grad_bar(e32), (net, k, e, e32)
        for k in RECURRENT:
            assert not view.view(grad, k).any()
        P = tr.Pa if net == "actor" else tr.Pc
        for k, ref in o64[net + "_new"].items():
            np.testing.assert_allclose(view.view(P, k).cpu().numpy(), ref.numpy(), rtol=1e-5, atol=2e-6)
    assert not tr.critic.view(tr.gradc, "Wo").any() and not tr.critic.view(tr.gradc, "bo").any()
    for h, (k, t) in zip(heads, [(k, t) for k in ("Wo", "bo") for t in (False, True)]):
        assert torch.equal(h, tr.critic_view(k, t))
    tr2, tup2, _, _ = make_trainer(cid)                      # a second run: the same bits
    tr2.train_policy_on_batch(tup2, gumbel=g, target_gumbel=tg)
    for x, y in zip(first, (tr2.Pa, tr2.Pc, tr2.grada, tr2.gradc, tr2.statsa, tr2.statsc)):
        assert torch.equal(x, y)


@pytest.mark.gpu
def test_target_updates_skip_the_heads():
    cid = "switch_td3_huber"
    tr, tup, g, tg = make_trainer(cid, tau=0.25)
    ta0, tc0 = tr.PTa.double().clone(), tr.PTc.double().clone()
    hl, ht = tr.critic_view("Wo").clone(), tr.critic_view("Wo", True).clone()
    for _ in range(2):
        tr.train_policy_on_batch(tup, gumbel=g, target_gumbel=tg)
    tr.soft_target_updates()
    n = tr.critic.heads
    np.testing.assert_allclose(tr.PTa.cpu().numpy(), (0.75 * ta0 + 0.25 * tr.Pa.double()).cpu().numpy(), rtol=1e-6,
                               atol=1e-7)
    np.testing.assert_allclose(tr.PTc[:n].cpu().numpy(), (0.75 * tc0 + 0.25 * tr.Pc.double())[:n].cpu().numpy(),
                               rtol=1e-6, atol=1e-7)
    tr.hard_target_updates()
    assert torch.equal(tr.PTa, tr.Pa) and torch.equal(tr.PTc[:n], tr.Pc[:n])
    assert torch.equal(hl, tr.critic_view("Wo")) and torch.equal(ht, tr.critic_view("Wo", True))
    assert not torch.equal(tr.critic_view("Wo"), tr.critic_view("Wo", True))


@pytest.mark.gpu
def test_device_noise_is_the_host_rng():
    """No injection == injection of g computed on the host from oracle.rng for the same seed and counter."""
    from minimarl.maddpg import GUMBEL_SALT, TARGET_GUMBEL_SALT
    from oracle import rng
    cid = "switch_td3_huber"
    c = R.make_case(cid)[0]
    b, n, a = np.meshgrid(np.arange(c.B), np.arange(c.N), np.arange(R.A), indexing="ij")

    def host(salt, counter):
        u = rng.rng_uniform(rng.rng_draw(np.uint64(11 ^ salt), counter, b, n * R.A + a)) + np.float32(1e-20)
        t = (-np.log(u.astype(np.float64)).astype(np.float32) + np.float32(1e-20)).astype(np.float32)
        return (-np.log(t.astype(np.float64)).astype(np.float32)).transpose(1, 0, 2).copy()

    tr, tup, _, _ = make_trainer(cid, noise_seed=11)
    tr2, tup2, _, _ = make_trainer(cid, noise_seed=11)
    for counter in range(2):
        tr.train_policy_on_batch(tup)
        tr2.train_policy_on_batch(tup2, gumbel=host(GUMBEL_SALT, counter), target_gumbel=host(TARGET_GUMBEL_SALT, counter))
        assert torch.equal(tr.Pa, tr2.Pa) and torch.equal(tr.Pc, tr2.Pc)


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [1, 33])
def test_get_actions(rows):
    cid = "b17_clip"
    tr, _, _, _ = make_trainer(cid)
    nets = R.make_case(cid)[1]
    rng = np.random.default_rng(rows)
    obs = rng.standard_normal((rows, 47)).astype(np.float32)
    g = rng.gumbel(size=(rows, R.A)).astype(np.float32)
    p = {k: torch.tensor(v, dtype=torch.float64) for k, v in nets["actor"].items()}
    z = R.net(p, torch.tensor(obs, dtype=torch.float64))
    assert R.top2_gap(z) >= 1e-3 and R.top2_gap(z + torch.tensor(g)) >= 1e-3
    logits, hot = tr.get_logits(obs)
    np.testing.assert_allclose(logits.cpu().numpy(), z.numpy(), rtol=1e-5, atol=2e-6)
    assert torch.equal(hot.cpu().argmax(-1), z.argmax(-1)) and torch.equal(hot.sum(-1).cpu(), torch.ones(rows))
    hot, _ = tr.get_actions(obs, use_gumbel=True, gumbel=g)
    assert torch.equal(hot.cpu().argmax(-1), (z + torch.tensor(g)).argmax(-1))
    tr2 = make_trainer(cid)[0]                               # acting noise replays from noise_seed and the call count
    tr2.act_calls = tr.act_calls
    for _ in range(2):
        a1, a2 = (t.get_actions(obs, explore=True, eps=0.5)[0] for t in (tr, tr2))
        assert torch.equal(a1, a2) and torch.equal(a1.sum(-1).cpu(), torch.ones(rows))


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(use_popart=True), dict(use_same_share_obs=False), dict(weight_decay=1e-4),
                                dict(layer_N=2), dict(use_value_active_masks=True), dict(multidiscrete=True),
                                dict(continuous=True), dict(n_policies=2), dict(hidden=32), dict(n_actions=4),
                                dict(obs_dim=48), dict(n_agents=9)])
def test_unsupported_settings_are_rejected_before_allocation(kw):
    from minimarl.maddpg import MADDPG
    torch.zeros(1, device="cuda")
    before = torch.cuda.memory_allocated()
    args = dict(n_agents=2, obs_dim=47, n_actions=5)
    args.update(kw)
    with pytest.raises(ValueError):
        MADDPG(**args)
    assert torch.cuda.memory_allocated() == before
    tr, tup, g, tg = make_trainer("b15")
    with pytest.raises(ValueError):
        tr.train_policy_on_batch(tup[:9] + (np.ones((2, 15, 5)), None) + tup[11:], gumbel=g)


@functools.lru_cache(maxsize=None)
def fixture_case(name):
    """A case of maddpg_ref's kind from what the reference's own classes recorded (tests/golden/make_golden_maddpg.py),
    the recording, and its huber_delta."""
    from minimarl.maddpg import ACTOR_REF, TRUNK_REF
    z = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    N, B, D, A, td3, per, huber, _ = (int(x) for x in z["meta"])
    gamma, lr, opti_eps, max_norm, delta, per_eps = (float(x) for x in z["hyper"])
    assert (A, gamma, lr, opti_eps, per_eps) == (R.A, R.GAMMA, R.LR, R.OPTI_EPS, R.PER_EPS)
    nets = {}
    for pre in ("actor", "target_actor", "critic", "target_critic"):
        crit = pre.endswith("critic")
        nets[pre] = {k: z[f"{pre}.{n}"] for k, n in (TRUNK_REF if crit else ACTOR_REF).items()}
        if crit:
            nets[pre]["Wo"] = np.concatenate([z[f"{pre}.q_outs.{h}.weight"] for h in range(1 + td3)])
            nets[pre]["bo"] = np.concatenate([z[f"{pre}.q_outs.{h}.bias"] for h in range(1 + td3)])
    batch = {k: z[k] for k in ("obs", "nobs", "cent_obs", "cent_nobs", "acts", "rewards", "dones_env", "valid")}
    batch["isw"] = z["is_weight"] if per else None
    c = R.Case(name, N, B, D, bool(td3), bool(per), bool(huber), max_norm, 0)
    rec = {"prio": z.get("new_priorities")}
    for net, names in (("actor", ACTOR_REF), ("critic", TRUNK_REF)):
        rec[net + "_grad"] = {k: z[f"grad.{net}.{n}"] for k, n in names.items()}
        rec[net + "_new"] = {k: z[f"post.{net}.{n}"] for k, n in names.items()}
    rec.update({k: float(z[k]) for k in ("critic_loss", "critic_grad_norm", "actor_loss", "actor_grad_norm")})
    case = (c, nets, batch, z["gumbel"], z["target_gumbel"])
    return case, rec, delta, R.update(case, torch.float64, delta=delta), R.update(case, torch.float32, delta=delta)


def check_recording(name, got):
    """got: losses, norms, prio, unclipped gradients and stepped parameters of one update of the fixture's case. The
    recorded gradients are those after clip_grad_norm_: ours get the recorded norm's factor."""
    case, rec, _, o64, o32 = fixture_case(name)
    for k in ("critic_loss", "critic_grad_norm", "actor_loss", "actor_grad_norm"):
        np.testing.assert_allclose(got[k], rec[k], rtol=2e-5, err_msg=k)
    if case[0].per:
        np.testing.assert_allclose(got["prio"], rec["prio"], rtol=2e-5)
    for net in ("actor", "critic"):
        coef = min(1.0, case[0].max_norm / (rec[net + "_grad_norm"] + 1e-6))
        for k, ref in rec[net + "_grad"].items():
            e32 = R.rel_l2(o32[net + "_grad"][k], o64[net + "_grad"][k])
            e = R.rel_l2(np.asarray(got[net + "_grad"][k], np.float64) * coef, ref)
            assert e <= grad_bar(e32), (net, k, e, e32)
        for k, ref in rec[net + "_new"].items():
            np.testing.assert_allclose(np.asarray(got[net + "_new"][k]), ref, rtol=1e-5, atol=2e-6, err_msg=k)


@pytest.mark.parametrize("name", ["maddpg", "matd3"])
def test_restatement_matches_the_reference_recording(name):
    """tests/maddpg_ref.py in float64 against the arrays the reference's own MADDPG / MATD3 classes recorded."""
    check_recording(name, fixture_case(name)[3])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["maddpg", "matd3"])
def test_maddpg_reference_fixture(name):
    """One update from the reference's state dicts and q_outs against what the reference itself recorded."""
    case, rec, delta, _, _ = fixture_case(name)
    tr, tup, g, tg = make_trainer(case, huber_delta=delta)
    info, prio, _ = tr.train_policy_on_batch(tup, gumbel=g, target_gumbel=tg)
    got = {k: float(info[k]) for k in ("critic_loss", "critic_grad_norm", "actor_loss", "actor_grad_norm")}
    got["prio"] = None if prio is None else prio.cpu().numpy()
    for net, view, grad, P in (("actor", tr.actor, tr.grada, tr.Pa), ("critic", tr.critic, tr.gradc, tr.Pc)):
        got[net + "_grad"] = {k: view.view(grad, k).cpu().numpy() for k in rec[net + "_grad"]}
        got[net + "_new"] = {k: view.view(P, k).cpu().numpy() for k in rec[net + "_new"]}
    check_recording(name, got)


@pytest.mark.gpu
def test_checkpoint_round_trip(tmp_path):
    """Save after one update, load into a fresh trainer: the next update gives the same bits, heads and counters too."""
    from minimarl.checkpoint import load_checkpoint, save_checkpoint
    cid = "switch_td3_huber"
    tr, tup, _, _ = make_trainer(cid, noise_seed=3, count_updates=True)
    tr.train_policy_on_batch(tup)
    tr.soft_target_updates()
    save_checkpoint(str(tmp_path / "m.safetensors"), maddpg=tr)
    tr2 = make_trainer("d94_td3_per", noise_seed=3, count_updates=True)[0]
    with pytest.raises(ValueError):
        load_checkpoint(str(tmp_path / "m.safetensors"), maddpg=tr2)          # another critic width
    from minimarl.maddpg import MADDPG
    c = R.make_case(cid)[0]
    tr2 = MADDPG(c.N, c.D, R.A, td3=True, lr=R.LR, opti_eps=R.OPTI_EPS, use_per=c.per, use_huber_loss=True,
                 huber_delta=R.DELTA, noise_seed=3, count_updates=True)
    load_checkpoint(str(tmp_path / "m.safetensors"), maddpg=tr2)
    assert (tr2.num_updates, tr2.calls) == (1, 1) and torch.equal(tr2.critic_view("Wo", True), tr.critic_view("Wo", True))
    infos = [t.train_policy_on_batch(tup)[0] for t in (tr, tr2)]
    assert sorted(infos[0]) == sorted(infos[1]) == ["critic_grad_norm", "critic_loss"]      # update 1 of interval 2
    for k in ("Pa", "Pc", "PTa", "PTc", "ma", "mc", "va", "vc", "stepa", "stepc"):
        assert torch.equal(getattr(tr, k), getattr(tr2, k)), k


@pytest.mark.gpu
def test_counted_updates_skip_the_actor():
    """count_updates=True with matd3's actor_update_interval 2: call 1 updates both, call 2 the critic alone."""
    tr, tup, g, tg = make_trainer("switch_td3_huber", count_updates=True)
    assert tr.actor_update_interval == 2
    info = tr.train_policy_on_batch(tup, gumbel=g, target_gumbel=tg)[0]
    assert info["update_actor"] is True and "actor_loss" in info
    pa, pc = tr.Pa.clone(), tr.Pc.clone()
    info = tr.train_policy_on_batch(tup, target_gumbel=tg)[0]
    assert sorted(info) == ["critic_grad_norm", "critic_loss"]
    assert torch.equal(pa, tr.Pa) and not torch.equal(pc, tr.Pc) and float(tr.stepa[0]) == 1.0
