"""Recurrent MADDPG / MATD3 trainer (minimarl.rmaddpg.RMADDPG over csrc/rmaddpg.hip) against the float64 restatement of
tests/rmaddpg_ref.py, with the float32 restatement as the summation-noise yardstick. Bars as in test_gpu_maddpg.py:
gradients rel-L2 <= max(8 e32, 2e-6), parameters rtol 1e-5 / atol 2e-6, scalars and priorities rtol 2e-5 (the float32
restatement meets 2e-5 in every case of the table, the long one included, so no bar is widened). The two recordings of
the reference's own classes (tests/golden/rmaddpg.npz, rmatd3.npz) are held to the same bars."""
import numpy as np
import pytest
import torch

import rmaddpg_ref as R
from offq_cases import MIN_KINK_MARGIN

IDS = list(R.CASES)


def make_trainer(cid, **kw):
    from minimarl.rmaddpg import RMADDPG
    c = R.ALL[cid]
    P, batch, g, tg = R.make_case(cid)
    tr = RMADDPG(c.N, c.D, R.A, c.T, c.B, td3=c.td3, gamma=R.GAMMA, lr=R.LR, opti_eps=R.OPTI_EPS,
                 max_grad_norm=c.max_norm, use_per=c.per, per_nu=R.NU, use_huber_loss=c.huber, huber_delta=R.DELTA,
                 per_eps=R.PER_EPS, **kw)
    if cid in R.FIXTURES:      # through the reference's state-dict names
        sds, tsd = R.load_fixture(cid)[2:]
        tr.load_reference_state(sds["actor"], sds["critic"], tsd["actor"], tsd["critic"])
        return tr, batch, g, tg
    for name, target in (("", False), ("target_", True)):
        for k, v in P[name + "actor"].items():
            tr.actor_view(k, target).copy_(v)
        for k, v in P[name + "critic"].items():
            tr.critic_view(k, target).copy_(v)
    return tr, batch, g, tg


def scalar_close(got, cid, key):
    np.testing.assert_allclose(np.asarray(got, np.float64), np.asarray(R.update(cid)[key], np.float64), rtol=2e-5,
                               err_msg=key)


def outputs(tr, info, prio):
    got = {k: float(info[k]) for k in ("critic_loss", "critic_grad_norm", "actor_loss", "actor_grad_norm")}
    got["prio"] = None if prio is None else prio.cpu().numpy()
    for net, view, grad, P in (("actor", tr.actor, tr.grada, tr.Pa), ("critic", tr.critic, tr.gradc, tr.Pc)):
        got[net + "_grad"] = {k: view.view(grad, k).cpu().numpy() for k in R.KEYS}
        got[net] = {k: view.view(P, k).cpu().numpy() for k in R.KEYS}
    return got


def check_recording(name, got):
    """got: losses, norms, prio, unclipped gradients and stepped parameters of one update of the fixture's case. The
    recorded gradients are those after clip_grad_norm_: ours get the recorded norm's factor."""
    z, c = R.load_fixture(name)[1], R.ALL[name]
    o64, o32 = R.update(name), R.update(name, torch.float32)
    for k in ("critic_loss", "critic_grad_norm", "actor_loss", "actor_grad_norm"):
        np.testing.assert_allclose(got[k], float(z[k]), rtol=2e-5, err_msg=k)
    if c.per:
        np.testing.assert_allclose(np.asarray(got["prio"], np.float64), z["new_priorities"], rtol=2e-5)
    for net in ("actor", "critic"):
        coef = min(1.0, c.max_norm / (float(z[net + "_grad_norm"]) + 1e-6))
        post = R.from_ref(z, net, f"post.{net}.")
        for k, ref in R.from_ref(z, net, f"grad.{net}.").items():
            e32 = R.rel_l2(o32[net + "_grad"][k], o64[net + "_grad"][k])
            e = R.rel_l2(np.asarray(got[net + "_grad"][k], np.float64) * coef, ref)
            assert e <= max(8 * e32, 2e-6), (net, k, e, e32)
            np.testing.assert_allclose(np.asarray(got[net][k]), post[k].numpy(), rtol=1e-5, atol=2e-6,
                                       err_msg=f"{net}.{k}")


@pytest.mark.parametrize("name", list(R.FIXTURES))
def test_restatement_matches_the_reference_recording(name):
    o = R.update(name)
    check_recording(name, dict(o, actor_grad={k: v.numpy() for k, v in o["actor_grad"].items()},
                               critic_grad={k: v.numpy() for k, v in o["critic_grad"].items()}))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(R.FIXTURES))
def test_rmaddpg_reference_fixture(name):
    tr, batch, g, tg = make_trainer(name)
    info, prio, _ = tr.train_policy_on_batch(batch, gumbel=g, target_gumbel=tg)
    check_recording(name, outputs(tr, info, prio))


@pytest.mark.parametrize("cid", IDS)
def test_preconditions(cid):
    c, o = R.CASES[cid], R.update(cid)
    assert o["gap_actor"] >= 1e-3 and o["gap_target"] >= 1e-3
    if c.huber:
        ae = o["err"].abs()
        assert 0.25 <= float((ae > R.DELTA).double().mean()) <= 0.75
        assert float((ae - R.DELTA).abs().min()) >= MIN_KINK_MARGIN
    if cid == "ck":
        assert min(o["critic_grad_norm"], o["actor_grad_norm"]) > c.max_norm
    dones, de = R.make_case(cid)[1][4:6]
    assert (dones != de).any()
    assert c.B < 3 or (de[0].sum() > 0 and de[-1].sum() < c.B and (c.T == 1 or de[-1].sum() > de[0].sum()))


def compare(tr, info, prio, cid, actor=True):
    o64, o32 = R.update(cid), R.update(cid, torch.float32)
    nets = (("critic", tr.critic, tr.gradc, tr.Pc),) + ((("actor", tr.actor, tr.grada, tr.Pa),) if actor else ())
    for net, view, grad, P in nets:
        scalar_close(float(info[net + "_loss"]), cid, net + "_loss")
        scalar_close(float(info[net + "_grad_norm"]), cid, net + "_grad_norm")
        for k, ref in o64[net + "_grad"].items():
            e32 = R.rel_l2(o32[net + "_grad"][k], ref)
            e = R.rel_l2(view.view(grad, k).cpu().numpy(), ref.numpy())
            assert e <= max(8 * e32, 2e-6), (net, k, e, e32)
            np.testing.assert_allclose(view.view(P, k).cpu().numpy(), o64[net][k].numpy(), rtol=1e-5, atol=2e-6,
                                       err_msg=f"{net}.{k}")
    if R.CASES[cid].per:
        scalar_close(prio.cpu().numpy(), cid, "prio")
    else:
        assert prio is None


@pytest.mark.gpu
@pytest.mark.parametrize("cid", IDS)
def test_update_matches_float64(cid):
    tr, batch, g, tg = make_trainer(cid)
    info, prio, _ = tr.train_policy_on_batch(batch, gumbel=g, target_gumbel=tg)
    assert info["update_actor"] is True
    compare(tr, info, prio, cid)
    first = [t.clone() for t in (tr.Pa, tr.Pc, tr.grada, tr.gradc, tr.statsa, tr.statsc, tr.prio)]
    tr2, batch, g, tg = make_trainer(cid)
    tr2.train_policy_on_batch(batch, gumbel=g, target_gumbel=tg)
    for x, y in zip(first, (tr2.Pa, tr2.Pc, tr2.grada, tr2.gradc, tr2.statsa, tr2.statsc, tr2.prio)):
        assert torch.equal(x, y)


@pytest.mark.gpu
def test_actor_interval():
    tr, batch, g, tg = make_trainer("sw")
    tr.train_policy_on_batch(batch, gumbel=g, target_gumbel=tg)
    Pa, Pc, stepa = tr.Pa.clone(), tr.Pc.clone(), tr.stepa.clone()
    info, _, _ = tr.train_policy_on_batch(batch, gumbel=g, target_gumbel=tg)
    assert sorted(info) == ["critic_grad_norm", "critic_loss", "update_actor"] and info["update_actor"] is False
    assert torch.equal(tr.Pa, Pa) and torch.equal(tr.stepa, stepa) and not torch.equal(tr.Pc, Pc)


@pytest.mark.gpu
def test_target_updates_cover_the_heads():
    tr = make_trainer("sw", tau=0.25)[0]
    old = [t.clone() for t in (tr.PTa, tr.PTc)]
    tr.soft_target_updates()
    for t, o, live in zip((tr.PTa, tr.PTc), old, (tr.Pa, tr.Pc)):
        torch.testing.assert_close(t, 0.75 * o + 0.25 * live, rtol=1e-6, atol=1e-7)
    assert not torch.equal(tr.PTc[tr.critic.heads:], old[1][tr.critic.heads:])
    tr.hard_target_updates()
    assert torch.equal(tr.PTa, tr.Pa) and torch.equal(tr.PTc, tr.Pc)


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [1, 33])
def test_get_actions_steps_the_hidden_state(rows):
    tr = make_trainer("ck")[0]
    obs = torch.randn(2, rows, 47, generator=torch.Generator().manual_seed(rows), dtype=torch.float64)
    ref = R.run(R.make_case("ck")[0]["actor"], obs)
    h = tr.init_hidden(-1, rows)
    for t in range(2):
        hot, h, _, logits = tr.get_actions(obs[t], h, return_logits=True)
        np.testing.assert_allclose(logits.cpu().numpy(), ref[t].numpy(), rtol=1e-5, atol=2e-6)
        assert torch.equal(hot.cpu().argmax(-1), ref[t].argmax(-1)) and (hot.sum(-1) == 1).all()


@pytest.mark.gpu
def test_checkpoint_round_trip(tmp_path):
    from minimarl.checkpoint import load_checkpoint, save_checkpoint
    tr, batch, g, tg = make_trainer("sw")
    tr.train_policy_on_batch(batch, gumbel=g, target_gumbel=tg)
    save_checkpoint(str(tmp_path / "c.safetensors"), rmaddpg=tr)
    tr2 = make_trainer("sw")[0]
    load_checkpoint(str(tmp_path / "c.safetensors"), rmaddpg=tr2)
    assert tr2.num_updates == 1
    for t in (tr, tr2):
        t.train_policy_on_batch(batch, gumbel=g, target_gumbel=tg)
    assert torch.equal(tr.Pc, tr2.Pc) and torch.equal(tr.Pa, tr2.Pa) and torch.equal(tr.mc, tr2.mc)
