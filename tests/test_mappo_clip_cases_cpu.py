"""CPU: the cases of tests/mappo_clip_cases.py build (their coverage, margin and class-stability conditions are
asserted by the builder), and they DISCRIMINATE: a loss seed that gets one of PPO's branches wrong lands further than
the GPU tests' bar (K_FP32 fp32 spreads) from the float64 oracle's gradient. This is the only place that is decided;
tests/test_gpu_mappo_clip.py then holds the kernels to that bar."""
import numpy as np
import pytest
import torch

import mappo_clip_cases as cc
from oracle import mappo as om

ACTOR, CRITIC = 0, 1
#            the one change to the loss (ramppo_network.py:68-92,150-166)                     the net it changes
MUTATIONS = {
    "surrogate_without_clip": ("s2 := s1", ACTOR),
    "clamp_straight_through": ("ratio + (clamp(ratio) - ratio).detach()", ACTOR),
    "value_loss_without_clipped_term": ("max(lo, lc) := lo", CRITIC),
    "value_clip_straight_through": ("dv + (clamp(dv) - dv).detach()", CRITIC),
    "max_gradient_always_unclipped_side": ("lo + (max(lo, lc) - lo).detach()", CRITIC),
    "huber_quadratic": ("huber(e) := e^2 / 2", CRITIC),
}


def _gradients(c, mutation=None):
    """The float64 unclipped gradients {(net, key)} of the oracle's loss on update 0 of a case, with one mutation."""
    with cc._default_dtype(torch.float64):
        PA, PC, b, vn, _ = c.batch(torch.float64, False, 0)
        pa = {k: v.detach().clone().requires_grad_(True) for k, v in PA.items()}
        pc = {k: v.detach().clone().requires_grad_(True) for k, v in PC.items()}
        lp, ent = om.evaluate_chunks(pa, b["obs"], b["ha0"], b["masks"], c.L, "actor", b["actions"], b["active_masks"])
        v = om.evaluate_chunks(pc, b.get("cent_obs", b["obs"]), b["hc0"], b["masks"], c.L, "critic")
        m = b["active_masks"]
        ratio = torch.exp(lp - b["action_log_probs"])
        s1 = ratio * b["adv"]
        rc = torch.clamp(ratio, 1.0 - c.clip, 1.0 + c.clip)
        if mutation == "clamp_straight_through":
            rc = ratio + (rc - ratio).detach()
        s2 = s1 if mutation == "surrogate_without_clip" else rc * b["adv"]
        pol = (-torch.sum(torch.min(s1, s2), dim=-1, keepdim=True) * m).sum() / m.sum()
        dv = v - b["value_preds"]
        dvc = dv.clamp(-c.clip, c.clip)
        if mutation == "value_clip_straight_through":
            dvc = dv + (dvc - dv).detach()
        tgt = vn.normalize(b["returns"])
        hub = (lambda e: e ** 2 / 2) if mutation == "huber_quadratic" else (lambda e: om.huber(e, c.huber_delta))
        lo, lc = hub(tgt - v), hub(tgt - (b["value_preds"] + dvc))
        if mutation == "value_loss_without_clipped_term":
            vl = lo
        elif mutation == "max_gradient_always_unclipped_side":
            vl = lo + (torch.max(lo, lc) - lo).detach()
        else:
            vl = torch.max(lo, lc)
        vloss = (vl * m).sum() / m.sum()
        ga = torch.autograd.grad(pol - ent * 0.01, [pa[k] for k in om.NET_KEYS])
        gc = torch.autograd.grad(vloss * 0.5, [pc[k] for k in om.NET_KEYS])
    out = {(ACTOR, k): g.numpy() for k, g in zip(om.NET_KEYS, ga)}
    out.update({(CRITIC, k): g.numpy() for k, g in zip(om.NET_KEYS, gc)})
    return out


@pytest.mark.parametrize("cid", list(cc.CASES))
def test_case_builds_and_its_ratio_is_off_one(cid):
    """The builder's assertions hold (mappo_clip_cases' docstring); huber_delta splits the rows; the float64 mean
    ratio of the first update differs from 1 by more than 1e-2."""
    c = cc.case(cid)
    print(cid, "huber_delta", c.huber_delta, "mean ratio", c.ratio0,
          {k: round(float(v), 3) for k, v in c.shares.items()})
    assert abs(c.ratio0 - 1.0) > 1e-2, c.ratio0
    assert c.clip == cc.CASES[cid][1] and 0.0 < c.huber_delta < 10.0
    g64, spread = c.grads
    assert len(g64) == c.n_updates * 2 * len(om.NET_KEYS) and all(np.isfinite(g).all() for g in g64.values())


def test_golden16_three_epochs_keep_their_classes_and_ratio():
    """golden16's three-epoch train(): every row keeps its class in every epoch of the three oracle runs (asserted
    by the builder); the float64 mean ratio over the epochs is off 1 by more than 1e-2 and is the reference's."""
    o64, spread, ratio = cc.train_answers("golden16")
    assert abs(ratio - 1.0) > 1e-2, ratio
    np.testing.assert_allclose(ratio, float(cc.case("golden16").fx["info.ratio"]), rtol=1e-5)


@pytest.mark.parametrize("cid", list(cc.CASES))
def test_unmutated_restatement_is_the_oracle(cid):
    """_gradients without a mutation is the case's own float64 oracle (so a mutation is the only difference)."""
    c = cc.case(cid)
    g64, _ = c.grads
    for (n, k), g in _gradients(c).items():
        np.testing.assert_allclose(g, g64[(0, n, k)], rtol=1e-9, atol=1e-14, err_msg=f"{cid} net {n} {k}")


@pytest.mark.parametrize("mutation", list(MUTATIONS))
@pytest.mark.parametrize("cid", list(cc.CASES))
def test_mutation_is_outside_the_bar(cid, mutation):
    """A loss with this one branch wrong gives a gradient more than K_FP32 spreads from the float64 oracle's on at
    least one tensor of the net it changes: the GPU tests' bar would catch it."""
    c = cc.case(cid)
    g64, spread = c.grads
    net = MUTATIONS[mutation][1]
    g = _gradients(c, mutation)
    worst = max(float(np.abs(g[(net, k)] - g64[(0, net, k)]).max()) / spread[(0, net, k)] for k in om.NET_KEYS)
    print(f"{cid} {mutation}: worst |mutated - f64| / spread = {worst:.3g}")
    assert worst > cc.K_FP32, f"{cid}: '{mutation}' moves no tensor by more than {cc.K_FP32} spreads ({worst:.3g})"
    plain = _gradients(c)
    for k in om.NET_KEYS:     # (and it changes nothing in the other net)
        np.testing.assert_array_equal(g[(1 - net, k)], plain[(1 - net, k)])
