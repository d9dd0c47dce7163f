"""GPU: the MAPPO loss seed with PPO's branches ACTIVE -- the surrogate clip, the clipped value loss' max and Huber's
linear arm -- in both of its copies (the fused MFMA pass csrc/mappo_grad.hip: mm_mappo_grad, mm_mappo_grad_mb and the
centralized-critic instantiation; the saves + wgrad path csrc/mappo.hip, MappoTrainer(fused=False)), on the cases of
tests/mappo_clip_cases.py, whose docstring states what the inputs guarantee (class coverage, margins to every branch
point, class stability across the oracle's runs) and tests/test_mappo_clip_cases_cpu.py shows that a seed with one
branch wrong lands millions of spreads away. Every other MAPPO test trains on a ratio of exactly 1 and |dv| < clip.

The bar is the project's and nothing new (tests/test_gpu_mappo.py's docstring): K_FP32 = 16 fp32 spreads (fp32 in
chunk order / fp32 in another order / float64) of the float64 oracle; against the golden's recorded values the
reference's own distance to float64 is added; the mean ratio at rtol 1e-5.

Measured on an MI355X, worst |device - f64| / spread over the tensors of a net (the bar is 16), actor / critic:
  epoch-0 gradients   golden16  fused 1.98 / 1.20   saves + wgrad 2.18 / 2.12
                      tiles70   fused 1.66 / 4.58   saves + wgrad 1.70 / 2.17
                      cent_n2   fused 2.29 / 1.32
                      mb16      update 0  2.08 / 1.81   update 1  1.66 / 1.38
  3-epoch train()     golden16  parameters fused 2.53 / 2.19, saves + wgrad 3.73 / 3.39; on both paths value_loss
                      0.47, policy_loss 1.04, dist_entropy 0.77, actor_grad_norm 1.52, critic_grad_norm 0.25;
                      mean ratio device 1.0235877, float64 1.0235876, golden 1.0235876
  plumbing (tiles70)  the default clip_param and huber_delta move the actor's gradient by 2.8e6 spreads and the
                      critic's by 1.2e7; the default huber_delta alone moves the critic's by 9.4e6
No arm of either copy of the seed was found wrong.
"""
import numpy as np
import pytest
import torch

import mappo_clip_cases as cc
import mappo_mb_ref as mb
from oracle import mappo as om

pytestmark = pytest.mark.gpu
DEV = "cuda"
K_FP32 = cc.K_FP32
NETS = ("actor", "critic")
FUSED = pytest.mark.parametrize("fused", [True, False], ids=["fused_mfma", "saves_wgrad"])


def _trainer(c, fused=True, **kw):
    """Policy, buffer and trainer of a case, with the case's clip_param and huber_delta unless kw says otherwise."""
    from minimarl.mappo import MappoBuffer, MappoPolicy, MappoTrainer
    p = MappoPolicy(cc.D, cc.A, cc.H, DEV, cent_agents=c.N if c.kind == "cent" else None)
    for net, P in ((p.actor, c.PA), (p.critic, c.PC)):
        for k in om.NET_KEYS:
            net.view(k).copy_(P[k].to(DEV))
    buf = MappoBuffer(c.T, c.E, c.N, cc.D, cc.H, DEV)
    buf.load_reference(c.data)
    kw.setdefault("clip_param", c.clip)
    kw.setdefault("huber_delta", c.huber_delta)
    tr = MappoTrainer(p, c.T, c.E * c.N, L=c.L, ppo_epoch=cc.TRAIN_EPOCHS, fused=fused, num_mini_batch=c.M, **kw)
    tr.load_value_normalizer(*c.vn0)
    return p, buf, tr


def _vn_update(tr):
    from minimarl._lib import lib
    assert lib().mm_mappo_vn_update(tr.vn.data_ptr(), tr.stats.data_ptr(), 0.99999, None) == 0


def _nan_grads(tr):
    tr.grad[0].fill_(float("nan"))
    tr.grad[1].fill_(float("nan"))


def _epoch0_gradients(c, fused=True, **kw):
    """The unclipped gradients of PPO epoch 0 on the device; on the fused path every entry of tr.grad is pre-filled
    with NaN (the pass writes all of them, pads included)."""
    p, buf, tr = _trainer(c, fused, **kw)
    tr.prepare(buf)
    _vn_update(tr)
    if fused:
        _nan_grads(tr)
    tr.gradients(buf)
    torch.cuda.synchronize()
    return p, tr


def _check_gradients(c, p, tr, u=0, golden=False):
    """Every tensor of both nets within K_FP32 spreads of the float64 oracle's update-u gradient (and, golden: of the
    reference's recorded one plus its own distance to float64); pads exactly zero; all finite. Prints the worst
    |device - f64| / spread per net."""
    g64, spread = c.grads
    for n, net in enumerate((p.actor, p.critic)):
        worst = 0.0
        for k in om.NET_KEYS:
            g = net.view(k, tr.grad[n]).cpu().numpy()
            want, sp = g64[(u, n, k)], spread[(u, n, k)]
            worst = max(worst, float(np.abs(g - want).max()) / sp)
            mb.assert_within(g, want, sp, f"{c.cid} update {u} {NETS[n]} {k} vs f64")
            if golden:
                ref = mb.golden_grad(c.fx, u, n, k)
                mb.assert_within(g, ref, sp, f"{c.cid} update {u} {NETS[n]} {k} vs golden",
                                 float(np.abs(ref - want).max()))
        print(f"WORST {c.cid} update {u} {NETS[n]}: |dev - f64| / spread = {worst:.2f}")
        pad = torch.ones_like(tr.grad[n], dtype=torch.bool)
        for k in om.NET_KEYS:
            net.view(k, pad).fill_(False)
        assert int(pad.sum()) > 0 and bool((tr.grad[n][pad] == 0).all()), "pads must carry zero gradient"
        assert bool(torch.isfinite(tr.grad[n]).all())


# ---------------------------------------------------------------- 1: epoch-0 gradients, both implementations
@FUSED
@pytest.mark.parametrize("cid", ["golden16", "tiles70"])
def test_epoch0_gradients_with_active_branches(cid, fused):
    """golden16 (16 chunks: less than a tile; also against the reference's recorded gradients) and tiles70 (70 chunks:
    a ragged last tile; clip_param 0.1), through mm_mappo_grad and through the saves + wgrad path."""
    c = cc.case(cid)
    p, tr = _epoch0_gradients(c, fused)
    _check_gradients(c, p, tr, golden=cid == "golden16")


# ---------------------------------------------------------------- 2: the two copies of the seed against each other
def test_fused_matches_saves_path_and_is_deterministic():
    """tiles70 at the bar of test_gpu_mappo.test_fused_gradients_match_saves_path_and_are_deterministic:
    |g_fused - g_saves| <= 1e-4 max|g| + 1e-4 |g|; two fused runs are bit-identical."""
    c = cc.case("tiles70")
    g = {}
    for fused in (True, False, True):
        _, tr = _epoch0_gradients(c, fused)
        got = [x.cpu().numpy().copy() for x in tr.grad]
        if fused in g:
            for n in (0, 1):
                np.testing.assert_array_equal(got[n], g[fused][n])
        g.setdefault(fused, got)
    for n in (0, 1):
        a, ref = g[True][n], g[False][n]
        assert np.isfinite(a).all() and np.abs(ref).max() > 0
        np.testing.assert_array_less(np.abs(a - ref), 1e-4 * np.abs(ref).max() + 1e-4 * np.abs(ref) + 1e-9)


# ---------------------------------------------------------------- 3: the centralized critic's value seed
def test_centralized_critic_epoch0_gradients():
    """cent_n2 (cent_agents 2, 20 chunks) against mappo_cv_ref.ppo_train_cv with the case's clip and huber_delta."""
    c = cc.case("cent_n2")
    p, tr = _epoch0_gradients(c)
    assert p.cent_agents == 2
    _check_gradients(c, p, tr)


# ---------------------------------------------------------------- 4: mm_mappo_grad_mb
def test_minibatch_gradients_of_updates_0_and_1():
    """mb16: the recorded permutation's first two minibatches of 5 chunks through gradients_mb, the second after the
    first's clip + Adam step; gradients and scratch pre-filled with NaN
    (test_gpu_mappo_mb.test_first_two_update_gradients_match_reference)."""
    c = cc.case("mb16")
    p, buf, tr = _trainer(c)
    native = tr.native_chunks(c.perms)
    tr.prepare(buf)
    ba = tr.bwd_args(buf)
    tr.gscr.fill_(float("nan"))
    for u in (0, 1):
        ch = native[0, u * tr.mbs:(u + 1) * tr.mbs]
        assert ch.numel() == 5
        tr.mb_stats(buf, ch)
        _vn_update(tr)
        _nan_grads(tr)
        tr.gradients_mb(buf, ch, ba)
        torch.cuda.synchronize()
        _check_gradients(c, p, tr, u)
        tr.clip_adam(u)


# ---------------------------------------------------------------- 5: three epochs of train()
@FUSED
def test_three_epoch_train_with_active_branches(fused):
    """golden16's train() (3 epochs; the rows keep their classes in every epoch, asserted by the builder):
    post-Adam parameters, ValueNorm state, the three losses and both gradient norms within K_FP32 spreads of the
    float64 oracle and of the golden (plus its own distance to float64); the mean ratio, for the first time at a
    value other than 1, at rtol 1e-5 against both."""
    c = cc.case("golden16")
    o64, spread, ratio64 = cc.train_answers("golden16")
    fx = c.fx
    p, buf, tr = _trainer(c, fused)
    assert tr.epochs == int(fx["epochs"])
    info = tr.train(buf)
    torch.cuda.synchronize()
    worst = {}
    for net, kind in ((p.actor, "actor"), (p.critic, "critic")):
        for k in om.NET_KEYS:
            got = net.view(k).cpu().numpy()
            after = fx[f"after.{kind}.{om.ref_name(k, kind)}"]
            worst[kind] = max(worst.get(kind, 0.0), float(np.abs(got - o64[(kind, k)]).max()) / spread[(kind, k)])
            mb.assert_within(got, o64[(kind, k)], spread[(kind, k)], f"{kind} {k} vs f64")
            mb.assert_within(got, after, spread[(kind, k)], f"{kind} {k} vs golden",
                             float(np.abs(after - o64[(kind, k)]).max()))
    vn = tr.value_normalizer_state()
    for key, mine, gk in (("vn_mean", "running_mean", "vn1.running_mean"),
                          ("vn_mean_sq", "running_mean_sq", "vn1.running_mean_sq")):
        mb.assert_within(vn[mine], o64[key], spread[key], key)
        mb.assert_within(vn[mine], fx[gk], spread[key], key + " vs golden", float(np.abs(fx[gk] - o64[key]).max()))
    for key in ("value_loss", "policy_loss", "dist_entropy", "actor_grad_norm", "critic_grad_norm"):
        worst[key] = abs(info[key] - float(o64[key])) / spread[key]
        mb.assert_within(info[key], o64[key], spread[key], key)
        mb.assert_within(info[key], float(fx["info." + key]), spread[key], key + " vs golden",
                         abs(float(fx["info." + key]) - float(o64[key])))
    print("WORST golden16 train():", ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    print(f"ratio: device {info['ratio']:.7f}, f64 {ratio64:.7f}, golden {float(fx['info.ratio']):.7f}")
    assert abs(ratio64 - 1.0) > 1e-2
    np.testing.assert_allclose(info["ratio"], ratio64, rtol=1e-5)
    np.testing.assert_allclose(info["ratio"], float(fx["info.ratio"]), rtol=1e-5)


# ---------------------------------------------------------------- 6: clip_param and huber_delta reach the kernels
@FUSED
def test_clip_param_and_huber_delta_reach_the_kernel(fused):
    """tiles70 (clip 0.1, the median delta): a trainer with the default clip_param and huber_delta gives gradients
    more than K_FP32 spreads from the case's on some tensor of each net; with the case's clip_param and only
    huber_delta left at its default the actor's are bit-identical and the critic's again differ."""
    c = cc.case("tiles70")
    _, spread = c.grads
    p, tr = _epoch0_gradients(c, fused)
    mine = [g.clone() for g in tr.grad]

    def off(tr2, n):
        net = (p.actor, p.critic)[n]
        return max(float((net.view(k, tr2.grad[n]) - net.view(k, mine[n])).abs().max()) / spread[(0, n, k)]
                   for k in om.NET_KEYS)

    _, dflt = _epoch0_gradients(c, fused, clip_param=0.2, huber_delta=10.0)
    assert dflt.clip == 0.2 and dflt.huber == 10.0 and (tr.clip, tr.huber) == (c.clip, c.huber_delta)
    for n in (0, 1):
        print(f"{NETS[n]}: default arguments move the gradient by {off(dflt, n):.3g} spreads")
        assert off(dflt, n) > K_FP32, f"{NETS[n]}: clip_param / huber_delta do not reach the kernel"
    _, hub = _epoch0_gradients(c, fused, huber_delta=10.0)
    assert torch.equal(hub.grad[0], mine[0]), "huber_delta changed the actor's gradient"
    print(f"critic: the default huber_delta alone moves the gradient by {off(hub, 1):.3g} spreads")
    assert off(hub, 1) > K_FP32, "huber_delta does not reach the kernel"
