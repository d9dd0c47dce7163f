"""GPU: OffQMix(..., prev_act_inp=True) (csrc/offq.hip, RowSrc) against the float64 oracle fed the explicit
concatenation cat(obs, prev), prev[:, 0] = 0, prev[:, t] = acts[:, t - 1]. One update per case; the bounds are those
of tests/test_gpu_offq_shapes.py (same arithmetic and precision, five more terms in the first layer):
gradients rel L2 <= max(8 x e32, 2e-6), e32 = the float32 oracle's error on the same case.

  one_row  N 1 T 1 B 1 D 47: step 0 has a zero previous action, step 1 has acts[0]; Whh gets exactly zero gradient
  d99      N 3 T 7 B 5 D 94: D' = 99 across both lane halves; N != B != T; 105 backward rows leave a 1-row tail group
  d8_vdn   N 2 T 3 B 4 D 3:  D' = 8, the padded LDS stride branch
  two_pass N 4 T 33 B 63 D 47: 8568 forward rows (> 2048 waves: the prefetch carries into a second pass) and 8316
           backward rows (> 2048 waves x 4 rows)

Measured worst err_hip / e32 per case (tensor, its err_hip), MI355X:
  one_row 2.03 (hyper_w1.2.bias, 3.9e-7)   d99 1.66 (hyper_b2.0.bias, 9.3e-8)
  d8_vdn 1.40 (lnr_w, 4.3e-7)              two_pass 0.83 (hyper_w1.2.bias, 1.8e-7)
Loss, Q_tot and grad_norm agree with float64 to 1.6e-7 or better in every case.
"""
import functools
import types

import numpy as np
import pytest
import torch

from offq_cases import (A, H, HYPER, MIN_KINK_MARGIN, MIN_TOP2_GAP, build_case, grad_keys, kink_inputs, make_batch,
                        random_agent, random_mixer, rel_l2)
from oracle import offq as ref
from test_gpu_offq_shapes import FLOOR, RATIO, agent_sd, sample

pytestmark = pytest.mark.gpu
#           N  T   B   D   K   Hh  mixer   dQ     PER    huber  seeds (params, target, batch)
CASES = {
    "one_row":  (1, 1, 1, 47, 1, 1, "qmix", True, True, False, (303, 304, 305)),
    "d99":      (3, 7, 5, 94, 5, 17, "qmix", False, True, True, (313, 314, 315)),
    "d8_vdn":   (2, 3, 4, 3, 32, 64, "vdn", True, True, False, (323, 324, 325)),
    "two_pass": (4, 33, 63, 47, 32, 64, "qmix", True, True, False, (343, 334, 335)),   # parameter seed 333 missed MIN_TOP2_GAP
}


def with_prev(obs, acts):
    """[N, T+1, B, D], [N, T, B, A] -> [N, T+1, B, D + A] (qmix.py:127-153)."""
    prev = np.concatenate([np.zeros_like(acts[:, :1]), acts], axis=1)
    return np.concatenate([obs, prev], axis=-1)


@functools.lru_cache(maxsize=None)
def case(cid):
    c = types.SimpleNamespace(id=cid, max_norm=10.0)
    c.N, c.T, c.B, c.D, c.K, c.Hh, c.mixer, c.double_q, c.use_per, c.huber, (ps, ts, bs) = CASES[cid]
    qm = c.mixer == "qmix"
    c.P, c.PT = random_agent(ps, c.D + A), random_agent(ts, c.D + A)
    c.M = random_mixer(ps, c.N, c.D, c.K, c.Hh) if qm else {}
    c.MT = random_mixer(ts, c.N, c.D, c.K, c.Hh) if qm else {}
    c.batch = make_batch(bs, c.N, c.T, c.B, c.D, c.use_per)
    c.cat = dict(c.batch, obs=with_prev(c.batch["obs"], c.batch["acts"]))
    kink_inputs(c.P, c.M, c.cat, adjust=True)
    assert kink_inputs(c.P, c.M, c.cat, adjust=False) >= MIN_KINK_MARGIN
    kw = dict(mixer=c.mixer, double_q=c.double_q, use_per=c.use_per, huber=c.huber, K=c.K, max_norm=c.max_norm,
              gamma=HYPER["gamma"], per_nu=HYPER["per_nu"], per_eps=HYPER["per_eps"], lr=HYPER["lr"], eps=HYPER["eps"])
    c.huber_delta = 10.0
    if c.huber:
        fw = ref.train_batch(c.P, c.M, c.PT, c.MT, c.cat, dtype=torch.float64, update=False, **kw)[2]
        c.huber_delta = float(fw["err"].abs()[fw["mask"] > 0].median())
    kw["huber_delta"] = c.huber_delta
    c.P64, c.M64, c.info64 = ref.train_batch(c.P, c.M, c.PT, c.MT, c.cat, dtype=torch.float64, **kw)
    c.info32 = ref.train_batch(c.P, c.M, c.PT, c.MT, c.cat, dtype=torch.float32, **kw)[2]
    with torch.no_grad():
        c.q64 = ref.agent_q_seq(c.P, ref.stack_agents(torch.tensor(c.cat["obs"])), dtype=torch.float64)[0]
    top2 = c.q64.topk(2, dim=-1)[0]
    assert float((top2[..., 0] - top2[..., 1]).min()) >= MIN_TOP2_GAP
    return c


def make_trainer(c, **kw):
    from minimarl.offq import OffQMix
    tr = OffQMix(c.N, c.D, A, c.T, c.B, mixer=c.mixer, mixer_hidden=c.K, hyper_hidden=c.Hh, gamma=HYPER["gamma"],
                 lr=HYPER["lr"], opti_eps=HYPER["eps"], max_grad_norm=c.max_norm, use_double_q=c.double_q,
                 use_per=c.use_per, use_huber_loss=c.huber, huber_delta=c.huber_delta, per_nu=HYPER["per_nu"],
                 per_eps=HYPER["per_eps"], **kw)
    qm = c.mixer == "qmix"
    tr.load_reference_state(agent_sd(c.P), {k: v.numpy() for k, v in c.M.items()} if qm else None,
                            agent_sd(c.PT), {k: v.numpy() for k, v in c.MT.items()} if qm else None)
    return tr


def one_update(c, with_q, **kw):
    tr = make_trainer(c, **kw)
    out = {}
    if with_q:
        xs = ref.stack_agents(torch.tensor(c.cat["obs"]))          # [T+1, N*B, D + A]
        out["q"] = tr.get_q_values(xs[..., :c.D].cuda(), prev_actions=xs[..., c.D:].cuda())[0].cpu()
    info, prio, _ = tr.train_policy_on_batch(sample(c))
    torch.cuda.synchronize()
    out.update({k: float(v) for k, v in info.items()})
    out["prio"], out["grad"], out["P"] = prio.cpu().clone(), tr.grad.cpu().clone(), tr.P.cpu().clone()
    for name in ("grad", "P"):
        out[name + "_of"] = {(kind, k): (tr.agent_view if kind == "agent" else tr.mixer_view)(k, out[name]).numpy()
                             for kind, k in grad_keys(c)}
    return out


@functools.lru_cache(maxsize=None)
def run_case(cid):
    return one_update(case(cid), True, prev_act_inp=True)


@pytest.mark.parametrize("cid", list(CASES))
def test_prev_act_update_vs_fp64(cid):
    c, o = case(cid), run_case(cid)
    q64 = c.q64.numpy()
    assert np.array_equal(o["q"].numpy().argmax(-1), q64.argmax(-1))
    np.testing.assert_allclose(o["q"].numpy(), q64, rtol=1e-4, atol=1e-5)
    for k, k64 in (("loss", "loss"), ("Q_tot", "q_tot"), ("grad_norm", "grad_norm")):
        print(f"{cid} {k}: hip {o[k]:.9g} fp64 {c.info64[k64]:.9g} rel {abs(o[k] / c.info64[k64] - 1):.3g}")
        np.testing.assert_allclose(o[k], c.info64[k64], rtol=2e-5)
    np.testing.assert_allclose(o["prio"].numpy(), c.info64["priorities"], rtol=2e-5)
    g64, g32 = c.info64["raw_grads"], c.info32["raw_grads"]
    gmax = max(float(g.abs().max()) for g in g64.values())
    if c.T == 1:
        assert not bool(g64["Whh"].any())
    bad, worst = [], (0.0, None, 0.0)
    for kind, k in grad_keys(c):
        g = o["grad_of"][kind, k]
        assert g.shape == tuple(g64[k].shape)
        if not bool(g64[k].any()):
            if not np.abs(g).max() <= FLOOR * gmax:
                bad.append(f"{k}: fp64 gradient is 0, hip max |g| {np.abs(g).max():.3g}")
            continue
        e32, e = rel_l2(g32[k].numpy(), g64[k].numpy()), rel_l2(g, g64[k].numpy())
        worst = max(worst, (e / e32, k, e))
        if not e <= max(RATIO * e32, FLOOR):
            bad.append(f"{k}: rel L2 {e:.3g} > max({RATIO:g} x {e32:.3g}, {FLOOR:g})")
    print(f"{cid}: worst err_hip / e32 = {worst[0]:.2f} ({worst[1]}, err {worst[2]:.3g})")
    assert not bad, "\n".join(bad)
    for kind, k in grad_keys(c):
        new64 = (c.P64 if kind == "agent" else c.M64)[k].numpy()
        np.testing.assert_allclose(o["P_of"][kind, k], new64, rtol=1e-5, atol=2e-6, err_msg=k)
    if cid == "d99":
        # the five action columns carry gradient of their own: a kernel that ignored them would pass the obs columns
        for k, sl in (("ln0_w", np.s_[c.D:]), ("ln0_b", np.s_[c.D:]), ("W1", np.s_[:, c.D:])):
            want = g64[k].numpy()[sl]
            assert np.abs(want).min() > 0 and want.shape[-1] == A
            assert rel_l2(o["grad_of"]["agent", k][sl], want) <= max(RATIO * rel_l2(g32[k].numpy()[sl], want), FLOOR)


@pytest.mark.parametrize("cid", list(CASES))
def test_prev_act_deterministic(cid):
    o, o2 = run_case(cid), one_update(case(cid), False, prev_act_inp=True)
    assert torch.equal(o["grad"], o2["grad"]) and torch.equal(o["P"], o2["P"])


@pytest.mark.parametrize("L,R,D,target", [(1, 1, 47, False), (2, 70, 94, True), (3, 1400, 3, False)])
def test_prev_act_q_values_vs_fp64(L, R, D, target):
    """get_q_values on its own, non-zero h0, random one-hot previous actions; 3 x 1400 rows are past the one-net cap
    of 256 blocks x 16 waves."""
    from minimarl.offq import OffQMix
    from minimarl.synth import gen_obs
    P, PT = random_agent(401, D + A), random_agent(402, D + A)
    tr = OffQMix(2, D, A, 2, 2, mixer="vdn", prev_act_inp=True)
    tr.load_reference_state(agent_sd(P), None, agent_sd(PT), None)
    rng = np.random.default_rng(403)
    x = torch.tensor(gen_obs(rng, (L, R, D)))
    pa = torch.nn.functional.one_hot(torch.tensor(rng.integers(0, A, (L, R))), A).float()
    h0 = torch.tensor(rng.standard_normal((R, H)).astype(np.float32) * 0.3)
    with torch.no_grad():
        q64, h64 = ref.agent_q_seq(PT if target else P, torch.cat([x, pa], -1), h0, dtype=torch.float64)
    q, h = tr.get_q_values(x.cuda(), h0.cuda(), target=target, prev_actions=pa.cuda())
    assert q.shape == (L, R, A) and h.shape == (R, H)
    np.testing.assert_allclose(q.cpu().numpy(), q64.numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(h.cpu().numpy(), h64.numpy(), rtol=1e-4, atol=1e-5)
    if not target:
        top2 = q64[0].topk(2, dim=-1)[0]
        assert float((top2[:, 0] - top2[:, 1]).min()) >= MIN_TOP2_GAP
        act, _, gq = tr.get_actions(x[0].cuda(), h0.cuda(), prev_actions=pa[0].cuda())
        assert torch.equal(act.cpu().argmax(-1), q64[0].argmax(-1)) and bool((act.sum(-1) == 1).all())
        np.testing.assert_allclose(gq.cpu().numpy()[:, 0], q64[0].max(-1)[0].numpy(), rtol=1e-4, atol=1e-5)


def test_default_is_unchanged():
    """prev_act_inp=False gives the bits of a trainer built without the keyword (existing odd_d94 case)."""
    c = build_case("odd_d94")
    assert torch.equal(one_update(c, False, prev_act_inp=False)["grad"], one_update(c, False)["grad"])
