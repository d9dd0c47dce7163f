"""GPU parity of MAPPO with a centralized critic (use_centralized_V: MappoPolicy(cent_agents=N), the critic reads
the env's share_obs) against the reference's golden vectors (tests/golden/mappo_cv_*.npz) and the restatement
(tests/mappo_cv_ref.py), at tests/test_gpu_mappo.py's tolerances: forwards rtol 1e-5 / atol 2e-6; gradients and
trained parameters within K_FP32 = 16 fp32 spreads of the f64 restatement (mappo_cv_ref.fp32_spread: fp32 vs
permuted-order fp32 vs f64)."""
import ctypes

import numpy as np
import pytest
import torch

import mappo_cv_ref as cv
from oracle import mappo as om

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = dict(rtol=1e-5, atol=2e-6)
K_FP32 = 16
D, A, H = 47, 5, 32


def _assert_within(got, want, spread, what):
    err = float(np.abs(np.asarray(got, np.float64) - want).max())
    print(f"{what}: |dev - f64| = {err:.3e}, {K_FP32} x spread = {K_FP32 * spread:.3e}")
    assert err <= K_FP32 * spread, f"{what}: |dev - f64| = {err:.3e} > {K_FP32} x spread {spread:.3e}"


def _policy(fx, N, prefix=""):
    from minimarl.mappo import MappoPolicy
    p = MappoPolicy(D, A, H, DEV, cent_agents=N)
    p.actor.load_reference_state(fx, prefix + "actor.")
    p.critic.load_reference_state(fx, prefix + "critic.")
    return p


def _oracle_nets(p):
    return ({k: p.actor.view(k).detach().cpu().clone() for k in om.NET_KEYS},
            {k: p.critic.view(k).detach().cpu().clone() for k in om.NET_KEYS})


# ---------------------------------------------------------------- 1, 2: forwards
@pytest.mark.parametrize("name", ["n2", "n8"])
def test_get_actions_and_values_match_reference(golden, name):
    """get_actions / get_values vs the golden, in the grouped form (cent_obs NULL: the kernel gathers the env's
    adjacent obs rows) and the explicit form (cent_obs [R, N*D]); the two forms bit-identical."""
    fx = cv.case(golden("mappo_cv_fwd"), name)
    E, N = int(fx["E"]), int(fx["N"])
    p = _policy(fx, N)
    t = lambda k: torch.from_numpy(fx[k]).to(DEV)
    cent = torch.from_numpy(cv.share_obs(fx["obs"].reshape(E, N, -1)).reshape(E * N, -1)).to(DEV)
    outs = []
    for co in (None, cent):
        v, a, lp, ha, hc = p.get_actions(t("obs"), t("ha")[:, 0], t("hc")[:, 0], t("masks"), actions=t("actions"),
                                         cent_obs=co)
        v2 = p.get_values(t("obs") if co is None else co, t("hc")[:, 0], t("masks"))
        torch.cuda.synchronize()
        np.testing.assert_allclose(v.cpu().numpy(), fx["values"], **TOL)
        np.testing.assert_allclose(v2.cpu().numpy(), fx["values_only"], **TOL)
        np.testing.assert_allclose(lp.cpu().numpy(), fx["logp"], **TOL)
        np.testing.assert_allclose(ha.cpu().numpy(), fx["ha_out"][:, 0], **TOL)
        np.testing.assert_allclose(hc.cpu().numpy(), fx["hc_out"][:, 0], **TOL)
        outs.append((v, v2, hc))
    for x, y in zip(*outs):
        assert torch.equal(x, y), "grouped and explicit cent_obs forms differ"


def test_rollout_forward_partial_tiles():
    """E 9, N 8: 72 rows = 2 tiles of 32 + 8. Values / log-probs / hiddens vs the restatement; rows beyond
    ``rows`` of every output stay untouched (sentinel-filled, 32 rows longer than the batch)."""
    from minimarl._lib import MM_MAPPO_VALUES
    from minimarl.mappo import MappoPolicy
    E, N = 9, 8
    R = E * N
    p = MappoPolicy(D, A, H, DEV, seed=5, cent_agents=N)
    PA, PC = _oracle_nets(p)
    g = torch.Generator().manual_seed(2)
    obs = (torch.rand(R, D, generator=g) < 0.3).float()
    obs[:, :2] = torch.rand(R, 2, generator=g)
    ha, hc = torch.randn(R, H, generator=g) * 0.5, torch.randn(R, H, generator=g) * 0.5
    masks = torch.ones(R, 1)
    masks[[3, 40, 71]] = 0.0
    act = torch.randint(0, A, (R, 1), generator=g)
    cent = torch.from_numpy(cv.share_obs(obs.numpy().reshape(E, N, D)).reshape(R, N * D))
    v, lp, ha2, hc2 = cv.get_actions_cv(PA, PC, obs, cent, ha, hc, masks, act)
    S = 777.0
    o_ha, o_hc = torch.full((R + 32, H), S, device=DEV), torch.full((R + 32, H), S, device=DEV)
    o_lp, o_v = torch.full((R + 32,), S, device=DEV), torch.full((R + 32,), S, device=DEV)
    # (the arguments hold raw pointers: the device inputs stay referenced until both launches have run)
    d_in = [x.to(DEV) for x in (obs, ha, hc, masks.reshape(-1), act.reshape(-1).to(torch.int32))]
    a = p.rollout_args(*d_in[:4], o_ha, o_hc, o_lp, o_v, act_in=d_in[4])
    p._fwd(a)
    o_v2, o_hc2 = torch.full((R + 32,), S, device=DEV), torch.full((R + 32, H), S, device=DEV)
    a.net[1].out, a.net[1].h_out, a.mode = o_v2.data_ptr(), o_hc2.data_ptr(), MM_MAPPO_VALUES
    p._fwd(a)
    torch.cuda.synchronize()
    for got, want in ((o_v, v[:, 0]), (o_v2, v[:, 0]), (o_lp, lp[:, 0]), (o_ha, ha2), (o_hc, hc2), (o_hc2, hc2)):
        np.testing.assert_allclose(got[:R].cpu().numpy(), want.numpy(), **TOL)
        assert bool((got[R:] == S).all()), "rows beyond `rows` were written"


# ---------------------------------------------------------------- 3 - 5: the fused gradient pass
def _trainer_from_fixture(fx, hc_distinct=False):
    from minimarl.mappo import MappoBuffer, MappoTrainer
    E, N, T, L = (int(fx[k]) for k in ("E", "N", "T", "L"))
    p = _policy(fx, N, "before.")
    PA, PC, data, vn0, nch = cv.train_inputs(fx)
    if hc_distinct:   # critic hiddens distinct per agent: a per-env shortcut that assumes them equal fails
        rng = np.random.default_rng(9)
        data["rnn_states_critic"] = (rng.standard_normal(data["rnn_states_critic"].shape) * 0.5).astype(np.float32)
    buf = MappoBuffer(T, E, N, D, H, DEV)
    buf.load_reference(data)
    tr = MappoTrainer(p, T, E * N, L=L, ppo_epoch=int(fx["epochs"]))
    tr.load_value_normalizer(*vn0)
    return p, buf, tr, (PA, PC, data, vn0, nch)


def _epoch0_gradients(tr, buf):
    from minimarl._lib import lib
    tr.prepare(buf)
    assert lib().mm_mappo_vn_update(tr.vn.data_ptr(), tr.stats.data_ptr(), 0.99999, None) == 0
    tr.grad[0].fill_(float("nan"))      # the fused pass writes every entry (pads included)
    tr.grad[1].fill_(float("nan"))
    tr.gradients(buf)
    torch.cuda.synchronize()


def _check_gradients(p, tr, oracle_in, L, fx=None):
    PA, PC, data, vn0, nch = oracle_in
    g64, spread = cv.fp32_spread(
        lambda dt, pm: cv.unclipped_grads(cv.ppo_train_cv(PA, PC, data, vn0, 1, L, perms=pm, dtype=dt)[0]), nch)
    for n, (net, tag) in enumerate(((p.actor, "a"), (p.critic, "c"))):
        kind = "actor" if n == 0 else "critic"
        for k in om.NET_KEYS:
            g = net.view(k, tr.grad[n]).cpu().numpy()
            _assert_within(g, g64[(n, k)], spread[(n, k)], f"{kind} {k} vs f64")
            if fx is not None:   # the reference's own fp32 gradients (clipped -> divided by its clip coefficient)
                coef = min(1.0, 0.5 / (float(fx["norms"][n]) + 1e-6))
                ref = fx[f"grad{tag}0.{om.ref_name(k, kind)}"] / coef
                ref_err = float(np.abs(ref - g64[(n, k)]).max())
                assert np.abs(g - ref).max() <= K_FP32 * spread[(n, k)] + ref_err, f"{kind} {k} vs golden"
        # pads of the flat layout carry exactly zero gradient (every entry was pre-filled with NaN): the entries no
        # tensor's logical view covers
        pad = torch.ones_like(tr.grad[n], dtype=torch.bool)
        for k in om.NET_KEYS:
            net.view(k, pad).fill_(False)
        assert int(pad.sum()) == net.total - sum(int(np.prod(net.shape(k))) for k in om.NET_KEYS) > 0
        assert bool((tr.grad[n][pad] == 0).all()), "non-zero gradient in a pad"
        assert bool(torch.isfinite(tr.grad[n]).all())


@pytest.mark.parametrize("name,hc_distinct", [("n2", False), ("n2", True), ("n8", False)],
                         ids=["n2", "n2_distinct_critic_hiddens", "n8"])
def test_first_epoch_gradients_match_reference(golden, name, hc_distinct):
    """Unclipped gradients of PPO epoch 0 of the fused pass on the golden buffers (N 2: 20 chunks, a partial
    tile; N 8: Dc 376, the last feature tile 24 wide), each tensor within K_FP32 fp32 spreads of the f64
    restatement, and the reference's own gradients within the same bar plus their own distance to f64.
    With the critic hiddens overwritten by values distinct per agent the golden gradients no longer apply (they
    were recorded on the stored hiddens): that case is held to the f64 restatement on the same buffer."""
    fx = cv.case(golden("mappo_cv_train"), name)
    p, buf, tr, oin = _trainer_from_fixture(fx, hc_distinct)
    _epoch0_gradients(tr, buf)
    _check_gradients(p, tr, oin, int(fx["L"]), None if hc_distinct else fx)


def _ref_layout(b, E, N):
    """MappoBuffer [T(+1), E*N, ...] -> the reference SharedReplayBuffer layout [T(+1), E, N, ..., 1]."""
    c = lambda t: t.detach().cpu().numpy()  # noqa: E731
    T1 = b.obs.shape[0]
    d = {"obs": c(b.obs).reshape(T1, E, N, -1),
         "rnn_states": c(b.rnn_states).reshape(T1, E, N, 1, -1),
         "rnn_states_critic": c(b.rnn_states_critic).reshape(T1, E, N, 1, -1),
         "actions": c(b.actions).astype(np.float32).reshape(T1 - 1, E, N, 1)}
    for k in ("action_log_probs", "rewards"):
        d[k] = c(getattr(b, k)).reshape(T1 - 1, E, N, 1)
    for k in ("value_preds", "returns", "masks", "active_masks"):
        d[k] = c(getattr(b, k)).reshape(T1, E, N, 1)
    return d


@pytest.fixture(scope="module")
def rollout_case():
    """A device rollout, E 9, N 8, T 10, L 5, max_steps 7 (resets fall inside chunks; 144 chunks = 4.5 tiles),
    prepared for the epoch-0 gradients. Shared by the gradient and the determinism test."""
    from minimarl._lib import lib
    from minimarl.env import VecEnv
    from minimarl.mappo import MappoPolicy, MappoRunner
    E, N, T, L = 9, 8, 10, 5
    env = VecEnv(E, N, max_steps=7, device=DEV)
    p = MappoPolicy(env.obs_dim, A, H, DEV, seed=3, cent_agents=N)
    PA, PC = _oracle_nets(p)
    r = MappoRunner(env, p, T=T, L=L, ppo_epoch=1, seed=11)
    r.warmup()
    r.rollout()
    r.compute()
    torch.cuda.synchronize()
    tr = r.trainer
    vn0 = [float(x) for x in tr.vn.cpu().numpy()]
    data = _ref_layout(r.buf, E, N)
    assert (data["masks"][[t for t in range(1, T) if t % L]] == 0).any(), "no reset inside a chunk"
    tr.prepare(r.buf)
    assert lib().mm_mappo_vn_update(tr.vn.data_ptr(), tr.stats.data_ptr(), 0.99999, None) == 0
    return p, r, (PA, PC, data, vn0, T * E * N // L), L


def _rollout_gradients(r):
    tr = r.trainer
    tr.grad[0].fill_(float("nan"))
    tr.grad[1].fill_(float("nan"))
    tr.gradients(r.buf)
    torch.cuda.synchronize()
    return [g.clone() for g in tr.grad]


def test_first_epoch_gradients_on_a_device_rollout(rollout_case):
    p, r, oin, L = rollout_case
    # the rollout's values are the centralized critic's: the restatement's get_values on the stored inputs
    PA, PC, data, _, _ = oin
    t = 4
    v, _ = om.net_step(PC, torch.from_numpy(cv.share_obs(data["obs"][t]).reshape(-1, 8 * D)),
                       torch.from_numpy(data["rnn_states_critic"][t, :, :, 0].reshape(-1, H)),
                       torch.from_numpy(data["masks"][t].reshape(-1, 1)))
    np.testing.assert_allclose(data["value_preds"][t].reshape(-1), v.numpy()[:, 0], **TOL)
    _rollout_gradients(r)
    _check_gradients(p, r.trainer, oin, L)


def test_gradients_are_deterministic(rollout_case):
    _, r, _, _ = rollout_case
    g1, g2 = _rollout_gradients(r), _rollout_gradients(r)
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)


def test_ppo_train_matches_reference(golden):
    """The N 2 golden train() (3 epochs): post-Adam parameters, ValueNorm state and the train_info log, at the
    bars of tests/test_gpu_mappo.py::test_ppo_train_matches_reference."""
    fx = cv.case(golden("mappo_cv_train"), "n2")
    p, buf, tr, (PA, PC, data, vn0, nch) = _trainer_from_fixture(fx)
    EP, L = int(fx["epochs"]), int(fx["L"])
    o64, spread = cv.fp32_spread(
        lambda dt, pm: cv.train_outputs(*cv.ppo_train_cv(PA, PC, data, vn0, EP, L, perms=pm, dtype=dt)), nch)
    info = tr.train(buf)
    torch.cuda.synchronize()
    for net, kind in ((p.actor, "actor"), (p.critic, "critic")):
        for k in om.NET_KEYS:
            got = net.view(k).cpu().numpy()
            after = fx[f"after.{kind}.{om.ref_name(k, kind)}"]
            _assert_within(got, o64[(kind, k)], spread[(kind, k)], f"{kind} {k} vs f64")
            ref_err = float(np.abs(after - o64[(kind, k)]).max())
            assert np.abs(got - after).max() <= K_FP32 * spread[(kind, k)] + ref_err, f"{kind} {k} vs golden"
    vn = tr.value_normalizer_state()
    _assert_within(vn["running_mean"], o64["vn_mean"], spread["vn_mean"], "vn mean")
    _assert_within(vn["running_mean_sq"], o64["vn_mean_sq"], spread["vn_mean_sq"], "vn mean_sq")
    for key in ("value_loss", "policy_loss", "dist_entropy", "actor_grad_norm", "critic_grad_norm"):
        _assert_within(info[key], o64[key], spread[key], key)
        ref_err = abs(float(fx["info." + key]) - float(o64[key]))
        assert abs(info[key] - float(fx["info." + key])) <= K_FP32 * spread[key] + ref_err, key
    np.testing.assert_allclose(info["ratio"], float(fx["info.ratio"]), rtol=1e-5)


# ---------------------------------------------------------------- 6: runner
def test_runner_episode_end_to_end():
    """E 64, N 8, T 20, L 5, 2 PPO epochs: finite train info, parameters moved, and the stored values agree
    across the agents of an env (the same share_obs, zero-start critic hiddens, per-env masks)."""
    from minimarl.env import VecEnv
    from minimarl.mappo import MappoPolicy, MappoRunner
    E, N, T = 64, 8, 20
    env = VecEnv(E, N, max_steps=12, device=DEV)
    p = MappoPolicy(env.obs_dim, A, H, DEV, seed=0, cent_agents=N)
    r = MappoRunner(env, p, T=T, L=5, ppo_epoch=2, seed=1)
    before = [p.actor.flat.clone(), p.critic.flat.clone()]
    r.warmup()
    info = r.run_episode()
    torch.cuda.synchronize()
    assert all(np.isfinite(v) for v in info.values()), info
    vp = r.buf.value_preds.view(T + 1, E, N).cpu().numpy()
    np.testing.assert_allclose(vp, np.broadcast_to(vp[:, :, :1], vp.shape), **TOL)
    assert np.abs(vp).max() > 0
    assert float((p.actor.flat - before[0]).abs().max()) > 0 and float((p.critic.flat - before[1]).abs().max()) > 0
    with pytest.raises(ValueError, match="cent_agents"):
        MappoRunner(env, MappoPolicy(env.obs_dim, A, H, DEV, seed=0, cent_agents=2), T=T)


# ---------------------------------------------------------------- 7: adapters
class _Space:
    def __init__(self, shape=None, n=None):
        self.shape, self.n = shape, n


def test_r_mappo_policy_adapter_centralized(golden):
    """R_MAPPOPolicy(args with use_centralized_V, Space(47), Space(94)): get_values / get_actions /
    evaluate_actions with explicit cent_obs vs the reference's outputs."""
    from types import SimpleNamespace
    from minimarl.adapters import R_MAPPOPolicy
    fx = cv.case(golden("mappo_cv_fwd"), "n2")
    E, N = int(fx["E"]), int(fx["N"])
    args = SimpleNamespace(hidden_size=32, actor_lr=1e-4, critic_lr=1e-4, opti_eps=1e-5, weight_decay=0, seed=1,
                           use_centralized_V=True)
    pol = R_MAPPOPolicy(args, _Space((D,)), _Space((N * D,)), _Space(n=A), DEV)
    pol.actor.load_reference_state(fx, "actor.")
    pol.critic.load_reference_state(fx, "critic.")
    t = lambda k: torch.from_numpy(fx[k])  # noqa: E731
    cent = torch.from_numpy(cv.share_obs(fx["obs"].reshape(E, N, -1)).reshape(E * N, -1))
    v = pol.get_values(cent, t("hc"), t("masks"))
    np.testing.assert_allclose(v.cpu().numpy(), fx["values_only"], **TOL)
    v, a, lp, ha, hc = pol.get_actions(t("obs"), cent, t("ha"), t("hc"), t("masks"))
    assert a.shape == (E * N, 1) and hc.shape == (E * N, 1, H)
    np.testing.assert_allclose(v.cpu().numpy(), fx["values"], **TOL)
    np.testing.assert_allclose(ha.cpu().numpy(), fx["ha_out"], **TOL)
    np.testing.assert_allclose(hc.cpu().numpy(), fx["hc_out"], **TOL)
    PA = om.net_from_state(fx, "actor.", "actor")
    logits, _ = om.net_step(PA, t("obs"), t("ha")[:, 0], t("masks"))
    np.testing.assert_allclose(lp.cpu().numpy(), torch.log_softmax(logits, -1).gather(1, a.cpu()).numpy(), **TOL)
    vals, lps, ent = pol.evaluate_actions(t("seq_cent_obs"), t("seq_obs"), t("seq_ha"), t("seq_hc"),
                                          t("seq_actions"), t("seq_masks"), active_masks=t("seq_active"))
    np.testing.assert_allclose(vals.cpu().numpy(), fx["seq_values"], **TOL)
    np.testing.assert_allclose(lps.cpu().numpy(), fx["seq_logp"], **TOL)
    np.testing.assert_allclose(float(ent), float(fx["seq_entropy"]), rtol=1e-5)
    act, _ = pol.act(t("obs"), t("ha"), t("masks"), deterministic=True)
    np.testing.assert_array_equal(act.cpu().numpy()[:, 0], logits.argmax(-1).numpy())


# ---------------------------------------------------------------- 8: refusals (an error code, no launch)
def test_refusals(tmp_path):
    from minimarl._lib import MM_MAPPO_ROLLOUT, MappoDims, lib
    from minimarl.checkpoint import load_checkpoint, save_checkpoint
    from minimarl.mappo import MappoPolicy, MappoTrainer
    p = MappoPolicy(D, A, H, DEV, seed=1, cent_agents=2)
    R = 6
    S = 777.0
    z = lambda *s: torch.zeros(*s, device=DEV)
    outs = [torch.full((R, H), S, device=DEV), torch.full((R, H), S, device=DEV), torch.full((R,), S, device=DEV),
            torch.full((R,), S, device=DEV)]
    # cent_agents = 3: unsupported dims, through mm_last_error
    d_in = [z(R, D), z(R, H), z(R, H), torch.zeros(R, dtype=torch.int32, device=DEV)]   # (kept referenced)
    a = p.rollout_args(*d_in[:3], None, *outs, act_in=d_in[3])
    d3 = MappoDims(D, H, A, 3)
    assert lib().mm_mappo_fwd(ctypes.byref(d3), ctypes.byref(a), None) != 0
    assert "cent_agents=3" in lib().mm_last_error().decode()
    assert lib().mm_mappo_grad_scratch_count(ctypes.byref(d3), 5, 10, 6) < 0
    with pytest.raises(RuntimeError, match="unsupported dims"):
        MappoPolicy(D, A, H, DEV, cent_agents=3)
    # rows not a multiple of cent_agents with cent_obs NULL
    a.rows = 5
    assert a.mode == MM_MAPPO_ROLLOUT
    assert lib().mm_mappo_fwd(ctypes.byref(p.dims), ctypes.byref(a), None) != 0
    assert "multiple of cent_agents" in lib().mm_last_error().decode()
    torch.cuda.synchronize()
    assert all(bool((o == S).all()) for o in outs), "a refused call wrote its outputs"
    # the non-fused training path
    with pytest.raises(NotImplementedError, match="fused=False"):
        MappoTrainer(p, 10, 6, L=5, fused=False)
    # a decentralized checkpoint into a centralized trainer, and the reverse
    dec = MappoTrainer(MappoPolicy(D, A, H, DEV, seed=1), 10, 6, L=5)
    cen = MappoTrainer(p, 10, 6, L=5)
    path = str(tmp_path / "dec.safetensors")
    save_checkpoint(path, mappo=dec)
    with pytest.raises(ValueError, match=r"critic input width 48 .* critic input width 94"):
        load_checkpoint(path, mappo=cen)
    save_checkpoint(path, mappo=cen)
    with pytest.raises(ValueError, match=r"critic input width 96 .* critic input width 47"):
        load_checkpoint(path, mappo=dec)
