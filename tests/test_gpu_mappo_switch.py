"""GPU: MAPPO on Switch2 (obs_dim 3: row, column, clock; critic width 3, or 6 with a centralized critic over the 2
agents) -- the (3, 1) and (3, 2) instantiations of the MFMA rollout forward, the fused gradient passes (all chunks /
a chunk list, all rows / a row list) and the per-thread saves + wgrad path, MappoRunner / MappoEvaluator on
SwitchVecEnv -- against the reference's goldens at that width (tests/golden/mappo_sw_*.npz) and the f64 restatement
(tests/mappo_sw_cases.py: oracle.mappo with mappo_mb_ref / mappo_cv_ref / mappo_ff_ref, unchanged).

Tolerances are the project's, reused: forward values, log-probs and hiddens rtol 1e-5, atol 2e-6; returns rtol 1e-5,
atol 1e-5; gradients, post-Adam parameters, ValueNorm state and the train() log K_FP32 = 16 fp32 spreads (fp32 in
order / fp32 shuffled within each minibatch / f64; tests/mappo_mb_ref.py's docstring, the procedure of
tests/test_gpu_mappo.py's _fp32_spread) of the f64 run, plus a golden value's own distance to the f64 run where the
comparison is against the golden; mean ratio and pre-clip norms rtol 1e-5 (tests/test_gpu_mappo_ff.py)."""
import ctypes

import numpy as np
import pytest
import torch

import mappo_ff_ref as ff
import mappo_mb_ref as mb
import mappo_sw_cases as sw
from oracle import mappo as om
from oracle.switch import SwitchOracle, SwitchSpec

pytestmark = pytest.mark.gpu
DEV = "cuda"
D, A, H, N = sw.D, sw.A, sw.H, sw.N
TOL = dict(rtol=1e-5, atol=2e-6)
MODES = {"rec_d": (True, False), "rec_c": (True, True), "ff_d": (False, False), "ff_c": (False, True)}


def _policy(recurrent, cent, fx=None, prefix="", seed=None):
    from minimarl.mappo import MappoPolicy
    p = MappoPolicy(D, A, H, DEV, seed=seed, cent_agents=N if cent else None, recurrent=recurrent)
    if fx is not None:
        p.actor.load_reference_state(fx, prefix + "actor.")
        p.critic.load_reference_state(fx, prefix + "critic.")
    return p


def _oracle_nets(p):
    ks = sw.keys(p.recurrent)
    return ({k: p.actor.view(k).detach().cpu().clone() for k in ks},
            {k: p.critic.view(k).detach().cpu().clone() for k in ks})


def _trainer(fx, recurrent, cent, **kw):
    from minimarl.mappo import MappoBuffer, MappoTrainer
    E, T, L = (int(fx[k]) for k in ("E", "T", "L"))
    p = _policy(recurrent, cent, fx, "before.")
    buf = MappoBuffer(T, E, N, D, H, DEV, recurrent=recurrent)
    buf.load_reference({k[5:]: v for k, v in fx.items() if k.startswith("data.")})
    tr = MappoTrainer(p, T, E * N, L, ppo_epoch=int(fx["epochs"]), **kw)
    tr.load_value_normalizer(float(fx["vn0.running_mean"][0]), float(fx["vn0.running_mean_sq"][0]),
                             float(fx["vn0.debiasing_term"]))
    return p, buf, tr


def _nan_grads(tr):
    tr.grad[0].fill_(float("nan"))
    tr.grad[1].fill_(float("nan"))


def _vn_update(tr):
    from minimarl._lib import lib
    assert lib().mm_mappo_vn_update(tr.vn.data_ptr(), tr.stats.data_ptr(), 0.99999, None) == 0


def _three_calls(tr, call):
    """``call()`` three times on equal inputs, grad pre-filled with NaN each time: finite and bit-identical; tr.grad
    holds the last call's."""
    first = None
    for c in range(3):
        _nan_grads(tr)
        call()
        torch.cuda.synchronize()
        if first is None:
            first = [g.clone() for g in tr.grad]
        for n in (0, 1):
            assert bool(torch.isfinite(tr.grad[n]).all()) and float(tr.grad[n].abs().max()) > 0
            assert torch.equal(first[n], tr.grad[n]), f"net {n}: call {c} differs from call 0 on equal inputs"


class _Bars:
    """mb.assert_within over many figures: every figure is printed and checked, the misses are raised together."""

    def __init__(self):
        self.missed = []

    def __call__(self, got, want, spread, what, extra=0.0):
        try:
            mb.assert_within(got, want, spread, what, extra)
        except AssertionError as e:
            self.missed.append(str(e))

    def check(self):
        assert not self.missed, "\n".join(self.missed)


def _check_grads(p, tr, g64, spread, u, what, golden=None):
    for n, net in enumerate((p.actor, p.critic)):
        for k in sw.keys(p.recurrent):
            g = net.view(k, tr.grad[n]).cpu().numpy()
            mb.assert_within(g, g64[(u, n, k)], spread[(u, n, k)], f"{what} net {n} {k} vs f64")
            if golden is not None:
                ref = mb.golden_grad(golden, u, n, k)
                mb.assert_within(g, ref, spread[(u, n, k)], f"{what} net {n} {k} vs golden",
                                 float(np.abs(ref - g64[(u, n, k)]).max()))
        pad = torch.ones_like(tr.grad[n], dtype=torch.bool)
        for k in sw.keys(p.recurrent):
            net.view(k, pad).fill_(False)
        assert bool((tr.grad[n][pad] == 0).all()), "pads (and a feed-forward net's recurrent tensors): zero gradient"


# ---------------------------------------------------------------- 1: forward vs golden
@pytest.mark.parametrize("name", list(MODES))
def test_forward_matches_golden(name):
    """get_actions (the recorded actions evaluated; a sample from injected uniforms against the build's inverse-CDF
    sampler; deterministic = first argmax) and get_values against mappo_sw_fwd.npz, recurrent and feed-forward, critic
    width 3 and 6 (share_obs read from the env's adjacent rows and from an explicit cent_obs: bit-identical)."""
    recurrent, cent = MODES[name]
    fx = sw.fwd_case(name)
    p = _policy(recurrent, cent, fx)
    t = lambda k: torch.from_numpy(fx[k]).to(DEV)  # noqa: E731
    obs, ha, hc, masks = t("obs"), t("ha")[:, 0].contiguous(), t("hc")[:, 0].contiguous(), t("masks")
    v, a, lp, ha2, hc2 = p.get_actions(obs, ha, hc, masks, actions=t("actions"))
    np.testing.assert_allclose(v.cpu().numpy(), fx["values"], **TOL)
    np.testing.assert_allclose(lp.cpu().numpy(), fx["logp"], **TOL)
    np.testing.assert_allclose(ha2.cpu().numpy(), fx["ha_out"][:, 0], **TOL)
    np.testing.assert_allclose(hc2.cpu().numpy(), fx["hc_out"][:, 0], **TOL)
    gv = p.get_values(obs, hc, masks)
    np.testing.assert_allclose(gv.cpu().numpy(), fx["get_values"], **TOL)
    if cent:
        co = sw.share(fx["obs"], int(fx["E"])).to(DEV)
        v2, _, lp2, _, hc3 = p.get_actions(obs, ha, hc, masks, actions=t("actions"), cent_obs=co)
        assert torch.equal(v, v2) and torch.equal(lp, lp2) and torch.equal(p.get_values(co, hc, masks), gv)
        assert not recurrent or torch.equal(hc2, hc3)
    # the sampler and the mode against the restatement's logits
    PA, _ = sw.nets(fx, recurrent)
    logits = (om.net_step(PA, obs.cpu(), ha.cpu(), masks.cpu())[0] if recurrent else ff.net_out(PA, obs.cpu()))
    u = torch.rand(obs.shape[0], generator=torch.Generator().manual_seed(3))
    _, a_u, lp_u, _, _ = p.get_actions(obs, ha, hc, masks, u=u.to(DEV))
    want = om.sample_actions(logits, u)
    np.testing.assert_array_equal(a_u.cpu().numpy()[:, 0], want.numpy())
    np.testing.assert_allclose(lp_u.cpu().numpy(), om.categorical(logits)[0].gather(1, want.view(-1, 1)).numpy(), **TOL)
    R = obs.shape[0]
    outs = [torch.empty(R, device=DEV) for _ in range(2)] + [torch.empty(R, H, device=DEV) for _ in range(2)]
    act_d = torch.empty(R, dtype=torch.int32, device=DEV)
    m1 = masks.reshape(-1).contiguous()
    args = (p.rollout_args(obs, ha, hc, m1, outs[2], outs[3], outs[0], outs[1], act_out=act_d) if recurrent
            else p.rollout_args(obs, logp_out=outs[0], value_out=outs[1], act_out=act_d))
    args.deterministic = 1
    p._fwd(args)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(act_d.cpu().numpy(), logits.argmax(-1).numpy())


def test_saves_wgrad_path_and_evaluate_actions_match_reference():
    """The fused=False path at obs_dim 3 (MappoShape<3, 32, 5>: per-thread TRAIN forward with saves, mm_mappo_bwd,
    mm_mappo_wgrad; decentralized critic): its epoch-0 gradients against the f64 restatement and the golden, twice bit
    for bit; R_MAPPOPolicy.evaluate_actions (the TRAIN forward's saves) on the fixture's 16 chunks against
    om.evaluate_chunks; a centralized critic is refused by this path."""
    from types import SimpleNamespace
    from minimarl.adapters import R_MAPPOPolicy
    from minimarl.mappo import MappoTrainer
    fx, _, (g64, spread), _, _ = sw.oracle_case("rec_d", "m1")
    p, buf, tr = _trainer(fx, True, False, fused=False)
    tr.prepare(buf)
    _vn_update(tr)
    outs = []
    for _ in range(2):
        tr.grad[0].zero_()
        tr.grad[1].zero_()
        tr.gradients(buf)
        torch.cuda.synchronize()
        outs.append([g.clone() for g in tr.grad])
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    for n, net in enumerate((p.actor, p.critic)):
        for k in om.NET_KEYS:
            g = net.view(k, tr.grad[n]).cpu().numpy()
            mb.assert_within(g, g64[(0, n, k)], spread[(0, n, k)], f"saves + wgrad net {n} {k} vs f64")
            ref = mb.golden_grad(fx, 0, n, k)
            mb.assert_within(g, ref, spread[(0, n, k)], f"saves + wgrad net {n} {k} vs golden",
                             float(np.abs(ref - g64[(0, n, k)]).max()))
    with pytest.raises(NotImplementedError, match="fused=False does not support a centralized critic"):
        MappoTrainer(_policy(True, True, seed=1), 10, 8, fused=False)
    # evaluate_actions on one minibatch holding every chunk (rows (l, j))
    data = {k[5:]: v for k, v in fx.items() if k.startswith("data.")}
    b = om.chunk_batch(data, np.zeros_like(data["returns"][:-1]), 5)
    PA, PC = sw.nets(fx, True, "before.")
    lp, ent = om.evaluate_chunks(PA, b["obs"], b["ha0"], b["masks"], 5, "actor", b["actions"], b["active_masks"])
    v = om.evaluate_chunks(PC, b["obs"], b["hc0"], b["masks"], 5, "critic")
    pol = R_MAPPOPolicy(SimpleNamespace(hidden_size=32, seed=1), _Space((3,)), _Space((3,)), _Space(n=A), DEV)
    pol.actor.load_reference_state(fx, "before.actor.")
    pol.critic.load_reference_state(fx, "before.critic.")
    v_d, lp_d, ent_d = pol.evaluate_actions(b["obs"], b["obs"], b["ha0"][:, None], b["hc0"][:, None], b["actions"],
                                            b["masks"], None, b["active_masks"])
    np.testing.assert_allclose(v_d.cpu().numpy(), v.numpy(), **TOL)
    np.testing.assert_allclose(lp_d.cpu().numpy(), lp.numpy(), **TOL)
    np.testing.assert_allclose(float(ent_d), float(ent), rtol=1e-5)


# ---------------------------------------------------------------- 2: epoch-0 gradients and a short train()
@pytest.mark.parametrize("run", ["m1", "m2"])
@pytest.mark.parametrize("name", list(MODES))
def test_first_update_gradients_and_train_match_reference(name, run):
    """E 4, N 2, T 10, L 5, 3 epochs (16 chunks / 80 rows: one partial tile per pass). m1: one full-batch update per
    epoch; m2: num_mini_batch 2 through the recorded permutations (8 chunks / 40 rows per update). The first update's
    unclipped gradients (three calls, bit-identical) against the f64 restatement and, for m1, the golden's recorded
    gradients; then train(): post-Adam parameters, ValueNorm state and the train() log against both, mean ratio and the
    pre-clip norms at rtol 1e-5."""
    recurrent, cent = MODES[name]
    fx, (o64, spread), (g64, gspread), _, _ = sw.oracle_case(name, run)
    M, EP = int(fx["train_batch_size"]), int(fx["epochs"])
    p, buf, tr = _trainer(fx, recurrent, cent, num_mini_batch=M)
    tr.prepare(buf)
    if M == 1:
        _vn_update(tr)
        _three_calls(tr, lambda: tr.gradients(buf))
    else:
        chunks = tr.native_chunks(fx["perms"])[0, :tr.mbs]
        assert chunks.numel() == (8 if recurrent else 40)
        tr.mb_stats(buf, chunks)
        _vn_update(tr)
        _three_calls(tr, lambda: tr.gradients_mb(buf, chunks))
    _check_grads(p, tr, g64, gspread, 0, f"{name} {run} update 0", golden=fx if M == 1 else None)
    # ---- train() from the same start
    p, buf, tr = _trainer(fx, recurrent, cent, num_mini_batch=M)
    bars = _Bars()
    info = tr.train(buf, perms=fx["perms"] if M > 1 else None)
    torch.cuda.synchronize()
    for net, kind in ((p.actor, "actor"), (p.critic, "critic")):
        for k in sw.keys(recurrent):
            got = net.view(k).cpu().numpy()
            after = fx[f"after.{kind}.{om.ref_name(k, kind)}"]
            bars(got, o64[(kind, k)], spread[(kind, k)], f"{kind} {k} vs f64")
            bars(got, after, spread[(kind, k)], f"{kind} {k} vs golden",
                             float(np.abs(after - o64[(kind, k)]).max()))
    vn = tr.value_normalizer_state()
    for key, mine, gk in (("vn_mean", "running_mean", "vn1.running_mean"),
                          ("vn_mean_sq", "running_mean_sq", "vn1.running_mean_sq")):
        bars(vn[mine], o64[key], spread[key], key)
        bars(vn[mine], fx[gk], spread[key], key + " vs golden", float(np.abs(fx[gk] - o64[key]).max()))
    for key in ("value_loss", "policy_loss", "dist_entropy", "actor_grad_norm", "critic_grad_norm"):
        bars(info[key], o64[key], spread[key], key)
        bars(info[key], float(fx["info." + key]), spread[key], key + " vs golden",
                         abs(float(fx["info." + key]) - float(o64[key])))
    bars.check()
    np.testing.assert_allclose(info["ratio"], float(fx["info.ratio"]), rtol=1e-5)
    assert tr.norms.shape == (2, EP * M)
    np.testing.assert_allclose(tr.norms.cpu().numpy().T.reshape(-1), fx["norms"], rtol=1e-5)


# ---------------------------------------------------------------- 3: tile coverage
def _ref_layout(b, E):
    """A MappoBuffer [T(+1), E*N, ...] -> the reference SharedReplayBuffer layout [T(+1), E, N, ..., 1]."""
    c = lambda t: t.detach().cpu().numpy()  # noqa: E731
    T1 = b.obs.shape[0]
    d = {"obs": c(b.obs).reshape(T1, E, N, -1), "actions": c(b.actions).astype(np.float32).reshape(T1 - 1, E, N, 1)}
    if b.recurrent:
        d["rnn_states"] = c(b.rnn_states).reshape(T1, E, N, 1, -1)
        d["rnn_states_critic"] = c(b.rnn_states_critic).reshape(T1, E, N, 1, -1)
    for k in ("action_log_probs", "rewards"):
        d[k] = c(getattr(b, k)).reshape(T1 - 1, E, N, 1)
    for k in ("value_preds", "returns", "masks", "active_masks"):
        d[k] = c(getattr(b, k)).reshape(T1, E, N, 1)
    return d


def _device_rollout(recurrent, cent, E, T, max_steps):
    from minimarl.env import SwitchVecEnv
    from minimarl.mappo import MappoRunner
    env = SwitchVecEnv(E, N, max_steps=max_steps, device=DEV)
    p = _policy(recurrent, cent, seed=3)
    nets = _oracle_nets(p)
    r = MappoRunner(env, p, T=T, L=5, ppo_epoch=1, seed=11)
    r.warmup()
    r.rollout()
    r.compute()
    torch.cuda.synchronize()
    vn0 = [float(x) for x in r.trainer.vn.cpu().numpy()]
    return p, r, nets, vn0, _ref_layout(r.buf, E)


@pytest.mark.parametrize("E", [4100, 3], ids=["second_tile", "tiny"])
@pytest.mark.parametrize("name", list(MODES))
def test_gradient_tiles_repeatable_vs_oracle(name, E):
    """Every kept gradient kernel of the 3-wide shapes -- recurrent: pass G + pass M over all chunks and over a chunk
    list (the *_mb kernels); feed-forward: the one pass over all rows and over a row list -- on a device rollout on
    SwitchVecEnv (max_steps 3, or 2 at T 2: resets inside the buffer), one full-batch update, three calls on equal
    inputs compared bit for bit, then against the f64 restatement at the spread bar. A tile is 32 chunks (pass G) or 32 rows (pass M,
    the feed-forward pass); every pass launches NB = 128 blocks per net, of 4 waves (pass G, the feed-forward pass:
    512 waves) or 8 waves (pass M at these widths: 1024 waves), a wave taking the tiles wave, wave + waves, ...
      second_tile, recurrent (E 4100, N 2, T 10, L 5): 16400 chunks = 512 x 32 + 16 -> 513 tiles in pass G: wave 0
        takes two tiles, its second (the last) holds 16 chunks; 82000 rows = 2562 x 32 + 16 -> 2563 tiles in pass M:
        waves 0..514 take three tiles, the others two, the last tile holds 16 rows;
      second_tile, feed-forward (E 4100, N 2, T 2): 16400 rows -> 513 tiles on 512 waves, the last one half empty;
      tiny (E 3, N 2, T 5, L 5): 6 chunks -> pass G's only tile has 6 of 32 lanes valid; 30 rows -> one tile of 30."""
    recurrent, cent = MODES[name]
    T = 5 if E == 3 else (10 if recurrent else 2)
    p, r, (PA, PC), vn0, data = _device_rollout(recurrent, cent, E, T, 2 if T == 2 else 3)
    tr, buf = r.trainer, r.buf
    units = tr.n_chunks
    assert units == (T * E * N // 5 if recurrent else T * E * N)
    if E == 4100:
        assert units == 16400 and (units + 31) // 32 == 513 and tr.rows == (82000 if recurrent else 16400)
    else:
        assert units == (6 if recurrent else 30) and tr.rows == 30
    assert (data["masks"][1:T + 1] == 0).any() and (data["active_masks"] == 1).all()

    def f(dt, shuffle):
        if recurrent:
            rec = mb.ppo_train_mb(PA, PC, data, vn0, 1, 5, np.arange(units)[None], 1, dtype=dt, shuffle=shuffle,
                                  cent=cent)[0]
            return mb.update_grads(rec, (0,))
        rec = ff.ppo_train_ff(PA, PC, data, vn0, 1, None, 1, dtype=dt, shuffle=shuffle, cent=cent)[0]
        return ff.update_grads(rec, (0,))

    g64, spread = mb.fp32_spread(f)
    tr.prepare(buf)
    _vn_update(tr)
    ba = tr.bwd_args(buf)
    _three_calls(tr, lambda: tr.gradients(buf, ba=ba))
    _check_grads(p, tr, g64, spread, 0, f"{name} E {E} all")
    perm = torch.randperm(units, generator=torch.Generator().manual_seed(5)).to(torch.int32).to(DEV)
    _three_calls(tr, lambda: tr.gradients_mb(buf, perm, ba))
    _check_grads(p, tr, g64, spread, 0, f"{name} E {E} list")


# ---------------------------------------------------------------- 4: runner vs the oracle env
# scripted agents (actions through injected uniforms: the fresh policy's head has gain 0.01, every action's probability
# is 0.2 to within a percent, so u = 0.2 a + 0.1 draws action a). Agent 0: (0,1) down, five times right, up -> its
# target (0,6) at step 7. Agent 1: waits at (0,5) while agent 0 passes below it, then from step 6 down, five times
# left, up -> (0,0) at step 12: the shortest joint arrival (the corridor is one cell wide).
_A0 = [0, 3, 3, 3, 3, 3, 2]
_A1 = [4, 4, 4, 4, 4, 0, 1, 1, 1, 1, 1, 2]


@pytest.mark.parametrize("max_steps", [7, 14])
@pytest.mark.parametrize("name", ["rec_d", "rec_c", "ff_d"])
def test_runner_rollout_matches_oracle_env(name, max_steps):
    """MappoRunner on SwitchVecEnv, E 64, N 2, T 20, uniforms injected: envs 0..7 follow the script above, the others
    walk at random. max_steps 7 (two resets inside the rollout, all by timeout: an env cannot finish earlier, the
    joint arrival needs 12 steps; the scripted agent 0 collects its +5 on the timeout step) and max_steps 14 (the
    scripted envs finish early, by arrival at step 12, the others at 14). The stored actions replayed through
    oracle/switch.py step by step: obs[t + 1] (the auto-reset current obs), rewards, masks[t + 1] (zero for both
    agents of a finished env) exactly, active_masks all ones, hiddens zero where the env finished; the stored actions
    are the sampler's for the injected uniforms; compute()'s returns against om.compute_returns."""
    from minimarl.env import SwitchVecEnv
    from minimarl.mappo import MappoRunner
    from minimarl.qnet import ptr
    recurrent, cent = MODES[name]
    E, T = 64, 20
    env = SwitchVecEnv(E, N, max_steps=max_steps, device=DEV)
    p = _policy(recurrent, cent, seed=4)
    PA, PC = _oracle_nets(p)
    r = MappoRunner(env, p, T=T, L=5, ppo_epoch=1, seed=2)
    u = torch.rand(T, E, N, generator=torch.Generator().manual_seed(8))
    ep_len = 12 if max_steps == 14 else 7          # the scripted envs' episode length
    for t in range(T):
        k = t % ep_len
        u[t, :8, 0] = 0.2 * (_A0[k] if k < len(_A0) else 4) + 0.1
        u[t, :8, 1] = 0.2 * (_A1[k] if k < len(_A1) else 4) + 0.1
    u_dev = u.reshape(T, E * N).contiguous().to(DEV)
    for t in range(T):
        r.args[t].u = ptr(u_dev[t])
    r.warmup()
    r.rollout()
    r.compute()
    torch.cuda.synchronize()
    b = r.buf
    obs, acts = b.obs.cpu().numpy(), b.actions.cpu().numpy().astype(np.int64)
    masks, rew = b.masks.cpu().numpy(), b.rewards.cpu().numpy()
    ora = SwitchOracle(SwitchSpec(N, max_steps), E)
    np.testing.assert_array_equal(obs[0].reshape(E, N, D), ora.obs())
    early = 0
    for t in range(T):
        _, rw, _, dn = ora.step(acts[t].reshape(E, N))
        early += int((dn & (ora.steps < max_steps)).sum())
        ora.reset_envs(dn)
        np.testing.assert_array_equal(obs[t + 1].reshape(E, N, D), ora.obs(), err_msg=f"obs[{t + 1}]")
        np.testing.assert_array_equal(rew[t].reshape(E, N), rw, err_msg=f"rewards[{t}]")
        np.testing.assert_array_equal(masks[t + 1].reshape(E, N), np.repeat((~dn)[:, None], N, 1).astype(np.float32))
    assert np.all(b.active_masks.cpu().numpy() == 1.0) and np.all(masks[0] == 1)
    np.testing.assert_array_equal(acts[:ep_len, :2 * 8:2].T, np.tile((_A0 + [4] * 5)[:ep_len], (8, 1)))
    assert (rew[6].reshape(E, N)[:8, 0] == 5.0).all(), "the scripted agent 0 arrives at step 7"
    if max_steps == 14:
        assert early == 8 and (rew[11].reshape(E, N)[:8, 1] == 5.0).all() and (masks[12].reshape(E, N)[:8] == 0).all()
        assert (masks[12].reshape(E, N)[8:] == 1).all() and (masks[14].reshape(E, N)[8:] == 0).all()
    else:
        assert early == 0 and (masks[7] == 0).all() and (masks[14] == 0).all() and masks[1:].sum() == (T - 2) * E * N
    # the stored actions, log-probs and values of two steps against the restatement on the stored inputs
    for t in (0, 9):
        o_t, m_t = torch.from_numpy(obs[t]), torch.from_numpy(masks[t]).view(-1, 1)
        co = sw.share(obs[t], E) if cent else o_t
        if recurrent:
            ha, hc = b.rnn_states[t].cpu(), b.rnn_states_critic[t].cpu()
            logits, ha2 = om.net_step(PA, o_t, ha, m_t)
            v, hc2 = om.net_step(PC, co, hc, m_t)
            keep = torch.from_numpy(masks[t + 1]).view(-1, 1)
            np.testing.assert_allclose(b.rnn_states[t + 1].cpu().numpy(), (ha2 * keep).numpy(), **TOL)
            np.testing.assert_allclose(b.rnn_states_critic[t + 1].cpu().numpy(), (hc2 * keep).numpy(), **TOL)
        else:
            logits, v = ff.net_out(PA, o_t), ff.net_out(PC, co)
        want = om.sample_actions(logits, u[t].reshape(-1))
        np.testing.assert_array_equal(acts[t], want.numpy())
        np.testing.assert_allclose(b.action_log_probs[t].cpu().numpy(),
                                   om.categorical(logits)[0].gather(1, want.view(-1, 1)).numpy()[:, 0], **TOL)
        np.testing.assert_allclose(b.value_preds[t].cpu().numpy(), v.numpy()[:, 0], **TOL)
    if recurrent:
        for hs in (b.rnn_states, b.rnn_states_critic):
            hz = hs.abs().sum(-1).cpu().numpy() == 0
            assert np.all(hz[1:][masks[1:] == 0]) and not np.any(hz[1:][masks[1:] == 1])
    else:
        assert b.rnn_states is None and b.rnn_states_critic is None
    vn = r.trainer.vn
    ret_ref, _ = om.compute_returns(rew[..., None], b.value_preds.cpu().numpy()[..., None], masks[..., None],
                                    b.value_preds[T].cpu().numpy()[..., None],
                                    om.ValueNorm(*[float(x) for x in vn.cpu().numpy()]), 0.99, 0.95)
    np.testing.assert_allclose(b.returns[:T].cpu().numpy(), ret_ref[:T, :, 0], rtol=1e-5, atol=1e-5)
    before = torch.cat([p.actor.flat, p.critic.flat]).clone()
    info = r.train()
    torch.cuda.synchronize()
    after = torch.cat([p.actor.flat, p.critic.flat])
    assert all(np.isfinite(x) for x in info.values()) and bool(torch.isfinite(after).all())
    assert not torch.equal(before, after) and torch.equal(b.obs[0], b.obs[T])


# ---------------------------------------------------------------- 5: evaluator
@pytest.mark.parametrize("name", ["rec_d", "ff_c"])
def test_evaluator_scores_equal_host_replay(name):
    """MappoEvaluator(env="switch"), E 5 test envs, max_steps 10, both policy modes: the per-env scores equal a host
    replay through oracle/switch.py of the restatement's deterministic actions (first argmax; the policy head is
    scaled by 100 so the restatement's and the device's logits cannot rank two actions differently -- asserted on the
    logit gaps), the per-step rewards summed over the agents in f32 until the env-level done. Checkers stays the
    default env."""
    from minimarl.evaluate import MappoEvaluator
    recurrent, cent = MODES[name]
    E, steps = 5, 10
    p = _policy(recurrent, cent, seed=6)
    p.actor.view("Wo").mul_(100.0)
    PA, _ = _oracle_nets(p)
    ev = MappoEvaluator(E, N, steps, env="switch", device=DEV)
    assert ev.env.obs_dim == 3 and MappoEvaluator(2, N, steps, device=DEV).env.obs_dim == 47
    mean, score = ev.run(p)
    mean2, score2 = ev.run(p)
    ora = SwitchOracle(SwitchSpec(N, steps), E)
    obs = ora.obs()
    h = torch.zeros(E * N, H)
    want, active = np.zeros(E, np.float32), np.ones(E, bool)
    for _ in range(steps):
        o_t = torch.from_numpy(obs.reshape(E * N, D))
        if recurrent:
            logits, h = om.net_step(PA, o_t, h, torch.ones(E * N, 1))
        else:
            logits = ff.net_out(PA, o_t)
        top = torch.topk(logits, 2, -1).values
        assert float((top[:, 0] - top[:, 1]).min()) > 1e-4, "a near-tie would make the argmax comparison ambiguous"
        obs, rw, _, dn = ora.step(logits.argmax(-1).numpy().reshape(E, N))
        sr = np.zeros(E, np.float32)
        for j in range(N):
            sr = sr + rw[:, j]
        want = np.where(active, want + sr, want).astype(np.float32)
        active &= ~dn
    assert not active.any()
    np.testing.assert_array_equal(score.cpu().numpy(), want)
    assert torch.equal(score, score2) and mean == mean2 == float(score.mean())
    with pytest.raises(ValueError, match="obs_dim"):
        MappoEvaluator(2, N, steps, device=DEV).run(p)


# ---------------------------------------------------------------- 6: checkpoint, adapter
def _small_runner(recurrent=True, cent=False, seed=11):
    from minimarl.env import SwitchVecEnv
    from minimarl.mappo import MappoRunner
    env = SwitchVecEnv(6, N, max_steps=7, device=DEV)
    p = _policy(recurrent, cent, seed=3)
    r = MappoRunner(env, p, T=10, L=5, ppo_epoch=2, seed=seed)
    r.warmup()
    r.rollout()
    r.compute()
    return p, r


@pytest.mark.parametrize("cent", [False, True], ids=["critic3", "critic6"])
def test_checkpoint_round_trip_and_width_error(tmp_path, cent):
    """A Switch MappoTrainer after one train(): saved and loaded into a fresh one it continues bit-identically; a
    D = 47 checkpoint is refused with the trainer's critic-width error (48 = 47 padded to 4 against width 3 | 6)."""
    from minimarl.checkpoint import load_checkpoint, save_checkpoint
    from minimarl.mappo import MappoPolicy, MappoTrainer
    p, r = _small_runner(cent=cent)
    r.trainer.train(r.buf)
    path = str(tmp_path / "sw.safetensors")
    save_checkpoint(path, mappo=r.trainer)
    p2 = _policy(True, cent, seed=9)
    tr2 = MappoTrainer(p2, 10, 12, L=5, ppo_epoch=2)
    load_checkpoint(path, mappo=tr2)
    assert torch.equal(p2.actor.flat, p.actor.flat) and torch.equal(p2.critic.flat, p.critic.flat)
    assert torch.equal(tr2.vn, r.trainer.vn) and tr2.train_calls == 1
    r.trainer.train(r.buf)
    tr2.train(r.buf)
    torch.cuda.synchronize()
    assert torch.equal(p2.actor.flat, p.actor.flat) and torch.equal(p2.critic.flat, p.critic.flat)
    wide = MappoTrainer(MappoPolicy(47, A, H, DEV, seed=1), 10, 12, L=5)
    save_checkpoint(path, mappo=wide)
    before = p2.critic.flat.clone()
    with pytest.raises(ValueError, match=rf"critic input width 48 .* critic input width {6 if cent else 3}"):
        load_checkpoint(path, mappo=tr2)
    assert torch.equal(before, p2.critic.flat)


class _Space:
    def __init__(self, shape=None, n=None):
        self.shape, self.n = shape, n


@pytest.mark.parametrize("name", ["rec_d", "rec_c", "ff_c"])
def test_r_mappo_policy_adapter(name):
    """R_MAPPOPolicy with obs_space (3,) and cent_obs_space (3,) | (6,): the forward golden through the reference's
    signatures."""
    from types import SimpleNamespace
    from minimarl.adapters import R_MAPPOPolicy
    recurrent, cent = MODES[name]
    fx = sw.fwd_case(name)
    args = SimpleNamespace(hidden_size=32, seed=1, use_centralized_V=cent,
                           algorithm_name="rmappo" if recurrent else "mappo")
    pol = R_MAPPOPolicy(args, _Space((3,)), _Space((6,) if cent else (3,)), _Space(n=A), DEV)
    assert pol.cent_agents == (2 if cent else None) and pol.recurrent is recurrent
    pol.actor.load_reference_state(fx, "actor.")
    pol.critic.load_reference_state(fx, "critic.")
    t = lambda k: torch.from_numpy(fx[k])  # noqa: E731
    co = sw.share(fx["obs"], int(fx["E"])) if cent else t("obs")
    np.testing.assert_allclose(pol.get_values(co, t("hc"), t("masks")).cpu().numpy(), fx["get_values"], **TOL)
    v, a, lp, ha2, hc2 = pol.get_actions(t("obs"), co, t("ha"), t("hc"), t("masks"))
    np.testing.assert_allclose(v.cpu().numpy(), fx["values"], **TOL)
    assert a.shape == (12, 1) and int(a.min()) >= 0 and int(a.max()) < A
    if recurrent:
        np.testing.assert_allclose(ha2.cpu().numpy(), fx["ha_out"], **TOL)
        np.testing.assert_allclose(hc2.cpu().numpy(), fx["hc_out"], **TOL)


# ---------------------------------------------------------------- 7: refusals
def test_refusals_name_the_cause_and_launch_nothing():
    from minimarl._lib import MappoDims, lib
    from minimarl.env import SwitchVecEnv, VecEnv
    from minimarl.mappo import MappoPolicy, MappoRunner
    p = _policy(True, False, seed=1)
    with pytest.raises(ValueError, match="full_observable=True"):
        MappoRunner(SwitchVecEnv(4, N, max_steps=5, full_observable=True, device=DEV), p, T=5)
    with pytest.raises(ValueError, match="clock=False"):
        MappoRunner(SwitchVecEnv(4, N, max_steps=5, clock=False, device=DEV), p, T=5)
    with pytest.raises(ValueError, match="cent_agents=2 != the env's 3 agents"):
        MappoRunner(SwitchVecEnv(4, 3, max_steps=5, device=DEV), _policy(True, True, seed=1), T=5)
    with pytest.raises(ValueError, match="obs_dim 3 != the env's obs_dim 47"):
        MappoRunner(VecEnv(4, N, max_steps=5, device=DEV), p, T=5)
    # a decentralized critic runs with any Switch agent count
    r3 = MappoRunner(SwitchVecEnv(4, 3, max_steps=5, device=DEV), p, T=5, ppo_epoch=1)
    r3.warmup()
    assert all(np.isfinite(x) for x in r3.run_episode().values())
    # (3, n) shapes that are not built: refused by name, by the policy and by every C entry point, nothing written
    for n in (3, 4):
        with pytest.raises(RuntimeError, match=rf"cent_agents={n} .*the 3-wide shapes built are"):
            MappoPolicy(D, A, H, DEV, cent_agents=n)
    L_ = lib()
    R, S = 12, 777.0
    outs = [torch.full((R,), S, device=DEV), torch.full((R,), S, device=DEV)]
    obs = torch.rand(R, D, device=DEV)
    act = torch.zeros(R, dtype=torch.int32, device=DEV)
    hid = torch.zeros(R, H, device=DEV)
    a = p.rollout_args(obs, hid, hid, None, None, None, outs[0], outs[1], act_in=act)
    for bad in (MappoDims(D, H, A, 4), MappoDims(D, H, A, 3), MappoDims(6, H, A, 0), MappoDims(D, 64, A, 0)):
        assert L_.mm_mappo_fwd(ctypes.byref(bad), ctypes.byref(a), None) != 0
        assert "unsupported dims" in L_.mm_last_error().decode()
        assert L_.mm_mappo_ff_fwd(ctypes.byref(bad), ctypes.byref(a), None) != 0
        assert L_.mm_mappo_grad_scratch_count(ctypes.byref(bad), 5, 10, 12) < 0
        assert L_.mm_mappo_ff_grad_scratch_count(ctypes.byref(bad)) < 0
    assert L_.mm_mappo_fwd(ctypes.byref(MappoDims(D, H, A, 4)), ctypes.byref(a), None) != 0
    assert "critic input width 12" in L_.mm_last_error().decode()
    torch.cuda.synchronize()
    assert all(bool((o == S).all()) for o in outs), "a refused call wrote"
