"""GPU: feed-forward MAPPO (the reference's algorithm_name "mappo": MappoPolicy(recurrent=False) -> mm_mappo_ff_fwd,
mm_mappo_ff_grad, mm_mappo_ff_insert) against the reference's goldens with the two recurrent flags off
(tests/golden/mappo_ff_fwd.npz, mappo_ff_train.npz) and the restatement tests/mappo_ff_ref.py.

Tolerances are the project's: forward values and log-probs rtol 1e-5, atol 2e-6 (tests/test_gpu_mappo.py's TOL);
gradients, post-Adam parameters, ValueNorm state and losses K_FP32 = 16 fp32 spreads (fp32 in order / fp32 shuffled
within each minibatch / f64) of the f64 run, plus a golden value's own distance to the f64 run where the comparison
is against the golden (tests/mappo_mb_ref.py's docstring); mean ratio and pre-clip norms rtol 1e-5."""
import ctypes
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mappo_cv_ref as cv
import mappo_ff_ref as ff
import mappo_mb_ref as mb
from oracle import mappo as om

pytestmark = pytest.mark.gpu
DEV = "cuda"
D, A, H = 47, 5, 32
TOL = dict(rtol=1e-5, atol=2e-6)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _policy(fx=None, N=None, prefix="before.", seed=None):
    from minimarl.mappo import MappoPolicy
    p = MappoPolicy(D, A, H, DEV, seed=seed, cent_agents=N, recurrent=False)
    if fx is not None:
        p.actor.load_reference_state(fx, prefix + "actor.")
        p.critic.load_reference_state(fx, prefix + "critic.")
    return p


def _oracle_nets(p):
    return ({k: p.actor.view(k).detach().cpu().clone() for k in ff.FF_KEYS},
            {k: p.critic.view(k).detach().cpu().clone() for k in ff.FF_KEYS})


def _trainer(fx, cent=False, **kw):
    from minimarl.mappo import MappoBuffer, MappoTrainer
    E, N, T = (int(fx[k]) for k in ("E", "N", "T"))
    p = _policy(fx, N if cent else None)
    _, _, data, vn0, _ = ff.train_inputs(fx)
    buf = MappoBuffer(T, E, N, D, H, DEV, recurrent=False)
    buf.load_reference(data)
    tr = MappoTrainer(p, T, E * N, ppo_epoch=int(fx["epochs"]), **kw)
    tr.load_value_normalizer(*vn0)
    return p, buf, tr


@functools.lru_cache(maxsize=None)
def _golden_case():
    """The golden train fixture and the restatement's three runs on it (computed once, read-only): train outputs and
    the unclipped gradients of updates 0, 1 and 2, each as (f64 values, fp32 spreads)."""
    fx = dict(np.load(os.path.join(GOLDEN, "mappo_ff_train.npz")))
    PA, PC, data, vn0, _ = ff.train_inputs(fx)
    EP, M = int(fx["epochs"]), int(fx["train_batch_size"])
    runs = {}

    def run(dt, shuffle):
        if (dt, shuffle) not in runs:
            runs[(dt, shuffle)] = ff.ppo_train_ff(PA, PC, data, vn0, EP, fx["perms"], M, dtype=dt, shuffle=shuffle)
        return runs[(dt, shuffle)]

    train = mb.fp32_spread(lambda dt, sh: ff.train_outputs(*run(dt, sh)))
    grads = mb.fp32_spread(lambda dt, sh: ff.update_grads(run(dt, sh)[0], (0, 1, 2)))
    return fx, train, grads, M


def _nan_grads(tr):
    tr.grad[0].fill_(float("nan"))
    tr.grad[1].fill_(float("nan"))


def _vn_update(tr):
    from minimarl._lib import lib
    assert lib().mm_mappo_vn_update(tr.vn.data_ptr(), tr.stats.data_ptr(), 0.99999, None) == 0


def _recurrent_slots(net):
    from minimarl.mappo import RECURRENT_KEYS
    m = torch.zeros_like(net.flat, dtype=torch.bool)
    for k in RECURRENT_KEYS:
        net.view(k, m).fill_(True)
    return m


def _gen_obs(R, seed, width=D):
    g = torch.Generator().manual_seed(seed)
    obs = (torch.rand(R, width, generator=g) < 0.3).float()
    obs[:, :2] = torch.rand(R, 2, generator=g)
    return obs, g


# ---------------------------------------------------------------- 1: forward
def test_forward_matches_reference_and_sampler(golden):
    """get_actions / get_values against mappo_ff_fwd.npz with the recorded actions; the hiddens come back as given
    (None included); the sampler against om.sample_actions with injected u; deterministic = first argmax; equal
    (seed, counter) draw equal actions."""
    fx = golden("mappo_ff_fwd")
    p = _policy(fx, prefix="")
    assert sorted(p.actor.state_dict()) == sorted(om.ref_name(k, "actor") for k in ff.FF_KEYS)
    t = lambda k: torch.from_numpy(fx[k]).to(DEV)  # noqa: E731
    obs, ha, hc = t("obs"), t("ha")[:, 0], t("hc")[:, 0]
    v, a, lp, ha2, hc2 = p.get_actions(obs, ha, hc, t("masks"), actions=t("actions"))
    assert ha2 is ha and hc2 is hc
    np.testing.assert_allclose(v.cpu().numpy(), fx["values"], **TOL)
    np.testing.assert_allclose(lp.cpu().numpy(), fx["logp"], **TOL)
    np.testing.assert_allclose(p.get_values(obs, hc, t("masks")).cpu().numpy(), fx["get_values"], **TOL)
    np.testing.assert_allclose(p.get_values(obs).cpu().numpy(), fx["get_values"], **TOL)
    v0, _, lp0, n0, n1 = p.get_actions(obs, actions=t("actions"))
    assert n0 is None and n1 is None and torch.equal(v0, v) and torch.equal(lp0, lp)
    # the sampler
    PA, PC = _oracle_nets(p)
    logits = ff.net_out(PA, obs.cpu())
    u = torch.rand(obs.shape[0], generator=torch.Generator().manual_seed(3))
    _, a_u, lp_u, _, _ = p.get_actions(obs, u=u.to(DEV))
    want = om.sample_actions(logits, u)
    np.testing.assert_array_equal(a_u.cpu().numpy()[:, 0], want.numpy())
    np.testing.assert_allclose(lp_u.cpu().numpy(), om.categorical(logits)[0].gather(1, want.view(-1, 1)).numpy(), **TOL)
    # the mode
    R = obs.shape[0]
    lp_d, v_d = torch.empty(R, device=DEV), torch.empty(R, device=DEV)
    act_d = torch.empty(R, dtype=torch.int32, device=DEV)
    args = p.rollout_args(obs, logp_out=lp_d, value_out=v_d, act_out=act_d)
    args.deterministic = 1
    p._fwd(args)
    np.testing.assert_array_equal(act_d.cpu().numpy(), logits.argmax(-1).numpy())
    # the counter RNG
    _, a1, _, _, _ = p.get_actions(obs, seed=5, counter=9)
    _, a2, _, _, _ = p.get_actions(obs, seed=5, counter=9)
    assert torch.equal(a1, a2) and int(a1.min()) >= 0 and int(a1.max()) < A


@pytest.mark.parametrize("rows", [1, 31, 33, 131105])
def test_rollout_tile_edges(rows):
    """Values and log-probs of given actions against the restatement, and a VALUES-mode launch; rows beyond ``rows``
    of every output stay untouched (sentinel-filled, 32 rows longer). mm_mappo_ff_fwd launches
    min(ceil(tiles / 4), 1024) blocks of 4 waves, one 32-row tile per wave up to 1024 x 4 x 32 = 131072 rows; 131105
    rows are 4098 tiles: waves 0 and 1 of block 0 take a second tile, the last one holding a single row."""
    from minimarl._lib import MM_MAPPO_VALUES
    p = _policy(seed=5)
    PA, PC = _oracle_nets(p)
    obs, g = _gen_obs(rows, 2)
    act = torch.randint(0, A, (rows, 1), generator=g)
    v, _, lp = ff.get_actions(PA, PC, obs, actions=act)
    S = 777.0
    o_lp, o_v, o_v2 = (torch.full((rows + 32,), S, device=DEV) for _ in range(3))
    d_in = [obs.to(DEV), act.reshape(-1).to(torch.int32).to(DEV)]   # (kept referenced: the arguments hold pointers)
    a = p.rollout_args(d_in[0], logp_out=o_lp, value_out=o_v, act_in=d_in[1])
    p._fwd(a)
    a.net[1].out, a.mode = o_v2.data_ptr(), MM_MAPPO_VALUES
    p._fwd(a)
    torch.cuda.synchronize()
    for got, want in ((o_v, v[:, 0]), (o_v2, v[:, 0]), (o_lp, lp[:, 0])):
        np.testing.assert_allclose(got[:rows].cpu().numpy(), want.numpy(), **TOL)
        assert bool((got[rows:] == S).all()), "rows beyond `rows` were written"


@pytest.mark.parametrize("N", [2, 8])
def test_forward_centralized_critic(N):
    """E 9: the critic on share_obs (Dc 94 | 376), read from the env's adjacent obs rows and from an explicit
    cent_obs: equal to each other bit for bit and to the restatement. N 8: 72 rows = 2 tiles + 8."""
    E = 9
    R = E * N
    p = _policy(N=N, seed=7)
    PA, PC = _oracle_nets(p)
    obs, g = _gen_obs(R, 4)
    act = torch.randint(0, A, (R, 1), generator=g)
    cent = torch.from_numpy(cv.share_obs(obs.numpy().reshape(E, N, D)).reshape(R, N * D))
    v, _, lp = ff.get_actions(PA, PC, obs, cent_obs=cent, actions=act)
    v1, _, lp1, _, _ = p.get_actions(obs.to(DEV), actions=act.to(DEV))
    v2, _, lp2, _, _ = p.get_actions(obs.to(DEV), actions=act.to(DEV), cent_obs=cent.to(DEV))
    assert torch.equal(v1, v2) and torch.equal(lp1, lp2)
    assert torch.equal(p.get_values(obs.to(DEV)), v1) and torch.equal(p.get_values(cent.to(DEV)), v1)
    np.testing.assert_allclose(v1.cpu().numpy(), v.numpy(), **TOL)
    np.testing.assert_allclose(lp1.cpu().numpy(), lp.numpy(), **TOL)


# ---------------------------------------------------------------- 2: the golden train()
def test_ppo_train_three_row_minibatches_matches_reference():
    """train(perms = the recorded randperms): 3 epochs x 3 minibatches of 26 of the 80 rows (less than a tile), 2
    rows dropped per epoch, a ValueNorm update and an active count per minibatch: post-Adam parameters, ValueNorm
    state and train_info against the f64 restatement and the golden; mean ratio and the 18 pre-clip norms (in update
    order) at rtol 1e-5; the six recurrent tensors stay exactly zero."""
    fx, (o64, spread), _, M = _golden_case()
    p, buf, tr = _trainer(fx, num_mini_batch=M)
    assert (tr.n_chunks, tr.mbs, tr.L) == (80, 26, 1) and buf.rnn_states is None and buf.rnn_states_critic is None
    info = tr.train(buf, perms=fx["perms"])
    torch.cuda.synchronize()
    assert tr.norms.shape == (2, int(fx["epochs"]) * M)
    for net, kind in ((p.actor, "actor"), (p.critic, "critic")):
        for k in ff.FF_KEYS:
            got = net.view(k).cpu().numpy()
            after = fx[f"after.{kind}.{om.ref_name(k, kind)}"]
            mb.assert_within(got, o64[(kind, k)], spread[(kind, k)], f"{kind} {k} vs f64")
            mb.assert_within(got, after, spread[(kind, k)], f"{kind} {k} vs golden",
                             float(np.abs(after - o64[(kind, k)]).max()))
        assert bool((net.flat[_recurrent_slots(net)] == 0).all()), "the recurrent tensors must stay zero"
    vn = tr.value_normalizer_state()
    for key, mine, gk in (("vn_mean", "running_mean", "vn1.running_mean"),
                          ("vn_mean_sq", "running_mean_sq", "vn1.running_mean_sq")):
        mb.assert_within(vn[mine], o64[key], spread[key], key)
        mb.assert_within(vn[mine], fx[gk], spread[key], key + " vs golden", float(np.abs(fx[gk] - o64[key]).max()))
    for key in ("value_loss", "policy_loss", "dist_entropy", "actor_grad_norm", "critic_grad_norm"):
        mb.assert_within(info[key], o64[key], spread[key], key)
        mb.assert_within(info[key], float(fx["info." + key]), spread[key], key + " vs golden",
                         abs(float(fx["info." + key]) - float(o64[key])))
    np.testing.assert_allclose(info["ratio"], float(fx["info.ratio"]), rtol=1e-5)
    np.testing.assert_allclose(tr.norms.cpu().numpy().T.reshape(-1), fx["norms"], rtol=1e-5)


# ---------------------------------------------------------------- 3: gradients of updates 0, 1 and 2
def test_first_three_update_gradients_match_reference():
    """Unclipped gradients of updates 0, 1 and 2 (each after the previous one's Adam step), grad pre-filled with NaN:
    every entry against the f64 restatement and the golden's recorded gradients, pads zero, the six recurrent
    tensors' gradients exactly zero, everything finite. Update 2 holds the one inactive row (55): its active count is
    25 of its 26 rows."""
    fx, _, (g64, spread), M = _golden_case()
    p, buf, tr = _trainer(fx, num_mini_batch=M)
    native = tr.native_chunks(fx["perms"])
    np.testing.assert_array_equal(native.cpu().numpy(), fx["perms"])
    tr.prepare(buf)
    ba = tr.bwd_args(buf)
    for u in (0, 1, 2):
        rows = native[0, u * tr.mbs:(u + 1) * tr.mbs]
        assert rows.numel() == 26
        tr.mb_stats(buf, rows)
        _vn_update(tr)
        _nan_grads(tr)
        tr.gradients_mb(buf, rows, ba)
        torch.cuda.synchronize()
        assert float(tr.stats[2]) == (25.0 if u == 2 else 26.0)
        for n, net in enumerate((p.actor, p.critic)):
            for k in ff.FF_KEYS:
                g = net.view(k, tr.grad[n]).cpu().numpy()
                mb.assert_within(g, g64[(u, n, k)], spread[(u, n, k)], f"update {u} net {n} {k} vs f64")
                ref = mb.golden_grad(fx, u, n, k)
                mb.assert_within(g, ref, spread[(u, n, k)], f"update {u} net {n} {k} vs golden",
                                 float(np.abs(ref - g64[(u, n, k)]).max()))
            pad = torch.ones_like(tr.grad[n], dtype=torch.bool)
            for k in ff.FF_KEYS:
                net.view(k, pad).fill_(False)
            rec = _recurrent_slots(net)
            assert int(rec.sum()) == 6 * H * H + 6 * H + 2 * H and bool((tr.grad[n][rec] == 0).all())
            pad &= ~rec
            assert int(pad.sum()) > 0 and bool((tr.grad[n][pad] == 0).all()), "pads must carry zero gradient"
            assert bool(torch.isfinite(tr.grad[n]).all())
        tr.clip_adam(u)


# ---------------------------------------------------------------- 4: bit-identity
@pytest.mark.parametrize("cent", [False, True], ids=["golden", "centralized_n2"])
def test_row_list_of_all_rows_is_bit_identical_to_all_rows(golden, cent):
    """mm_mappo_ff_grad with rows = arange(T * EN) gives the rows = NULL gradients bit for bit, and two identical
    calls are bit-identical, decentralized and centralized critic (N 2, cent_agents 2)."""
    fx = cv.case(golden("mappo_cv_train"), "n2") if cent else golden("mappo_ff_train")
    p, buf, tr = _trainer(fx, cent=cent)
    tr.prepare(buf)
    _vn_update(tr)
    outs = []
    for rows in (None, None, torch.arange(tr.rows, dtype=torch.int32, device=DEV)):
        _nan_grads(tr)
        if rows is None:
            tr.gradients(buf)
        else:
            tr.gradients_mb(buf, rows)
        torch.cuda.synchronize()
        outs.append([g.clone() for g in tr.grad])
    for n in (0, 1):
        assert bool(torch.isfinite(outs[0][n]).all()) and float(outs[0][n].abs().max()) > 0
        assert torch.equal(outs[0][n], outs[1][n]), f"net {n}: two equal calls differ"
        assert torch.equal(outs[0][n], outs[2][n]), f"net {n}: row list vs all rows"


# ---------------------------------------------------------------- 5: a second tile per wave, Dc 376
def _ref_layout(b, E, N):
    """A feed-forward MappoBuffer [T(+1), E*N, ...] -> the reference SharedReplayBuffer layout [T(+1), E, N, ..., 1]."""
    c = lambda t: t.detach().cpu().numpy()  # noqa: E731
    T1 = b.obs.shape[0]
    d = {"obs": c(b.obs).reshape(T1, E, N, -1), "actions": c(b.actions).astype(np.float32).reshape(T1 - 1, E, N, 1)}
    for k in ("action_log_probs", "rewards"):
        d[k] = c(getattr(b, k)).reshape(T1 - 1, E, N, 1)
    for k in ("value_preds", "returns", "masks", "active_masks"):
        d[k] = c(getattr(b, k)).reshape(T1, E, N, 1)
    return d


def _device_rollout(E, N, cent, T, M):
    from minimarl.env import VecEnv
    from minimarl.mappo import MappoPolicy, MappoRunner
    env = VecEnv(E, N, max_steps=3, device=DEV)
    p = MappoPolicy(env.obs_dim, A, H, DEV, seed=3, cent_agents=N if cent else None, recurrent=False)
    nets = _oracle_nets(p)
    r = MappoRunner(env, p, T=T, ppo_epoch=1, seed=11, num_mini_batch=M)
    r.warmup()
    r.rollout()
    r.compute()
    torch.cuda.synchronize()
    vn0 = [float(x) for x in r.trainer.vn.cpu().numpy()]
    return p, r, nets, vn0, _ref_layout(r.buf, E, N)


@pytest.mark.parametrize("E,N,cent", [(2100, 8, False), (8200, 2, True)], ids=["n8", "centralized_n2"])
def test_second_tile_per_wave_one_epoch_vs_oracle(E, N, cent):
    """T 4, M 2 on a device rollout with max_steps 3. The gradient pass launches 128 blocks per net of 4 waves (512
    waves; fewer than pass M's at most 1024 the sizes were chosen for), one 32-row tile per wave and turn. N 8,
    E 2100: 33600 rows per minibatch = 1050 tiles, a third tile for 26 waves; N 2 centralized, E 8200: 32800 rows =
    1025 tiles. One epoch's two updates (the second after the first's clip + Adam step) against the restatement fed
    the device's buffer and the device's permutation, each update's gradients computed three times on equal inputs
    and compared bit for bit."""
    T, M = 4, 2
    p, r, (PA, PC), vn0, data = _device_rollout(E, N, cent, T, M)
    tr, buf = r.trainer, r.buf
    assert tr.mbs > 32 * 1024 and (data["masks"][1:T] == 0).any()
    perms = tr.draw_perms().cpu().numpy()
    native = tr._to_native(torch.as_tensor(perms, device=DEV))

    def f(dt, shuffle):
        rec = ff.ppo_train_ff(PA, PC, data, vn0, 1, perms, M, dtype=dt, shuffle=shuffle, cent=cent)[0]
        return ff.update_grads(rec, (0, 1))

    o64, spread = mb.fp32_spread(f)
    tr.prepare(buf)
    ba = tr.bwd_args(buf)
    for u in (0, 1):
        _list_gradients(tr, buf, native[0, u * tr.mbs:(u + 1) * tr.mbs], ba)
        _check_update(p, tr, o64, spread, u, "second tile")
        tr.clip_adam(u)


def test_centralized_critic_dc376_one_epoch_vs_oracle():
    """N 8 centralized (critic input 376 wide, 3 waves per block), E 5, T 4: 160 rows = 5 tiles, one full-batch epoch
    (rows in buffer order) against the restatement."""
    E, N, T = 5, 8, 4
    p, r, (PA, PC), vn0, data = _device_rollout(E, N, True, T, 1)
    tr, buf = r.trainer, r.buf

    def f(dt, shuffle):
        perms = np.arange(T * E * N)[None]
        rec = ff.ppo_train_ff(PA, PC, data, vn0, 1, perms, 1, dtype=dt, shuffle=shuffle, cent=True)[0]
        return ff.update_grads(rec, (0,))

    o64, spread = mb.fp32_spread(f)
    tr.prepare(buf)
    _vn_update(tr)
    _nan_grads(tr)
    tr.gradients(buf)
    torch.cuda.synchronize()
    for n, net in enumerate((p.actor, p.critic)):
        for k in ff.FF_KEYS:
            mb.assert_within(net.view(k, tr.grad[n]).cpu().numpy(), o64[(0, n, k)], spread[(0, n, k)], f"net {n} {k}")
        assert bool(torch.isfinite(tr.grad[n]).all()) and bool((tr.grad[n][_recurrent_slots(net)] == 0).all())


def _check_update(p, tr, o64, spread, u, what):
    for n, net in enumerate((p.actor, p.critic)):
        for k in ff.FF_KEYS:
            mb.assert_within(net.view(k, tr.grad[n]).cpu().numpy(), o64[(u, n, k)], spread[(u, n, k)],
                             f"{what} update {u} net {n} {k}")


def _list_gradients(tr, buf, rows, ba, calls=3):
    """mb_stats + ValueNorm update once, then ``calls`` gradient calls on the same list: they must agree bit for bit
    (grad pre-filled with NaN each time); tr.grad holds the last call's."""
    tr.mb_stats(buf, rows)
    _vn_update(tr)
    first = None
    for c in range(calls):
        _nan_grads(tr)
        tr.gradients_mb(buf, rows, ba)
        torch.cuda.synchronize()
        if first is None:
            first = [g.clone() for g in tr.grad]
        for n in (0, 1):
            assert bool(torch.isfinite(tr.grad[n]).all())
            assert torch.equal(first[n], tr.grad[n]), f"net {n}: call {c} differs from call 0 on equal inputs"


def test_centralized_n8_all_rows_second_tile_per_wave_and_row_list_refused():
    """cent_agents 8 (critic input 376 wide: 128 blocks of 3 waves per net = 384 waves). E 800, N 8, T 4 on a device
    rollout with max_steps 3: 25600 rows = 800 tiles, so every wave takes a second tile and 32 a third, carrying
    their accumulators (and what the compiler keeps in scratch) across tiles. One full-batch epoch (rows = NULL)
    against the restatement, computed three times on equal inputs and compared bit for bit. A row list is refused
    for this shape, by the C entry point (an error, gradients untouched) and by the trainer."""
    from minimarl._lib import lib
    from minimarl.mappo import MappoTrainer
    E, N, T = 800, 8, 4
    p, r, (PA, PC), vn0, data = _device_rollout(E, N, True, T, 1)
    tr, buf = r.trainer, r.buf
    assert tr.rows == 25600 and tr.rows > 2 * 32 * 3 * 128 and (data["masks"][1:T] == 0).any()

    def f(dt, shuffle):
        rec = ff.ppo_train_ff(PA, PC, data, vn0, 1, None, 1, dtype=dt, shuffle=shuffle, cent=True)[0]
        return ff.update_grads(rec, (0,))

    o64, spread = mb.fp32_spread(f)
    tr.prepare(buf)
    _vn_update(tr)
    ba = tr.bwd_args(buf)
    first = None
    for c in range(3):
        _nan_grads(tr)
        tr.gradients(buf, ba=ba)
        torch.cuda.synchronize()
        first = first or [g.clone() for g in tr.grad]
        for n in (0, 1):
            assert torch.equal(first[n], tr.grad[n]), f"net {n}: call {c} differs from call 0 on equal inputs"
    _check_update(p, tr, o64, spread, 0, "n8 centralized, all rows")
    for n, net in enumerate((p.actor, p.critic)):
        assert bool(torch.isfinite(tr.grad[n]).all()) and bool((tr.grad[n][_recurrent_slots(net)] == 0).all())
    # the row list
    _nan_grads(tr)
    rows = torch.arange(tr.rows, dtype=torch.int32, device=DEV)
    assert lib().mm_mappo_ff_grad(ctypes.byref(p.dims), ctypes.byref(ba), rows.data_ptr(), tr.rows,
                                  tr.grad[0].data_ptr(), tr.grad[1].data_ptr(), tr.gscr.data_ptr(), None) != 0
    assert "row list is not supported with cent_agents=8" in lib().mm_last_error().decode()
    torch.cuda.synchronize()
    assert bool(torch.isnan(tr.grad[0]).all()) and bool(torch.isnan(tr.grad[1]).all()), "a refused call wrote"
    with pytest.raises(NotImplementedError, match="cent_agents=8"):
        MappoTrainer(p, T, E * N, num_mini_batch=2)


@pytest.mark.parametrize("lo,hi", [(0, 32), (256, 512), (8192, 16384), (0, 33600)],
                         ids=["one_tile", "one_block", "256_tiles", "whole_minibatch"])
def test_sub_lists_repeatable_vs_oracle(lo, hi):
    """N 8, E 2100, T 4 on a device rollout: slices of one drawn permutation as minibatches of their own (one tile;
    8 tiles, a single block's waves; 256 tiles; 1050 tiles), each against the restatement run on exactly those rows,
    the gradients computed three times on equal inputs and compared bit for bit."""
    E, N, T = 2100, 8, 4
    p, r, (PA, PC), vn0, data = _device_rollout(E, N, False, T, 2)
    tr, buf = r.trainer, r.buf
    perms = tr.draw_perms().cpu().numpy()
    sub = perms[0][lo:hi]

    def f(dt, shuffle):
        rec = ff.ppo_train_ff(PA, PC, data, vn0, 1, sub[None], 1, dtype=dt, shuffle=shuffle)[0]
        return ff.update_grads(rec, (0,))

    o64, spread = mb.fp32_spread(f)
    tr.prepare(buf)
    rows = torch.as_tensor(sub, device=DEV).to(torch.int32).contiguous()
    _list_gradients(tr, buf, rows, tr.bwd_args(buf))
    _check_update(p, tr, o64, spread, 0, f"rows[{lo}:{hi}]")


# ---------------------------------------------------------------- 6: runner, evaluator, adapter
def _small_runner(num_mini_batch=1, seed=11, **pkw):
    from minimarl.env import VecEnv
    from minimarl.mappo import MappoPolicy, MappoRunner
    env = VecEnv(6, 2, max_steps=7, device=DEV)
    p = MappoPolicy(env.obs_dim, A, H, DEV, seed=3, **pkw)
    r = MappoRunner(env, p, T=10, L=5, ppo_epoch=2, seed=seed, num_mini_batch=num_mini_batch)
    r.warmup()
    r.rollout()
    r.compute()
    return p, r


def _params(p):
    return torch.cat([p.actor.flat, p.critic.flat]).clone()


def test_runner_episode_and_evaluator():
    """E 6, N 2, T 10: an episode moves the parameters and stays finite, the buffer holds no hidden arrays, resets
    reach the masks; MappoEvaluator.run returns the same scores twice."""
    from minimarl.evaluate import MappoEvaluator
    p, r = _small_runner(recurrent=False)
    before = _params(p)
    assert r.buf.rnn_states is None and r.buf.rnn_states_critic is None
    assert bool((r.buf.masks[1:] == 0).any()) and int(r.counter) == 10
    info = r.train()
    info2 = r.run_episode()
    torch.cuda.synchronize()
    assert all(np.isfinite(v) for v in list(info.values()) + list(info2.values())), (info, info2)
    after = _params(p)
    assert bool(torch.isfinite(after).all()) and not torch.equal(before, after)
    for net in (p.actor, p.critic):
        assert bool((net.flat[_recurrent_slots(net)] == 0).all())
    ev = MappoEvaluator(8, 2, 20, device=DEV)
    m1, s1 = ev.run(p)
    m2, s2 = ev.run(p)
    assert m1 == m2 and torch.equal(s1, s2) and bool(torch.isfinite(s1).all())


class _Space:
    def __init__(self, shape=None, n=None):
        self.shape, self.n = shape, n


@pytest.mark.parametrize("how", [dict(use_recurrent_policy=False), dict(algorithm_name="mappo")],
                         ids=["use_recurrent_policy", "algorithm_name"])
def test_r_mappo_policy_adapter(golden, how):
    """R_MAPPOPolicy with the feed-forward switch: the forward golden through the reference signatures, the
    rnn_states handed back unchanged, act(deterministic) = first argmax, evaluate_actions refused."""
    from minimarl.adapters import R_MAPPOPolicy
    fx = golden("mappo_ff_fwd")
    args = SimpleNamespace(hidden_size=32, actor_lr=1e-4, critic_lr=1e-4, opti_eps=1e-5, weight_decay=0, seed=1, **how)
    pol = R_MAPPOPolicy(args, _Space((D,)), _Space((D,)), _Space(n=A), DEV)
    assert pol.recurrent is False and pol.policy.recurrent is False
    pol.actor.load_reference_state(fx, "actor.")
    pol.critic.load_reference_state(fx, "critic.")
    t = lambda k: torch.from_numpy(fx[k])  # noqa: E731
    ha, hc = t("ha"), t("hc")
    np.testing.assert_allclose(pol.get_values(t("obs"), hc, t("masks")).cpu().numpy(), fx["get_values"], **TOL)
    v, a, lp, ha2, hc2 = pol.get_actions(t("obs"), t("obs"), ha, hc, t("masks"))
    assert a.shape == (fx["obs"].shape[0], 1) and ha2 is ha and hc2 is hc
    np.testing.assert_allclose(v.cpu().numpy(), fx["values"], **TOL)
    logits = ff.net_out(ff.nets(fx)[0], t("obs"))
    np.testing.assert_allclose(lp.cpu().numpy(), torch.log_softmax(logits, -1).gather(1, a.cpu()).numpy(), **TOL)
    act, ha3 = pol.act(t("obs"), ha, t("masks"), deterministic=True)
    assert ha3 is ha
    np.testing.assert_array_equal(act.cpu().numpy()[:, 0], logits.argmax(-1).numpy())
    with pytest.raises(NotImplementedError, match="feed-forward"):
        pol.evaluate_actions(t("obs"), t("obs"), ha, hc, t("actions"), t("masks"))
    # the naive recurrent flag keeps the RNNLayer (r_actor_critic.py:46)
    args2 = SimpleNamespace(hidden_size=32, seed=1, use_recurrent_policy=False, use_naive_recurrent_policy=True)
    assert R_MAPPOPolicy(args2, _Space((D,)), _Space((D,)), _Space(n=A), DEV).recurrent is True


def test_config_switch():
    from minimarl.config import MappoTrainConfig
    assert MappoTrainConfig().algorithm_name == "rmappo" and MappoTrainConfig().recurrent is True
    assert MappoTrainConfig(algorithm_name="mappo").recurrent is False
    with pytest.raises(ValueError, match="algorithm_name"):
        MappoTrainConfig(algorithm_name="ippo2")


# ---------------------------------------------------------------- 7: refusals and guards
def test_refusals_and_guards(tmp_path):
    from minimarl._lib import MM_MAPPO_TRAIN, MappoDims, lib
    from minimarl.checkpoint import load_checkpoint, save_checkpoint
    from minimarl.mappo import MappoPolicy, MappoTrainer
    p, r = _small_runner(3, recurrent=False)
    tr, buf = r.trainer, r.buf
    L_ = lib()
    # unsupported dims: an error through mm_last_error, nothing launched
    R, S = 12, 777.0
    outs = [torch.full((R,), S, device=DEV), torch.full((R,), S, device=DEV)]
    a = p.rollout_args(buf.obs[0], logp_out=outs[0], value_out=outs[1], act_in=buf.actions[0])
    for bad in (MappoDims(D, H, A, 3), MappoDims(48, H, A, 0), MappoDims(D, 64, A, 0), MappoDims(94, H, A, 2)):
        assert L_.mm_mappo_ff_fwd(ctypes.byref(bad), ctypes.byref(a), None) != 0
        assert "unsupported dims" in L_.mm_last_error().decode()
        assert L_.mm_mappo_ff_grad_scratch_count(ctypes.byref(bad)) < 0
        _nan_grads(tr)
        assert L_.mm_mappo_ff_grad(ctypes.byref(bad), ctypes.byref(tr.bwd_args(buf)), None, 0, tr.grad[0].data_ptr(),
                                   tr.grad[1].data_ptr(), tr.gscr.data_ptr(), None) != 0
    a.mode = MM_MAPPO_TRAIN
    assert L_.mm_mappo_ff_fwd(ctypes.byref(p.dims), ctypes.byref(a), None) != 0
    # a row list longer than the buffer, or empty
    rows = torch.arange(tr.rows, dtype=torch.int32, device=DEV)
    for n_rows in (0, tr.rows + 1):
        assert L_.mm_mappo_ff_grad(ctypes.byref(p.dims), ctypes.byref(tr.bwd_args(buf)), rows.data_ptr(), n_rows,
                                   tr.grad[0].data_ptr(), tr.grad[1].data_ptr(), tr.gscr.data_ptr(), None) != 0
    torch.cuda.synchronize()
    assert all(bool((o == S).all()) for o in outs) and bool(torch.isnan(tr.grad[0]).all()), "a refused call wrote"
    # the trainer's refusals
    with pytest.raises(NotImplementedError, match="fused=False"):
        MappoTrainer(p, 10, 12, fused=False)
    with pytest.raises(NotImplementedError, match="all-reduce"):
        MappoTrainer(p, 10, 12, num_mini_batch=2, grad_allreduce=lambda t: 1)
    with pytest.raises(NotImplementedError, match="exceeds"):
        MappoTrainer(p, 10, 12, num_mini_batch=121)
    # perms: [epochs, T * EN] permutations of the rows
    assert tr.n_chunks == 120 and tr.mbs == 40
    good = np.stack([np.random.default_rng(e).permutation(tr.n_chunks) for e in range(tr.epochs)])
    bad = good.copy()
    bad[1, 0] = bad[1, 1]
    before = _params(p)
    with pytest.raises(ValueError, match=r"perms\[1\] is not a permutation of the 120 rows"):
        tr.train(buf, perms=bad)
    with pytest.raises(ValueError, match="shape"):
        tr.train(buf, perms=good[:, :24])
    assert torch.equal(before, _params(p)) and tr.train_calls == 0
    info = tr.train(buf, perms=good)
    torch.cuda.synchronize()
    assert not torch.equal(before, _params(p)) and tr.train_calls == 1 and np.isfinite(info["ratio"])
    # checkpoints do not cross modes; a file without the field is a recurrent one
    rec = MappoTrainer(MappoPolicy(D, A, H, DEV, seed=1), 10, 12, L=5)
    path = str(tmp_path / "ff.safetensors")
    save_checkpoint(path, mappo=tr)
    with pytest.raises(ValueError, match="feed-forward"):
        load_checkpoint(path, mappo=rec)
    load_checkpoint(path, mappo=MappoTrainer(_policy(seed=9), 10, 12))
    save_checkpoint(path, mappo=rec)
    with pytest.raises(ValueError, match="recurrent"):
        load_checkpoint(path, mappo=tr)
    ts = {k: v.clone() for k, v in rec.checkpoint_tensors()[0].items()}
    rec.restore_tensors(ts, {})
    with pytest.raises(ValueError, match="recurrent"):
        tr.restore_tensors(ts, {})


def test_one_minibatch_with_allreduce_hooks():
    """M = 1 with grad_allreduce keeps working through the same hooks: a one-replica all-reduce (identity, world 1)
    gives the parameters of the run without it bit for bit, and the hook saw the sums and both gradients."""
    from minimarl.mappo import MappoTrainer
    outs, calls = [], []

    def hook(t):
        calls.append(tuple(t.shape))
        return 1

    for ar in (None, hook):
        p, r = _small_runner(recurrent=False)
        tr = MappoTrainer(p, 10, 12, ppo_epoch=2, grad_allreduce=ar)
        tr.train(r.buf)
        torch.cuda.synchronize()
        outs.append(_params(p))
    assert torch.equal(outs[0], outs[1])
    assert len(calls) == 1 + 2 * 2 and calls[0] == (5,)


def test_perm_seed_determinism_and_checkpoint_resume(tmp_path):
    """Equal perm_seed -> equal parameters after two train() calls, another seed -> different ones; a checkpoint
    taken between the two calls resumes to the same parameters bit for bit."""
    from minimarl.checkpoint import load_checkpoint, save_checkpoint
    from minimarl.mappo import MappoTrainer

    def two_calls(perm_seed, save=None, resume=None):
        p, r = _small_runner(3, recurrent=False)
        tr = MappoTrainer(p, 10, 12, ppo_epoch=2, num_mini_batch=3, perm_seed=perm_seed)
        if resume is None:
            tr.train(r.buf)
            if save is not None:
                save_checkpoint(save, trainer=tr)
        else:
            meta = load_checkpoint(resume, trainer=tr)
            assert tr.train_calls == 1 and meta["trainer"]["scalars"]["recurrent"] == 0, meta
        tr.train(r.buf)
        torch.cuda.synchronize()
        return _params(p), tr

    path = str(tmp_path / "ffmb.safetensors")
    a, tr_a = two_calls(7, save=path)
    b, _ = two_calls(7)
    c, _ = two_calls(8)
    d, _ = two_calls(7, resume=path)
    assert torch.equal(a, b), "equal perm_seed must give equal parameters"
    assert not torch.equal(a, c), "another perm_seed must give other permutations"
    assert torch.equal(a, d), "resumed run must draw the uninterrupted run's permutations"
    p0, p1 = tr_a.draw_perms(0), tr_a.draw_perms(1)
    assert p0.shape == (2, 120) and not torch.equal(p0, p1) and not torch.equal(p0[0], p0[1])


def test_recurrent_true_equals_the_default():
    """recurrent=True and omitting the argument are the same path: bit-identical parameters before and after a
    train(). (That this path still computes what it did before the feed-forward mode existed is what the untouched
    bit-identity tests of the recurrent kernels check, not this test.)"""
    p1, r1 = _small_runner()
    p2, r2 = _small_runner(recurrent=True)
    assert torch.equal(_params(p1), _params(p2)) and r2.buf.rnn_states is not None
    for r in (r1, r2):
        r.train()
    torch.cuda.synchronize()
    assert torch.equal(_params(p1), _params(p2))
