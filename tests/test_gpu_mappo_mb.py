"""GPU: MAPPO's PPO minibatches over shuffled chunks (MappoTrainer(num_mini_batch=M > 1): mm_mappo_mb_stats +
mm_mappo_vn_update + mm_mappo_grad_mb + mm_clip_adam per minibatch) against the reference's golden train() with
train_batch_size 3 (tests/golden/mappo_mb_train.npz) and the restatement tests/mappo_mb_ref.py, whose docstring
states the tolerance rule: K_FP32 = 16 fp32 spreads (fp32 / fp32 shuffled within each minibatch / f64) of the f64
run, plus a golden value's own distance to the f64 run where the comparison is against the golden."""
import functools
import os

import numpy as np
import pytest
import torch

import mappo_cv_ref as cv
import mappo_mb_ref as mb
from oracle import mappo as om

pytestmark = pytest.mark.gpu
DEV = "cuda"
D, A, H = 47, 5, 32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _policy(fx, N=None, prefix="before."):
    from minimarl.mappo import MappoPolicy
    p = MappoPolicy(D, A, H, DEV, cent_agents=N)
    p.actor.load_reference_state(fx, prefix + "actor.")
    p.critic.load_reference_state(fx, prefix + "critic.")
    return p


def _trainer(fx, cent=False, **kw):
    from minimarl.mappo import MappoBuffer, MappoTrainer
    E, N, T, L = (int(fx[k]) for k in ("E", "N", "T", "L"))
    p = _policy(fx, N if cent else None)
    PA, PC, data, vn0, nch = cv.train_inputs(fx)
    buf = MappoBuffer(T, E, N, D, H, DEV)
    buf.load_reference(data)
    tr = MappoTrainer(p, T, E * N, L=L, ppo_epoch=int(fx["epochs"]), **kw)
    tr.load_value_normalizer(*vn0)
    return p, buf, tr


@functools.lru_cache(maxsize=None)
def _golden_case():
    """The golden fixture and the restatement's three runs on it (computed once, read-only): train outputs and the
    unclipped gradients of the first two updates, each as (f64 values, fp32 spreads)."""
    fx = dict(np.load(os.path.join(GOLDEN, "mappo_mb_train.npz")))
    PA, PC, data, vn0, _ = cv.train_inputs(fx)
    EP, L, M = int(fx["epochs"]), int(fx["L"]), int(fx["train_batch_size"])
    runs = {}

    def run(dt, shuffle):
        if (dt, shuffle) not in runs:
            runs[(dt, shuffle)] = mb.ppo_train_mb(PA, PC, data, vn0, EP, L, fx["perms"], M, dtype=dt, shuffle=shuffle)
        return runs[(dt, shuffle)]

    train = mb.fp32_spread(lambda dt, sh: mb.train_outputs(*run(dt, sh)))
    grads = mb.fp32_spread(lambda dt, sh: mb.update_grads(run(dt, sh)[0], (0, 1)))
    return fx, train, grads, M


def _nan_grads(tr):
    tr.grad[0].fill_(float("nan"))
    tr.grad[1].fill_(float("nan"))


def _vn_update(tr):
    from minimarl._lib import lib
    assert lib().mm_mappo_vn_update(tr.vn.data_ptr(), tr.stats.data_ptr(), 0.99999, None) == 0


# ---------------------------------------------------------------- 1: the golden train()
def test_ppo_train_three_minibatches_matches_reference():
    """train(perms = the recorded randperms), 3 epochs x 3 minibatches of 5 chunks (less than a tile), 1 of the 16
    chunks dropped per epoch, in-chunk mask zeros and inactive rows, a ValueNorm update per minibatch: post-Adam
    parameters, ValueNorm state and train_info against the f64 restatement and the golden; mean ratio rtol 1e-5."""
    fx, (o64, spread), _, M = _golden_case()
    p, buf, tr = _trainer(fx, num_mini_batch=M)
    info = tr.train(buf, perms=fx["perms"])
    torch.cuda.synchronize()
    assert tr.norms.shape == (2, int(fx["epochs"]) * M)
    for net, kind in ((p.actor, "actor"), (p.critic, "critic")):
        for k in om.NET_KEYS:
            got = net.view(k).cpu().numpy()
            after = fx[f"after.{kind}.{om.ref_name(k, kind)}"]
            mb.assert_within(got, o64[(kind, k)], spread[(kind, k)], f"{kind} {k} vs f64")
            mb.assert_within(got, after, spread[(kind, k)], f"{kind} {k} vs golden",
                             float(np.abs(after - o64[(kind, k)]).max()))
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
    # the pre-clip norms of the nine updates, in update order
    nrm = tr.norms.cpu().numpy()
    np.testing.assert_allclose(nrm.T.reshape(-1), fx["norms"], rtol=1e-5)


# ---------------------------------------------------------------- 2: gradients of the first two updates
def test_first_two_update_gradients_match_reference():
    """Unclipped gradients of update 0 (both nets, grad pre-filled with NaN: every entry, pads included, is written;
    the scratch pre-filled with NaN too: the MLP pass reads no d x2 row the recurrent pass did not write), then,
    after its Adam step and without clearing the scratch, of update 1 on the next 5 chunks (a stale d x2 row of
    update 0 leaking in would show): against the f64 restatement and the golden's recorded gradients."""
    fx, _, (g64, spread), M = _golden_case()
    p, buf, tr = _trainer(fx, num_mini_batch=M)
    native = tr.native_chunks(fx["perms"])
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
        for n, net in enumerate((p.actor, p.critic)):
            for k in om.NET_KEYS:
                g = net.view(k, tr.grad[n]).cpu().numpy()
                mb.assert_within(g, g64[(u, n, k)], spread[(u, n, k)], f"update {u} net {n} {k} vs f64")
                ref = mb.golden_grad(fx, u, n, k)
                mb.assert_within(g, ref, spread[(u, n, k)], f"update {u} net {n} {k} vs golden",
                                 float(np.abs(ref - g64[(u, n, k)]).max()))
            pad = torch.ones_like(tr.grad[n], dtype=torch.bool)
            for k in om.NET_KEYS:
                net.view(k, pad).fill_(False)
            assert int(pad.sum()) > 0 and bool((tr.grad[n][pad] == 0).all()), "pads must carry zero gradient"
            assert bool(torch.isfinite(tr.grad[n]).all())
        tr.clip_adam(u)


# ---------------------------------------------------------------- 3: bit-identity with the full-batch pass
@pytest.mark.parametrize("cent", [False, True], ids=["golden", "centralized_n2"])
def test_all_chunks_in_native_order_is_bit_identical_to_mappo_grad(golden, cent):
    """mm_mappo_grad_mb with chunks = arange(n_chunks) (native order) on the stats of prepare() + one vn_update
    gives mm_mappo_grad's gradients bit for bit, decentralized and centralized critic (N 2, cent_agents 2)."""
    fx = cv.case(golden("mappo_cv_train"), "n2") if cent else golden("mappo_mb_train")
    p, buf, tr = _trainer(fx, cent=cent)
    tr.prepare(buf)
    _vn_update(tr)
    _nan_grads(tr)
    tr.gradients(buf)
    full = [g.clone() for g in tr.grad]
    _nan_grads(tr)
    tr.gradients_mb(buf, torch.arange(tr.n_chunks, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    for n in (0, 1):
        assert bool(torch.isfinite(full[n]).all())
        assert torch.equal(full[n], tr.grad[n]), f"net {n}"


# ---------------------------------------------------------------- 4: a second tile per wave
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


@pytest.mark.parametrize("E,N,cent", [(2100, 8, False), (8200, 2, True)], ids=["n8", "centralized_n2"])
def test_second_tile_per_wave_one_epoch_vs_oracle(E, N, cent):
    """L 2, T 4, M 2 on a device rollout with max_steps 3 (episodes end inside chunks). N 8, E 2100: 16800 chunks
    per minibatch = 525 tiles over the recurrent pass's 512 waves, 33600 row-steps = 1050 tiles over the MLP pass's
    at most 1024 waves. N 2 centralized, E 8200: 16400 chunks = 513 tiles, 32800 row-steps = 1025 tiles. One
    epoch's two updates (the gradients of both; the second is taken after the first's clip + Adam step) against the
    restatement fed the device's buffer and the device's permutation."""
    from minimarl.env import VecEnv
    from minimarl.mappo import MappoPolicy, MappoRunner, chunks_native_to_ref
    T, L, M = 4, 2, 2
    env = VecEnv(E, N, max_steps=3, device=DEV)
    p = MappoPolicy(env.obs_dim, A, H, DEV, seed=3, cent_agents=N if cent else None)
    PA = {k: p.actor.view(k).detach().cpu().clone() for k in om.NET_KEYS}
    PC = {k: p.critic.view(k).detach().cpu().clone() for k in om.NET_KEYS}
    r = MappoRunner(env, p, T=T, L=L, ppo_epoch=1, seed=11, num_mini_batch=M)
    r.warmup()
    r.rollout()
    r.compute()
    torch.cuda.synchronize()
    tr, buf = r.trainer, r.buf
    assert tr.mbs > 16384 and tr.mbs * L > 32768
    vn0 = [float(x) for x in tr.vn.cpu().numpy()]
    data = _ref_layout(buf, E, N)
    assert (data["masks"][[t for t in range(1, T) if t % L]] == 0).any(), "no reset inside a chunk"
    perms = tr.draw_perms().cpu().numpy()
    native = tr._to_native(torch.as_tensor(perms, device=DEV))
    np.testing.assert_array_equal(chunks_native_to_ref(native.cpu().numpy().astype(np.int64), T, L, E * N), perms)

    def f(dt, shuffle):
        rec = mb.ppo_train_mb(PA, PC, data, vn0, 1, L, perms, M, dtype=dt, shuffle=shuffle, cent=cent)[0]
        return mb.update_grads(rec, (0, 1))

    o64, spread = mb.fp32_spread(f)
    tr.prepare(buf)
    ba = tr.bwd_args(buf)
    for u in (0, 1):
        ch = native[0, u * tr.mbs:(u + 1) * tr.mbs]
        tr.mb_stats(buf, ch)
        _vn_update(tr)
        _nan_grads(tr)
        tr.gradients_mb(buf, ch, ba)
        torch.cuda.synchronize()
        for n, net in enumerate((p.actor, p.critic)):
            for k in om.NET_KEYS:
                mb.assert_within(net.view(k, tr.grad[n]).cpu().numpy(), o64[(u, n, k)], spread[(u, n, k)],
                                 f"update {u} net {n} {k}")
        tr.clip_adam(u)


# ---------------------------------------------------------------- 5: mm_mappo_mb_stats alone
def test_mb_stats_alone():
    """Active count exact, return moments at rtol 1e-6 against numpy over the listed rows, slots 0, 1, 5, 6 (and the
    unused 7) untouched. T 6, L 3, EN 37, 41 of the 74 chunks in a random order."""
    from minimarl._lib import lib
    T, L, EN, n = 6, 3, 37, 41
    rng = np.random.default_rng(5)
    ret = (rng.standard_normal((T + 1, EN)) * 3 + 1).astype(np.float32)
    act = (rng.random((T + 1, EN)) > 0.3).astype(np.float32)
    chunks = rng.permutation(T // L * EN)[:n].astype(np.int32)
    rows = np.array([[(c // EN * L + l) * EN + c % EN for l in range(L)] for c in chunks]).reshape(-1)
    stats0 = np.array([0.25, 1.5, -1.0, -2.0, -3.0, 0.75, 2.5, 9.0], np.float32)
    d = lambda x: torch.from_numpy(x).to(DEV)  # noqa: E731
    ret_d, act_d, ch_d, stats = d(ret), d(act), d(chunks), d(stats0.copy())
    part = torch.zeros(3 * 256, dtype=torch.float64, device=DEV)
    assert lib().mm_mappo_mb_stats(ret_d.data_ptr(), act_d.data_ptr(), ch_d.data_ptr(), n, L, T, EN, part.data_ptr(),
                                   stats.data_ptr(), None) == 0
    torch.cuda.synchronize()
    got = stats.cpu().numpy()
    r64 = ret.reshape(-1)[rows].astype(np.float64)
    assert got[2] == float((act.reshape(-1)[rows] != 0).sum())
    np.testing.assert_allclose(got[3], r64.mean(), rtol=1e-6)
    np.testing.assert_allclose(got[4], (r64 ** 2).mean(), rtol=1e-6)
    np.testing.assert_array_equal(got[[0, 1, 5, 6, 7]], stats0[[0, 1, 5, 6, 7]])
    # argument checks
    args = [ret_d.data_ptr(), act_d.data_ptr(), ch_d.data_ptr(), n, L, T, EN, part.data_ptr(), stats.data_ptr(), None]
    for i, bad in ((2, None), (3, 0), (4, 4), (3, T // L * EN + 1)):
        a = list(args)
        a[i] = bad
        assert lib().mm_mappo_mb_stats(*a) != 0, (i, bad)


# ---------------------------------------------------------------- 6: interface
def _small_runner(num_mini_batch=None, seed=11, **kw):
    from minimarl.env import VecEnv
    from minimarl.mappo import MappoPolicy, MappoRunner
    env = VecEnv(6, 2, max_steps=7, device=DEV)
    p = MappoPolicy(env.obs_dim, A, H, DEV, seed=3)
    extra = {} if num_mini_batch is None else {"num_mini_batch": num_mini_batch}
    r = MappoRunner(env, p, T=10, L=5, ppo_epoch=2, seed=seed, **extra, **kw)
    r.warmup()
    r.rollout()
    r.compute()
    return p, r


def _params(p):
    return torch.cat([p.actor.flat, p.critic.flat]).clone()


def test_refusals_and_perms_validation():
    from minimarl.mappo import MappoPolicy, MappoTrainer
    p = MappoPolicy(D, A, H, DEV, seed=0)
    with pytest.raises(NotImplementedError, match="fused"):
        MappoTrainer(p, 10, 8, L=5, num_mini_batch=2, fused=False)
    with pytest.raises(NotImplementedError, match="all-reduce"):
        MappoTrainer(p, 10, 8, L=5, num_mini_batch=2, grad_allreduce=lambda t: 1)
    with pytest.raises(NotImplementedError, match="no chunk"):
        MappoTrainer(p, 10, 8, L=5, num_mini_batch=17)
    p, r = _small_runner(3)
    tr = r.trainer
    good = np.stack([np.random.default_rng(e).permutation(tr.n_chunks) for e in range(tr.epochs)])
    bad = good.copy()
    bad[1, 0] = bad[1, 1]
    before = _params(p)
    with pytest.raises(ValueError, match=r"perms\[1\] is not a permutation"):
        tr.train(r.buf, perms=bad)
    with pytest.raises(ValueError, match="shape"):
        tr.train(r.buf, perms=good[:1])
    with pytest.raises(ValueError, match="not a permutation"):
        tr.train(r.buf, perms=good + 1)
    assert torch.equal(before, _params(p)) and tr.train_calls == 0
    tr.train(r.buf, perms=good)
    torch.cuda.synchronize()
    assert not torch.equal(before, _params(p)) and tr.train_calls == 1


def test_perm_seed_determinism_and_checkpoint_resume(tmp_path):
    """Equal perm_seed -> equal parameters after two train() calls, another seed -> different ones; a checkpoint
    taken between the two calls resumes to the same parameters bit for bit (the train-call counter travels in the
    checkpoint's scalars; a file without it loads with the counter at 0)."""
    from minimarl.checkpoint import load_checkpoint, save_checkpoint
    from minimarl.mappo import MappoTrainer

    def two_calls(perm_seed, save=None, resume=None):
        p, r = _small_runner(3)
        tr = MappoTrainer(p, 10, 12, L=5, ppo_epoch=2, num_mini_batch=3, perm_seed=perm_seed)
        if resume is None:
            tr.train(r.buf)
            if save is not None:
                save_checkpoint(save, trainer=tr)
        else:
            meta = load_checkpoint(resume, trainer=tr)
            assert tr.train_calls == 1, meta
        tr.train(r.buf)
        torch.cuda.synchronize()
        return _params(p), tr

    path = str(tmp_path / "mb.safetensors")
    a, tr_a = two_calls(7, save=path)
    b, _ = two_calls(7)
    c, _ = two_calls(8)
    d, _ = two_calls(7, resume=path)
    assert torch.equal(a, b), "equal perm_seed must give equal parameters"
    assert not torch.equal(a, c), "another perm_seed must give other permutations"
    assert torch.equal(a, d), "resumed run must draw the uninterrupted run's permutations"
    assert tr_a.train_calls == 2
    # the two calls drew different permutations, an epoch's differ too
    p0, p1 = tr_a.draw_perms(0), tr_a.draw_perms(1)
    assert not torch.equal(p0, p1) and not torch.equal(p0[0], p0[1])
    # an older file (no train_calls among the scalars) still loads
    tr_a.restore_tensors({k: v.clone() for k, v in tr_a.checkpoint_tensors()[0].items()}, {})
    assert tr_a.train_calls == 0


def test_one_minibatch_is_todays_path():
    """num_mini_batch=1 gives parameters bit-identical to a trainer constructed without the argument."""
    p1, r1 = _small_runner(None)
    p2, r2 = _small_runner(1)
    for r in (r1, r2):
        r.train()
    torch.cuda.synchronize()
    assert r2.trainer.perm_gen is None and r2.trainer.norms.shape == (2, 2)
    assert torch.equal(_params(p1), _params(p2))
