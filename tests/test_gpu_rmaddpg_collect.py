"""GPU: the one-launch rmaddpg / rmatd3 episode collector (csrc/rmaddpg_collect.hip via minimarl.rmaddpg_runner) and
RMADDPGRunner against the CPU oracles (oracle/, tests/offq_collect_ref.py, tests/offq_switch_ref.py, the float64 actor of
tests/rmaddpg_ref.py).
Cases (env, E, N, T, max_steps, eps, common reward); a block holds min(128 / N, 64) envs, so E 70 is two blocks with a
short last tile, N 3 the non-power-of-two row split, (16, 8) the widest critic the trainer allows. T 7 / max_steps 5 runs
two post-done steps in every env, T 5 / max_steps 100 finishes none. Logit bound: rtol 1e-4 / atol 1e-5, the project's
bound for this exact-f32 MFMA GRU forward (tests/test_gpu_offq_collect.py)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import offq_switch_ref
import rmaddpg_ref
from offq_collect_ref import common_sum, draws, step_not_done
from oracle.env import EnvSpec, VecEnvOracle
from oracle.switch import SwitchSpec
from test_gpu_maddpg_collect import gumbel
from test_gpu_moffq_collect import case_id, make_env

pytestmark = pytest.mark.gpu

SEED, NOISE_SEED, COUNTER0 = 1234, 11, 3
RTOL, ATOL = 1e-4, 1e-5
SHAPES = [("checkers", E, N, 7, 5) for E, N in ((40, 2), (24, 3), (16, 8), (70, 2))]
SHAPES += [("checkers", 40, 2, 5, 100), ("switch", 40, 2, 7, 5), ("switch", 70, 4, 7, 5)]
CASES = [s + ((0.3, 0.0, 1.0)[i % 3], i % 2 == 0) for i, s in enumerate(SHAPES)]
FIELDS = ("obs", "acts", "rewards", "dones", "dones_env")


def make_actor(N, D, T, seed=7):
    """The head scaled by 30 (gain 0.01 makes every logit a near-tie), every bias / LayerNorm vector off 0 / 1."""
    from minimarl.rmaddpg import RMADDPG
    tr = RMADDPG(N, D, 5, T, 8, seed=seed, noise_seed=NOISE_SEED)
    g = torch.Generator().manual_seed(seed + 100)
    tr.actor_view("Wo").mul_(30.0)
    for k in rmaddpg_ref.KEYS:
        v = tr.actor_view(k)
        if v.dim() == 1:
            v.add_((0.1 * torch.randn(v.shape, generator=g)).to(v.device))
    return tr


def replay(kind, E, N, T, ms, act, common):
    """The episode with the actions given, from reset, no step after done, through the oracle env."""
    if kind == "switch":
        return offq_switch_ref.replay(SwitchSpec(N, max_steps=ms), E, lambda t, obs: act[t], T, common)
    env, done, ret = VecEnvOracle(EnvSpec(N, max_steps=ms), E), np.zeros(E, bool), np.zeros(E, np.float32)
    out = {k: [] for k in FIELDS[2:]}
    obs = [env.observe()]
    for t in range(T):
        rew, done = step_not_done(env, act[t], done)
        rew = np.repeat(common_sum(rew)[:, None], N, 1) if common else rew
        obs.append(env.observe())
        out["rewards"].append(rew[..., None])
        out["dones"].append(np.repeat(done[:, None, None], N, 1))
        out["dones_env"].append(done[:, None])
        ret = (ret + rew[:, 0]).astype(np.float32)
    return dict({k: np.stack(v).astype(np.float32) for k, v in out.items()}, obs=np.stack(obs), returns=ret)


@functools.lru_cache(maxsize=None)
def run_case(kind, E, N, T, ms, eps, common, explore=True, with_q=True):
    """One episode at counter COUNTER0; host arrays, computed once, read-only."""
    from minimarl._lib import check, lib
    from minimarl.qnet import ptr, stream_handle
    from minimarl.rmaddpg_runner import RMADDPGCollector
    D = 3 if kind == "switch" else 47
    tr = make_actor(N, D, T)
    col = RMADDPGCollector(make_env(kind, E, N, ms), tr, T, SEED, common_reward=common, with_q=with_q, explore=explore)
    col.counter.fill_(COUNTER0)
    fields, returns, _ = col.collect(eps)
    out = {k: v.cpu().numpy() for k, v in fields.items()}
    out["returns"] = returns.cpu().numpy()
    if with_q:      # the float64 actor over the stored observations, hidden state carried from zero through all T steps
        P = {k: tr.actor_view(k).double().cpu() for k in rmaddpg_ref.KEYS}
        with torch.no_grad():
            z = rmaddpg_ref.run(P, fields["obs"][:T].reshape(T, E * N, D).double().cpu())
        out.update(q=col.q.cpu().numpy(), z64=z.numpy().reshape(T, E, N, 5))
        dr = [draws(SEED, COUNTER0 + t, E, N, 5) for t in range(T)]
        out["random"] = np.stack([u < np.float32(eps) for u, _ in dr]) & explore
        out["rand_act"] = np.stack([ra for _, ra in dr])
        out["g"] = np.stack([gumbel(col.gumbel_seed, COUNTER0 + t, E, N) for t in range(T)])
        dev = torch.empty(T, N, E, 5, device="cuda")
        for t in range(T):
            check(lib().mm_maddpg_gumbel(ctypes.byref(tr.dims), ptr(dev[t]), E, col.gumbel_seed, COUNTER0 + t,
                                         stream_handle(tr.device)), "maddpg_gumbel")
        out["g_dev"] = dev.permute(0, 2, 1, 3).cpu().numpy()
    for v in out.values():
        v.setflags(write=False)
    return out


def assert_argmax_within_bound(o, z):      # non-random rows: z[stored action] >= max(z) - 2 (rtol max|z64| + atol)
    slack = 2 * (RTOL * np.abs(o["z64"]).max(-1) + ATOL)
    za = np.take_along_axis(z, o["acts"].argmax(-1)[..., None], -1)[..., 0]
    bad = ~o["random"] & (za < z.max(-1) - slack)
    assert not bad.any(), (int(bad.sum()), float((z.max(-1) - za)[bad].max()))
    return slack


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_env_exact(case):
    """Replay the stored actions through the oracle env from reset, no step after done: every field bit-equal."""
    kind, E, N, T, ms, eps, common = case
    o = run_case(*case)
    acts = o["acts"]
    assert ((acts == 0) | (acts == 1)).all() and (acts.sum(-1) == 1).all()
    cpu = replay(kind, E, N, T, ms, acts.argmax(-1), common)
    for k in ("obs", "rewards", "dones", "dones_env", "returns"):
        np.testing.assert_array_equal(o[k], cpu[k], err_msg=k)
    assert (o["dones_env"][-1] == (ms < T)).all()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_logits_exploration_and_noise(case):
    """q_out vs the fp64 GRU actor; the uniform actions; the noise is the documented stream and decides the other rows."""
    o, eps = run_case(*case), case[5]
    z, g = o["z64"], o["g"]
    np.testing.assert_allclose(o["q"], z, rtol=RTOL, atol=ATOL)
    rnd = o["random"]
    np.testing.assert_array_equal(o["acts"].argmax(-1)[rnd], o["rand_act"][rnd])
    assert rnd.all() if eps == 1.0 else (not rnd.any() if eps == 0.0 else (rnd.any() and not rnd.all()))
    np.testing.assert_array_equal(g, o["g_dev"])
    slack = assert_argmax_within_bound(o, z + g)
    if eps < 1.0:     # rows the noise decides: the noisy winner beats the noise-free one by more than the bound
        zg = z + g
        gain = zg.max(-1) - np.take_along_axis(zg, z.argmax(-1)[..., None], -1)[..., 0]
        assert (~rnd & (gain > slack)).any()


@pytest.mark.parametrize("case", [CASES[0], CASES[6]], ids=case_id)      # both tiles
def test_explore_false_is_greedy_whatever_eps(case):
    o = run_case(*case, explore=False)
    assert_argmax_within_bound(o, o["z64"])
    other = run_case(*case[:5], 1.0, case[6], explore=False)
    for k in FIELDS + ("q", "returns"):
        np.testing.assert_array_equal(o[k], other[k], err_msg=k)


@pytest.mark.parametrize("case", [CASES[2], CASES[5]], ids=case_id)      # both tiles, eps 1
def test_warmup_shortcut_stores_the_same_bits(case):
    assert case[5] == 1.0
    o, short = run_case(*case), run_case(*case, with_q=False)
    for k in FIELDS + ("returns",):
        np.testing.assert_array_equal(short[k], o[k], err_msg=k)


def test_graph_capture_replay_equals_eager():
    from minimarl.qnet import graph_capture
    from minimarl.rmaddpg_runner import RMADDPGCollector
    tr, T = make_actor(2, 47, 7), 7
    eager, cap = (RMADDPGCollector(make_env("checkers", 40, 2, 5), tr, T, SEED, with_q=True) for _ in range(2))
    cap.collect(0.3)                       # first launch outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with graph_capture(g):
        cap.launch()
    for c0, eps in ((0, 0.3), (21, 0.6)):   # epsilon and the counter reach the replay through device memory
        eager.counter.fill_(c0)
        want, wret, _ = eager.collect(eps)
        for t in cap.fields.values():
            t.zero_()
        cap.counter.fill_(c0)
        cap.set_epsilon(eps)
        g.replay()
        torch.cuda.synchronize()
        for k in want:
            assert torch.equal(want[k], cap.fields[k]), (k, c0)
        assert torch.equal(wret, cap.returns) and torch.equal(eager.q, cap.q)
        assert int(cap.counter.item()) == c0 + T


@pytest.mark.parametrize("algo", ["rmaddpg", "rmatd3"])
@pytest.mark.parametrize("env", ["checkers", "switch"])
def test_runner(env, algo):
    from minimarl import RMADDPGRunner
    from minimarl._lib import lib
    from minimarl.config import OffQTrainConfig
    err0 = lib().mm_last_error()
    r = RMADDPGRunner(OffQTrainConfig(env=env, algorithm_name=algo, n_envs=16, n_agents=2, episode_length=7,
                                      buffer_size=64, batch_size=8, seed=3))
    tr = r.trainer
    pa0, pc0, pta0 = tr.Pa.clone(), tr.Pc.clone(), tr.PTa.clone()
    r.warmup()                              # max(batch 8, 5 random episodes) // 16 + 1 = one collect of 16 episodes
    assert len(r.buffer) == 16 and r.num_episodes_collected == 16 and r.total_train_steps == 0
    assert float(r.collector.eps.item()) == 1.0
    updated = []
    for it in range(3):
        assert r.run() == (it + 2) * 16 * 7
        updated.append(r.train_infos[0]["update_actor"])
    assert updated == [True, algo == "rmaddpg", True]
    assert len(r.buffer) == 64
    assert (r.total_env_steps, r.num_episodes_collected, r.total_train_steps) == (4 * 16 * 7, 64, 3)
    assert r.last_train_episode == 64 and int(r.collector.counter.item()) == 4 * 7
    assert float(r.collector.eps.item()) == np.float32(max(0.05, 1.0 - (1.0 - 0.05) / 50000 * (3 * 16 * 7)))
    info = r.train_infos[0]
    assert np.isfinite(float(info["critic_loss"])) and np.isfinite(float(info["actor_loss"]))
    for p0, p in ((pa0, tr.Pa), (pc0, tr.Pc), (pta0, tr.PTa)):     # PTa moved: the soft update ran
        assert not torch.equal(p0, p) and torch.isfinite(p).all()
    r.buffer.check_errors()
    assert lib().mm_last_error() == err0    # the library's error string is sticky: the run must not have set one
