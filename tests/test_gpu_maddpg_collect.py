"""GPU: the one-launch maddpg / matd3 transition collector (csrc/maddpg_collect.hip via minimarl.maddpg_runner), its
write into a replay ring and MADDPGRunner, against the CPU oracles (oracle/, tests/moffq_ref.py).
Cases (env, E, N, T, max_steps, eps, common reward); a block holds min(128 / N, 64) envs, so E 70 is two blocks with a
short last tile, N 3 the non-power-of-two row split, (16, 8) the widest critic the trainer allows. T 7 / max_steps 3
resets every env twice inside the window, T 5 / max_steps 100 none. Logit bound: rtol 1e-4 / atol 1e-5, the project's
bound for this exact-f32 MFMA forward (tests/test_gpu_offq_collect.py)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from moffq_ref import AGENT_KEYS, agent_q
from offq_collect_ref import draws
from oracle import rng
from test_gpu_moffq_collect import FIELDS, case_id, make_env, replay

pytestmark = pytest.mark.gpu

SEED, NOISE_SEED, COUNTER0 = 1234, 11, 3
RTOL, ATOL = 1e-4, 1e-5
SHAPES = [("checkers", E, N, 7, 3) for E, N in ((40, 2), (24, 3), (16, 8), (70, 2))]
SHAPES += [("checkers", 40, 2, 5, 100), ("switch", 40, 2, 7, 3), ("switch", 70, 4, 7, 3)]
CASES = [s + ((0.3, 0.0, 1.0)[i % 3], i % 2 == 0) for i, s in enumerate(SHAPES)]


def make_actor(N, D, seed=7):
    """The head scaled by 30 (gain 0.01 makes every logit a near-tie), every bias / LayerNorm vector off 0 / 1."""
    from minimarl.maddpg import MADDPG
    tr = MADDPG(N, D, 5, seed=seed, noise_seed=NOISE_SEED)
    g = torch.Generator().manual_seed(seed + 100)
    tr.actor_view("Wo").mul_(30.0)
    for k in AGENT_KEYS:
        v = tr.actor_view(k)
        if v.dim() == 1:
            v.add_((0.1 * torch.randn(v.shape, generator=g)).to(v.device))
    return tr


def gumbel(seed, ctr, E, N):      # host twin of mm_maddpg_gumbel, as [E, N, A]
    e, n, k = np.meshgrid(np.arange(E), np.arange(N), np.arange(5), indexing="ij")
    u = rng.rng_uniform(rng.rng_draw(np.uint64(seed), np.uint64(ctr), e, n * 5 + k)) + np.float32(1e-20)
    t = (-np.log(u.astype(np.float64)).astype(np.float32) + np.float32(1e-20)).astype(np.float32)
    return -np.log(t.astype(np.float64)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def run_case(kind, E, N, T, ms, eps, common, explore=True):
    """One window into the staging tensors at counter COUNTER0; host arrays, computed once, read-only."""
    from minimarl._lib import check, lib
    from minimarl.maddpg_runner import MADDPGCollector
    from minimarl.qnet import ptr, stream_handle
    D, n = (3 if kind == "switch" else 47), T * E
    tr = make_actor(N, D)
    col = MADDPGCollector(make_env(kind, E, N, ms), tr, T, SEED, common_reward=common, with_q=True, explore=explore)
    col.counter.fill_(COUNTER0)
    fields, returns = col.collect(eps)
    out = {k: v.cpu().numpy() for k, v in fields.items()}
    out.update(q=col.q.cpu().numpy(), returns=returns.cpu().numpy(), n_done=col.n_done.cpu().numpy())
    P = {k: tr.actor_view(k).double().cpu() for k in AGENT_KEYS}
    out["z64"] = agent_q(P, fields["obs"].reshape(n * N, D).double().cpu()).numpy().reshape(n, N, 5)
    dr = [draws(SEED, COUNTER0 + t, E, N, 5) for t in range(T)]
    out["random"] = np.stack([u < np.float32(eps) for u, _ in dr]).reshape(n, N) & explore
    out["rand_act"] = np.stack([ra for _, ra in dr]).reshape(n, N)
    out["g"] = np.stack([gumbel(col.gumbel_seed, COUNTER0 + t, E, N) for t in range(T)]).reshape(n, N, 5)
    dev = torch.empty(T, N, E, 5, device="cuda")
    for t in range(T):
        check(lib().mm_maddpg_gumbel(ctypes.byref(tr.dims), ptr(dev[t]), E, col.gumbel_seed, COUNTER0 + t,
                                     stream_handle(tr.device)), "maddpg_gumbel")
    out["g_dev"] = dev.permute(0, 2, 1, 3).reshape(n, N, 5).cpu().numpy()
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
    """Replay the stored actions through the oracle env with reset-on-done: every field bit-equal."""
    kind, E, N, T, ms, eps, common = case
    o = run_case(*case)
    acts = o["acts"]
    assert ((acts == 0) | (acts == 1)).all() and (acts.sum(-1) == 1).all()
    cpu = replay(kind, E, N, T, ms, acts.argmax(-1).reshape(T, E, N), common)
    for k in FIELDS[:2] + FIELDS[3:] + ("returns", "n_done"):
        np.testing.assert_array_equal(o[k].reshape(cpu[k].shape), cpu[k], err_msg=k)
    assert (o["n_done"] == (T // ms if ms < T else 0)).all()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_logits_exploration_and_noise(case):
    """q_out vs the fp64 forward; the uniform actions; the noise is the documented stream and decides the other rows."""
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


@pytest.mark.parametrize("case", [CASES[0], CASES[6]], ids=case_id)      # both tiles, at eps 0.3 and eps 1
def test_explore_false_is_greedy_whatever_eps(case):
    o = run_case(*case, explore=False)
    assert_argmax_within_bound(o, o["z64"])
    other = run_case(*case[:5], 1.0, case[6], explore=False)
    for k in FIELDS + ("q", "returns", "n_done"):
        np.testing.assert_array_equal(o[k], other[k], err_msg=k)


@pytest.mark.parametrize("case", [CASES[3], CASES[6]], ids=case_id)
def test_ring_equals_staging(case):
    """The window written at first = size - 10 of a ring of T E + 5 slots, gathered by slot, is the staging run."""
    from minimarl.maddpg_runner import MADDPGCollector
    from minimarl.mlpbuf import MlpReplayBuffer
    kind, E, N, T, ms, eps, common = case
    o, D, n, size = run_case(*case), (3 if kind == "switch" else 47), T * E, T * E + 5
    col = MADDPGCollector(make_env(kind, E, N, ms), make_actor(N, D), T, SEED, common_reward=common)
    info = {"policy_0": {"obs_space": (D,), "share_obs_space": (N * D,), "act_space": (5,)}}
    buf = MlpReplayBuffer(info, {"policy_0": list(range(N))}, size, True, False, device="cuda", store_share=False)
    z = lambda *s: torch.zeros((size - 10,) + s, device="cuda")   # noqa: E731
    buf.insert(size - 10, z(N, D), z(N * D), z(N, 5), z(N, 1), z(N, D), z(N * D), z(N, 1), z(1), z(N, 1))
    col.counter.fill_(COUNTER0)
    col.set_epsilon(eps)
    slots = buf.insert_collected(col)
    np.testing.assert_array_equal(slots, (size - 10 + np.arange(n)) % size)
    got = buf.sample(n, inds=slots)
    for i, k in ((0, "obs"), (2, "acts"), (3, "rewards"), (4, "next_obs"), (6, "dones"), (8, "valid_transition")):
        np.testing.assert_array_equal(got[i]["policy_0"].cpu().numpy().transpose(1, 0, 2), o[k], err_msg=k)
    np.testing.assert_array_equal(got[7]["policy_0"].cpu().numpy(), o["dones_env"])


def test_graph_capture_replay_equals_eager():
    from minimarl.maddpg_runner import MADDPGCollector
    from minimarl.qnet import graph_capture
    tr, T = make_actor(2, 47), 7
    eager, cap = (MADDPGCollector(make_env("checkers", 40, 2, 3), tr, T, SEED, with_q=True) for _ in range(2))
    cap.collect(0.3)                       # first launch outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with graph_capture(g):
        cap.launch()
    for c0, eps in ((0, 0.3), (21, 0.6)):   # epsilon and the counter reach the replay through device memory
        eager.counter.fill_(c0)
        want, wret = eager.collect(eps)
        for t in cap.fields.values():
            t.zero_()
        cap.counter.fill_(c0)
        cap.set_epsilon(eps)
        g.replay()
        torch.cuda.synchronize()
        for k in want:
            assert torch.equal(want[k], cap.fields[k]), (k, c0)
        assert torch.equal(wret, cap.returns) and torch.equal(eager.q, cap.q) and torch.equal(eager.n_done, cap.n_done)


@pytest.mark.parametrize("algo", ["maddpg", "matd3"])
@pytest.mark.parametrize("env", ["checkers", "switch"])
def test_runner(env, algo):
    from minimarl import MADDPGRunner
    from minimarl._lib import lib
    from minimarl.config import OffQTrainConfig
    err0 = lib().mm_last_error()
    r = MADDPGRunner(OffQTrainConfig(env=env, algorithm_name=algo, n_envs=16, n_agents=2, episode_length=7,
                                     buffer_size=256, batch_size=8, seed=3))
    tr = r.trainer
    pa0, pc0, pta0 = tr.Pa.clone(), tr.Pc.clone(), tr.PTa.clone()
    r.warmup()                              # max(batch 8, 5 random episodes) // 16 + 1 = one window of 7 x 16
    assert len(r.buffer) == 112 and r.num_episodes_collected == 16 and r.total_train_steps == 0
    assert float(r.collector.eps.item()) == 1.0
    for it in range(3):
        assert r.run() == (it + 2) * 112
    assert len(r.buffer) == 256 and r.buffer.current_i == 4 * 112 - 256
    assert (r.total_env_steps, r.num_episodes_collected, r.total_train_steps) == (4 * 112, 64, 3)
    assert r.last_train_episode == 64 and int(r.collector.counter.item()) == 4 * 7
    assert float(r.collector.eps.item()) == np.float32(max(0.05, 1.0 - (1.0 - 0.05) / 50000 * (3 * 112)))
    info = r.train_infos[0]
    assert np.isfinite(float(info["critic_loss"])) and np.isfinite(float(info["actor_loss"]))
    for p0, p in ((pa0, tr.Pa), (pc0, tr.Pc), (pta0, tr.PTa)):     # PTa moved: the soft update ran
        assert not torch.equal(p0, p) and torch.isfinite(p).all()
    r.buffer.check_errors()
    assert lib().mm_last_error() == err0    # the library's error string is sticky: the run must not have set one
