"""GPU: the one-launch offpolicy episode collector (csrc/offq_collect.hip via minimarl.offq_runner.OffQCollector),
RecReplayBuffer.insert_collected (mm_erb_insert_concat) and OffQRunner against the CPU oracles.

Shapes: (E, N) = (40, 2), (24, 3), (16, 8) fit one block's env tile with an odd N and an E that is no multiple of
it; (70, 2) and (40, 8) span 2 and 3 blocks with a short last tile. T = 7 with max_steps 5 runs the post-done path
for 2 steps in every env; T = 5 with max_steps 100 finishes no env."""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

from offq_collect_ref import common_sum, draws, step_not_done
from oracle import offq as ref
from oracle.env import EnvSpec, VecEnvOracle

pytestmark = pytest.mark.gpu

SEED, COUNTER0 = 1234, 0
RTOL, ATOL = 1e-4, 1e-5          # the tolerance of tests/test_gpu_offq.py for mm_offq_q_values
SHAPES = [(40, 2), (24, 3), (16, 8)]
EPISODES = [(7, 5), (5, 100)]    # (T, max_steps)
CASES = [(E, N, T, ms, eps, common) for (E, N), (T, ms), eps, common in
         itertools.product(SHAPES, EPISODES, (0.0, 0.3, 1.0), (True, False))]
CASES += [(70, 2, 7, 5, 0.3, True), (40, 8, 7, 5, 0.3, False)]   # more than one block


def make_policy(N, T, mixer="vdn", seed=7):
    """OffQMix(seed=...) with the Q head scaled by 10 (greedy actions are not all near-ties) and every bias and
    LayerNorm parameter moved off its 0 / 1 default, so each of them shows in Q."""
    from minimarl.offq import AGENT_KEYS, OffQMix
    tr = OffQMix(N, 47, 5, T, 8, mixer=mixer, seed=seed)
    g = torch.Generator().manual_seed(seed + 100)
    tr.agent_view("Wo").mul_(10.0)
    for k in AGENT_KEYS:
        v = tr.agent_view(k)
        if v.dim() == 1:
            v.add_((0.1 * torch.randn(v.shape, generator=g)).to(v.device))
    tr.hard_target_updates()
    return tr


@functools.lru_cache(maxsize=None)
def run_case(E, N, T, max_steps, eps, common):
    """One collect; everything the checks need as host arrays (computed once, shared, not modified)."""
    from minimarl.env import VecEnv
    from minimarl.offq_runner import OffQCollector
    tr = make_policy(N, T)
    env = VecEnv(E, N, max_steps=max_steps, device="cuda")
    col = OffQCollector(env, tr, T, SEED, common_reward=common, with_q=True)
    fields, returns, acts = col.collect(eps)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in fields.items()}
    out["q"], out["returns"] = col.q.cpu().numpy(), returns.cpu().numpy()
    obs_seq = fields["obs"][:T].reshape(T, E * N, 47)
    out["q_lib"] = tr.get_q_values(obs_seq)[0].reshape(T, E, N, 5).cpu().numpy()
    P = ref.agent_from_state(tr.state_dict()[0], prefix="")
    with torch.no_grad():
        out["q_ref"] = ref.agent_q_seq(P, obs_seq.cpu())[0].numpy().reshape(T, E, N, 5)
    dr = [draws(SEED, COUNTER0 + t, E, N, 5) for t in range(T)]
    out["explore"] = np.stack([u < np.float32(eps) for u, _ in dr])
    out["rand_act"] = np.stack([ra for _, ra in dr])
    for v in out.values():
        v.setflags(write=False)
    return out


def case_id(c):
    return "E{}-N{}-T{}-ms{}-eps{}-{}".format(*c[:5], "common" if c[5] else "own")


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_env_exact(case):
    """Replay the stored actions through the oracle env from reset: observations, rewards and dones bit-equal."""
    E, N, T, ms, eps, common = case
    o = run_case(*case)
    env = VecEnvOracle(EnvSpec(N, max_steps=ms), E)
    done = np.zeros(E, bool)
    act = o["acts"].argmax(-1)
    ret = np.zeros(E, np.float32)
    for t in range(T):
        np.testing.assert_array_equal(o["obs"][t], env.observe(), err_msg=f"obs t={t}")
        was_done = done.copy()
        rew, done = step_not_done(env, act[t], done)
        if common:
            want = np.repeat(common_sum(rew)[:, None], N, 1)
            np.testing.assert_allclose(o["rewards"][t, :, :, 0], want, rtol=1e-6, atol=0, err_msg=f"rew t={t}")
        else:
            np.testing.assert_array_equal(o["rewards"][t, :, :, 0], rew, err_msg=f"rew t={t}")
        assert (o["rewards"][t][was_done] == 0).all()
        np.testing.assert_array_equal(o["dones_env"][t, :, 0], done.astype(np.float32))
        np.testing.assert_array_equal(o["dones"][t, :, :, 0], np.repeat(done[:, None], N, 1).astype(np.float32))
        ret = (ret + o["rewards"][t, :, 0, 0]).astype(np.float32)
    np.testing.assert_array_equal(o["obs"][T], env.observe(), err_msg="final obs")
    np.testing.assert_array_equal(o["returns"], ret)
    if ms < T:
        assert done.all() and (o["dones_env"][ms - 1:] == 1).all()
        for t in range(ms, T + 1):          # the observation stays at the terminal one
            np.testing.assert_array_equal(o["obs"][t], o["obs"][ms])
    else:
        assert not done.any()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_exploration_exact(case):
    o = run_case(*case)
    acts = o["acts"]
    assert ((acts == 0) | (acts == 1)).all() and (acts.sum(-1) == 1).all()
    a = acts.argmax(-1)
    ex = o["explore"]
    np.testing.assert_array_equal(a[ex], o["rand_act"][ex])
    eps = case[4]
    assert ex.all() if eps == 1.0 else (not ex.any() if eps == 0.0 else (ex.any() and not ex.all()))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_q_values(case):
    o = run_case(*case)
    np.testing.assert_allclose(o["q"], o["q_ref"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(o["q"], o["q_lib"], rtol=RTOL, atol=ATOL)
    assert np.abs(o["q_ref"]).max() > 0.05      # the scaled head gives Q values well above the tolerance


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_greedy_no_exclusions(case):
    """Every greedy row: the oracle Q of the stored action is within twice the Q bound of the oracle maximum."""
    o = run_case(*case)
    q = o["q_ref"].astype(np.float64)
    a = o["acts"].argmax(-1)
    qa = np.take_along_axis(q, a[..., None], -1)[..., 0]
    slack = 2 * (RTOL * np.abs(q).max(-1) + ATOL)
    greedy = ~o["explore"]
    bad = greedy & (qa < q.max(-1) - slack)
    assert not bad.any(), (int(bad.sum()), float((q.max(-1) - qa)[bad].max()))
    if case[4] == 0.0:
        assert greedy.all()


def test_rng_stream():
    from minimarl.env import VecEnv
    from minimarl.offq_runner import OffQCollector
    E, N, T = 24, 3, 7
    tr = make_policy(N, T)
    env = VecEnv(E, N, max_steps=5, device="cuda")
    c1 = OffQCollector(env, tr, T, SEED)
    c2 = OffQCollector(VecEnv(E, N, max_steps=5, device="cuda"), tr, T, SEED)
    f1, r1, _ = c1.collect(1.0)
    first = {k: v.clone() for k, v in f1.items()}
    f2, r2, _ = c2.collect(1.0)
    for k in first:
        assert torch.equal(first[k], f2[k]), k
    assert torch.equal(r1, r2)
    # the first episode equals the cached case's draws at counter 0, the second one those at counter T
    a1 = first["acts"].argmax(-1).cpu().numpy()
    np.testing.assert_array_equal(a1[0], draws(SEED, 0, E, N, 5)[1])
    f1b, _, _ = c1.collect(1.0)
    a2 = f1b["acts"].argmax(-1).cpu().numpy()
    assert int(c1.counter.item()) == 2 * T
    np.testing.assert_array_equal(a2[0], draws(SEED, T, E, N, 5)[1])
    assert (a1 != a2).any()
    # the env handle's state plays no part: stepping it between collects changes nothing
    env.step(torch.zeros(E, N, dtype=torch.int32, device="cuda"))
    c3 = OffQCollector(env, tr, T, SEED)
    f3, _, _ = c3.collect(1.0)
    for k in first:
        assert torch.equal(first[k], f3[k]), k


def test_unsupported_dims_report_error():
    from minimarl._lib import lib
    from minimarl.env import VecEnv
    from minimarl.offq import OffQMix
    from minimarl.offq_runner import OffQCollector
    env = VecEnv(8, 2, max_steps=5, full_observable=True, device="cuda")      # D = 94: not built for this path
    tr = OffQMix(2, 94, 5, 5, 4, mixer="vdn", seed=1)
    assert lib().mm_offq_collect_supported(env.handle(), ctypes.byref(tr.dims), 8, 5) == 0
    with pytest.raises(RuntimeError, match="offq_collect: unsupported configuration"):
        OffQCollector(env, tr, 5, SEED)
    env2 = VecEnv(8, 3, max_steps=5, device="cuda")
    tr2 = OffQMix(2, 47, 5, 5, 4, mixer="vdn", seed=1)                         # agents differ from the env's
    with pytest.raises(RuntimeError, match="n_agents"):
        OffQCollector(env2, tr2, 5, SEED)


def make_buffer(N, T, size, same_share, prioritized=False):
    from minimarl.recbuf import PrioritizedRecReplayBuffer, RecReplayBuffer
    info = {"policy_0": {"obs_space": (47,), "share_obs_space": (N * 47,), "act_space": (5,)}}
    agents = {"policy_0": list(range(N))}
    if prioritized:
        return PrioritizedRecReplayBuffer(0.6, info, agents, size, T, same_share, False, device="cuda")
    return RecReplayBuffer(info, agents, size, T, same_share, False, device="cuda")


@pytest.mark.parametrize("same_share", [True, False])
@pytest.mark.parametrize("E,N", [(24, 3), (16, 8)])
def test_insert_collected(E, N, same_share):
    from minimarl.env import VecEnv
    from minimarl.offq_runner import OffQCollector
    T = 7
    tr = make_policy(N, T)
    col = OffQCollector(VecEnv(E, N, max_steps=5, device="cuda"), tr, T, SEED)
    fields, _, _ = col.collect(0.3)
    size = E + 5
    buf, buf_m = make_buffer(N, T, size, same_share), make_buffer(N, T, size, same_share)
    # a first insert of 9 episodes moves the ring cursor, the second wraps around the end of the ring
    part = {k: v[:, :9].contiguous() for k, v in fields.items()}
    share = fields["obs"].reshape(T + 1, E, 1, N * 47).expand(T + 1, E, N, N * 47).contiguous()
    pid = "policy_0"
    for f, n in ((part, 9), (fields, E)):
        idx = buf.insert_collected(n, f)
        sh = share[:, :n].contiguous()
        idx_m = buf_m.insert(n, {pid: f["obs"]}, {pid: sh}, {pid: f["acts"]}, {pid: f["rewards"]}, {pid: f["dones"]},
                             {pid: f["dones_env"]})
        np.testing.assert_array_equal(idx, idx_m)
    np.testing.assert_array_equal(idx, (9 + np.arange(E)) % size)
    assert len(buf) == len(buf_m) == size
    got = buf.sample(E, inds=idx)
    got_m = buf_m.sample(E, inds=idx)
    names = ("obs", "share_obs", "acts", "rewards", "dones", "dones_env")
    g = {k: got[i][pid] for i, k in enumerate(names)}
    for i, k in enumerate(names):
        assert torch.equal(g[k], got_m[i][pid]), k
    # sample layout: obs [N, T+1, B, D]; acts / rewards / dones [N, T, B, X]; dones_env [T, B, 1]
    assert torch.equal(g["obs"], fields["obs"].permute(2, 0, 1, 3))
    assert torch.equal(g["acts"], fields["acts"].permute(2, 0, 1, 3))
    assert torch.equal(g["rewards"], fields["rewards"].permute(2, 0, 1, 3))
    assert torch.equal(g["dones"], fields["dones"].permute(2, 0, 1, 3))
    assert torch.equal(g["dones_env"], fields["dones_env"])
    cat = col.share_obs                                          # [T+1, E, N*D]
    assert torch.equal(cat, torch.cat([fields["obs"][:, :, n] for n in range(N)], -1))
    if same_share:
        assert torch.equal(g["share_obs"], cat)
    else:
        assert torch.equal(g["share_obs"], cat.unsqueeze(0).expand(N, T + 1, E, N * 47))
    # the whole ring, the first insert's surviving slots included
    allidx = np.arange(size)
    for x, y in zip(buf.sample(size, inds=allidx)[:6], buf_m.sample(size, inds=allidx)[:6]):
        assert torch.equal(x[pid], y[pid])
    buf.check_errors()


def test_insert_concat_requires_concat_share_dim():
    from minimarl.recbuf import RecReplayBuffer
    info = {"policy_0": {"obs_space": (47,), "share_obs_space": (50,), "act_space": (5,)}}
    buf = RecReplayBuffer(info, {"policy_0": [0, 1]}, 4, 3, True, False, device="cuda")
    z = lambda *s: torch.zeros(*s, device="cuda")   # noqa: E731
    f = {"obs": z(4, 2, 2, 47), "acts": z(3, 2, 2, 5), "rewards": z(3, 2, 2, 1), "dones": z(3, 2, 2, 1),
         "dones_env": z(3, 2, 1)}
    with pytest.raises(RuntimeError, match="must be N \\* D"):
        buf.insert_collected(2, f)
    assert len(buf) == 0


@pytest.mark.parametrize("algo", ["qmix", "vdn"])
def test_runner(algo):
    from minimarl import OffQRunner
    from minimarl._lib import lib
    from minimarl.config import OffQTrainConfig
    err0 = lib().mm_last_error()
    cfg = OffQTrainConfig(algorithm_name=algo, n_envs=16, n_agents=2, episode_length=7, buffer_size=64, batch_size=8,
                          seed=3)
    r = OffQRunner(cfg)
    p0 = r.trainer.P.clone()
    r.warmup()
    assert len(r.buffer) == 16 and r.num_episodes_collected == 16 and r.total_train_steps == 0
    assert float(r.collector.eps.item()) == 1.0
    for it in range(3):
        steps = r.run()
        assert steps == (it + 2) * 16 * 7
    assert len(r.buffer) == 64
    assert (r.total_env_steps, r.num_episodes_collected, r.total_train_steps) == (4 * 16 * 7, 64, 3)
    assert r.last_train_episode == 64 and int(r.collector.counter.item()) == 4 * 7
    eps_want = np.float32(max(0.05, 1.0 - (1.0 - 0.05) / 50000 * (3 * 16 * 7)))
    assert float(r.collector.eps.item()) == eps_want
    info = r.train_infos[0]
    assert np.isfinite(float(info["loss"])) and np.isfinite(float(info["grad_norm"]))
    assert np.isfinite(float(r.env_info["average_episode_rewards"]))
    assert not torch.equal(p0, r.trainer.P) and torch.isfinite(r.trainer.P).all()
    assert not torch.equal(r.trainer.P, r.trainer.PT)            # soft target update: tau 0.005
    r.buffer.check_errors()
    # the library's error string is sticky: the run must not have set one
    assert lib().mm_last_error() == err0
    if err0 == b"":
        assert lib().mm_last_error() == b""


def test_graph_capture_replay_equals_eager():
    from minimarl.env import VecEnv
    from minimarl.offq_runner import OffQCollector
    from minimarl.qnet import graph_capture
    E, N, T = 40, 2, 7
    tr = make_policy(N, T)
    eager = OffQCollector(VecEnv(E, N, max_steps=5, device="cuda"), tr, T, SEED, with_q=True)
    cap = OffQCollector(VecEnv(E, N, max_steps=5, device="cuda"), tr, T, SEED, with_q=True)
    cap.collect(0.3)                       # first launch outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with graph_capture(g):
        cap.launch()
    for c0, eps in ((0, 0.3), (21, 0.6)):  # epsilon and the counter reach the replay through device memory
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
        ex = np.stack([draws(SEED, c0 + t, E, N, 5)[0] < np.float32(eps) for t in range(T)])
        ra = np.stack([draws(SEED, c0 + t, E, N, 5)[1] for t in range(T)])
        a = cap.fields["acts"].argmax(-1).cpu().numpy()
        np.testing.assert_array_equal(a[ex], ra[ex])
