"""GPU: the one-launch feed-forward transition collector (csrc/moffq_collect.hip via minimarl.moffq_runner), its write
into a replay ring and MOffQRunner, against the CPU oracles (oracle/env.py, oracle/switch.py, tests/moffq_ref.py).

Cases (env, E, N, T, max_steps, eps, common reward); a block holds min(128 / N, 64) envs, so (70, 2) and (70, 4) are
two blocks with a short last tile. T 7 with max_steps 3 resets every env twice inside the window, T 5 with max_steps
100 resets none. Q bound: rtol 1e-4 / atol 1e-5, the project's bound for this exact-f32 MFMA forward
(tests/test_gpu_offq_collect.py)."""
import functools

import numpy as np
import pytest
import torch

from moffq_ref import AGENT_KEYS, agent_q
from offq_collect_ref import common_sum, draws
from oracle.env import EnvSpec, VecEnvOracle
from oracle.switch import SwitchOracle, SwitchSpec

pytestmark = pytest.mark.gpu

SEED = 1234
RTOL, ATOL = 1e-4, 1e-5
SHAPES = [("checkers", E, N, T, ms) for E, N in ((40, 2), (24, 3), (16, 8), (70, 2)) for T, ms in ((7, 3), (5, 100))]
SHAPES += [("switch", 40, 2, 7, 3), ("switch", 70, 4, 7, 3)]
CASES = [s + ((0.3, 0.0, 1.0)[i % 3], i % 2 == 0) for i, s in enumerate(SHAPES)]
FIELDS = ("obs", "next_obs", "acts", "rewards", "dones", "dones_env", "valid_transition")


def make_policy(N, D, mixer="vdn", seed=7):
    """MOffQMix(seed=...) with the Q head scaled by 10 (greedy actions are not all near-ties) and every bias and
    LayerNorm parameter moved off its 0 / 1 default, so each of them shows in Q."""
    from minimarl.moffq import MOffQMix
    tr = MOffQMix(N, D, 5, mixer=mixer, seed=seed)
    g = torch.Generator().manual_seed(seed + 100)
    tr.agent_view("Wo").mul_(10.0)
    for k in AGENT_KEYS:
        v = tr.agent_view(k)
        if v.dim() == 1:
            v.add_((0.1 * torch.randn(v.shape, generator=g)).to(v.device))
    tr.hard_target_updates()
    return tr


def make_env(kind, E, N, ms):
    from minimarl.env import SwitchVecEnv, VecEnv
    return (SwitchVecEnv if kind == "switch" else VecEnv)(E, N, max_steps=ms, device="cuda")


def replay(kind, E, N, T, ms, act, common):
    """The window with the actions given, reset-on-done, through the oracle env: the fields as [T, E, ...]."""
    sw = kind == "switch"
    env = SwitchOracle(SwitchSpec(N, max_steps=ms), E) if sw else VecEnvOracle(EnvSpec(N, max_steps=ms), E)
    observe = env.obs if sw else env.observe
    out = {k: [] for k in FIELDS}
    ret, nd = np.zeros(E, np.float32), np.zeros(E, np.int32)
    for t in range(T):
        out["obs"].append(observe())
        out["valid_transition"].append(1.0 - env.adone if sw else np.ones((E, N)))
        if sw:
            nobs, rew, adone, done = env.step(act[t])
        else:
            nobs, rew, done = env.step(act[t])
            adone = np.repeat(done[:, None], N, 1)
        rew = np.repeat(common_sum(rew)[:, None], N, 1) if common else rew
        for k, v in (("next_obs", nobs), ("rewards", rew), ("dones", adone), ("dones_env", done)):
            out[k].append(v)
        ret, nd = (ret + rew[:, 0]).astype(np.float32), nd + done
        env.reset_envs(done)
    res = {k: np.stack(v).astype(np.float32) for k, v in out.items() if v}
    return dict(res, returns=ret, n_done=nd)


@functools.lru_cache(maxsize=None)
def run_case(kind, E, N, T, ms, eps, common):
    """One window into the staging tensors and the same window into a ring; host arrays, computed once, read-only."""
    from minimarl.mlpbuf import MlpReplayBuffer
    from minimarl.moffq_runner import MOffQCollector
    D, n = (3 if kind == "switch" else 47), T * E
    tr = make_policy(N, D)
    col = MOffQCollector(make_env(kind, E, N, ms), tr, T, SEED, common_reward=common, with_q=True)
    fields, returns = col.collect(eps)
    out = {k: v.cpu().numpy() for k, v in fields.items()}
    out.update(q=col.q.cpu().numpy(), returns=returns.cpu().numpy(), n_done=col.n_done.cpu().numpy())
    obs = fields["obs"].reshape(n * N, D)
    out["q_lib"] = tr.get_q_values(obs).reshape(n, N, 5).cpu().numpy()
    P = {k: tr.agent_view(k).double().cpu() for k in AGENT_KEYS}
    out["q_ref"] = agent_q(P, obs.double().cpu()).numpy().reshape(n, N, 5)
    dr = [draws(SEED, t, E, N, 5) for t in range(T)]
    out["explore"] = np.stack([u < np.float32(eps) for u, _ in dr]).reshape(n, N)
    out["rand_act"] = np.stack([ra for _, ra in dr]).reshape(n, N)
    # the same window written in place into a ring whose cursor stands 10 slots before the end
    size = n + 5
    info = {"policy_0": {"obs_space": (D,), "share_obs_space": (N * D,), "act_space": (5,)}}
    buf = MlpReplayBuffer(info, {"policy_0": list(range(N))}, size, True, False, device="cuda", store_share=False)
    rows = {k: fields[k].shape[1:] for k in FIELDS}
    z = lambda k: torch.zeros((size - 10,) + tuple(rows.get(k, (N * D,))), device="cuda")   # noqa: E731
    buf.insert(size - 10, *[z(k) for k in ("obs", "s", "acts", "rewards", "next_obs", "s", "dones", "dones_env",
                                           "valid_transition")])
    col.counter.zero_()
    out["slots"] = buf.insert_collected(col)
    got = buf.sample(n, inds=out["slots"])
    names = ("obs", "share_obs", "acts", "rewards", "next_obs", "next_share_obs", "dones", "dones_env",
             "valid_transition")
    for k, x in zip(names, got[:9]):
        x = x["policy_0"].cpu().numpy()
        out["ring_" + k] = x.transpose(1, 0, 2) if x.ndim == 3 else x
    out["ring_len"], out["ring_cur"] = np.int64(len(buf)), np.int64(buf.current_i)
    buf.check_errors()
    for v in out.values():
        v.setflags(write=False)
    return out


def case_id(c):
    return "{}-E{}-N{}-T{}-ms{}-eps{}-{}".format(*c[:6], "common" if c[6] else "own")


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_env_exact(case):
    """Replay the stored actions through the oracle env with reset-on-done: every field bit-equal."""
    kind, E, N, T, ms, eps, common = case
    o = run_case(*case)
    cpu = replay(kind, E, N, T, ms, o["acts"].argmax(-1).reshape(T, E, N), common)
    for k in FIELDS[:2] + FIELDS[3:]:
        np.testing.assert_array_equal(o[k].reshape(cpu[k].shape), cpu[k], err_msg=k)
    np.testing.assert_array_equal(o["returns"], cpu["returns"])
    np.testing.assert_array_equal(o["n_done"], cpu["n_done"])
    de = o["dones_env"].reshape(T, E)
    if ms < T:      # every env resets at steps ms - 1 and 2 ms - 1: terminal next_obs, the reset obs in the next transition
        assert (o["n_done"] == T // ms).all() and (de[ms - 1] == 1).all() and (de[:ms - 1] == 0).all()
        obs, nobs = o["obs"].reshape(T, E, N, -1), o["next_obs"].reshape(T, E, N, -1)
        np.testing.assert_array_equal(obs[ms], obs[0])
        assert (nobs[ms - 1] != obs[ms]).any()
        np.testing.assert_array_equal(nobs[:ms - 1], obs[1:ms])
    else:
        assert not de.any() and not o["n_done"].any()
    if kind == "switch":
        np.testing.assert_array_equal(de, o["dones"].reshape(T, E, N).min(-1))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_exploration_exact(case):
    o = run_case(*case)
    acts, ex, eps = o["acts"], o["explore"], case[5]
    assert ((acts == 0) | (acts == 1)).all() and (acts.sum(-1) == 1).all()
    np.testing.assert_array_equal(acts.argmax(-1)[ex], o["rand_act"][ex])
    assert ex.all() if eps == 1.0 else (not ex.any() if eps == 0.0 else (ex.any() and not ex.all()))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_q_values_and_greedy_rows(case):
    """Q against the fp64 forward and the library's own; every greedy row's stored action lies within twice the Q
    bound of the reference maximum, no exclusions."""
    o = run_case(*case)
    q = o["q_ref"]
    err = np.abs(o["q"] - q) / (RTOL * np.abs(q) + ATOL)
    print(f"{case_id(case)}: max |q - q64| / bound {err.max():.3g}, max |q64| {np.abs(q).max():.3g}")
    np.testing.assert_allclose(o["q"], q, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(o["q_lib"], q, rtol=RTOL, atol=ATOL)
    assert np.abs(q).max() > 0.05      # the scaled head gives Q values well above the tolerance
    qa = np.take_along_axis(q, o["acts"].argmax(-1)[..., None], -1)[..., 0]
    bad = ~o["explore"] & (qa < q.max(-1) - 2 * (RTOL * np.abs(q).max(-1) + ATOL))
    assert not bad.any(), (int(bad.sum()), float((q.max(-1) - qa)[bad].max()))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_ring_equals_staging(case):
    """The window written at first = size - 10 of a ring of T E + 5 slots, gathered by slot, is the staging run."""
    kind, E, N, T = case[:4]
    o, n = run_case(*case), T * E
    size = n + 5
    np.testing.assert_array_equal(o["slots"], (size - 10 + np.arange(n)) % size)
    assert int(o["ring_len"]) == size and int(o["ring_cur"]) == n - 10
    for k in FIELDS:
        np.testing.assert_array_equal(o["ring_" + k], o[k], err_msg=k)
    np.testing.assert_array_equal(o["ring_share_obs"], o["obs"].reshape(n, -1))
    np.testing.assert_array_equal(o["ring_next_share_obs"], o["next_obs"].reshape(n, -1))


@pytest.mark.parametrize("leaf_mode", ["slots", "reference"])
@pytest.mark.parametrize("kind", ["checkers", "switch"])
def test_collect_into_ring_with_cursor_at_size(kind, leaf_mode):
    """buffer_size = 2 T E: the second window leaves the cursor at current_i = size, the third starts at slot 0."""
    from minimarl.mlpbuf import PrioritizedMlpReplayBuffer
    from minimarl.moffq_runner import MOffQCollector
    E, N, T, ms = 24, 3, 7, 3
    D, n = (3 if kind == "switch" else 47), T * E
    col = MOffQCollector(make_env(kind, E, N, ms), make_policy(N, D), T, SEED)
    info = {"policy_0": {"obs_space": (D,), "share_obs_space": (N * D,), "act_space": (5,)}}
    buf = PrioritizedMlpReplayBuffer(0.6, info, {"policy_0": list(range(N))}, 2 * n, True, False, device="cuda",
                                     leaf_mode=leaf_mode, store_share=False)
    col.set_epsilon(0.3)
    for w in range(3):
        slots = buf.insert_collected(col)
        np.testing.assert_array_equal(slots, (w % 2) * n + np.arange(n))
        assert buf.current_i == (w % 2 + 1) * n and len(buf) == min(w + 1, 2) * n
    leaves = buf.trees()[0][buf.trees()[0].size // 2:][:2 * n]
    want = np.ones(2 * n) if leaf_mode == "slots" else np.isin(np.arange(2 * n), (0, n)).astype(np.float64)
    np.testing.assert_array_equal(leaves, want)
    got = buf.sample_inds(torch.as_tensor(slots).cuda())
    col.counter.fill_(2 * T)                # the third window again, into the staging tensors
    fields, _ = col.collect(0.3)
    for i, k in ((0, "obs"), (2, "acts"), (3, "rewards"), (4, "next_obs"), (6, "dones"), (8, "valid_transition")):
        assert torch.equal(got[i]["policy_0"], fields[k].transpose(0, 1)), k
    assert torch.equal(got[7]["policy_0"], fields["dones_env"])
    assert torch.equal(got[1]["policy_0"], fields["obs"].reshape(n, N * D))
    buf.check_errors()


@pytest.mark.parametrize("kind", ["checkers", "switch"])
def test_graph_capture_replay_equals_eager(kind):
    from minimarl.moffq_runner import MOffQCollector
    from minimarl.qnet import graph_capture
    E, N, T, ms = 40, 2, 7, 3
    tr = make_policy(N, 3 if kind == "switch" else 47)
    eager, cap = (MOffQCollector(make_env(kind, E, N, ms), tr, T, SEED, with_q=True) for _ in range(2))
    cap.collect(0.3)                       # first launch outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with graph_capture(g):
        cap.launch()
    for c0, eps in ((0, 0.3), (21, 0.6), (5, 1.0)):   # epsilon and the counter reach the replay through device memory
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
        assert int(cap.counter.item()) == c0 + T
        a = cap.fields["acts"].argmax(-1).cpu().numpy().reshape(T, E, N)
        for t in range(T):
            u, ra = draws(SEED, c0 + t, E, N, 5)
            np.testing.assert_array_equal(a[t][u < np.float32(eps)], ra[u < np.float32(eps)])


@pytest.mark.parametrize("algo", ["mqmix", "mvdn"])
@pytest.mark.parametrize("env", ["checkers", "switch"])
def test_runner(env, algo):
    from minimarl import MOffQRunner
    from minimarl._lib import lib
    from minimarl.config import OffQTrainConfig
    err0 = lib().mm_last_error()
    r = MOffQRunner(OffQTrainConfig(env=env, algorithm_name=algo, n_envs=16, n_agents=2, episode_length=7,
                                    buffer_size=256, batch_size=8, seed=3))
    p0 = r.trainer.P.clone()
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
    assert np.isfinite(float(info["loss"])) and np.isfinite(float(info["grad_norm"]))
    assert np.isfinite(float(r.env_info["average_episode_rewards"]))
    assert not torch.equal(p0, r.trainer.P) and torch.isfinite(r.trainer.P).all()
    s, _ = r.buffer.trees()
    assert (s[256:512] > 0).all()           # leaf_mode slots: every written slot holds mass
    for _ in range(13):                     # the 16th window ends at the ring's end (16 x 112 = 7 x 256), the 17th starts over
        r.run()
    assert r.buffer.current_i == 112 and r.total_train_steps == 16 and torch.isfinite(r.trainer.P).all()
    r.buffer.check_errors()
    assert lib().mm_last_error() == err0    # the library's error string is sticky: the run must not have set one
