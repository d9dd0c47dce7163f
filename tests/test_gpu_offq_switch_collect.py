"""GPU: the one-launch offpolicy episode collector on Switch (csrc/offq_collect.hip offq_collect_switch_kernel via
minimarl.offq_runner.OffQCollector), RecReplayBuffer.insert_collected at D = 3 and OffQRunner(env="switch") against
the CPU oracles (oracle/switch.py through tests/offq_switch_ref.py, oracle/offq.py).

Cases (E, N, T, max_steps); a block holds min(128 / N, 64) envs. Short: (40, 2, 7, 5) and (24, 3, 7, 5), one block
each, the post-done path for 2 steps in every env, at eps 0, 0.3, 1 and common / own reward. Long, eps 1 only (the
actions are then the RNG's draws whatever the net, so what they reach is a fact of the RNG and the oracle, asserted
below from the CPU replay): (70, 2, 100, 100), (50, 3, 100, 100), (40, 4, 100, 100), two blocks each with a short
last tile; they cover early arrival, a parked agent blocking a cell, per-agent dones, an env finishing before
max_steps (N = 2 only) and LayerNorm-0 rows of zero variance.

Q tolerance: the kernel's Q against the float64 oracle on the stored observations, in units of the project's
collector bound: u(x) = max |x - q64| / (1e-4 |q64| + 1e-5), required u(q_hip) <= max(1, 8 u(q32)) with q32 the
float32 oracle on the same inputs (8 = RATIO of tests/test_gpu_offq_shapes.py). LayerNorm 0 over three nearly equal
features multiplies rounding by up to 1 / sqrt(1e-5): the fixed bound does not hold for the float32 oracle itself
over the 100-step cases. Policy: random_agent(7, 3) with the Q head scaled by 10 (max |Q| about 50).
Measured, MI355X, u(q_hip) / u(get_q_values) / u(q32) -> bound, per shape (common and own reward give the same Q):
  E40-N2-T7    eps 0: 0.11 / 0.11 / 0.08 -> 1     eps 0.3: 0.43 / 0.39 / 1.26 -> 10.1   eps 1: 0.71 / 0.66 / 0.50 -> 4.0
  E24-N3-T7    eps 0: 0.11 / 0.11 / 0.08 -> 1     eps 0.3: 0.43 / 0.14 / 1.26 -> 10.1   eps 1: 0.71 / 0.66 / 0.50 -> 4.0
  E70-N2-T100  eps 1: 1.26 / 1.50 / 1.56 -> 12.5
  E50-N3-T100  eps 1: 2.29 / 2.51 / 2.81 -> 22.5
  E40-N4-T100  eps 1: 2.58 / 1.97 / 1.89 -> 15.1
Worst u(q_hip) / u(q32) per case: 1.44 (the eps 0 short cases), 1.42 (eps 1 short), 1.37 (E40-N4-T100), below 1
elsewhere. The collector never needed more than 2.6 units of the fixed bound, the float32 oracle up to 2.8.
"""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

from offq_cases import random_agent
from offq_collect_ref import draws
from offq_switch_cases import q_units
from offq_switch_ref import arrival_stats, ln0_variance, replay
from oracle import offq as ref
from oracle.switch import SwitchSpec
from test_gpu_offq_shapes import RATIO, agent_sd

pytestmark = pytest.mark.gpu

SEED, COUNTER0 = 1234, 0
RTOL, ATOL = 1e-4, 1e-5          # the collector bound of tests/test_gpu_offq_collect.py: the unit of u
SHORT = [(40, 2, 7, 5), (24, 3, 7, 5)]
# (E, N, T, max_steps) -> minimum of (envs with some but not all agents home early, envs with all agents home early)
LONG = {(70, 2, 100, 100): (10, 2), (50, 3, 100, 100): (10, 0), (40, 4, 100, 100): (8, 0)}
CASES = [s + (eps, common) for s, eps, common in itertools.product(SHORT, (0.0, 0.3, 1.0), (True, False))]
CASES += [s + (1.0, common) for s, common in itertools.product(LONG, (True, False))]


def make_policy(N, T, mixer="vdn", seed=7):
    """OffQMix with random_agent(seed, 3) as both nets and the Q head scaled by 10: no bias or LayerNorm parameter
    sits at its 0 / 1 default and greedy actions are not all near-ties."""
    from minimarl.offq import OffQMix
    tr = OffQMix(N, 3, 5, T, 8, mixer=mixer, seed=seed)
    P = random_agent(seed, 3)
    P["Wo"] = P["Wo"] * 10.0
    m_sd = {k: v.cpu().numpy() for k, v in tr.state_dict()[1].items()} if mixer == "qmix" else None
    tr.load_reference_state(agent_sd(P), m_sd)
    return tr


def make_env(E, N, max_steps, **kw):
    from minimarl.env import SwitchVecEnv
    return SwitchVecEnv(E, N, max_steps=max_steps, device="cuda", **kw)


@functools.lru_cache(maxsize=None)
def run_case(E, N, T, max_steps, eps, common):
    """One collect; everything the checks need as host arrays (computed once, shared, not modified)."""
    from minimarl.offq_runner import OffQCollector
    tr = make_policy(N, T)
    col = OffQCollector(make_env(E, N, max_steps), tr, T, SEED, common_reward=common, with_q=True)
    fields, returns, acts = col.collect(eps)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in fields.items()}
    out["q"], out["returns"] = col.q.cpu().numpy(), returns.cpu().numpy()
    obs_seq = fields["obs"][:T].reshape(T, E * N, 3)
    out["q_lib"] = tr.get_q_values(obs_seq)[0].reshape(T, E, N, 5).cpu().numpy()
    P = ref.agent_from_state(tr.state_dict()[0], prefix="")
    with torch.no_grad():
        out["q64"] = ref.agent_q_seq(P, obs_seq.cpu(), dtype=torch.float64)[0].numpy().reshape(T, E, N, 5)
        out["q32"] = ref.agent_q_seq(P, obs_seq.cpu())[0].numpy().reshape(T, E, N, 5)
    dr = [draws(SEED, COUNTER0 + t, E, N, 5) for t in range(T)]
    out["explore"] = np.stack([u < np.float32(eps) for u, _ in dr])
    out["rand_act"] = np.stack([ra for _, ra in dr])
    # the CPU replay of the stored actions from reset
    act = out["acts"].argmax(-1)
    cpu = replay(SwitchSpec(N, max_steps=max_steps), E, lambda t, obs: act[t], T, common)
    out.update({"cpu_" + k: v for k, v in cpu.items()})
    for v in out.values():
        v.setflags(write=False)
    return out


def case_id(c):
    return "E{}-N{}-T{}-ms{}-eps{}-{}".format(*c[:5], "common" if c[5] else "own")


def q_bound(o):
    """(u(q32), the bound on u(q_hip)) of a case."""
    u32 = q_units(o["q32"], o["q64"], RTOL, ATOL)
    return u32, max(1.0, RATIO * u32)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_env_exact(case):
    """Replay the stored actions through the oracle env from reset: every field bit-equal."""
    E, N, T, ms, eps, common = case
    o = run_case(*case)
    for k in ("obs", "rewards", "dones", "dones_env", "returns"):
        np.testing.assert_array_equal(o[k], o["cpu_" + k], err_msg=k)
    de = o["dones_env"][..., 0]
    assert (o["rewards"][~o["cpu_stepped"]] == 0).all()
    np.testing.assert_array_equal(de, o["dones"][..., 0].min(-1))
    if ms < T:
        assert (de[ms - 1:] == 1).all() and (de[:ms - 1] == 0).all()
        for t in range(ms, T + 1):          # the observation, its clock included, stays at the terminal one
            np.testing.assert_array_equal(o["obs"][t], o["obs"][ms])
        assert (o["obs"][ms, :, :, 2] == 1.0).all()
    if (E, N, T, ms) in LONG:
        assert eps == 1.0
        s = arrival_stats({"agent_rewards": o["cpu_agent_rewards"]}, ms)
        some_min, all_min = LONG[E, N, T, ms]
        assert s["some"] >= some_min and s["all"] >= all_min, s
        assert int((de[ms - 2] == 1).sum()) == s["all"]               # these envs run the post-done path
        assert (o["dones"][..., 0] != de[:, :, None]).any()           # per-agent dones differ from dones_env
        assert ln0_variance(o["obs"]).min() < 1e-4                    # degenerate LayerNorm-0 rows
        if not common:
            assert int((o["rewards"] == 5).sum()) == int((o["cpu_agent_rewards"] == 5).sum()) >= s["agents"]


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
    u32, bound = q_bound(o)
    u, ulib = q_units(o["q"], o["q64"], RTOL, ATOL), q_units(o["q_lib"], o["q64"], RTOL, ATOL)
    print(f"{case_id(case)}: u(q_hip) {u:.3g} u(q_lib) {ulib:.3g} u(q32) {u32:.3g} bound {bound:.3g} "
          f"max |q64| {np.abs(o['q64']).max():.3g}")
    assert u <= bound and ulib <= bound
    assert np.abs(o["q64"]).max() > 0.05      # the scaled head gives Q values well above the tolerance


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_greedy_no_exclusions(case):
    """Every greedy row: the oracle Q of the stored action is within twice the Q bound of the oracle maximum."""
    o = run_case(*case)
    q = o["q64"]
    a = o["acts"].argmax(-1)
    qa = np.take_along_axis(q, a[..., None], -1)[..., 0]
    slack = 2 * q_bound(o)[1] * (RTOL * np.abs(q).max(-1) + ATOL)
    greedy = ~o["explore"]
    bad = greedy & (qa < q.max(-1) - slack)
    assert not bad.any(), (int(bad.sum()), float((q.max(-1) - qa)[bad].max()))
    if case[4] == 0.0:
        assert greedy.all()


def test_rng_stream():
    from minimarl.offq_runner import OffQCollector
    E, N, T = 24, 3, 7
    tr = make_policy(N, T)
    env = make_env(E, N, 5)
    c1 = OffQCollector(env, tr, T, SEED)
    c2 = OffQCollector(make_env(E, N, 5), tr, T, SEED)
    f1, r1, _ = c1.collect(1.0)
    first = {k: v.clone() for k, v in f1.items()}
    f2, r2, _ = c2.collect(1.0)
    for k in first:
        assert torch.equal(first[k], f2[k]), k
    assert torch.equal(r1, r2)
    # the first episode equals the draws at counter 0, the second one those at counter T
    a1 = first["acts"].argmax(-1).cpu().numpy()
    np.testing.assert_array_equal(a1[0], draws(SEED, 0, E, N, 5)[1])
    f1b, _, _ = c1.collect(1.0)
    a2 = f1b["acts"].argmax(-1).cpu().numpy()
    assert int(c1.counter.item()) == 2 * T
    np.testing.assert_array_equal(a2[0], draws(SEED, T, E, N, 5)[1])
    assert (a1 != a2).any()
    # the env handle's state plays no part: stepping it between collects changes nothing, and is not changed
    env.step(torch.ones(E, N, dtype=torch.int32, device="cuda"))
    before = env.get_state()
    c3 = OffQCollector(env, tr, T, SEED)
    f3, _, _ = c3.collect(1.0)
    for k in first:
        assert torch.equal(first[k], f3[k]), k
    for x, y in zip(before, env.get_state()):
        np.testing.assert_array_equal(x, y)
    assert before[2].tolist() == [1] * E


def test_unsupported_configurations_report_error():
    from minimarl._lib import lib
    from minimarl.env import VecEnv
    from minimarl.offq import OffQMix
    from minimarl.offq_runner import OffQCollector
    sup = lib().mm_offq_collect_switch_supported
    tr = OffQMix(2, 3, 5, 5, 4, mixer="vdn", seed=1)
    ok = make_env(8, 2, 5)
    assert sup(ok.handle(), ctypes.byref(tr.dims), 8, 5) == 1
    assert sup(ok.handle(), ctypes.byref(tr.dims), 0, 5) == 0 and sup(ok.handle(), ctypes.byref(tr.dims), 8, 0) == 0
    assert sup(ok.handle(), ctypes.byref(tr.dims), 8, 65537) == 0
    full = make_env(8, 2, 5, full_observable=True)                # D = 6: not built for this path
    tr6 = OffQMix(2, 3, 5, 5, 4, mixer="vdn", seed=1)
    assert sup(full.handle(), ctypes.byref(tr6.dims), 8, 5) == 0
    with pytest.raises(RuntimeError, match="offq_collect_switch: unsupported configuration.*full_observable"):
        OffQCollector(full, tr6, 5, SEED)
    noclock = make_env(8, 2, 5, clock=False)                      # D = 2
    with pytest.raises(RuntimeError, match="offq_collect_switch: unsupported configuration.*clock"):
        OffQCollector(noclock, tr, 5, SEED)
    with pytest.raises(RuntimeError, match="n_agents"):          # agents differ from the env's
        OffQCollector(make_env(8, 3, 5), tr, 5, SEED)
    tr47 = OffQMix(2, 47, 5, 5, 4, mixer="vdn", seed=1)           # a Checkers policy
    assert sup(ok.handle(), ctypes.byref(tr47.dims), 8, 5) == 0
    with pytest.raises(RuntimeError, match="offq_collect_switch: unsupported configuration.*D 3"):
        OffQCollector(ok, tr47, 5, SEED)
    # and the Checkers entry point still rejects a Switch policy
    with pytest.raises(RuntimeError, match="offq_collect: unsupported configuration"):
        OffQCollector(VecEnv(8, 2, max_steps=5, device="cuda"), tr, 5, SEED)


def make_buffer(N, T, size, same_share, prioritized=False):
    from minimarl.recbuf import PrioritizedRecReplayBuffer, RecReplayBuffer
    info = {"policy_0": {"obs_space": (3,), "share_obs_space": (N * 3,), "act_space": (5,)}}
    agents = {"policy_0": list(range(N))}
    if prioritized:
        return PrioritizedRecReplayBuffer(0.6, info, agents, size, T, same_share, False, device="cuda")
    return RecReplayBuffer(info, agents, size, T, same_share, False, device="cuda")


@pytest.mark.parametrize("same_share", [True, False])
@pytest.mark.parametrize("E,N", [(24, 3), (21, 4)])
def test_insert_collected(E, N, same_share):
    from minimarl.offq_runner import OffQCollector
    T = 7
    tr = make_policy(N, T)
    col = OffQCollector(make_env(E, N, 5), tr, T, SEED)
    fields, _, _ = col.collect(0.3)
    size = E + 5
    buf, buf_m = make_buffer(N, T, size, same_share), make_buffer(N, T, size, same_share)
    # a first insert of 9 episodes moves the ring cursor, the second wraps around the end of the ring
    part = {k: v[:, :9].contiguous() for k, v in fields.items()}
    share = fields["obs"].reshape(T + 1, E, 1, N * 3).expand(T + 1, E, N, N * 3).contiguous()
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
    for k in ("obs", "acts", "rewards", "dones"):
        assert torch.equal(g[k], fields[k].permute(2, 0, 1, 3)), k
    assert torch.equal(g["dones_env"], fields["dones_env"])
    cat = col.share_obs                                          # [T+1, E, N*D]: a view, not a copy
    assert cat.data_ptr() == fields["obs"].data_ptr()
    assert torch.equal(cat, torch.cat([fields["obs"][:, :, n] for n in range(N)], -1))
    if same_share:
        assert torch.equal(g["share_obs"], cat)
    else:
        assert torch.equal(g["share_obs"], cat.unsqueeze(0).expand(N, T + 1, E, N * 3))
    allidx = np.arange(size)
    for x, y in zip(buf.sample(size, inds=allidx)[:6], buf_m.sample(size, inds=allidx)[:6]):
        assert torch.equal(x[pid], y[pid])
    buf.check_errors()


@pytest.mark.parametrize("algo", ["qmix", "vdn"])
def test_runner(algo):
    from minimarl import OffQRunner
    from minimarl._lib import lib
    from minimarl.config import OffQTrainConfig
    from minimarl.env import SwitchVecEnv
    err0 = lib().mm_last_error()
    cfg = OffQTrainConfig(env="switch", algorithm_name=algo, n_envs=16, episode_length=7, buffer_size=64, batch_size=8)
    r = OffQRunner(cfg)
    assert isinstance(r.env, SwitchVecEnv) and r.env.obs_dim == 3 and r.trainer.D == 3 and r.trainer.S == 6
    assert r.env.cfg.max_steps == 7 and r.env.cfg.clock == 1 and r.env.cfg.full_observable == 0
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


def test_graph_capture_replay_equals_eager():
    from minimarl.offq_runner import OffQCollector
    from minimarl.qnet import graph_capture
    E, N, T = 40, 2, 7
    tr = make_policy(N, T)
    eager = OffQCollector(make_env(E, N, 5), tr, T, SEED, with_q=True)
    cap = OffQCollector(make_env(E, N, 5), tr, T, SEED, with_q=True)
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
        assert ex.any() and not ex.all()
