"""CPU: the Switch collector's ABI is declared, exported and bound, ``OffQTrainConfig.env``, and the bookkeeping of
the CPU restatement (tests/offq_switch_ref.py) that tests/test_gpu_offq_switch_collect.py relies on, the long cases'
preconditions included (they are facts of the counter RNG and oracle/switch.py, not of any kernel)."""
import functools
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from offq_collect_ref import draws
from offq_switch_ref import arrival_stats, collect_ref, ln0_variance, random_episodes
from oracle.switch import FINAL, SwitchSpec
from test_offq_collect_cpu import params

NEW_SYMBOLS = ("mm_offq_collect_switch", "mm_offq_collect_switch_supported")
SEED = 1234
# (E, N, T, max_steps) -> (envs with some but not all agents home early: count, asserted minimum;
#                          agents home early; envs with all agents home early: count, asserted minimum)
LONG = {(70, 2, 100, 100): (17, 10, 23, 3, 2), (50, 3, 100, 100): (21, 10, 25, 0, 0),
        (40, 4, 100, 100): (14, 8, 16, 0, 0)}


def test_switch_collect_symbols_declared_and_exported():
    txt = open(os.path.join(ROOT, "include", "minimarl.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(mm_[a-z0-9_]+)\s*\(", txt))
    from minimarl._lib import lib, symbols
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} not declared in include/minimarl.h"
        assert hasattr(lib(), name), f"{name} declared but not exported"
        assert name in symbols(), f"{name} has no ctypes signature"


def test_config_env_field():
    import dataclasses
    from minimarl.config import OffQTrainConfig
    assert OffQTrainConfig().env == "checkers"
    assert dataclasses.fields(OffQTrainConfig)[-1].name == "env"
    assert OffQTrainConfig(env="switch").env == "switch"


def test_trainer_dims_d3_accepted_by_abi():
    """D = 3 with the mixer state of 2, 3 and 4 agents (no device is touched)."""
    import ctypes
    from minimarl._lib import MM_OFFQ_QMIX, OffqDims, c_i64, lib
    for N in (2, 3, 4):
        d = OffqDims(N, 3, 64, 5, MM_OFFQ_QMIX, 3 * N, 32, 64)
        na, nm = c_i64(), c_i64()
        assert lib().mm_offq_param_counts(ctypes.byref(d), ctypes.byref(na), ctypes.byref(nm)) == 0
        H, Dp, Ap = 64, 4, 8       # the MGeo<3, 64, 5> flat layout
        assert na.value == 2 * Dp + H * Dp + 3 * H + H * H + 3 * H + 6 * H * H + 6 * H + 2 * H + Ap * H + Ap
        assert lib().mm_offq_workspace_bytes(ctypes.byref(d), 7, 8) > 0
    d = OffqDims(2, 4, 64, 5, MM_OFFQ_QMIX, 8, 32, 64)
    assert lib().mm_offq_workspace_bytes(ctypes.byref(d), 7, 8) == -1
    assert lib().mm_offq_param_counts(ctypes.byref(d), ctypes.byref(na), ctypes.byref(nm)) == -22
    assert b"3|47|94" in lib().mm_last_error()


@functools.lru_cache(maxsize=None)
def long_case(case):
    E, N, T, ms = case
    o = random_episodes(SEED, 0, E, N, T, ms, common_reward=False)
    for v in o.values():
        v.setflags(write=False)
    return o


def check_bookkeeping(o, N, T, ms, step_cost=np.float32(-0.01)):
    dones, de = o["dones"][..., 0], o["dones_env"][..., 0]
    assert (np.diff(dones, axis=0) >= 0).all() and (np.diff(de, axis=0) >= 0).all()       # monotone
    np.testing.assert_array_equal(de, dones.min(-1))                                        # the all-agent AND
    if ms <= T:
        assert (dones[ms - 1:] == 1).all()
    rew, stepped = o["agent_rewards"], o["stepped"]
    paid = rew == np.float32(5)
    assert (paid.sum(0) <= 1).all()                                                         # +5 once per agent
    # an agent is done before max_steps exactly from its +5 step on; its cell is then its target and never changes
    for t in range(min(T, ms - 1)):
        np.testing.assert_array_equal(dones[t] == 1, paid[:t + 1].any(0))
    for t in range(T):
        fin = dones[t] == 1
        np.testing.assert_array_equal(o["pos"][t + 1][fin], o["pos"][min(t + 2, T)][fin])
        home = paid[:t + 1].any(0)
        np.testing.assert_array_equal(o["pos"][t + 1][home], np.broadcast_to(FINAL[:N], home.shape + (2,))[home])
    # while the env runs every agent gets step_cost or +5, a finished one step_cost; afterwards 0 and a frozen obs
    assert ((rew == step_cost) | paid)[stepped].all() and (rew[~stepped] == 0).all()
    assert (o["rewards"][~stepped] == 0).all()
    np.testing.assert_array_equal(stepped[1:], de[:-1] == 0)
    for t in range(1, T):
        np.testing.assert_array_equal(o["obs"][t + 1][~stepped[t]], o["obs"][t][~stepped[t]])
    # the clock counts the steps taken
    np.testing.assert_array_equal(o["obs"][1:, :, 0, 2], (np.cumsum(stepped, 0) / ms).astype(np.float32))


@pytest.mark.parametrize("case", list(LONG), ids=lambda c: "E{}-N{}-T{}-ms{}".format(*c))
def test_long_case_preconditions(case):
    E, N, T, ms = case
    o = long_case(case)
    check_bookkeeping(o, N, T, ms)
    s = arrival_stats(o, ms)
    some, some_min, agents, all_, all_min = LONG[case]
    assert (s["some"], s["agents"], s["all"]) == (some, agents, all_)
    assert s["some"] >= some_min and s["all"] >= all_min
    de = o["dones_env"][..., 0]
    assert int((de[ms - 2] == 1).sum()) == all_           # these envs finish before max_steps: the post-done path
    dones = o["dones"][..., 0]
    assert (dones != de[:, :, None]).any()                 # per-agent dones differ from dones_env
    var = ln0_variance(o["obs"])
    assert var.min() < 1e-4                                # LayerNorm 0 rows with tiny or zero variance
    if case == (70, 2, 100, 100):
        assert (int((var < 1e-4).sum()), var.size, float(var.min())) == (93, 14140, 0.0)
    # the actions are the RNG's draws
    np.testing.assert_array_equal(o["acts"][3].argmax(-1), draws(SEED, 3, E, N, 5)[1])


def test_long_case_blocking_by_parked_agent():
    """In the N = 2 long case some mover is refused a cell that a finished agent holds."""
    E, N, T, ms = 70, 2, 100, 100
    o = long_case((E, N, T, ms))
    act, pos, dones = o["acts"].argmax(-1), o["pos"], o["dones"][..., 0]
    dr, dc = np.array([1, 0, -1, 0, 0]), np.array([0, -1, 0, 1, 0])
    blocked = 0
    for t in range(1, T):
        for e in range(E):
            if not o["stepped"][t, e]:
                continue
            for k in range(N):
                j = 1 - k
                if dones[t - 1, e, k] == 0 and dones[t - 1, e, j] == 1 and act[t, e, k] != 4:
                    tgt = pos[t, e, k] + (dr[act[t, e, k]], dc[act[t, e, k]])
                    if (tgt == pos[t, e, j]).all():
                        assert (pos[t + 1, e, k] == pos[t, e, k]).all()
                        blocked += 1
    assert blocked >= 1


@pytest.mark.parametrize("common", [False, True])
@pytest.mark.parametrize("E,N", [(12, 2), (9, 3)])
def test_ref_short_case(E, N, common):
    T, ms = 7, 5
    o = collect_ref(params(2, D=3), SwitchSpec(N, max_steps=ms), E, T, 0.3, seed=9, counter0=0, common_reward=common)
    check_bookkeeping(o, N, T, ms)
    assert o["explore"].any() and not o["explore"].all()
    a = o["acts"].argmax(-1)
    np.testing.assert_array_equal(a[o["explore"]], o["rand_act"][o["explore"]])
    np.testing.assert_array_equal(a[~o["explore"]], o["q"].argmax(-1)[~o["explore"]])
    assert (o["dones_env"][ms - 1:] == 1).all() and (o["dones_env"][:ms - 1] == 0).all()
    if common:
        np.testing.assert_array_equal(o["rewards"][:, :, 0, 0], o["rewards"][:, :, N - 1, 0])
        np.testing.assert_allclose(o["rewards"][:, :, 0, 0], o["agent_rewards"].sum(-1), rtol=1e-6, atol=1e-7)
    else:
        np.testing.assert_array_equal(o["rewards"][..., 0], o["agent_rewards"])
    np.testing.assert_array_equal(o["returns"], o["rewards"][:, :, 0, 0].sum(0, dtype=np.float32))
