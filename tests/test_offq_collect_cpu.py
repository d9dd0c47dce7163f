"""CPU: the offpolicy episode collector's ABI is declared and exported, and the properties of its CPU restatement
(tests/offq_collect_ref.py) that the GPU tests rely on."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from offq_collect_ref import collect_ref, draws
from oracle.env import EnvSpec

NEW_SYMBOLS = ("mm_offq_collect", "mm_offq_collect_supported", "mm_erb_insert_concat")


def test_collect_symbols_declared_and_exported():
    txt = open(os.path.join(ROOT, "include", "minimarl.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(mm_[a-z0-9_]+)\s*\(", txt))
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} not declared in include/minimarl.h"
    from minimarl._lib import LIB_PATH, lib, symbols
    if not os.path.exists(LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    L = lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), f"{name} declared but not exported"
        assert name in symbols(), f"{name} has no ctypes signature"


def test_python_surface():
    import minimarl
    from minimarl.config import OffQTrainConfig
    assert minimarl.OffQCollector.__name__ == "OffQCollector" and minimarl.OffQRunner.__name__ == "OffQRunner"
    c = OffQTrainConfig()
    # offpolicy/config.py defaults
    assert (c.episode_length, c.buffer_size, c.batch_size) == (100, 10000, 32)
    assert (c.epsilon_start, c.epsilon_finish, c.epsilon_anneal_time) == (1.0, 0.05, 50000)
    assert (c.num_random_episodes, c.train_interval_episode, c.hard_update_interval_episode) == (5, 1, 200)
    assert c.use_soft_update and c.use_common_reward and c.per_beta_start == 0.4 and c.n_envs >= 1
    from minimarl.offq_runner import DecayThenFlatSchedule
    s = DecayThenFlatSchedule(1.0, 0.05, 50000)
    assert s.eval(0) == 1.0 and s.eval(10 ** 7) == 0.05 and abs(s.eval(25000) - 0.525) < 1e-12


def params(seed, D=47, H=64, A=5, q_scale=10.0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    P = {"ln0_w": 1 + 0.1 * r(D), "ln0_b": 0.1 * r(D), "W1": r(H, D) * (2.0 / D) ** 0.5, "b1": 0.1 * r(H),
         "ln1_w": 1 + 0.1 * r(H), "ln1_b": 0.1 * r(H), "W2": r(H, H) * (2.0 / H) ** 0.5, "b2": 0.1 * r(H),
         "ln2_w": 1 + 0.1 * r(H), "ln2_b": 0.1 * r(H), "Wih": r(3 * H, H) / H ** 0.5, "Whh": r(3 * H, H) / H ** 0.5,
         "bih": 0.1 * r(3 * H), "bhh": 0.1 * r(3 * H), "lnr_w": 1 + 0.1 * r(H), "lnr_b": 0.1 * r(H),
         "Wo": q_scale * r(A, H) / H ** 0.5, "bo": 0.1 * r(A)}
    return P


E, N, T = 12, 3, 7
SPEC = EnvSpec(N, max_steps=5)


def test_ref_eps0_never_explores_and_is_greedy():
    o = collect_ref(params(1), SPEC, E, T, 0.0, seed=5, counter0=11, common_reward=False)
    assert not o["explore"].any()
    np.testing.assert_array_equal(o["acts"].argmax(-1), o["q"].argmax(-1))
    np.testing.assert_array_equal(o["acts"].sum(-1), 1.0)


def test_ref_eps1_takes_every_random_action():
    o = collect_ref(params(1), SPEC, E, T, 1.0, seed=5, counter0=11, common_reward=False)
    assert o["explore"].all()
    np.testing.assert_array_equal(o["acts"].argmax(-1), o["rand_act"])
    u, ra = draws(5, 11 + 3, E, N, 5)
    np.testing.assert_array_equal(o["rand_act"][3], ra)
    assert ((u >= 0) & (u < 1)).all() and len(np.unique(o["rand_act"])) == 5


@pytest.mark.parametrize("common", [False, True])
def test_ref_after_done(common):
    o = collect_ref(params(2), SPEC, E, T, 0.3, seed=9, counter0=0, common_reward=common)
    # max_steps 5 < T 7: every env is done from step 4 on (index 4 = the fifth step)
    assert (o["dones_env"][4:] == 1).all() and (o["dones"][4:] == 1).all()
    first = o["dones_env"][:, :, 0].argmax(0)            # first done step of each env
    for e in range(E):
        f = first[e]
        assert (o["dones_env"][:f, e] == 0).all()
        assert (o["rewards"][f + 1:, e] == 0).all() and (o["agent_rewards"][f + 1:, e] == 0).all()
        for t in range(f + 1, T + 1):
            np.testing.assert_array_equal(o["obs"][t, e], o["obs"][f + 1, e])
    if common:
        np.testing.assert_array_equal(o["rewards"][:, :, 0, 0], o["rewards"][:, :, N - 1, 0])
        np.testing.assert_allclose(o["rewards"][:, :, 0, 0], o["agent_rewards"].sum(-1), rtol=1e-6, atol=1e-7)
    else:
        np.testing.assert_array_equal(o["rewards"][..., 0], o["agent_rewards"])
    np.testing.assert_array_equal(o["returns"], o["rewards"][:, :, 0, 0].sum(0))
