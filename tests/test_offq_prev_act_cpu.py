"""CPU: the prev_act_inp variant of the episode QMix / VDN trainer at the ABI (no device is touched): the agent
layout is MGeo<D + 5, 64, 5>, the one new symbol is declared, exported and bound, every other user of mm_offq_dims
refuses the flag, and the Python front end refuses what it cannot serve."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

H, A, Ap = 64, 5, 8


def dims(D, flag=1, N=2):
    from minimarl._lib import MM_OFFQ_QMIX, OffqDims
    return OffqDims(N, D, H, A, MM_OFFQ_QMIX, N * D, 32, 64, flag)


@pytest.mark.parametrize("D", [3, 47, 94])
def test_param_counts_are_the_wide_layout(D):
    from minimarl._lib import c_i64, lib
    d, na, nm, nm0 = dims(D), c_i64(), c_i64(), c_i64()
    assert lib().mm_offq_param_counts(ctypes.byref(d), ctypes.byref(na), ctypes.byref(nm)) == 0
    Dp = (D + A + 3) // 4 * 4
    assert na.value == 2 * Dp + H * Dp + 3 * H + H * H + 3 * H + 6 * H * H + 6 * H + 2 * H + Ap * H + Ap
    assert lib().mm_offq_workspace_bytes(ctypes.byref(d), 7, 8) > 0
    d0, na0 = dims(D, 0), c_i64()
    assert lib().mm_offq_param_counts(ctypes.byref(d0), ctypes.byref(na0), ctypes.byref(nm0)) == 0
    assert na.value - na0.value == (Dp - (D + 3) // 4 * 4) * (2 + H) and nm.value == nm0.value   # the mixer has no actions


def test_symbol_declared_exported_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "minimarl.h")).read(), flags=re.S)
    from minimarl._lib import lib, symbols
    name = "mm_offq_q_values_prev"
    assert name in set(re.findall(r"\b(mm_[a-z0-9_]+)\s*\(", txt))
    assert hasattr(lib(), name) and name in symbols()


def test_c_side_refusals():
    from minimarl._lib import lib
    L, d = lib(), dims(47)
    assert L.mm_moffq_workspace_bytes(ctypes.byref(d), 8) == -1
    assert b"prev_act_inp" in L.mm_last_error()
    assert L.mm_offq_collect_supported(None, ctypes.byref(d), 4, 5) == 0
    assert L.mm_moffq_collect_supported(None, ctypes.byref(d), 4, 5) == 0
    for name in ("mm_offq_collect", "mm_offq_collect_switch", "mm_moffq_collect", "mm_moffq_collect_switch"):
        assert getattr(L, name)(None, ctypes.byref(d), None, None, 4, 5, None) == -22      # the flag is named first
        assert b"prev_act_inp" in L.mm_last_error(), name
    assert L.mm_offq_q_values(ctypes.byref(d), 8, 8, None, 8, None, 1, 1, 8, 1 << 20, None) == -22
    assert b"prev_act_inp" in L.mm_last_error() and b"mm_offq_q_values_prev" in L.mm_last_error()
    assert L.mm_offq_q_values_prev(ctypes.byref(dims(47, 0)), 8, 8, 8, None, 8, None, 1, 1, 8, 1 << 20, None) == -22


def test_python_side_refusals():
    import torch
    from minimarl.offq import OffQMix
    from minimarl.offq_runner import OffQCollector
    on = OffQMix(2, 47, A, 3, 2, mixer="vdn", device="cpu", prev_act_inp=True)
    off = OffQMix(2, 47, A, 3, 2, mixer="vdn", device="cpu")
    assert on.D == 47 and on.agent_shape("W1") == (H, 52) and on.agent_view("ln0_w").shape == (52,)
    assert off.agent_shape("W1") == (H, 47) and "prev_act_inp" not in off.checkpoint_tensors()[1]
    with pytest.raises(ValueError, match="prev_actions"):
        on.get_q_values(torch.zeros(4, 47))
    with pytest.raises(ValueError, match="prev_actions"):
        off.get_q_values(torch.zeros(4, 47), prev_actions=torch.zeros(4, A))
    with pytest.raises(NotImplementedError, match="prev_act_inp"):
        OffQCollector(None, on, 3, seed=1)
    ts, sc = on.checkpoint_tensors()
    assert sc["prev_act_inp"] is True
    with pytest.raises(ValueError, match="prev_act_inp"):
        off.restore_tensors(ts, sc)
