"""CPU: the C ABI of the MADDPG / MATD3 trainer (mm_maddpg_*) is declared in include/minimarl.h, exported by the
library and bound by minimarl._lib; the public names resolve without a GPU."""
import os
import re

import pytest

from conftest import ROOT

WANT = {"mm_maddpg_param_counts", "mm_maddpg_workspace_bytes", "mm_maddpg_critic_grad", "mm_maddpg_actor_grad",
        "mm_maddpg_logits", "mm_maddpg_gumbel"}


def test_symbols_declared_bound_and_exported():
    from minimarl._lib import LIB_PATH, lib, symbols
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "minimarl.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(mm_maddpg[a-z0-9_]*)\s*\(", txt)) == WANT
    assert WANT <= set(symbols())
    if not os.path.exists(LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    for name in WANT:
        assert hasattr(lib(), name), name


def test_public_names():
    import minimarl
    assert "MADDPG" in minimarl.__all__ and minimarl.MADDPG.__name__ == "MADDPG"
    with pytest.raises(ValueError):
        minimarl.MADDPG(2, 47, 5, use_popart=True, device="cpu")
