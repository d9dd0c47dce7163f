"""CPU: the C ABI of the recurrent MADDPG / MATD3 trainer (mm_rmaddpg_*) is declared under include/, exported by the
library and bound by minimarl._lib; the public names resolve without a GPU."""
import os
import re

import pytest

from conftest import ROOT

WANT = {"mm_rmaddpg_param_counts", "mm_rmaddpg_workspace_bytes", "mm_rmaddpg_critic_grad", "mm_rmaddpg_actor_grad",
        "mm_rmaddpg_step"}


def test_symbols_declared_bound_and_exported():
    from minimarl._lib import LIB_PATH, lib, symbols
    txt = open(os.path.join(ROOT, "include", "minimarl_rmaddpg.h")).read()
    assert '#include "minimarl_rmaddpg.h"' in open(os.path.join(ROOT, "include", "minimarl.h")).read()
    assert set(re.findall(r"\b(mm_rmaddpg[a-z0-9_]*)\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))) == WANT
    assert WANT <= set(symbols())
    if not os.path.exists(LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    for name in WANT:
        assert hasattr(lib(), name), name


@pytest.mark.parametrize("kw", [dict(prev_act_inp=True), dict(use_popart=True), dict(recurrent_N=2),
                                dict(use_same_share_obs=False), dict(n_policies=2)])
def test_public_names(kw):
    import minimarl
    assert "RMADDPG" in minimarl.__all__ and minimarl.RMADDPG.__name__ == "RMADDPG"
    with pytest.raises(ValueError):
        minimarl.RMADDPG(2, 47, 5, 4, 5, device="cpu", **kw)
    with pytest.raises(ValueError):
        minimarl.RMADDPG(9, 47, 5, 4, 5, device="cpu")       # critic width 468 > 416
