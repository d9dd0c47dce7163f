"""CPU: the C ABI of the rmaddpg / rmatd3 episode collector (mm_rmaddpg_collect*) is declared in
include/minimarl_rmaddpg_collect.h, which include/minimarl.h includes, exported by the library and bound by
minimarl._lib; "rmaddpg" / "rmatd3" belong to RMADDPGRunner alone."""
import os
import re

import pytest

from conftest import ROOT

WANT = {"mm_rmaddpg_collect", "mm_rmaddpg_collect_supported", "mm_rmaddpg_collect_switch",
        "mm_rmaddpg_collect_switch_supported"}


def test_symbols_declared_bound_and_exported():
    from minimarl._lib import LIB_PATH, lib, symbols
    txt = open(os.path.join(ROOT, "include", "minimarl_rmaddpg_collect.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert set(re.findall(r"\b(mm_rmaddpg_collect[a-z0-9_]*)\s*\(", txt)) == WANT
    assert '#include "minimarl_rmaddpg_collect.h"' in open(os.path.join(ROOT, "include", "minimarl.h")).read()
    assert WANT <= set(symbols())
    if not os.path.exists(LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    assert all(hasattr(lib(), name) for name in WANT)


@pytest.mark.parametrize("algo", ["rmaddpg", "rmatd3"])
def test_public_names_and_algorithm_names(algo):
    import minimarl
    from minimarl.config import OffQTrainConfig
    assert {"RMADDPGCollector", "RMADDPGRunner"} <= set(minimarl.__all__)
    cfg = OffQTrainConfig(algorithm_name=algo)
    assert cfg.algorithm_name in minimarl.RMADDPGRunner.ALGORITHMS
    for other in (minimarl.OffQRunner, minimarl.MOffQRunner, minimarl.MADDPGRunner):
        with pytest.raises(AssertionError):
            other(cfg)
