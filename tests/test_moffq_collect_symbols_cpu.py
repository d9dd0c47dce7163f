"""CPU: the C ABI of the transition collector and the transition replay (mm_moffq_collect*, mm_mlpbuf_*) is declared
in include/minimarl.h, exported by the library and bound by minimarl._lib; the public names resolve without a GPU."""
import os
import re

import pytest

from conftest import ROOT

WANT = {"mm_moffq_collect", "mm_moffq_collect_supported", "mm_moffq_collect_switch",
        "mm_moffq_collect_switch_supported", "mm_mlpbuf_create", "mm_mlpbuf_destroy", "mm_mlpbuf_insert",
        "mm_mlpbuf_stores", "mm_mlpbuf_advance", "mm_mlpbuf_len", "mm_mlpbuf_current", "mm_mlpbuf_it_capacity",
        "mm_mlpbuf_sample_prioritized", "mm_mlpbuf_sample_uniform", "mm_mlpbuf_gather", "mm_mlpbuf_update_priorities",
        "mm_mlpbuf_copy_state"}


def test_symbols_declared_bound_and_exported():
    from minimarl._lib import LIB_PATH, lib, symbols
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "minimarl.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mm_(?:moffq_collect|mlpbuf)[a-z0-9_]*)\s*\(", txt))
    assert declared == WANT
    assert WANT <= set(symbols())
    if not os.path.exists(LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    for name in WANT:
        assert hasattr(lib(), name), name


def test_public_names():
    import minimarl
    from minimarl.config import OffQTrainConfig
    for name in ("MOffQCollector", "MOffQRunner", "MlpReplayBuffer", "PrioritizedMlpReplayBuffer"):
        assert name in minimarl.__all__ and getattr(minimarl, name).__name__ == name
    with pytest.raises(AssertionError):                      # OffQRunner keeps to qmix / vdn
        minimarl.OffQRunner(OffQTrainConfig(algorithm_name="mqmix"))
    with pytest.raises(AssertionError):
        minimarl.MOffQRunner(OffQTrainConfig(algorithm_name="qmix"))
