"""minimarl — MI355X-native QMIX / VDN rollout-and-learn hot path (HIP kernels behind a C ABI).

Product path only: everything here runs through libminimarl.so (built from
``mini-marl_amd/csrc`` for gfx950). Importing this package does not touch the
GPU; the first op loads the library and raises if it was not built.
"""
from ._lib import lib, symbols  # noqa: F401

_LAZY = {"OffQCollector": "offq_runner", "OffQRunner": "offq_runner",
         "MOffQCollector": "moffq_runner", "MOffQRunner": "moffq_runner",
         "MlpReplayBuffer": "mlpbuf", "PrioritizedMlpReplayBuffer": "mlpbuf", "MADDPG": "maddpg",
         "MADDPGCollector": "maddpg_runner", "MADDPGRunner": "maddpg_runner", "RMADDPG": "rmaddpg",
         "RMADDPGCollector": "rmaddpg_runner", "RMADDPGRunner": "rmaddpg_runner"}
__all__ = ["lib", "symbols"] + list(_LAZY)


def __getattr__(name):
    # the offpolicy collectors, runners and the transition replay, imported on first use
    if name in _LAZY:
        import importlib
        return getattr(importlib.import_module("." + _LAZY[name], __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
