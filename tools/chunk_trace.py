"""Per-step timeline of ONE chunk-persistent launch (10 steps, 4096 envs x 8 agents), from the MM_ROLL_DEBUG build's
s_memrealtime stamps (csrc/agent_fwd.hip MM_CSTAMP, 100 MHz). The fp16x3 step loop runs each block as four 64-env
groups; stamped are, per behavior block and group, the group's dynamics wave and one other wave: per step 0 loop top,
1 hand-off words seen and the group past its reads of the previous step (dynamics wave), 2 dynamics done (dynamics
wave) / seen done (other wave), 3 forward done. Prints, per group, the medians over behavior blocks of each phase per
step, the per-step period and the group's lead over group 0 at each loop top, in us, and the in-kernel shader clock
(s_memtime / s_memrealtime around each block's step loop, after ~0.5 s of back-to-back launches: MI355X_MICROARCH.md
DVFS check). GPU only; needs `make -C mini-marl_amd debug` (CHUNK_TRACE_LIB = another MM_ROLL_DEBUG build)."""
import ctypes
import json
import os
import sys

import numpy as np
import torch

os.environ["MM_ROLL_TRACE"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mini-marl_amd")]
import minimarl._lib as L  # noqa: E402

L.LIB_PATH = os.path.abspath(os.environ.get("CHUNK_TRACE_LIB") or
                             os.path.join(ROOT, "mini-marl_amd", "lib_dbg", "libminimarl.so"))
from minimarl.engine import RolloutEngine  # noqa: E402

E, N, C = 4096, 8, 10
NG, NS = 4, 12                                      # groups per block, stamped steps (MM_CSTAMP)
assert L.lib().mm_debug_trace(None, 0) == 0
eng = RolloutEngine(E, N, f1=64, g=64, h=64, chunk=C, capacity=4 * E, seed=1, device="cuda", persistent=True)
for _ in range(3):
    eng.run_steps(20, 0.1)
out = {"lib": os.path.relpath(L.LIB_PATH, ROOT)}
for _ in range(2000):                               # ~0.5 s of back-to-back launches before the stamped ones (DVFS)
    eng.chunk_only(C)
r2 = lambda a: np.round(a, 2).tolist()              # noqa: E731
for rep in range(2):
    torch.cuda.synchronize()
    eng.chunk_only(C)
    torch.cuda.synchronize()
    buf = np.zeros(65536, np.uint64)
    assert L.lib().mm_debug_trace(buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), 65536) == 0
    nbb = (E // 256) * N                            # behavior blocks
    assert nbb * NG * 2 * NS * 4 <= 60000
    tr = buf[: nbb * NG * 2 * NS * 4].reshape(nbb, NG, 2, NS, 4).astype(np.int64)[:, :, :, :C, :]
    t0 = tr[tr > 0].min()
    rel = np.where(tr > 0, (tr - t0) * 0.01, np.nan)   # [block, group, dynamics wave / other wave, step, stamp]
    for j in range(NG):
        d, o = rel[:, j, 0], rel[:, j, 1]
        per = np.nanmedian(np.diff(d[:, :, 0], axis=1), axis=0)
        wait = np.nanmedian(d[:, 1:, 1] - d[:, 1:, 0], axis=0)
        dyn = np.nanmedian(d[:, :, 2] - np.where(np.isnan(d[:, :, 1]), d[:, :, 0], d[:, :, 1]), axis=0)
        fwd_d = np.nanmedian(d[:, :, 3] - d[:, :, 2], axis=0)
        owait = np.nanmedian(o[:, :, 2] - o[:, :, 0], axis=0)
        fwd_o = np.nanmedian(o[:, :, 3] - o[:, :, 2], axis=0)
        lead = np.nanmedian(rel[:, 0, 0, :, 0] - d[:, :, 0], axis=0)
        end = np.nanmax(rel[:, j, :, C - 1, 3])
        print(f"rep {rep} group {j}: period {r2(per)}\n  dynamics wave: wait {r2(wait)}\n    dyn {r2(dyn)}\n"
              f"    fwd {r2(fwd_d)}\n  other wave: wait for dynamics {r2(owait)}\n    fwd {r2(fwd_o)}\n"
              f"  loop top ahead of group 0 by {r2(lead)}  last end {end:.2f}")
        out[f"rep{rep}_group{j}"] = {"period": per.tolist(), "wait": wait.tolist(), "dyn": dyn.tolist(),
                                      "fwd_dyn_wave": fwd_d.tolist(), "other_wait": owait.tolist(),
                                      "fwd_other_wave": fwd_o.tolist(), "lead": lead.tolist(), "end": float(end)}
    # in-kernel clock: delta s_memtime / delta s_memrealtime x 100 MHz around every block's step loop
    nb = 2 * nbb
    ck = buf[60000:60000 + 4 * nb].reshape(nb, 4).astype(np.float64)
    ghz = (ck[:, 2] - ck[:, 0]) / np.maximum(ck[:, 3] - ck[:, 1], 1) * 0.1
    print(f"rep {rep} in-kernel clock GHz: median {np.median(ghz):.3f} min {ghz.min():.3f} max {ghz.max():.3f}")
    out[f"rep{rep}_clock_ghz_median"] = float(np.median(ghz))
print(json.dumps(out))
eng.check_errors()
