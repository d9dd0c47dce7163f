"""CPU: the PPO-minibatch restatement (tests/mappo_mb_ref.py) against the reference's golden train() with
train_batch_size 3 (tests/golden/mappo_mb_train.npz), and the chunk renumbering minimarl.mappo feeds the kernels."""
import numpy as np
import pytest
import torch

import mappo_cv_ref as cv
import mappo_mb_ref as mb
from oracle import mappo as om


def test_oracle_loop_reproduces_the_golden_minibatch_train(golden):
    """The fp32 loop on the recorded perms: after.* within K_FP32 fp32 spreads of the f64 run plus the golden's own
    distance to it (mappo_mb_ref's rule), the 18 pre-clip norms at rtol 1e-5. 16 chunks, 3 minibatches of 5, one
    chunk dropped per epoch, 9 updates."""
    fx = golden("mappo_mb_train")
    PA, PC, data, vn0, nch = cv.train_inputs(fx)
    EP, L, M = int(fx["epochs"]), int(fx["L"]), int(fx["train_batch_size"])
    assert (nch, M, fx["perms"].shape) == (16, 3, (EP, 16))
    runs = {}

    def f(dt, shuffle):
        rec, PA2, PC2, vn = mb.ppo_train_mb(PA, PC, data, vn0, EP, L, fx["perms"], M, dtype=dt, shuffle=shuffle)
        runs[(dt, shuffle)] = rec
        return mb.train_outputs(rec, PA2, PC2, vn)

    o64, spread = mb.fp32_spread(f)
    o32 = f(torch.float32, False)
    rec = runs[(torch.float32, False)]
    assert len(rec) == EP * M == 9 and all(r["rows"] == 5 * L for r in rec)
    for kind in ("actor", "critic"):
        for k in om.NET_KEYS:
            after = fx[f"after.{kind}.{om.ref_name(k, kind)}"]
            ref_err = float(np.abs(after - o64[(kind, k)]).max())
            mb.assert_within(o32[(kind, k)], after, spread[(kind, k)], f"{kind} {k} vs golden", ref_err)
    np.testing.assert_allclose([x for r in rec for x in (r["na"], r["nc"])], fx["norms"], rtol=1e-5)
    for key, gk in (("vn_mean", "vn1.running_mean"), ("vn_mean_sq", "vn1.running_mean_sq")):
        mb.assert_within(o32[key], fx[gk], spread[key], key, float(np.abs(fx[gk] - o64[key]).max()))
    np.testing.assert_allclose(o32["ratio"], float(fx["info.ratio"]), rtol=1e-5)


@pytest.mark.parametrize("T,L,EN", [(10, 5, 8), (4, 2, 6), (3, 1, 5)])
def test_chunk_renumbering_round_trips(T, L, EN):
    """reference c = en * (T / L) + kc <-> native kc * EN + en: a bijection of [0, T * EN / L), both ways, that maps
    a chunk to the same (kc, en), on numpy arrays and torch tensors."""
    from minimarl.mappo import chunks_native_to_ref, chunks_ref_to_native
    K, n = T // L, T // L * EN
    ref = np.arange(n)
    nat = chunks_ref_to_native(ref, T, L, EN)
    assert sorted(nat.tolist()) == list(range(n))
    np.testing.assert_array_equal(chunks_native_to_ref(nat, T, L, EN), ref)
    np.testing.assert_array_equal(chunks_ref_to_native(chunks_native_to_ref(ref, T, L, EN), T, L, EN), ref)
    for en in range(EN):
        for kc in range(K):
            assert nat[en * K + kc] == kc * EN + en
    t = chunks_ref_to_native(torch.from_numpy(ref), T, L, EN)
    np.testing.assert_array_equal(t.numpy(), nat)
