"""CPU: the feed-forward MAPPO restatement (tests/mappo_ff_ref.py) against the reference's goldens with the two
recurrent flags off (tests/golden/mappo_ff_fwd.npz, mappo_ff_train.npz): pins the oracle the GPU tests compare with."""
import numpy as np
import torch

import mappo_ff_ref as ff
import mappo_mb_ref as mb
from oracle import mappo as om

TOL = dict(rtol=1e-5, atol=2e-6)   # forward values and log-probs (tests/test_gpu_mappo.py)


def test_forward_reproduces_the_golden_get_actions(golden):
    """Values and log-probs of the recorded actions; the hiddens the reference hands back are its inputs; the 12
    tensors per net are all the fixture's nets hold."""
    fx = golden("mappo_ff_fwd")
    PA, PC = ff.nets(fx)
    assert sorted(k for k in fx if k.startswith("actor.")) == sorted("actor." + om.ref_name(k, "actor")
                                                                      for k in ff.FF_KEYS)
    assert sorted(k for k in fx if k.startswith("critic.")) == sorted("critic." + om.ref_name(k, "critic")
                                                                       for k in ff.FF_KEYS)
    v, a, lp = ff.get_actions(PA, PC, torch.from_numpy(fx["obs"]), actions=torch.from_numpy(fx["actions"]))
    np.testing.assert_allclose(v.numpy(), fx["values"], **TOL)
    np.testing.assert_allclose(v.numpy(), fx["get_values"], **TOL)
    np.testing.assert_allclose(lp.numpy(), fx["logp"], **TOL)
    np.testing.assert_array_equal(fx["ha_out"], fx["ha"])
    np.testing.assert_array_equal(fx["hc_out"], fx["hc"])


def test_oracle_loop_reproduces_the_golden_row_minibatch_train(golden):
    """The fp32 loop on the recorded row permutations: after.*, the ValueNorm state and the first three updates'
    gradients within K_FP32 fp32 spreads of the f64 run plus the golden's own distance to it (mappo_mb_ref's rule),
    the 18 pre-clip norms and the mean ratio at rtol 1e-5. 80 rows, 3 minibatches of 26, 2 rows dropped per epoch, 9
    updates; the one inactive row (55) first appears in update 2."""
    fx = golden("mappo_ff_train")
    PA, PC, data, vn0, rows = ff.train_inputs(fx)
    EP, M = int(fx["epochs"]), int(fx["train_batch_size"])
    assert (rows, M, fx["perms"].shape) == (80, 3, (EP, 80))
    runs = {}

    def run(dt, shuffle):
        if (dt, shuffle) not in runs:
            runs[(dt, shuffle)] = ff.ppo_train_ff(PA, PC, data, vn0, EP, fx["perms"], M, dtype=dt, shuffle=shuffle)
        return runs[(dt, shuffle)]

    o64, spread = mb.fp32_spread(lambda dt, sh: ff.train_outputs(*run(dt, sh)))
    g64, gspread = mb.fp32_spread(lambda dt, sh: ff.update_grads(run(dt, sh)[0], (0, 1, 2)))
    rec = run(torch.float32, False)[0]
    o32 = ff.train_outputs(*run(torch.float32, False))
    g32 = ff.update_grads(rec, (0, 1, 2))
    assert len(rec) == EP * M == 9 and all(r["rows"] == 26 for r in rec)
    assert [r["active"] for r in rec[:3]] == [26.0, 26.0, 25.0]
    for kind in ("actor", "critic"):
        for k in ff.FF_KEYS:
            after = fx[f"after.{kind}.{om.ref_name(k, kind)}"]
            ref_err = float(np.abs(after - o64[(kind, k)]).max())
            mb.assert_within(o32[(kind, k)], after, spread[(kind, k)], f"{kind} {k} vs golden", ref_err)
    for u in (0, 1, 2):
        for n in (0, 1):
            for k in ff.FF_KEYS:
                ref = mb.golden_grad(fx, u, n, k)
                mb.assert_within(g32[(u, n, k)], ref, gspread[(u, n, k)], f"update {u} net {n} {k} vs golden",
                                 float(np.abs(ref - g64[(u, n, k)]).max()))
    np.testing.assert_allclose(o32["norms"], fx["norms"], rtol=1e-5)
    for key, gk in (("vn_mean", "vn1.running_mean"), ("vn_mean_sq", "vn1.running_mean_sq")):
        mb.assert_within(o32[key], fx[gk], spread[key], key, float(np.abs(fx[gk] - o64[key]).max()))
    np.testing.assert_allclose(o32["ratio"], float(fx["info.ratio"]), rtol=1e-5)
